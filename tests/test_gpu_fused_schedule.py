"""Schedule-independence of the DSI-less kernels (k_vote_fuse_argmax, k_vote_fuse_argmax_2cu, k_vote_fuse_argmax_alg2): which
workgroup votes a (band, plane) pair, how many workgroups there are and in which order one workgroup meets the pairs of a
band change no bit of the depth map.

Every other test of these kernels runs them at ONE workgroup count (the CU count of the device the suite runs on) and with
whatever draw order the hardware happens to produce.  Here the count and the order are test inputs, through two hooks of the
EXPERIMENTS flavour of the engine (dsi_test_fused_grid_blocks, dsi_test_fused_solo) and its knob DSI_FUSED_INTERLEAVE; that
library is loaded only by child processes that opt in with DSI_ENGINE_EXPERIMENTS=1 (tests/fused_schedule_child.py), run one
after another, each with a time limit and its exit status checked.

The expected result of every run is the engine's own unfused path in the same child at the default settings --
evaluateDSI_batch x n, the fusion materialised, collapseMaxZSlice -- and the comparison `array_equal` on depth, confidence
and index.  Every case first asserts, on the fused DSI it has downloaded, that its input can show an order dependence at all:
at least 100 columns and 1 % of all columns whose non-zero maximum is attained on two or more planes, and at least 10 % of
empty columns (tied at 0 on every plane: index 0).  Measured with the CPU oracle while writing the test (columns / empty /
tied): 160 x 96 x 64, two cameras 15360 / 3631 / 6746, three 15360 / 3652 / 3490, four 15360 / 4901 / 7032; 160 x 96 x 100
15360 / 3134 / 5371; 160 x 96 x 20, three cameras 15360 / 3391 / 1947; 96 x 72 x 32 6912 / 1704 / 2621; the Alg. 2 window
6912 / 1803 / 2082 (time_camera) and 6912 / 1760 / 2722 (camera_time).
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case):
    env = dict(os.environ, DSI_ENGINE_EXPERIMENTS="1")
    env.pop("DSI_FUSED_INTERLEAVE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "fused_schedule_child.py"), case], capture_output=True, text=True,
                       env=env, timeout=120)
    print(r.stdout)
    different = [ln for ln in r.stdout.splitlines() if ln.startswith("DIFFERENT")]
    assert r.returncode == 0 and ("SCHEDULE_OK " + case) in r.stdout and not different, \
        "%d runs differ:\n%s\n%s" % (len(different), "\n".join(different[:12]), r.stdout[-1500:] + r.stderr[-3000:])


@pytest.mark.parametrize("case", ["solo_packed", "solo_vfill", "solo_three", "solo_four", "solo_three_bands"])
def test_draw_order_within_a_band_changes_no_bit(built, case):
    """The ORDER, pinned without any timing: the one-workgroup-per-CU kernel in its dealt mode, launched as a single
    workgroup that acts as workgroup 0 of XCD k.  It begins at pair P k / 8, draws that pair once more, runs to the end of
    the pair list, wraps to pair 0 and ends at pair P k / 8 - 1: with one band of 64 planes (160 x 96 x 64: 98 x 160 cells,
    above the two-per-CU kernel's 10 x 1024, within every mapping's and the four-camera kernel's 16 x 1024) the wrap is a
    draw that DESCENDS inside the band the workgroup is in -- what a dealt workgroup of a full launch meets when its XCD's
    counter is dry and another XCD hands it a lower pair of the same band.  The running arg-max keeps the first maximum with
    a strict compare, which is the reference's first maximum only while the planes ascend; so the pair loop re-opens the
    band (emit, reset) at a pair that does not ascend.  Without that every tied column whose first tied plane lies below
    k nz / 8 keeps a later plane, and every empty column the index k nz / 8 instead of 0.

    k = 1, 4, 7 for: two cameras on the packed stream (the instantiation that defers camera 1's arg-max update), two
    cameras on the vector fill (mapping 5), three cameras, four cameras fused by the geometric-mean tree; and k = 7 with
    three bands (the workgroup begins inside band 2 and re-enters it after bands 0 and 1).  The input condition counts only
    columns tied ACROSS the wrap: first tied plane below the first plane voted, another tied plane at or above it
    (measured, of 15360 columns: two cameras 2774 / 2712 / 1620 for k = 1 / 4 / 7, three 1362 / 1424 / 831, four 4053 / 6104 /
    3594, three bands 923).  Last, the same mapper runs the device's own launch again (the hook switched off).

    On the kernel as it was before the band was re-opened (one run on an MI355X, the hooks applied) the four one-band
    cases fail, confidence equal and depth / index different at, for k = 1 / 4 / 7: 6405 / 6343 / 5251 of 15360 pixels (two
    cameras, either mapping), 5014 / 5076 / 4483 (three), 8954 / 11005 / 8495 (four) -- the counts a CPU model of the draw
    order gives on the oracle's fused DSI.  The three-band case passes there too: the workgroup leaves band 2 for bands 0
    and 1 before it returns, and a band change always re-opened the band."""
    run_case(case)


@pytest.mark.parametrize("case", ["count_one_band", "count_three_bands", "count_three_bands_four_cameras",
                                  "count_twelve_bands", "count_two_per_cu", "count_two_per_cu_twelve_bands", "count_alg2",
                                  "count_alg2_fifteen_bands"])
def test_workgroup_count_and_dealing_mode_change_no_bit(built, case):
    """The workgroup COUNT, pinned: 8, 32 and 64 (a CPX- or QPX-partitioned device has 32 or 64 CUs; then a workgroup
    carries many pairs of one band) and the device's own, seen alike by the launches, the balanced partition and the trace.
    These runs do NOT control the order in which a dealt workgroup meets its pairs -- that is the hardware's timing, and
    the test above is the one that pins it; they pin the count, and with it the stretch arithmetic of every mode.

    Modes: contiguous pieces (DSI_FUSED_INTERLEAVE 0), pairs in turn (1), pairs dealt from the XCDs' counters (2; called
    twice on the same output mapper: the counters behind the keys must be zero again) and the balanced partition
    (k_fused_splits, dsi_test_fused_fixed_cost >= 0; two cameras, one-per-CU kernels).  Kernels and shapes: the one-per-CU
    kernel with one band of 100 planes (stretches of 12 and 13 pairs), with three bands (neighbouring XCDs share a band; two
    cameras on the vector fill, and four cameras) and with 12 bands x 20 planes, three cameras on the vector fill (240
    pairs: a forced count of 256 leaves workgroups without a pair; the vector fill keeps bands this small on the kernel
    that deals); the two-per-CU kernel (2 x count workgroups, no balanced partition, dealt = in turn there) at 96 x 72 x 32
    and at the same 12 bands x 20 planes on the packed stream; and k_vote_fuse_argmax_alg2 on one process_method-2 window
    (two sub-intervals, MIN across cameras, arithmetic mean over time; one band, and 15 bands of 5 rows) against process_2 +
    the arg-max of its two DSIs.

    That the forced count and mode took effect, and which kernel a case reaches, is not taken on trust: after every run the
    child asserts what dsi_test_fused_last_launch reports -- grid size, bp.interleave, kernel, balanced partition."""
    run_case(case)
