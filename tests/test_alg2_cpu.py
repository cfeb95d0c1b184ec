"""Alg. 2 windows without a DSI, the parts that need no GPU: the sub-interval split (Python and the engine's host helper
against a literal restatement of process2.cpp / process5.cpp), the planner's fixed limits and the ISA of the new kernel."""
import os
import re
import subprocess

import pytest

from dvs_mcemvs_amd import engine as E, process
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def literal_split(n_events, n_sub, shuffled):
    """process2.cpp:46-47, :105-107 (idx_first_ev += per) and process5.cpp:89-93, :135-150, line by line: lists of
    event indices per sub-interval."""
    per = n_events // n_sub
    idx_first_ev = (n_sub // 2) * per if shuffled else 0
    out = []
    for _ in range(n_sub):
        if shuffled and idx_first_ev + per >= n_events:
            subset = list(range(idx_first_ev, n_events)) + list(range(0, idx_first_ev + per - n_events))
            idx_first_ev = idx_first_ev + per - n_events
        else:
            subset = list(range(idx_first_ev, idx_first_ev + per))
            idx_first_ev += per
        out.append(subset)
    return out


def expand(ranges):
    return [list(range(b0, e0)) + list(range(b1, e1)) for b0, e0, b1, e1 in ranges]


CASES = [(10_000, 1), (10_000, 3), (10_001, 4), (10_007, 5), (9_000, 8), (3_000, 8), (0, 4), (5, 8), (4_096, 2),
         (4_097, 3), (8 * 1000, 8), (7, 7), (12, 3)]


@pytest.mark.parametrize("n_events,n_sub", CASES)
def test_split_python(n_events, n_sub):
    for pm in (2, 5):
        for camera in (0, 1):
            shuffled = pm == 5 and camera == 1
            assert expand(process.subinterval_ranges(n_events, n_sub, pm, camera)) == literal_split(n_events, n_sub, shuffled)


@pytest.mark.parametrize("n_events,n_sub", CASES)
def test_split_engine_helper(built, n_events, n_sub):
    for pm in (2, 5):
        for camera in (0, 1):
            assert E.alg2_subintervals(n_events, n_sub, pm, camera) == process.subinterval_ranges(n_events, n_sub, pm, camera)


def test_split_wrap_lands_on_the_end(built):
    """A wrap that lands exactly on |E1| (idx + per == |E1|, the `>=` case): the whole range first, an EMPTY second
    segment, and the next sub-interval starts at 0."""
    n, n_sub = 12, 3   # per 4, shift 1: idx 4 -> 8; 8 + 4 == 12 -> wrap with an empty head; then 0
    r = E.alg2_subintervals(n, n_sub, 5, 1)
    assert r == [(4, 8, 0, 0), (8, 12, 0, 0), (0, 4, 0, 0)]
    assert r == process.subinterval_ranges(n, n_sub, 5, 1)
    assert expand(r) == literal_split(n, n_sub, True)
    # the shuffled camera's sub-intervals agree with process.shuffled_subintervals (the yardstick's index arrays)
    for n_events, k in CASES:
        if n_events:
            assert [list(s) for s in process.shuffled_subintervals(n_events, k)] == literal_split(n_events, k, True)


def test_split_helper_arguments(built):
    for args in ((100, 0, 2, 0), (100, 4, 3, 0), (100, 4, 2, 2)):
        with pytest.raises(E.DsiError) as e:
            E.alg2_subintervals(*args)
        assert e.value.code == E.ERR_INVALID


def test_planner(built):
    """The engine's planner (dsi_alg2_plan), which the Python and the C++ streams share: at most 8 sub-intervals, rows the
    kernel's smallest register plan holds (3 rows of 6 x 1024 cells with camera_time, 12 x 1024 without), and at most
    1.25 M events per sub-interval."""
    assert process.alg2_plan(4, 1_000_000, 346) == "fused"
    assert process.alg2_plan(8, 2_000_000, 346) == "fused"
    assert process.alg2_plan(9, 1_000, 346) == "materialize"
    assert process.alg2_plan(2, 2_500_001, 346) == "materialize"
    assert process.alg2_plan(8, 20_000_000, 346) == "materialize"
    assert process.alg2_plan(2, 1_000, 2048) == "fused" and process.alg2_plan(2, 1_000, 2049) == "materialize"
    assert process.alg2_plan(2, 1_000, 4096, camera_time=False) == "fused"
    assert process.alg2_plan(2, 1_000, 4097, camera_time=False) == "materialize"


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_alg2_kernels_isa():
    """Every instantiation of k_vote_fuse_argmax_alg2 (lane mappings 1, 3, 5, 6 x camera_time on / off): no scratch, no
    VGPR spills, at most 128 VGPRs (one 1024-thread workgroup per CU)."""
    text = kernel_asm_text()
    seen = set()
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_vote_fuse_argmax_alg2" not in name:
            continue
        seen.add(name)
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0, name
        assert val("vgpr_count") <= 128, name
        # Scalar spills: the voting streams fill the SGPR file (106), and what the pair loop keeps beside them -- the
        # batch table's kernarg pointer, the pair and band bounds, the fusion switches -- goes to VGPR lanes (v_writelane /
        # v_readlane, no scratch) between the phases, as in the existing fused kernels (27-138 there).  Bounded per
        # instantiation so that a regression shows: the vector-fill mappings 5 / 6 keep ~30 more scalars of their own.
        mapping = int(re.search(r"k_vote_fuse_argmax_alg2ILi(\d)E", name).group(1))
        assert val("sgpr_spill_count") <= (8 if mapping in (1, 3) else 40), name
    assert len(seen) == 8, sorted(seen)


def test_cpp_alg2_stream_compiles_and_refuses_without_gpu(built, tmp_path):
    """dsi::full_sequence_depth_maps_alg2 and its test program compile against the installed headers (-Werror); without a
    GPU the program refuses to run (tests/test_gpu_alg2_stream.py runs it on one)."""
    exe = str(tmp_path / "test_alg2_stream")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_alg2_stream.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    import dvs_mcemvs_amd as d
    if d.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "no GPU" in r.stdout + r.stderr, r.stdout + r.stderr
