"""The tie resolver's reference-order sums (k_tie_hits_binned, k_tie_partition, k_tie_colscan / k_tie_scan,
k_tie_sort_runs<1024 | 2048 | 4096>, k_tie_add_runs) against the oracle's plain fp32 event-order DSI, BIT FOR BIT, on
streams whose run lengths are chosen (tests/tie_run_cases.py): every class of run and its edges (1024 | 1025,
2048 | 2049, 4096 | 4097), the windowed path with its narrowing and widening, one-packet buckets, the LDS table and the
global-atomic partition on long runs, 1 / 14 / 256 stretches, the counted repeat of the event pass, 256 planes.

tests/test_tie_run_cases_cpu.py proves on the CPU that these streams would show a wrong order: the same packets in
another order change the bits of the reference's sums on every rung of 64 votes and more.  Values are compared as
uint32 with array_equal; votes against the count made from the pixels alone.
"""
import numpy as np
import pytest

import dvs_mcemvs_amd as d
import tie_run_cases as T
from dvs_mcemvs_amd import engine
from oracle import oracle as orc
from test_gpu_exact_voxels import assert_bits
from tie_run_reference import reference

pytestmark = pytest.mark.gpu


def _open(ctx, case, mapper=None):
    nz, lo, hi = case.shape
    m = mapper or d.MapperEMVS(ctx, case.cam, d.ShapeDSI(0, 0, nz, lo, hi, 0.0))
    return m, d.EventBatch(ctx, case.x, case.y, case.Rt, case.first)


def _check_all(m, batch, name):
    case = T.case(name)
    vox = np.arange(case.votes.size, dtype=np.uint32)
    values, votes = m.exactVoxels(batch, vox)
    assert_bits(values, reference(name).reshape(-1), name)
    assert np.array_equal(votes, case.votes.reshape(-1)), "%s: %d vote counts differ" % (
        name, int((votes != case.votes.reshape(-1)).sum()))


def _one_call(ctx, name):
    m, b = _open(ctx, T.case(name))
    try:
        _check_all(m, b, name)
    finally:
        m.close()
        b.close()


@pytest.fixture(scope="module")
def ladder(ctx):
    m, b = _open(ctx, T.ladder())
    yield m, b
    m.close()
    b.close()


# ---- 1. the ladder, every voxel ----------------------------------------------------------------------------------------
def test_ladder_every_voxel(ladder):
    """Runs of 1 .. 20,000 votes: all three sort classes at their edges, the windowed path, rows of the addition kernel
    that end at different turns -- 3,840 ranks in one call."""
    m, b = ladder
    assert np.array_equal(m.raw_depths_vec_, orc.depth_planes(T.MIN_DEPTH, T.MAX_DEPTH, T.LADDER_DIMS[2]))
    _check_all(m, b, "ladder")


# ---- 2. subsets and the order of the list ------------------------------------------------------------------------------
def _rung(n, plane=None):
    x, y, _ = [h for h in T.ladder_hot() if h[2] == n][0]
    v = np.sort(T.rung_voxels(T.LADDER_DIMS, x, y))
    nx, ny, _ = T.LADDER_DIMS
    return v if plane is None else v[v // (nx * ny) == plane]


def _ask(ladder, vox, what):
    m, b = ladder
    vox = np.asarray(vox, np.uint32)
    values, votes = m.exactVoxels(b, vox)
    assert_bits(values, reference("ladder").reshape(-1)[vox], what)
    assert np.array_equal(votes, T.ladder().votes.reshape(-1)[vox]), what
    return votes


def test_ladder_shuffled_list_with_duplicates(ladder):
    rng = np.random.default_rng(1)
    vox = rng.permutation(T.ladder().votes.size).astype(np.uint32)
    vox = np.concatenate([vox[:3000], vox[100:600], _rung(20000), _rung(4097)[::-1], vox[:7]])
    votes = _ask(ladder, vox, "shuffled, duplicates")
    assert votes.max() == 20000


@pytest.mark.parametrize("rung", [4097, 20000])
def test_ladder_single_voxels(ladder, rung):
    """One rank: one workgroup of the sort, one busy row of one wave in the addition kernel."""
    for v in _rung(rung):
        assert _ask(ladder, [v], "voxel %d alone" % v)[0] == rung


@pytest.mark.parametrize("n", [1, 2, 3, 5, 15, 17, 31, 63, 65, 67])
def test_ladder_lists_that_fill_no_wave_or_workgroup(ladder, n):
    """A wave of k_tie_add_runs holds 4 runs and a workgroup 16: lists whose length is a multiple of neither, long and
    short runs mixed in the last, partly filled wave."""
    pool = np.concatenate([_rung(20000), _rung(4097), _rung(2049), _rung(1025), _rung(65), _rung(17), _rung(1)])
    _ask(ladder, np.sort(pool)[::max(1, pool.size // n)][:n], "%d voxels" % n)
    _ask(ladder, pool[:n], "the first %d" % n)


@pytest.mark.parametrize("before", [13, 14, 15, 16])
def test_ladder_empty_waves_between_long_runs(ladder, before):
    """64 consecutive voxels WITHOUT votes between long runs in the sorted list: whole waves of k_tie_add_runs (4 runs)
    and whole workgroups (16) leave through the empty-wave exit while their neighbours add thousands of votes; `before`
    shifts the empty stretch against the wave boundaries."""
    nx, ny, nz = T.LADDER_DIMS
    empty = 7 * nx + np.arange(64, dtype=np.uint32)                       # plane 0, row 7: below the hot rows, left of
    assert not T.ladder().votes.reshape(-1)[empty].any()                  # the far region
    head = np.sort(np.concatenate([_rung(n, plane=0) for n in (20000, 8193, 8192, 4097)]))[:before]
    tail = np.sort(np.concatenate([_rung(n, plane=1) for n in (20000, 8191, 4096, 2049)]))
    assert head.max() < empty.min() and empty.max() < tail.min()
    votes = _ask(ladder, np.concatenate([head, empty, tail]), "empty waves, %d runs before" % before)
    assert (votes[before:before + 64] == 0).all() and votes[:before].min() >= 4097 and votes[before + 64:].min() >= 2049


def test_ladder_only_empty_voxels(ladder):
    nx = T.LADDER_DIMS[0]
    votes = T.ladder().votes.reshape(-1)
    _ask(ladder, 7 * nx + np.arange(64, dtype=np.uint32), "64 empty voxels")
    _ask(ladder, np.flatnonzero(votes == 0)[:1001], "1,001 empty voxels")
    _ask(ladder, [0], "one empty voxel")


# ---- 3. shared columns, temporal layouts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.SHARED_CASES + T.LAYOUT_CASES + ["burst pair"])
def test_shared_columns_and_temporal_layouts(ctx, name):
    """Two pixels voting the same voxels inside every packet; a run as one burst (1,024: ONE bucket of 1,024 words, ordered
    by counting), spread, a cluster with a tail (windows narrow in the cluster and widen behind it), two clusters."""
    _one_call(ctx, name)


# ---- 4. stream sizes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.SIZE_CASES)
def test_stream_sizes(ctx, name):
    """No whole packet (nothing votes: every value and count is zero), one packet, one packet and an event left over,
    two and three packets: positions of 10, 11 and 12 bits."""
    _one_call(ctx, name)


# ---- 5. partition paths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.PARTITION_CASES)
def test_partition_paths(ctx, name):
    """30,720 ranks (the LDS table + k_tie_colscan) with 1, 14 and 256 stretches -- the column scan's tail alone, one
    unrolled turn and a tail, 32 unrolled turns -- and 33,792 ranks (one global atomic per vote), with hot pixels of 2,049
    and 4,097 votes.  How the streams' sizes follow from launch_tie_partition_sums' rule:
    test_tie_run_cases_cpu.test_partition_cases_straddle_the_rank_and_stretch_thresholds."""
    _one_call(ctx, "partition: " + name)


# ---- 6. scratch growth, both ways ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big_first", [True, False])
def test_counted_repeat_and_grown_scratch(ctx, big_first):
    """4.9 M records do not fit the 2^22 slots of a first pass: it only counts, and is repeated once with the counted room.
    On a fresh mapper that call comes first (then the ladder, in the grown scratch) or second (after the ladder)."""
    m, big = _open(ctx, T.growth())
    _, small = _open(ctx, T.ladder(), mapper=m)
    try:
        for name, b in ((("growth", big), ("ladder", small)) if big_first else (("ladder", small), ("growth", big))):
            _check_all(m, b, name)
    finally:
        for o in (m, big, small):
            o.close()


# ---- 7. two cameras through the whole resolver -----------------------------------------------------------------------------
def test_two_cameras_through_the_resolver(ctx):
    """camera x voxel ranks with long runs: two ladders (two seeds), fused by the harmonic mean, resolved with a gap of
    0.45.  Neighbouring planes of a hot column hold values within 0.64 .. 1 of each other (the corner weights change by
    1 / z per axis from plane to plane), so at least two planes of every hot column contend: the test derives the sure
    contenders from the oracle's fused volume and requires the resolver to have re-summed at least those."""
    names = ("ladder", "ladder, camera 1")
    pairs = [_open(ctx, T.case(n)) for n in names]
    ms, batches = [p[0] for p in pairs], [p[1] for p in pairs]
    out = d.MapperEMVS(ctx, T.ladder().cam, d.ShapeDSI(0, 0, T.LADDER_DIMS[2], T.MIN_DEPTH, T.MAX_DEPTH, 0.0))
    try:
        for m, b in zip(ms, batches):
            m.evaluateDSI_batch(b)
        out.computeDepthMapOfFusion(ms[0].dsi_, ms[1].dsi_, d.FUSE_HM)
        _, _, idx0 = out.fetchDepthMap()
        ref = orc.fuse2(reference(names[0]).copy(), reference(names[1]), d.FUSE_HM)
        rconf, ridx = orc.collapse_max_z(ref)
        info = out.resolveNearTies(ms, batches, d.FUSE_HM, rel_gap=0.45)
        depth, conf, idx = out.fetchDepthMap()
        assert info["gap_widenings"] == 0 and info["premise_ok"] == 1, info
        # the contenders, from the oracle: a voxel farther inside the gap than any rounding of the fused values
        # (1e-3 of the threshold; the engine's volumes are within 1e-4 of the oracle's) in a column with two such
        # voxels IS re-summed, in both cameras -- the columns of the longest runs among them
        best = ref.max(axis=0)
        sure = (best > 0) & (ref >= (best - np.float32(0.45) * best) * np.float32(1.001))
        sure &= sure.sum(axis=0) >= 2
        votes_sure = sum(int(T.case(n).votes[sure].sum()) for n in names)
        for rung in (20000, 8193, 8192, 8191, 4097):
            x, y, _ = [h for h in T.ladder_hot() if h[2] == rung][0]
            assert (sure[:, y:y + 2, x:x + 2].sum(axis=0) >= 2).all(), rung
        assert int(sure.sum()) >= 2 * 4 * len(T.LADDER) and votes_sure >= 2 * 2 * 4 * sum(T.LADDER)
        assert info["candidate_voxels"] >= int(sure.sum()) and info["votes"] >= votes_sure, (info, int(sure.sum()), votes_sure)
        assert np.array_equal(idx, ridx), "%d pixels differ; %r" % (int((idx != ridx).sum()), info)
        assert np.array_equal(depth, out.raw_depths_vec_[ridx])
        changed = idx != idx0
        assert int(changed.sum()) == info["changed_pixels"]
        assert_bits(conf[changed], rconf[changed], "confidence of the changed pixels")
        assert np.allclose(conf, rconf, rtol=1e-4, atol=1e-6)
        # the proof's own count of the votes (an independent kernel) against the count made from the pixels
        out.proveNearTies(ms, batches, d.FUSE_HM, rel_gap=0.45)
        vox = np.arange(T.ladder().votes.size, dtype=np.uint32)
        for c, n in enumerate(names):
            assert np.array_equal(out.proofVotes(c, vox), T.case(n).votes.reshape(-1)), n
    finally:
        for o in ms + batches + [out]:
            o.close()


# ---- 8. 256 planes ---------------------------------------------------------------------------------------------------------
def test_256_planes_every_voxel_of_one_full_packet(ctx):
    """4,096 hits per plane from one workgroup's packet.  Every voxel asked: 32,768 voxels are dealt to 16 workgroups of 16
    planes each (launch_tie_hits_binned: min(16, voxels / 1024) shares), 64 k hits per segment table of 512 k: it ANSWERS.
    The 1,024 voxels of a one-pixel burst asked alone are one share: 1 M hits in one table -- it REFUSES, and the next call
    on the same mapper is exact again."""
    m, b = _open(ctx, T.planes256())
    _, burst = _open(ctx, T.planes256_burst(), mapper=m)
    try:
        _check_all(m, b, "256 planes")
        _check_all(m, burst, "256 planes, burst")
        x, y, _ = T.PLANES256_HOT
        with pytest.raises(d.DsiError) as err:
            m.exactVoxels(burst, T.rung_voxels(T.PLANES256_DIMS, x, y))
        assert err.value.code == engine.ERR_INVALID and "a workgroup recorded more than 512 k votes" in str(err.value)
        _check_all(m, b, "256 planes")
    finally:
        for o in (m, b, burst):
            o.close()
