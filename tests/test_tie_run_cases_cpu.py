"""What the streams of tests/tie_run_cases.py are, proven on the CPU -- so that tests/test_gpu_tie_runs.py, which holds the
tie resolver's kernels to the oracle's fp32 event-order sums bit for bit on them, cannot pass on a wrong order:

(a) every voxel's run has the length the case says (counted from the oracle's own coordinates);
(b) the C oracle's DSI of every stream equals tests/independent_numpy.py's, bit for bit (weights down to 1e-3, runs
    of 20,000 votes: where the two had not met);
(c) ORDER SENSITIVITY: the same packets in another order (P1 .. P3 of tie_run_cases.reordered) change the bits of the
    reference's sums, while the exact integer sums (fill_voxel_grid_q31) stay what they were;
(d) the long runs take every branch of the window loop of k_tie_sort_runs<4096> (tie_run_cases.window_model);
(e) the thresholds the cases straddle are the ones in dsi_kernels.hip / dsi_engine.cpp: a retuning fails here.
"""
import functools
import os
import re

import numpy as np
import pytest

import independent_numpy as ind
import tie_run_cases as T
from tie_run_reference import oracle_mapper, reference

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dvs_mcemvs_amd", "csrc")
ORDERS = ("P1", "P2", "P3")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1)


def _dims(case):
    return case.cam[0], case.cam[1], case.shape[0]


# ---- (a) run lengths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_expected_votes_are_counted_from_the_oracles_coordinates(name):
    """Plain numpy over the oracle's stage A: X = (x0 a + bx) / d per event and plane, the accept test, four corners."""
    case = T.case(name)
    nx, ny, nz = _dims(case)
    count = np.zeros((nz, ny * nx), np.int64)
    if case.first.size:
        r = oracle_mapper(case, exact=True)
        assert np.array_equal(r.count, case.votes)          # the C oracle's own count of the votes
        xy, centers = r.stage_a(case.x, case.y, case.first.astype(np.int64), case.Rt)
        for k, idx, _ in ind._plane_votes(xy, centers, r.planes, r.Kv, nx, ny):
            np.add.at(count[k], idx.reshape(-1), 1)
    assert np.array_equal(count.reshape(nz, ny, nx), case.votes)


def test_every_ladder_length_occurs_on_exactly_its_own_voxels():
    case = T.ladder()
    nx, ny, nz = _dims(case)
    assert sorted(n for _, _, n in T.ladder_hot()) == sorted(T.LADDER)
    for x, y, n in T.ladder_hot():
        assert 2 <= x < nx - 3 and 2 <= y < ny - 3
        at = np.flatnonzero(case.votes.reshape(-1) == n)
        assert at.size == 4 * nz and np.array_equal(np.sort(T.rung_voxels((nx, ny, nz), x, y)), at), n
    xs = sorted(x for x, _, _ in T.ladder_hot())
    assert min(b - a for a, b in zip(xs, xs[1:])) >= 3
    background = np.setdiff1d(np.unique(case.votes), list(T.LADDER) + [0])
    assert background.size >= 20 and background.max() < 4096    # the far region: short runs of varied lengths
    assert case.x.size == T.LADDER_PACKETS * 1024


def test_stream_sizes_and_position_bits():
    bits = {n: T.pos_bits(T.stream_size(n).first.size) for n in T.STREAM_SIZES}
    assert bits == {1: 10, 1023: 10, 1024: 10, 1025: 10, 2049: 11, 3073: 12}
    for n in T.STREAM_SIZES:
        c = T.stream_size(n)
        assert c.x.size == n and c.first.size == n // 1024 and int(c.votes.sum()) == 16 * 1024 * (n // 1024)
    assert T.pos_bits(T.LADDER_PACKETS) == 17 and T.pos_bits(64) == 16 and T.pos_bits(256) == 18


def test_shared_columns_and_the_burst_are_what_they_say():
    for L in T.SHARED_LENGTHS:
        c = T.shared_columns(L)
        x, y = T.SHARED_XY
        assert (c.votes[:, y:y + 2, x] == L).all() and (c.votes[:, y:y + 2, x + 1] == 2 * L).all()
        assert (c.votes[:, y:y + 2, x + 2] == L).all()
        a, b = T.hot_positions(c, x, y), T.hot_positions(c, x + 1, y)
        assert np.array_equal(a + 1, b) and (a // 1024 == b // 1024).all()     # alternating, inside packets
    c = T.layout("burst", 1024)
    at = T.hot_positions(c, *T.LAYOUT_XY)
    assert at.size == 1024 and at[0] % 1024 == 0 and at[-1] - at[0] == 1023    # exactly one whole packet
    c = T.burst_pair()
    x, y = T.LAYOUT_XY
    assert (c.votes[:, y:y + 2, x + 1] == 1024).all()
    assert np.unique(np.concatenate([T.hot_positions(c, x, y), T.hot_positions(c, x + 1, y)]) // 1024).size == 1
    for name in T.LAYOUTS:
        for L in T.LAYOUT_LENGTHS:
            c = T.layout(name, L)
            assert c.first.size >= 64 and T.hot_positions(c, *T.LAYOUT_XY).size == L


# ---- (b) a second opinion on the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_the_oracle_equals_the_independent_restatement(name):
    case = T.case(name)
    nx, ny, nz = _dims(case)
    r = oracle_mapper(case)
    planes = ind.depth_planes(case.shape[1], case.shape[2], nz)
    assert np.array_equal(planes, r.planes)
    want = np.zeros((nz, ny, nx), np.float32)
    if case.first.size:
        xy, centers = [], []
        for k, f in enumerate(case.first.astype(np.int64)):
            C, H = ind.packet_geometry(case.Rt[k], r.K, r.Kv, planes[0])
            centers.append(C)
            xy.append(ind.warp_z0(case.x[f:f + 1024], case.y[f:f + 1024], H))
        ind.fill_voxel_grid(np.concatenate(xy), np.array(centers), planes, r.Kv, nx, ny, want)
    assert np.array_equal(_bits(reference(name)), _bits(want))
    assert bool(case.votes.any()) == bool(reference(name).any())


def test_the_ramp_reaches_small_and_large_weights():
    """A corner's weights run from about 1e-3 to about 1 over the stream (what makes an fp32 running sum order-dependent)."""
    case = T.ladder()
    r = oracle_mapper(case)
    xy, centers = r.stage_a(case.x, case.y, case.first.astype(np.int64), case.Rt)
    nx, ny, nz = _dims(case)
    k, idx, w = next(ind._plane_votes(xy, centers, r.planes, r.Kv, nx, ny))
    assert k == 0 and w.shape[0] == case.x.size             # every event is accepted on the nearest plane
    for corner in (0, 3):
        assert w[:, corner].min() < 4e-3 and w[:, corner].max() > 0.8 and w[:, corner].min() > 0
    first, last = w[:1024, 3].mean(), w[-1024:, 3].mean()
    assert first > 0.5 and last < 0.02                      # corner (1, 1): large early, small late


# ---- (c) order sensitivity -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _changed(name):
    """{P: bool per voxel: the reference's sum changes bits under P}; the exact integer sums must not change."""
    case = T.case(name)
    base = _bits(reference(name))
    acc = oracle_mapper(case, exact=True).acc
    out = {}
    for P in ORDERS:
        other = T.reordered(case, P)
        assert np.array_equal(oracle_mapper(other, exact=True).acc, acc), "%s: %s changes the multiset of votes" % (name, P)
        out[P] = _bits(oracle_mapper(other).dsi) != base
    return out


def _sensitive(name, voxels, orders=ORDERS):
    ch = _changed(name)
    for P in orders:
        assert 2 * int(ch[P][voxels].sum()) >= voxels.size, "%s: %s changes %d of %d voxels" % (
            name, P, int(ch[P][voxels].sum()), voxels.size)
    every = np.zeros(voxels.size, bool)
    for P in orders:
        every |= ch[P][voxels]
    assert every.all(), "%s: %d of %d voxels keep their bits under %s" % (name, int((~every).sum()), voxels.size, orders)


@pytest.mark.parametrize("rung", [n for n in T.LADDER if n >= 64])
def test_a_wrong_order_changes_the_bits_of_every_ladder_rung(rung):
    """Under EACH of P1, P2, P3 at least half of the rung's 4 nz voxels change bits, and every one of them changes under
    at least one.  (Holds for the committed SEED / JITTER; not for every seed.)"""
    x, y, _ = [h for h in T.ladder_hot() if h[2] == rung][0]
    _sensitive("ladder", T.rung_voxels(T.LADDER_DIMS, x, y))


@pytest.mark.parametrize("name", [n for n in T.LAYOUT_CASES if not n.startswith("burst")] + T.SHARED_CASES)
def test_a_wrong_order_changes_the_bits_of_every_layout(name):
    x, y = T.SHARED_XY if name in T.SHARED_CASES else T.LAYOUT_XY
    vox = T.rung_voxels(T.LADDER_DIMS, x, y)
    if name in T.SHARED_CASES:                               # all three columns of the pair
        vox = np.unique(np.concatenate([vox, T.rung_voxels(T.LADDER_DIMS, x + 1, y)]))
    _sensitive(name, vox)


@pytest.mark.parametrize("L", T.LAYOUT_LENGTHS)
def test_what_a_burst_can_and_cannot_show(L):
    """A burst is one pixel in consecutive positions, and a pixel's votes of one packet are EQUAL (the weights depend on
    the packet alone).  So a burst inside one packet (L = 1024) has an order-free sum -- no reordering can change it --
    and a longer one depends on the order of its few packets only: P1 reverses them (every voxel changes), P2 and P3
    move whole packets around a burst that straddles neither cut, and change nothing.  The burst cases pin the counts,
    the one-bucket path and the narrowing windows; the order INSIDE a one-packet bucket is pinned by `burst pair`."""
    name = "burst %d" % L
    vox = T.rung_voxels(T.LADDER_DIMS, *T.LAYOUT_XY)
    ch = _changed(name)
    assert not ch["P2"][vox].any() and not ch["P3"][vox].any()
    if L == 1024:
        assert not ch["P1"][vox].any()
    else:
        _sensitive(name, vox, orders=("P1",))


def test_the_order_inside_a_one_packet_bucket_shows_on_the_burst_pair():
    x, y = T.LAYOUT_XY
    shared = np.intersect1d(T.rung_voxels(T.LADDER_DIMS, x, y), T.rung_voxels(T.LADDER_DIMS, x + 1, y))
    assert shared.size == 2 * T.LADDER_DIMS[2]
    _sensitive("burst pair", shared, orders=("P1",))


# ---- (d) branch cover of the window loop ---------------------------------------------------------------------------------
def _windows(name):
    case = T.case(name)
    return T.window_model(T.hot_positions(case, *T.LAYOUT_XY), T.pos_bits(case.first.size))


def test_the_layouts_take_every_branch_of_the_window_loop():
    for L in (6000, 20000):
        narrowed, widened, n_sorted = _windows("cluster+tail %d" % L)
        assert narrowed == 2 and widened == 2 and n_sorted >= 12, (L, narrowed, widened, n_sorted)
        narrowed, widened, n_sorted = _windows("spread %d" % L)
        assert narrowed == 0 and widened == 0 and n_sorted >= 4
        assert _windows("burst %d" % L)[0] >= 1 and _windows("two clusters %d" % L)[0] >= 1
    # up to kTieRunLds = 4096 votes a run is sorted in one piece, whatever its layout: a burst of 3,000 is the one full
    # bucket of the (2048, 4096] class, not a window
    for name in T.LAYOUTS:
        for L in (1024, 3000):
            assert _windows("%s %d" % (name, L)) == (0, 0, 0)
    # the ladder's long rungs (random positions) enter the loop, too
    ladder = T.ladder()
    for x, y, n in T.ladder_hot():
        w = T.window_model(T.hot_positions(ladder, x, y), T.pos_bits(ladder.first.size))
        assert (w[2] >= 2) == (n > 4096), (n, w)


def test_window_model_on_hand_made_runs():
    assert T.window_model(np.arange(4096), 13) == (0, 0, 0)
    # 4,097 consecutive positions of 2^13: windows of 2^11 positions (4097 >> 2 = 1024 votes aimed at): two full ones (2,048
    # votes are not "more than CAP / 2"), one vote in the third, nothing in the fourth; widened once, at the aligned end
    assert T.window_model(np.arange(4097), 13) == (0, 1, 3)
    # 5,000 votes on 2^16 positions, 4,000 of them consecutive: the first window of 2^13 holds too many
    pos = np.concatenate([np.arange(4000), 4000 + 61 * np.arange(1000)])
    narrowed, widened, n_sorted = T.window_model(pos, 16)
    assert narrowed >= 1 and widened >= 1


# ---- the order in which the windows are appended ---------------------------------------------------------------------------
def _votes_in_event_order(case):
    """Per plane: (voxel index [n][4], fp32 weight [n][4]) of every event, in event order (all events of these cases are
    accepted on every plane)."""
    r = oracle_mapper(case)
    nx, ny, nz = _dims(case)
    xy, centers = r.stage_a(case.x, case.y, case.first.astype(np.int64), case.Rt)
    out = []
    for k, idx, w in ind._plane_votes(xy, centers, r.planes, r.Kv, nx, ny):
        assert idx.shape[0] == case.first.size * 1024
        out.append((idx, w))
    return out


def _sum_in_order(w):
    """x = 0; x += w[i] one by one in fp32 (np.add.accumulate is sequential)."""
    return np.add.accumulate(np.asarray(w, np.float32), dtype=np.float32)[-1] if len(w) else np.float32(0)


WINDOWED_RUNS = ([("ladder", h) for h in T.ladder_hot() if h[2] > 4096] +
                 [(n, T.LAYOUT_XY + (int(n.split()[-1]),)) for n in T.LAYOUT_CASES if int(n.split()[-1]) > 4096])


@pytest.mark.parametrize("name,hot", WINDOWED_RUNS, ids=["%s %d" % (n, h[2]) for n, h in WINDOWED_RUNS])
def test_windows_appended_in_another_order_change_the_bits(name, hot):
    """The windowed path of k_tie_sort_runs<4096> writes window after window at first + done.  Restated on the CPU: the
    run's weights, taken window by window as window_partition walks the positions and added one by one in fp32, give the
    oracle's bits; the same windows appended back to front (each still ascending inside: what writing a window BEFORE the
    previous one produces) change the bits of at least half of the run's voxels.  So a kernel that sorts every window
    correctly and appends them in a wrong order fails the GPU comparison on these runs."""
    case = T.case(name)
    x, y, n = hot
    nx, ny, nz = _dims(case)
    pos = T.hot_positions(case, x, y)
    assert pos.size == n
    windows = T.window_partition(pos, T.pos_bits(case.first.size))
    assert len(windows) >= 2 and sum(hi - lo for lo, hi in windows) == n
    votes = _votes_in_event_order(case)
    ref = reference(name)
    changed = 0
    for v in T.rung_voxels((nx, ny, nz), x, y):
        k, cell = divmod(int(v), nx * ny)
        idx, w = votes[k]
        at = idx[pos] == cell                               # one corner per event of the hot pixel
        assert (at.sum(axis=1) == 1).all()
        run = w[pos][at]                                    # the voxel's weights in event order
        forward = np.concatenate([run[lo:hi] for lo, hi in windows])
        assert _bits(_sum_in_order(forward))[0] == _bits(ref[k].reshape(-1)[cell])[0]
        backward = np.concatenate([run[lo:hi] for lo, hi in windows[::-1]])
        changed += int(_bits(_sum_in_order(backward))[0] != _bits(ref[k].reshape(-1)[cell])[0])
    assert 2 * changed >= 4 * nz, "%s: %d of %d voxels change" % (name, changed, 4 * nz)


# ---- partition paths: sizes from the rule ---------------------------------------------------------------------------------
def test_partition_cases_straddle_the_rank_and_stretch_thresholds():
    """launch_tie_partition_sums: stretches of max(8192, ceil(records / 256)) records.  records = 1024 x the segments the
    event pass hands out, one partly filled segment per (workgroup, voxel share) that recorded anything -- so the model
    counts hits per workgroup and share.  One stretch: 60 voting events in one packet of 512 (4 shares, one segment
    each: 4,096 records <= 8,192).  Tail: 2,089 voting events x 40 votes + ~40 partly filled segments = 110,592 records
    = 13.5 stretches of 8,192 (9 .. 15: one unrolled turn of k_tie_colscan and a tail of 6; a margin of a stretch either
    way).  256 stretches: 176 full packets x 40 votes = 7.2 M records > 256 x 8,192."""
    want = {"lds, 1 stretch": (30720, 1, 1), "lds, tail": (30720, 9, 15), "lds, 256 stretches": (30720, 256, 256),
            "global atomics": (33792, 2, 256)}
    for name in T.PARTITION_CASES:
        case = T.partition(name)
        ranks, lo, hi = want[name]
        model = T.partition_model(case)
        assert case.votes.size == ranks and lo <= model["stretches"] <= hi, (name, model)
        assert model["worst_block_hits"] < 512 * 1024
    assert T.partition_model(T.partition("lds, 1 stretch"))["records"] <= 8192 - 2048
    assert T.partition_model(T.partition("lds, 256 stretches"))["records"] > 3 * 256 * 8192
    for name in ("lds, tail", "lds, 256 stretches", "global atomics"):
        assert (T.partition(name).votes == 2049).sum() >= 4 * T.partition(name).shape[0]
    for name in ("lds, 256 stretches", "global atomics"):
        assert (T.partition(name).votes == 4097).sum() == 4 * T.partition(name).shape[0]
    # scratch growth: the big call does not fit the first pass's 2^22 records, the ladder does
    assert T.partition_model(T.growth())["records"] > (1 << 22) + (1 << 19)
    assert T.partition_model(T.ladder())["records"] < (1 << 21)
    # 256 planes, one packet: 4,096 hits per plane, 16 shares of 16 planes: 64 k hits per workgroup (it answers);
    # the burst's 1,024 voxels asked alone are ONE share: 1,024 events x 4 x 256 = 1 M hits > 512 k (it refuses)
    m = T.partition_model(T.planes256())
    assert m["shares"] == 16 and m["worst_block_hits"] == 65536 and m["records"] == 1 << 20
    assert (T.planes256().votes.reshape(256, -1).sum(axis=1) == 4096).all()
    assert int(T.planes256_burst().votes.sum()) == 1024 * 4 * 256 > 512 * 1024


# ---- (e) the thresholds in the source --------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_thresholds_the_cases_straddle_are_the_sources():
    k = _source("dsi_kernels.hip")
    e = _source("dsi_engine.cpp")

    def const(pattern, text=k):
        m = re.search(pattern, text)
        assert m, pattern
        return m.group(1)

    assert const(r"constexpr int kTieRunLds = (\d+);") == "4096"
    assert const(r"constexpr int kTiePartLdsRanks = (\d+);") == "30720"
    assert const(r"constexpr unsigned long long kTiePartStretches = (\d+)ull;") == "256"
    assert const(r"constexpr int kTieSegShift = (\d+);") == "10"
    assert const(r"constexpr int kTieMaxSegs = (\d+);") == "512"
    # the three classes of runs: (0, 1024], (1024, 2048], (2048, ..) in windows beyond 4096
    launches = re.findall(r"hipLaunchKernelGGL\(k_tie_sort_runs<(\w+)>, dim3\(n_ranks\), dim3\((\d+)\)", k)
    assert launches == [("1024", "256"), ("2048", "512"), ("kTieRunLds", "512")]
    assert "cnt <= (uint32_t)(CAP == 1024 ? 0 : CAP / 2) || (CAP != kTieRunLds && cnt > (uint32_t)CAP)) return;" in k
    # the window loop that window_model restates
    assert "> (unsigned long long)(CAP / 4)) --span_bits;" in k
    assert "if (n > (uint32_t)(CAP / 2)) {" in k
    assert "if (n < (uint32_t)(CAP / 16) && span_bits < pos_bits && (lo & ((1ull << (span_bits + 1)) - 1ull)) == 0ull) ++span_bits;" in k
    # buckets: the next power of two >= n, from 64
    assert re.search(r"int nb = 64;\s*while \(nb < n\) nb <<= 1;", k)
    # the addition kernel: rows of 16 lanes, 64 weights per row and turn
    assert "const int r = blockIdx.x * 16 + (int)(threadIdx.x >> 4);" in k and "fetch(base + 64, w);" in k
    # the partition: LDS table up to kTiePartLdsRanks ranks, stretches of >= 8192 records, at most kTiePartStretches
    assert "const int use_lds = n_ranks <= (unsigned)kTiePartLdsRanks ? 1 : 0;" in k
    assert "std::max<unsigned long long>(8192ull, (n_rec + kTiePartStretches - 1ull) / kTiePartStretches);" in k
    assert "for (; b + 8 <= n_stretches; b += 8) {" in k
    # the event pass's launch geometry that partition_model restates
    assert "const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, max_dynamic_lds() / lds));" in k
    assert "const int blocks = std::min(np, 256 * per_cu);" in k
    assert "int vshares = std::max(1, std::min(std::min(16, (nsv + 1023) / 1024), (256 * per_cu) / blocks));" in k
    assert "size_t max_dynamic_lds() { return 160 * 1024 - 128; }" in k
    assert "return (size_t)kPacket * 12 + (size_t)tie_tile_words(tiles) * 4 + (size_t)nz * sizeof(TiePlane) + (size_t)kTieMaxSegs * 4;" in k
    # ... with sizeof(TiePlane) = 12 floats = 48 bytes, the tile words and the tiling that partition_model restates
    assert re.search(r"struct alignas\(16\) TiePlane \{[^}]*float a, bx, by, d;[^}]*float ia, qx, qy;[^}]*float hw;[^}]*"
                     r"float c_lo, c_hi;[^}]*float pad_\[2\];\s*\};", k)
    assert len(re.findall(r"\bfloat\b", re.search(r"struct alignas\(16\) TiePlane \{([^}]*)\};", k).group(1))) == 5
    assert "inline int tie_tile_words(int tiles) { return ((tiles + 2) / 2 + 3) & ~3; }" in k
    assert const(r"constexpr int kTieMaxTiles = (\d+);") == "16384"
    assert "b.margin = 32;" in k and "for (b.shift = 2;; ++b.shift) {" in k
    assert "b.tx_n = (nx + 2 * b.margin + (1 << b.shift) - 1) >> b.shift;" in k
    assert "if (b.tx_n * b.ty_n <= kTieMaxTiles) break;" in k
    # the first pass records into 2^22 slots; positions take bits_for(packets x 1024) bits
    assert "size_t cap = std::max<size_t>(ts.keys.cap, (size_t)1 << 22);" in e
    assert "const unsigned pos_bits = bits_for((unsigned long long)np_max * dsi::kPacket);" in e
    assert '"a workgroup recorded more than %d k votes: too many voxels asked for"' in e
