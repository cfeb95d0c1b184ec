"""Event streams on which every voxel's run of votes has a CHOSEN length, for the exact tie resolver's kernels
(k_tie_hits_binned, k_tie_partition, k_tie_colscan / k_tie_scan, k_tie_sort_runs, k_tie_add_runs).  TEST INFRASTRUCTURE,
numpy only: tests/test_tie_run_cases_cpu.py proves on the CPU what these inputs are, tests/test_gpu_tie_runs.py feeds
them to the kernels.

Geometry.  R = I and a packet centre C = (Cx, Cy, 0): an event at pixel (x, y) lands on the plane of depth z at
(x + f Cx / z, y + f Cy / z) (mapper_emvs_stereo.cpp:108-120, :177-195 with Cz = 0: a = d = z0 z, bx = (z0 - z) f Cx).
Both shifts stay inside (0, 1) on every plane, so every event of a "hot pixel" (x, y) votes the same 2 x 2 voxels
(x .. x + 1, y .. y + 1) of every plane: a hot pixel with n events gives each of its 4 nz voxels a run of exactly n
votes, whatever the weights are (a zero-weight corner would still be a vote).  The weights depend on the packet alone:
the shift on the nearest plane runs from S_HI down to S_LO over the stream (plus a seeded jitter per packet), so the
weight of corner (1, 1) ramps from ~0.9 down to ~1e-3 and that of corner (0, 0) the other way.  Late small weights are
absorbed by a large fp32 running sum and early ones are not: that is what makes the reference's event-order sum depend
on the order, and a kernel that adds the right votes in a wrong order visible in the sum's bits.

A case is (x, y, first, Rt, cam, shape, votes): events (uint16), packet starts (uint32), poses [np][12] (float32),
cam = (width, height, fx, fy, cx, cy), shape = (dimZ, min_depth, max_depth), votes = the expected votes per voxel
[nz][ny][nx] (uint32), counted from the pixels alone.
"""
import functools
from collections import namedtuple

import numpy as np

PACKET = 1024
Case = namedtuple("Case", "x y first Rt cam shape votes")

# committed with the cases: tests/test_tie_run_cases_cpu.py (order sensitivity) holds for THESE values, not for every seed
SEED = 8
JITTER = 0.35           # width of the drawn part of a packet's shift around the trend over the stream (clipped)
S_HI, S_LO = 0.96, 0.04  # the shift on the nearest plane, first packet .. last packet
FOCAL = 64.0
MIN_DEPTH, MAX_DEPTH = 1.0, 2.0

LADDER = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
          8191, 8192, 8193, 20000)
LADDER_DIMS = (80, 12, 4)
LADDER_PACKETS = 72
LADDER_Y = 5
LAYOUTS = ("burst", "spread", "cluster+tail", "two clusters")
LAYOUT_LENGTHS = (1024, 3000, 6000, 20000)
LAYOUT_PACKETS = {1024: 64, 3000: 64, 6000: 64, 20000: 256}   # 20,000 votes need positions of > 16 bits to ever narrow
SHARED_LENGTHS = (1025, 4097)
SHARED_PACKETS = 16
STREAM_SIZES = (1, 1023, 1024, 1025, 2049, 3073)              # events in all: 0, 0, 1, 1, 2, 3 packets
SMALL_RUNGS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129)   # 627 votes: they fit one packet
PARTITION_CASES = ("lds, 1 stretch", "lds, tail", "lds, 256 stretches", "global atomics")


def bits_for(values):
    """dsi_engine.cpp: the bits that hold 0 .. values - 1 (at least one)."""
    b = 1
    while b < 64 and (1 << b) < values:
        b += 1
    return b


def pos_bits(n_packets):
    return bits_for(max(n_packets, 1) * PACKET)


def _cam(nx, ny):
    return (nx, ny, FOCAL, FOCAL, 0.5 * nx, 0.5 * ny)


def _poses(n_packets, rng):
    t = np.linspace(0.0, 1.0, n_packets) if n_packets > 1 else np.zeros(n_packets)
    u = np.clip(t[:, None] + JITTER * (rng.random((n_packets, 2)) - 0.5), 0.0, 1.0)
    shift = S_HI - (S_HI - S_LO) * u                       # on the plane at MIN_DEPTH; smaller on every other plane
    Rt = np.zeros((n_packets, 12), np.float32)
    Rt[:, 0] = Rt[:, 4] = Rt[:, 8] = 1.0
    Rt[:, 9:11] = -(shift * MIN_DEPTH / FOCAL)              # C = -R^T t (mapper_emvs_stereo.cpp:108)
    return Rt


def _build(dims, n_packets, seed, placed, fill, spread=(), tail_events=0):
    """placed: [(x, y, positions)], spread: [(x, y, n)] (n random free positions each), fill: ([(x, y)], weights) for
    every position left (a pixel of the last column votes nowhere: x + 1 < nx fails on every plane)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    Rt = _poses(n_packets, rng)
    N = n_packets * PACKET
    pixels = [(px, py) for px, py, _ in placed] + [(px, py) for px, py, _ in spread] + list(fill[0])
    label = np.full(N, -1, np.int64)
    for i, (_, _, at) in enumerate(placed):
        at = np.asarray(at, np.int64)
        assert np.unique(at).size == at.size and (label[at] < 0).all()
        label[at] = i
    free = rng.permutation(np.flatnonzero(label < 0))
    used = 0
    for i, (_, _, n) in enumerate(spread):
        label[free[used:used + n]] = len(placed) + i
        used += n
    rest = free[used:]
    base = len(placed) + len(spread)
    w = np.asarray(fill[1], np.float64)
    label[rest] = base + rng.choice(len(fill[0]), size=rest.size, p=w / w.sum())
    label = np.concatenate([label, np.full(tail_events, base, np.int64)])   # events behind the last whole packet
    px = np.array([p[0] for p in pixels], np.uint16)
    py = np.array([p[1] for p in pixels], np.uint16)
    votes = np.zeros((nz, ny, nx), np.uint32)
    per_pixel = np.bincount(label[:N], minlength=len(pixels))
    for (qx, qy), n in zip(pixels, per_pixel):
        if qx + 1 < nx and qy + 1 < ny:
            votes[:, qy:qy + 2, qx:qx + 2] += np.uint32(n)
    first = (np.arange(n_packets, dtype=np.int64) * PACKET).astype(np.uint32)
    return Case(px[label], py[label], first, Rt, _cam(nx, ny), (nz, MIN_DEPTH, MAX_DEPTH), votes)


def _far_region(nx, x0, ys, rng):
    """Background pixels >= 3 columns away from every hot pixel, with uneven shares: short runs of varied lengths."""
    pix = [(x, y) for x in range(x0, nx - 2) for y in ys]
    return pix, rng.dirichlet(np.full(len(pix), 0.7))


def rung_voxels(dims, x, y):
    """Linear indices of the 4 nz voxels of hot pixel (x, y)."""
    nx, ny, nz = dims
    z, dy, dx = np.meshgrid(np.arange(nz), np.arange(2), np.arange(2), indexing="ij")
    return (z * ny * nx + (y + dy) * nx + (x + dx)).reshape(-1).astype(np.uint32)


# ---- the ladder ------------------------------------------------------------------------------------------------------
def ladder_hot(lengths=LADDER):
    """[(x, y, votes)]: 3 columns apart, 2 from the border."""
    return [(2 + 3 * k, LADDER_Y, n) for k, n in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def ladder(seed=SEED, n_packets=LADDER_PACKETS, lengths=LADDER, tail_events=0):
    """One hot pixel per run length, its events spread uniformly over the stream; the other events on a far region."""
    nx, ny, nz = LADDER_DIMS
    hot = ladder_hot(lengths)
    assert sum(n for _, _, n in hot) <= n_packets * PACKET and (not hot or hot[-1][0] + 3 <= nx - 6)
    fill = _far_region(nx, nx - 6, range(2, ny - 2), np.random.default_rng(seed + 1000))
    return _build(LADDER_DIMS, n_packets, seed, [], fill, spread=hot, tail_events=tail_events)


@functools.lru_cache(maxsize=None)
def stream_size(n_events):
    """A ladder of the short rungs on a stream of n_events in all: whole packets only vote (mapper_emvs_stereo.cpp:88-105),
    so 1 and 1023 events vote nowhere, 1025 leaves one event behind its only packet."""
    n_packets = n_events // PACKET
    lengths = () if n_packets == 0 else SMALL_RUNGS + ((1023,) if n_packets >= 2 else ()) + ((1024,) if n_packets >= 3 else ())
    return ladder(SEED + n_events, n_packets, lengths, n_events - n_packets * PACKET)


@functools.lru_cache(maxsize=None)
def growth(seed=SEED + 5):
    """The ladder's grid with 300 packets: 16 votes per event, 4.9 M records -- more than the 2^22 a first pass has room for."""
    return ladder(seed, 300, (20000, 8193, 4097, 2049, 1025, 65))


# ---- shared columns --------------------------------------------------------------------------------------------------
SHARED_XY = (10, LADDER_Y)


@functools.lru_cache(maxsize=None)
def shared_columns(L, seed=SEED + 1):
    """Hot pixels (x, y) and (x + 1, y) with L events each, alternating: the voxels of column x + 1 collect both
    pixels' votes (2 L of them), with two different weights inside every packet."""
    nx, ny, nz = LADDER_DIMS
    N = SHARED_PACKETS * PACKET
    pair = (np.arange(L, dtype=np.int64) * (N // 2)) // L
    x, y = SHARED_XY
    fill = _far_region(nx, nx - 6, range(2, ny - 2), np.random.default_rng(seed + 1000))
    return _build(LADDER_DIMS, SHARED_PACKETS, seed + L, [(x, y, 2 * pair), (x + 1, y, 2 * pair + 1)], fill)


# ---- temporal layouts ------------------------------------------------------------------------------------------------
LAYOUT_XY = (10, LADDER_Y)


def layout_positions(layout, L, n_packets):
    N = n_packets * PACKET
    i = np.arange(L, dtype=np.int64)
    if layout == "burst":
        return 20 * PACKET + i                              # L = 1024: exactly packet 20
    if layout == "spread":
        return (i * N) // L
    h = L // 2
    if layout == "cluster+tail":
        cluster = 8 * PACKET + np.arange(h, dtype=np.int64)
        free = np.setdiff1d(np.arange(N, dtype=np.int64), cluster)
        return np.concatenate([cluster, free[(np.arange(L - h, dtype=np.int64) * free.size) // (L - h)]])
    if layout == "two clusters":
        return np.concatenate([np.arange(h, dtype=np.int64), N - (L - h) + np.arange(L - h, dtype=np.int64)])
    raise ValueError(layout)


@functools.lru_cache(maxsize=None)
def layout(name, L, seed=SEED + 2):
    nx, ny, nz = LADDER_DIMS
    n_packets = LAYOUT_PACKETS[L]
    fill = _far_region(nx, nx - 6, range(2, ny - 2), np.random.default_rng(seed + 1000))
    x, y = LAYOUT_XY
    return _build(LADDER_DIMS, n_packets, seed + L + 7 * LAYOUTS.index(name), [(x, y, layout_positions(name, L, n_packets))], fill)


@functools.lru_cache(maxsize=None)
def burst_pair(seed=SEED + 7):
    """A burst whose order shows: pixel (x, y) takes the first half of exactly one packet and (x + 1, y) the second, so
    the voxels of column x + 1 hold 1,024 votes of ONE packet (one sort bucket of 1,024 words): 512 of one weight, then
    512 of another."""
    nx, ny, nz = LADDER_DIMS
    fill = _far_region(nx, nx - 6, range(2, ny - 2), np.random.default_rng(seed + 1000))
    x, y = LAYOUT_XY
    slot = 20 * PACKET + np.arange(PACKET // 2, dtype=np.int64)
    return _build(LADDER_DIMS, LAYOUT_PACKETS[1024], seed, [(x, y, slot), (x + 1, y, slot + PACKET // 2)], fill)


# ---- partition paths -------------------------------------------------------------------------------------------------
PARTITION_HOT = ((3, 3), (7, 3), (11, 3))


@functools.lru_cache(maxsize=None)
def partition(name, seed=SEED + 3):
    """64 x 48 x 10 = 30,720 voxels = kTiePartLdsRanks (the LDS table), 64 x 48 x 11 = 33,792 (one global atomic per vote);
    the streams are sized by partition_model() below."""
    nx, ny = 64, 48
    nz = 11 if name == "global atomics" else 10
    rng = np.random.default_rng(seed + 1000)
    inside = [(x, y) for x in range(16, 60) for y in range(8, 44)]
    edge = ([(nx - 1, 5)], [1.0])                          # the last column: no vote on any plane
    if name == "lds, 1 stretch":
        # 512 packets, 60 voting events, all in packet 200
        at = 200 * PACKET + 17 * np.arange(60, dtype=np.int64)
        placed = [(20 + (i % 10), 10 + 2 * (i // 10), at[i:i + 1]) for i in range(60)]
        return _build((nx, ny, nz), 512, seed, placed, edge)
    if name == "lds, tail":
        spread = [(PARTITION_HOT[0][0], PARTITION_HOT[0][1], 2049)] + [(x, y, 1) for x, y in inside[:40]]
        return _build((nx, ny, nz), 3, seed, [], edge, spread=spread)
    n_packets = 176 if name == "lds, 256 stretches" else 24
    spread = [(PARTITION_HOT[0][0], PARTITION_HOT[0][1], 2049), (PARTITION_HOT[1][0], PARTITION_HOT[1][1], 4097),
              (PARTITION_HOT[2][0], PARTITION_HOT[2][1], 2049)]
    return _build((nx, ny, nz), n_packets, seed, [], (inside, rng.dirichlet(np.full(len(inside), 0.7))), spread=spread)


def tie_bin_tiles(nx, ny):
    """tie_bin_geom (dsi_kernels.hip): tiles of the packet's z0 locations."""
    shift = 2
    while True:
        tx = (nx + 64 + (1 << shift) - 1) >> shift
        ty = (ny + 64 + (1 << shift) - 1) >> shift
        if tx * ty <= 16384:
            return tx * ty
        shift += 1


def partition_model(case):
    """What launch_tie_hits_binned and launch_tie_partition_sums make of a call that asks EVERY voxel, restated from their rules -- control flow and sizes only, no arithmetic of the sums:
      blocks  = min(packets, 256 per_cu), per_cu = min(8, LDS / the block's LDS)        (a block takes packets k, k + blocks, ..)
      shares  = max(1, min(16, ceil(voxels / 1024), 256 per_cu / blocks))              (of the sorted voxel list)
      records = 1024 * sum over (block, share) of ceil(hits / 1024)                    (sentinel tails included)
      per     = max(8192, ceil(records / 256)),  stretches = ceil(records / per)
    -> dict(records, stretches, shares, worst_block_hits, first_pass_overflows)."""
    nx, ny, nz = case.cam[0], case.cam[1], case.shape[0]
    nsv = nx * ny * nz
    n_packets = case.first.size
    tiles = tie_bin_tiles(nx, ny)
    lds = PACKET * 12 + ((((tiles + 2) // 2) + 3) & ~3) * 4 + nz * 48 + 512 * 4
    per_cu = max(1, min(8, (160 * 1024 - 128) // lds))
    blocks = min(n_packets, 256 * per_cu)
    if blocks == 0:
        return dict(records=0, stretches=0, shares=0, worst_block_hits=0, first_pass_overflows=False)
    shares = max(1, min(16, (nsv + 1023) // 1024, (256 * per_cu) // blocks))
    v_per = (nsv + shares - 1) // shares
    N = n_packets * PACKET
    x, y = case.x[:N].astype(np.int64), case.y[:N].astype(np.int64)
    k = np.arange(N) // PACKET
    ok = (x + 1 < nx) & (y + 1 < ny)
    x, y, k = x[ok], y[ok], k[ok]
    hits = np.zeros((blocks, shares), np.int64)
    for z in range(nz):
        for dy in range(2):
            for dx in range(2):
                v = z * ny * nx + (y + dy) * nx + (x + dx)
                np.add.at(hits, (k % blocks, v // v_per), 1)
    records = int(((hits + PACKET - 1) // PACKET).sum()) * PACKET
    per = max(8192, (records + 255) // 256)
    return dict(records=records, stretches=(records + per - 1) // per, shares=shares, worst_block_hits=int(hits.max()),
                first_pass_overflows=records > (1 << 22))


# ---- 256 planes ------------------------------------------------------------------------------------------------------
PLANES256_DIMS = (16, 8, 256)
PLANES256_HOT = (3, 2, 300)


@functools.lru_cache(maxsize=None)
def planes256(seed=SEED + 4):
    """One full packet on 256 planes: 4,096 hits per plane, 1 M records from one packet."""
    nx, ny, nz = PLANES256_DIMS
    rng = np.random.default_rng(seed + 1000)
    inside = [(x, y) for x in range(7, 13) for y in range(2, 6)]
    return _build(PLANES256_DIMS, 1, seed, [], (inside, rng.dirichlet(np.full(len(inside), 0.7))), spread=[PLANES256_HOT])


@functools.lru_cache(maxsize=None)
def planes256_burst(seed=SEED + 6):
    """One full packet on ONE pixel: its 4 x 256 voxels alone, asked as a list, are one share of one workgroup, which
    would have to record 1 M votes."""
    x, y, _ = PLANES256_HOT
    return _build(PLANES256_DIMS, 1, seed, [(x, y, np.arange(PACKET))], ([(PLANES256_DIMS[0] - 1, 1)], [1.0]))


# ---- the window loop of k_tie_sort_runs<4096>, control flow only -------------------------------------------------------
def _walk_windows(positions, bits, cap):
    pos = np.sort(np.asarray(positions, np.int64))
    cnt = int(pos.size)
    assert np.unique(pos).size == cnt and (cnt == 0 or pos[-1] < (1 << bits))
    if cnt <= cap:
        return 0, 0, []
    span = bits
    while span > 0 and (cnt >> (bits - span)) > cap // 4:
        span -= 1
    lo = done = narrowed = widened = 0
    windows = []
    while lo < (1 << bits):
        hi = lo + (1 << span)
        n = int(np.searchsorted(pos, hi) - np.searchsorted(pos, lo))
        if n > cap // 2:
            span -= 1
            narrowed += 1
            continue
        if n:
            windows.append((done, done + n))
            done += n
        lo = hi
        if n < cap // 16 and span < bits and (lo & ((1 << (span + 1)) - 1)) == 0:
            span += 1
            widened += 1
    assert done == cnt
    return narrowed, widened, windows


def window_model(positions, bits, cap=4096):
    """How k_tie_sort_runs<kTieRunLds> walks a run of more than `cap` votes at the given event positions
    (bits = pos_bits): windows [lo, lo + 2^span) are narrowed while they hold more than cap / 2 votes, sorted and
    appended otherwise, and widened behind a window of fewer than cap / 16 votes where the wider window is aligned.
    -> (narrowed, widened, sorted).  Shorter runs never enter the loop: (0, 0, 0)."""
    narrowed, widened, windows = _walk_windows(positions, bits, cap)
    return narrowed, widened, len(windows)


def window_partition(positions, bits, cap=4096):
    """The windows that are sorted and appended, in the loop's order, as [begin, end) ranks of the run in event order."""
    return _walk_windows(positions, bits, cap)[2]


def hot_positions(case, x, y):
    """Event positions (packet * 1024 + slot) of pixel (x, y) in the packets of a case."""
    n = case.first.size * PACKET
    return np.flatnonzero((case.x[:n] == x) & (case.y[:n] == y))


# ---- the same packets in another order ---------------------------------------------------------------------------------
def reordered(case, which):
    """P1: packets reversed and events reversed inside packets; P2: the two halves of the stream swapped; P3: the first
    sixteenth of the packets (one at least) moved to the end.  Each packet keeps its own pose."""
    n_packets = case.first.size
    N = n_packets * PACKET
    xs, ys = case.x[:N].reshape(n_packets, PACKET), case.y[:N].reshape(n_packets, PACKET)
    if which == "P1":
        order, inner = np.arange(n_packets)[::-1], slice(None, None, -1)
    elif which == "P2":
        h = n_packets // 2
        order, inner = np.concatenate([np.arange(h, n_packets), np.arange(h)]), slice(None)
    elif which == "P3":
        s = max(1, n_packets // 16)
        order, inner = np.concatenate([np.arange(s, n_packets), np.arange(s)]), slice(None)
    else:
        raise ValueError(which)
    return case._replace(x=np.ascontiguousarray(xs[order][:, inner]).reshape(-1),
                         y=np.ascontiguousarray(ys[order][:, inner]).reshape(-1), Rt=np.ascontiguousarray(case.Rt[order]))


# ---- every case by name ----------------------------------------------------------------------------------------------
def _registry():
    reg = {"ladder": ladder, "ladder, camera 1": lambda: ladder(SEED + 9), "growth": growth, "burst pair": burst_pair,
           "256 planes": planes256, "256 planes, burst": planes256_burst}
    for L in SHARED_LENGTHS:
        reg["shared %d" % L] = functools.partial(shared_columns, L)
    for name in LAYOUTS:
        for L in LAYOUT_LENGTHS:
            reg["%s %d" % (name, L)] = functools.partial(layout, name, L)
    for n in STREAM_SIZES:
        reg["%d events" % n] = functools.partial(stream_size, n)
    for name in PARTITION_CASES:
        reg["partition: " + name] = functools.partial(partition, name)
    return reg


CASES = _registry()
LAYOUT_CASES = ["%s %d" % (name, L) for name in LAYOUTS for L in LAYOUT_LENGTHS]
SHARED_CASES = ["shared %d" % L for L in SHARED_LENGTHS]
SIZE_CASES = ["%d events" % n for n in STREAM_SIZES]


def case(name):
    return CASES[name]()
