"""The exact reference of the engine's voxels (CPU only).

DESIGN.md ("GPU vs oracle") states that every voxel the exact voting paths build is
fl32(sum trunc(fl32(w) * 2^31) * 2^-31): the exact integer sum of the truncated Q.31 weights, rounded to
fp32 once.  The reference of that statement exists twice -- oracle.fill_voxel_grid_q31 / q31_to_float (C)
and independent_numpy.fill_voxel_grid_q31 / q31_to_f32 (numpy, integer rounding) -- and the GPU tests
(test_gpu_exact_voxels.py) hold the engine to it bit for bit.  Here the two references are pinned against
each other, the conversion against exact rational arithmetic, and the reference's own fp32 event-order
sums against the summation-error interval of the exact sums.
"""
from fractions import Fraction

import numpy as np

import independent_numpy as ind
from oracle import oracle as orc

WITNESS = 2 ** 53 + 2 ** 30 + 2 ** 29 - 1       # fl32(v 2^-31) = 4194304.5; rounding through double gives 4194305.0


def random_packets(rng, n_packets, nx, ny, spread=0.3, cz_spread=0.5):
    """z0 locations + camera centres as fillVoxelGrid receives them (a copy of test_gpu_parity's generator)."""
    xy = np.empty((n_packets * 1024, 2), np.float32)
    xy[:, 0] = rng.uniform(-0.1 * nx, 1.1 * nx, xy.shape[0])
    xy[:, 1] = rng.uniform(-0.1 * ny, 1.1 * ny, xy.shape[0])
    centers = rng.normal(0, spread, (n_packets, 3)).astype(np.float32)
    centers[:, 2] = rng.normal(0, cz_spread, n_packets)
    return xy, centers


def special_coordinates(nx, ny):
    """The coordinates of test_vote_edge_cases: borders, signed zero, NaN, infinities, huge values."""
    return np.array([[0.0, 0.0], [nx - 1.0, 3.0], [nx - 1.0001, 3.0], [3.0, ny - 1.0], [-0.0, 5.0], [-1e-7, 5.0],
                     [np.nan, 1.0], [1.0, np.nan], [np.inf, 2.0], [2.0, -np.inf], [1e30, 1.0], [nx - 2.0, ny - 2.0],
                     [3.4e38, 3.4e38]], np.float32)


def exact_case(rng, nx, ny, n_packets, planes):
    """Random packets with the edge cases of the voting paths mixed in: the special coordinates (in every packet),
    duplicate bursts (a packet of ONE location: multiplicity 1024; a packet of 7 locations), a dead packet, a
    one-row packet, and the special camera centres of test_vote_edge_cases (identity, a = 0, d = 0, between planes,
    far behind, NaN).  n_packets >= 8."""
    assert n_packets >= 8
    xy, centers = random_packets(rng, n_packets, max(nx, 2), max(ny, 2))
    special = special_coordinates(nx, ny)
    for k in range(n_packets):
        xy[k * 1024 + 100:k * 1024 + 100 + special.shape[0]] = special
    burst = np.array([min(1.25, nx - 1.5), min(0.5, ny - 1.5)], np.float32)
    xy[6 * 1024:7 * 1024] = np.maximum(burst, 0.25)                           # multiplicity 1024
    pool = np.stack([rng.uniform(0, nx - 1, 7), rng.uniform(0, ny - 1, 7)], axis=1).astype(np.float32)
    xy[7 * 1024:8 * 1024] = pool[rng.integers(0, 7, 1024)]
    xy[4 * 1024:5 * 1024] = np.nan                                            # a dead packet
    xy[5 * 1024:6 * 1024, 1] = np.float32(0.25 * (ny - 1))                    # one row
    nz = len(planes)
    centers[0] = (0, 0, 0)
    centers[1] = (0.2, -0.1, planes[min(2, nz - 1)])
    centers[2] = (0.1, 0.1, planes[0])
    centers[3] = (0.0, 0.0, planes[min(3, nz - 1)] + 0.01)
    centers[4] = (5.0, -7.0, 100.0)
    centers[5] = (np.nan, 0.0, 0.0)
    centers[6] = (0, 0, 0)
    centers[7] = (0.01, 0.02, -0.05)
    return xy, centers


def _case_grid(nx, ny, nz):
    planes = orc.depth_planes(1.0, 6.5, nz)
    Kv = np.array([0.8 * max(nx, 4), 0.8 * max(nx, 4), 0.5 * nx, 0.5 * ny], np.float32)
    return planes, Kv


def test_c_and_numpy_exact_references_agree_bit_for_bit():
    """oracle.fill_voxel_grid_q31 against independent_numpy.fill_voxel_grid_q31 (sums AND vote counts), and the two
    Q33.31 -> fp32 conversions against each other, on random packets, the special coordinates and centres, duplicate
    bursts, odd widths, one plane and 2 x 2 grids."""
    rng = np.random.default_rng(2024)
    for nx, ny, nz, npk in ((96, 72, 12, 9), (131, 97, 7, 8), (41, 30, 6, 10), (2, 2, 1, 8), (9, 2, 3, 8), (40, 30, 1, 12)):
        planes, Kv = _case_grid(nx, ny, nz)
        xy, centers = exact_case(rng, nx, ny, npk, planes)
        acc_c, cnt_c = orc.fill_voxel_grid_q31(xy, centers, planes, Kv, nx, ny)
        acc_n, cnt_n = ind.fill_voxel_grid_q31(xy, centers, planes, Kv, nx, ny)
        assert np.array_equal(acc_c, acc_n), (nx, ny, nz)
        assert np.array_equal(cnt_c, cnt_n), (nx, ny, nz)
        assert cnt_c.sum() > 0 and acc_c.max() >= 1024 * 2 ** 29      # the burst: 1024 votes of weight >= 1/4
        f_c = orc.q31_to_float(acc_c)
        assert np.array_equal(f_c.view(np.uint32), ind.q31_volume_to_f32(acc_c).view(np.uint32))
        # the exact reference votes where the fp32 reference does: a positive truncated weight is a positive weight
        ref = orc.fill_voxel_grid(xy, centers, planes, Kv, nx, ny)
        assert np.all((acc_c == 0) | (ref > 0)) and np.all((cnt_c > 0) | (ref == 0))
    # accumulation: the q31 grids are added into, like fill_voxel_grid's
    acc2, cnt2 = orc.fill_voxel_grid_q31(xy, centers, planes, Kv, nx, ny, acc_c.copy(), cnt_c.copy())
    assert np.array_equal(acc2, 2 * acc_c) and np.array_equal(cnt2, 2 * cnt_c)


def _check_rounding(v, r):
    """r (fp32) is v * 2^-31 rounded to nearest, ties to even -- decided in exact rational arithmetic."""
    ex = Fraction(v, 2 ** 31)
    r = np.float32(r)
    d = abs(Fraction(float(r)) - ex)
    for nb in (np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))):
        dn = abs(Fraction(float(nb)) - ex)
        assert d <= dn, (v, float(r), float(nb))
        if d == dn:
            assert int(r.view(np.uint32)) & 1 == 0, ("tie not to even", v, float(r))


def test_q31_conversion_known_answers():
    cases = {2 ** 52 - 1: None, 2 ** 52: 2097152.0, 2 ** 53 - 1: 4194304.0, 2 ** 53: 4194304.0, WITNESS: 4194304.5,
             2 ** 63 + 1: 4294967296.0, 0: 0.0, 1: 2.0 ** -31, 2 ** 31: 1.0, 2 ** 64 - 1: 8589934592.0}
    for v, want in cases.items():
        got_c = orc.lib().orc_q31_to_float(v)
        got_n = ind.q31_to_f32(v)
        assert np.float32(got_c).view(np.uint32) == got_n.view(np.uint32), v
        _check_rounding(v, got_n)
        if want is not None:
            assert float(got_n) == want, (v, float(got_n), want)
    # the conversion the issue was about: through a double, the witness is rounded twice
    assert float(np.float32(np.float64(WITNESS) * 2.0 ** -31)) == 4194305.0
    # exact in both references below 2^52 (one rounding of an exact double): spot check against the plain formula
    rng = np.random.default_rng(5)
    small = rng.integers(0, 2 ** 52, 2000, dtype=np.uint64)
    assert np.array_equal(orc.q31_to_float(small), (small.astype(np.float64) * 2.0 ** -31).astype(np.float32))


def test_q31_conversion_every_binade():
    """Random v in every binade 2^40 .. 2^63 (and values next to fp32 rounding ties), both references against exact
    rational rounding."""
    rng = np.random.default_rng(77)
    vals = []
    for e in range(40, 64):
        lo = 2 ** e
        vals += [lo + int(rng.integers(0, 2 ** 62)) % lo for _ in range(40)]
        # ties of the fp32 rounding: 24 significant bits + exactly half an ulp, and one either side
        half = 1 << (e - 24)
        base = lo + (int(rng.integers(0, 2 ** 23)) << (e - 23))
        vals += [base + half - 1, base + half, base + half + 1, base + 3 * half]
    arr = np.array(vals, np.uint64)
    got_c = orc.q31_to_float(arr)
    for v, r in zip(vals, got_c):
        assert r.view(np.uint32) == ind.q31_to_f32(v).view(np.uint32), v
        _check_rounding(v, r)


def test_fp32_oracle_lies_in_the_summation_interval_of_the_exact_sums():
    """The relation between the two references the GPU tests rely on: the reference's fp32 event-order value R of a
    voxel with n votes lies in [max(0, E(1 - 2u) - n 2^-31)(1 - g), (E(1 + 2u) + n 2^-31)(1 + g)], E = fl32 of the
    exact Q33.31 sum, g = (n - 1)u / (1 - (n - 1)u), u = 2^-24 (the interval of test_the_proofs_interval_holds_the_
    reference_order_value): the truncation of a weight to the 2^-31 grid is one-sided, below 2^-31 per vote."""
    rng = np.random.default_rng(99)
    nx, ny, nz = 64, 48, 10
    planes, Kv = _case_grid(nx, ny, nz)
    xy, centers = exact_case(rng, nx, ny, 40, planes)
    pool = xy[rng.integers(0, xy.shape[0], 300)]
    xy[8 * 1024:20 * 1024] = pool[rng.integers(0, 300, 12 * 1024)]        # heavy voxels
    acc, n = orc.fill_voxel_grid_q31(xy, centers, planes, Kv, nx, ny)
    E = orc.q31_to_float(acc).astype(np.float64)
    R = orc.fill_voxel_grid(xy, centers, planes, Kv, nx, ny).astype(np.float64)
    n = n.astype(np.float64)
    u, q = 2.0 ** -24, n * 2.0 ** -31
    g = np.where(n > 0, (n - 1) * u / (1 - (n - 1) * u), 0.0)
    hi = (E * (1 + 2 * u) + q) * (1 + g)
    lo = np.maximum(0.0, E * (1 - 2 * u) - q) * (1 - g)
    assert np.all(R <= hi) and np.all(R >= lo), "%d voxels outside" % int(((R > hi) | (R < lo)).sum())
    assert np.all((n > 0) | ((E == 0) & (R == 0)))
    assert n.max() > 1000
    # the truncation is one-sided: the exact sum of the truncated weights never exceeds the real sum of the weights,
    # which the fp32 order value approximates to g -- E is never above R by more than the roundings
    assert np.all(E * (1 - 2 * u) <= R * (1 + g) + 1e-300)
