"""The world map's arithmetic without a GPU: the numpy restatement (tests/world_map_reference.py) against an independent
formulation in exact rationals, the centroid's error bound, the boundary cases, invert_pose and the argument checks of
the dsi_map_* entries (include/dsi_engine.h "the world map")."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import dvs_mcemvs_amd as d
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def random_pose(rng, scale=3.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return E.pose_matrix(np.concatenate([rng.uniform(-scale, scale, 3), q]))


def rn(fr):
    """a rational rounded to the nearest double, ties to even (what float(Fraction) does)"""
    return float(fr)


def fraction_map(calls, leaf):
    """The issue's arithmetic with every operation computed exactly in rationals and then rounded to double once --
    no numpy arithmetic, no floor of a double: cells as Python integers, sums as Python integers."""
    cells = {}
    rejected = 0
    L = Fraction(leaf)
    for serial, (xyz, T) in enumerate(calls):
        T = [float(v) for v in T]
        for p in np.asarray(xyz, np.float32):
            x, y, z = (Fraction(float(v)) if math.isfinite(float(v)) else None for v in p[:3])
            if x is None or y is None or z is None:
                rejected += 1
                continue
            c, F = [], []
            for a in range(3):
                r0, r1, r2, t = (Fraction(v) for v in T[4 * a:4 * a + 4])
                s = Fraction(rn(Fraction(rn(r0 * x)) + Fraction(rn(r1 * y))))
                s = Fraction(rn(s + Fraction(rn(r2 * z))))
                X = Fraction(rn(s + t))
                q = Fraction(rn(X / L))
                ci = q.numerator // q.denominator
                f = Fraction(rn(q - ci))
                c.append(ci)
                F.append((f * 2 ** 32).numerator // (f * 2 ** 32).denominator)
            if any(abs(ci) > 2 ** 20 - 2 for ci in c):
                rejected += 1
                continue
            st = cells.setdefault(tuple(c), [0, [0, 0, 0], set()])
            st[0] += 1
            for a in range(3):
                st[1][a] += F[a]
            st[2].add(serial)
    rows = []
    for c, (n, S, seen) in cells.items():
        key = sum((c[a] + 2 ** 20 - 1) << (21 * a) for a in range(3))
        m = [np.float32(rn((Fraction(c[a]) + Fraction(S[a] // n, 2 ** 32)) * L)) for a in range(3)]
        rows.append((key, n, len(seen), m))
    rows.sort(key=lambda r: r[0])
    return {"keys": np.array([r[0] for r in rows], np.uint64), "n": np.array([r[1] for r in rows], np.uint32),
            "windows": np.array([r[2] for r in rows], np.uint32),
            "xyz": np.array([r[3] for r in rows], np.float32).reshape(-1, 3)}, rejected


def test_restatement_matches_exact_rationals():
    rng = np.random.default_rng(5)
    leaf = 0.05
    calls = []
    for k in range(3):
        pts = rng.uniform(-0.4, 0.4, (130, 3)).astype(np.float32)
        pts[::17] = pts[1::17][:len(pts[::17])]               # duplicates
        calls.append((pts, random_pose(rng, 0.3)))
    calls[1][0][5] = [np.nan, 0, 0]
    calls[2][0][7] = [0, np.inf, 0]
    calls[2][0][9] = [1e6, 0, 0]                             # beyond the key's range at this leaf
    rm = ref.ReferenceMap(leaf)
    rej = sum(rm.integrate(p, T) for p, T in calls)
    want, want_rej = fraction_map(calls, leaf)
    assert rej == want_rej == 3
    got = rm.extract()
    assert len(got["keys"]) > 100 and got["n"].max() > 1 and got["windows"].max() > 1
    ref.assert_maps_equal(got, want)


def test_centroid_is_the_mean_within_the_quantum():
    """|centroid - float64 mean of the world positions| <= leaf * 2^-32 + one float32 ulp of the result.  The fractions
    are floored to 32 bits and so is their mean: together under two quanta of leaf * 2^-32, downwards; the final
    rounding adds at most half an ulp.  At this leaf a quantum (5.8e-11) is under half an ulp wherever |m| > 2^-9, so
    the bound holds with room; the double operations' own error, a few 2^-53 relative, sits far below both."""
    rng = np.random.default_rng(6)
    leaf = 0.25
    T = random_pose(rng)
    pts = rng.uniform(-2, 2, (4000, 3)).astype(np.float32)
    rm = ref.ReferenceMap(leaf)
    rm.integrate(pts, T)
    out = rm.extract()
    ok, c, _ = ref.cells(pts, T, leaf)
    assert ok.all()
    W = ref.world_positions(pts, T)
    k = ref.pack_key(c)
    assert out["n"].max() >= 3
    for i, key in enumerate(out["keys"]):
        mean = W[k == key].mean(axis=0)
        bound = leaf * 2.0 ** -32 + np.spacing(np.abs(out["xyz"][i]).astype(np.float32)).astype(np.float64)
        assert (np.abs(out["xyz"][i].astype(np.float64) - mean) <= bound).all()


def test_cell_faces_signed_zero_and_negative_cells():
    leaf = 0.125                                              # a power of two: k * leaf is exact in float32
    ks = np.array([-5, -1, 0, 1, 7, 1000], np.float64)
    pts = np.zeros((len(ks), 3), np.float32)
    pts[:, 0] = (ks * leaf).astype(np.float32)
    ok, c, F = ref.cells(pts, IDENTITY, leaf)
    assert ok.all() and np.array_equal(c[:, 0], ks.astype(np.int64)) and not F.any()
    # -0.0 is cell 0 with fraction 0, like +0.0
    ok, c, F = ref.cells(np.array([[-0.0, -0.0, 0.0]], np.float32), IDENTITY, leaf)
    assert ok.all() and not c.any() and not F.any()
    # just below a face: the cell below, fraction just under 1
    below = np.nextafter(np.float32(-0.25), np.float32(-1))
    ok, c, F = ref.cells(np.array([[below, 0, 0]], np.float32), IDENTITY, leaf)
    assert c[0, 0] == -3 and 2 ** 32 - 2 ** 12 < int(F[0, 0]) < 2 ** 32
    rm = ref.ReferenceMap(leaf)
    rm.integrate(np.array([[-0.3, -0.3, -0.3], [-0.3, -0.3, -0.3]], np.float32), IDENTITY)
    out = rm.extract()
    assert np.array_equal(ref.unpack_key(out["keys"]), [[-3, -3, -3]]) and out["n"][0] == 2
    assert np.array_equal(out["xyz"][0], np.float32([-0.3] * 3))   # 0.3f has 24 bits: the 32-bit fraction keeps them
    # the one inexact fraction: -2^-54 < q < 0 gives f = 1 and F = 2^32, the upper face of cell -1
    ok, c, F = ref.cells(np.array([[-1e-30, 0, 0]], np.float32), IDENTITY, leaf)
    assert ok.all() and c[0, 0] == -1 and int(F[0, 0]) == 2 ** 32


def test_out_of_range_rule():
    leaf = 1.0
    edge = float(2 ** 20 - 2)
    pts = np.array([[edge, 0, 0], [edge + 0.5, 0, 0], [edge + 1, 0, 0], [-edge, 0, 0], [-edge - 0.5, 0, 0],
                    [0, edge + 1, 0], [0, 0, -edge - 1], [0, -edge, edge]], np.float32)
    ok, c, _ = ref.cells(pts, IDENTITY, leaf)
    #                 c = 2^20-2  2^20-2  2^20-1  -(2^20-2)  -(2^20-1)  2^20-1   -(2^20-1)  in range
    assert ok.tolist() == [True, True, False, True, False, False, False, True]
    assert c[0, 0] == 2 ** 20 - 2 and c[3, 0] == -(2 ** 20 - 2)
    rm = ref.ReferenceMap(leaf)
    assert rm.integrate(pts, IDENTITY) == 4
    out = rm.extract()
    assert np.array_equal(ref.unpack_key(out["keys"]).max(axis=0), [2 ** 20 - 2, 0, 2 ** 20 - 2])
    assert out["keys"].min() > 0                              # 0 is the table's "empty"


def test_invert_pose_formula_and_round_trip(built):
    rng = np.random.default_rng(7)
    for _ in range(20):
        T = random_pose(rng)
        inv = d.invert_pose(T)
        assert np.array_equal(inv, ref.invert_pose(T))        # the formula, bit for bit
        back = d.invert_pose(inv)
        assert np.array_equal(back.reshape(3, 4)[:, :3], T.reshape(3, 4)[:, :3])
        assert np.abs(back - T).max() < 1e-14
    # the 7-vector form is the matrix of the same pose
    p7 = np.concatenate([[1.0, -2.0, 0.5], [np.cos(0.2), 0.0, np.sin(0.2), 0.0]])
    M = E.pose_matrix(p7).reshape(3, 4)
    assert np.allclose(M[:, :3] @ M[:, :3].T, np.eye(3), atol=1e-15) and np.array_equal(M[:, 3], p7[:3])
    assert np.allclose(M[:, :3] @ [0, 0, 1.0], [np.sin(0.4), 0, np.cos(0.4)])
    from dvs_mcemvs_amd import synthetic as syn
    q7 = syn.pose_inverse(p7)
    assert np.allclose(d.invert_pose(p7), E.pose_matrix(q7), atol=1e-15)


def test_abi_argument_checks_need_no_gpu(built):
    L = d.load_library()
    INV = E.ERR_INVALID
    vp = C.c_void_p
    out = vp()
    info = E._MapInfo()
    n = C.c_size_t()
    T = (C.c_double * 12)(*IDENTITY)
    xyz = (C.c_float * 3)()
    opts = E._PointCloudOptions(0.05, 3)
    assert L.dsi_invert_pose(None, T) == INV and L.dsi_invert_pose(T, None) == INV
    assert L.dsi_map_create(None, 0.05, 16, C.byref(out)) == INV and not out.value
    assert L.dsi_map_create(None, 0.0, 16, C.byref(out)) == INV
    assert L.dsi_map_create(None, 0.05, 7, C.byref(out)) == INV
    assert L.dsi_map_create(None, 0.05, 28, None) == INV
    assert L.dsi_map_destroy(None) == E.OK                     # like every destroy of the header
    assert L.dsi_map_reset(None) == INV
    assert L.dsi_map_integrate(None, xyz, 3, 1, T, C.byref(n)) == INV
    assert L.dsi_map_integrate_mapper(None, None, C.byref(opts), T, C.byref(n), C.byref(n)) == INV
    assert L.dsi_map_info(None, C.byref(info)) == INV
    assert L.dsi_map_count(None, 1, 1, C.byref(n)) == INV
    assert L.dsi_map_extract(None, 1, 1, None, None, None, None, 0, C.byref(n)) == INV
    assert b"null" in L.dsi_last_error()
    assert L.dsi_abi_version() == 10
