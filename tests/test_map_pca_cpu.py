"""The world map's local shape without a GPU (include/dsi_map_pca.h; DESIGN.md 7j "Local shape"): the restatement's integer
moments (tests/map_pca_reference.py) against a brute-force all-pairs computation in Python ints, dsx_pca_solve against the
restatement bit for bit and against numpy.linalg.eigh, the host solver under the host sanitizers in a program of its own,
the argument checks and symbols of the five dsx_* entry points, and the new kernels' resources."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_knn_reference as kref
import map_layout_cases as lc
import map_pca_reference as pr
from dvs_mcemvs_amd import engine as E
from kernel_asm import _hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_map_pca", "dsx_map_pca_fetch", "dsx_pca_solve", "dsx_map_pca_select", "dsx_map_prune_pca")
INSTANCES = (0, 1, 2, 4, 8, 16)
QUANTUM = float(pr.quantum_of(pr.LEAF))
SCENE_SETTINGS = ((0, 0.15), (0, 0.05), (3, 0.1), (5, 0.15), (16, 0.1), (8, 0.05))


# ---- the integer moments against brute force ----
def moment_scenes():
    out = [("scene k=%d r=%g" % (k, r), pr.scene_reference(), k, r) for k, r in ((0, 0.15), (5, 0.1), (16, 0.05))]
    cloud = pr.reference_of(pr.cloud_calls(), pr.LEAF)
    out += [("cloud k=%d r=%g" % (k, r), cloud, k, r) for k, r in ((0, 0.15), (0, 0.1), (3, 0.15), (8, 0.12))]
    lattice = pr.reference_of(kref.lattice_calls(), kref.LEAF)
    out += [("lattice k=%d r=%g" % (k, r), lattice, k, r) for k, r in ((3, 0.05), (8, 0.15))]
    return out


@pytest.mark.parametrize("scene", moment_scenes(), ids=lambda s: s[0])
def test_moments_equal_brute_force(scene):
    """The float32 rounding of a centroid may move it across a face of its cell, out of the box around the query's index
    (the caveat of dsi_map_knn.h): on these inputs it costs no neighbour -- the box rule's members are all pairs' members,
    and the nine integers are the same."""
    name, rm, k, radius = scene
    cells = rm.extract()
    got = pr.moments(cells, rm.leaf, radius, k)
    found, rows = pr.brute_force_moments(cells, rm.leaf, radius, k)
    lost = int((found - got["found"]).sum())
    print(name, "cells", len(found), "neighbours by all pairs", int(found.sum()), "lost by the box rule", lost,
          "largest neighbourhood", int(found.max(initial=0)))
    assert lost == 0 and np.array_equal(got["found"], found)
    assert np.array_equal(np.concatenate([got["s"], got["ss"]], axis=1), rows)
    assert found.sum() >= len(found)                                            # the scene has neighbours to lose
    if k > 0:
        assert found.max() <= k


def test_the_scene_has_every_shape_and_every_count():
    rm = pr.scene_reference()
    assert 1800 <= len(rm.keys) <= 2400
    for radius, reach in zip(pr.RADII, (1, 2, 3)):
        for k in pr.KS:
            sp = pr.scene_pass(k, radius)
            assert sp["reach"] == reach and sp["n_sparse"] + sum(sp["n_label"]) == sp["n_cells"] == len(rm.keys)
            assert sp["sum_members"] == int(sp["members"].astype(np.int64).sum())
    wide = pr.scene_pass(0, 0.15)
    assert min(wide["n_label"]) >= 100 and wide["members"].max() > 17            # the radius search goes past every k
    assert pr.scene_pass(3, 0.1)["found"].max() == 3 and pr.scene_pass(5, 0.1)["found"].max() == 5     # truncated lists
    narrow = pr.scene_pass(8, 0.05)
    assert narrow["n_sparse"] >= 500 and sum(narrow["n_label"]) >= 300
    xyz = wide["xyz"].astype(np.float64)
    plane, helix, noise = (xyz[:, 0] > -1) & (xyz[:, 0] < 2), xyz[:, 0] > 2, xyz[:, 0] < -2
    lab = wide["label"]
    print("plane", np.bincount(lab[plane], minlength=4), "helix", np.bincount(lab[helix], minlength=4), "noise", np.bincount(lab[noise], minlength=4))
    assert (lab[plane] == 2).mean() > 0.8 and (lab[helix] == 1).mean() > 0.5 and (lab[noise] == 3).mean() > 0.5
    n = wide["solved"]["normal_d"][plane & (lab == 2)]
    true = np.array([-0.35, 0.2, 1.0]) / np.linalg.norm([-0.35, 0.2, 1.0])
    assert np.degrees(np.arccos(np.abs(n @ true))).max() < 10.0                  # the patch's normal, up to the jitter


# ---- dsx_pca_solve against the restatement ----
HAND = [
    ("plane", 9, [0, 0, 0], [6 << 20, 0, 0, 6 << 20, 0, 0]),
    ("tilted plane", 5, [0, 0, 0], [2000, 0, 1000, 2000, 0, 500]),              # z = x / 2: C has rank 2
    ("line", 3, [0, 0, 0], [0, 0, 0, 0, 0, 2 << 20]),
    ("diagonal line", 3, [0, 0, 0], [200, 200, 200, 200, 200, 200]),
    ("m = 1", 1, [0, 0, 0], [0, 0, 0, 0, 0, 0]),
    ("equal eigenvalues", 27, [0, 0, 0], [18 << 20, 0, 0, 18 << 20, 0, 18 << 20]),
    ("two equal", 7, [0, 0, 0], [500, 0, 0, 500, 0, 100]),
    ("off centre", 4, [30, -60, 9], [1100, -500, 40, 1900, -90, 77]),
    ("largest", 343, [342 * 3073, -342 * 3073, 0], [342 * 3073 ** 2, -342 * 3073 ** 2, 0, 342 * 3073 ** 2, 0, 342 * 3073 ** 2]),
]


def solve_rows(m, mom, orient, p):
    return [E.pca_solve(int(m[i]), mom[i, :3], mom[i, 3:], QUANTUM, orient, pr.VIEWPOINT if orient else None, p[i] if orient else None)
            for i in range(len(m))]


def assert_rows_equal(got, want, i):
    assert got["label"] == want["label"][i] and got["flags"] == want["flags"][i], i
    for f in ("normal", "tangent", "eval"):
        assert np.array_equal(pr.bits(got[f]), pr.bits(want[f][i])), (f, i)
    for f in ("normal_d", "tangent_d", "lambda"):
        assert np.array_equal(got[f].view(np.uint64), np.ascontiguousarray(want[f][i]).view(np.uint64)), (f, i)


@pytest.mark.parametrize("setting", SCENE_SETTINGS, ids=lambda s: "k=%d r=%g" % s)
def test_solve_equals_the_restatement_on_every_scene_row(built, setting):
    k, radius = setting
    for orient in (False, True):
        sp = pr.scene_pass(k, radius, 2, orient)
        sol, p = sp["solved"], sp["xyz"].astype(np.float64)
        for i, got in enumerate(solve_rows(sp["members"], sp["moments"], orient, p)):
            assert_rows_equal(got, sol, i)


def test_solve_on_hand_made_moments(built):
    m = np.array([c[1] for c in HAND])
    mom = np.array([c[2] + c[3] for c in HAND], np.int64)
    for orient in (False, True):
        p = np.tile(np.array([[0.5, 0.25, 1.0]]), (len(HAND), 1))
        want = pr.solve(m, mom[:, :3], mom[:, 3:], QUANTUM, orient, pr.VIEWPOINT, p)
        rows = solve_rows(m, mom, orient, p)
        for i, got in enumerate(rows):
            assert_rows_equal(got, want, i)
    by = {c[0]: r for c, r in zip(HAND, solve_rows(m, mom, False, None))}
    r = by["plane"]
    assert r["label"] == 2 and r["flags"] == 1 and r["normal_d"].tolist() == [0, 0, 1] and r["lambda"][0] == 0 and r["lambda"][1] == r["lambda"][2]
    r = by["tilted plane"]
    n = np.array([-0.5, 0.0, 1.0]) / np.sqrt(1.25)
    assert r["label"] == 2 and r["flags"] & 1 and np.abs(r["normal_d"] - n).max() < 1e-14 and r["lambda"][0] < 1e-9 * r["lambda"][2]
    r = by["line"]
    assert r["label"] == 1 and r["flags"] == 2 and r["tangent_d"].tolist() == [0, 0, 1] and r["lambda"][:2].tolist() == [0, 0]
    r = by["diagonal line"]
    assert r["label"] == 1 and r["flags"] & 2 and np.abs(r["tangent_d"] - 1 / np.sqrt(3)).max() < 1e-14
    r = by["m = 1"]                                                             # nothing to rotate: V = I, the first of equals
    assert r["lambda"].tolist() == [0, 0, 0] and r["flags"] == 0 and r["label"] == 1 and not np.isnan(r["eval"]).any()
    assert r["normal_d"].tolist() == [1, 0, 0] and r["tangent_d"].tolist() == [0, 1, 0]
    r = by["equal eigenvalues"]
    assert r["label"] == 3 and r["flags"] == 0 and r["normal_d"].tolist() == [1, 0, 0] and r["tangent_d"].tolist() == [0, 1, 0]
    assert len(set(r["lambda"].tolist())) == 1
    r = by["two equal"]                                                         # z is the smallest; x and y tie: x comes first
    assert r["normal_d"].tolist() == [0, 0, 1] and r["tangent_d"].tolist() == [1, 0, 0] and r["flags"] == 1 and r["label"] == 2
    # the sign: towards the viewpoint, and the canonical one when the normal is perpendicular to the view
    up = E.pca_solve(9, [0, 0, 0], HAND[0][3], QUANTUM, True, (0, 0, 5.0), (0, 0, 1.0))
    down = E.pca_solve(9, [0, 0, 0], HAND[0][3], QUANTUM, True, (0, 0, -5.0), (0, 0, 1.0))
    level = E.pca_solve(9, [0, 0, 0], HAND[0][3], QUANTUM, True, (3.0, 0, 1.0), (0, 0, 1.0))
    assert up["normal"].tolist() == [0, 0, 1] and down["normal"].tolist() == [0, 0, -1] and level["normal"].tolist() == [0, 0, 1]
    assert down["tangent"].tolist() == up["tangent"].tolist()                   # the tangent keeps the canonical sign


def test_solve_refuses_what_no_pass_returns(built):
    L = d.load_library()
    row = E._PcaRow()
    i3, i6, d3 = C.c_int64 * 3, C.c_int64 * 6, C.c_double * 3

    def call(m, s, ss, quantum=QUANTUM, orient=0, vp=None, p=None, out=row):
        return L.dsx_pca_solve(m, i3(*s) if s is not None else None, i6(*ss) if ss is not None else None, quantum, orient,
                               d3(*vp) if vp is not None else None, d3(*p) if p is not None else None, C.byref(out) if out is not None else None)
    ok = ([0, 0, 0], [100, 0, 0, 100, 0, 100])
    assert call(3, *ok) == E.OK
    assert call(3, None, ok[1]) == E.ERR_INVALID and b"null" in L.dsi_last_error()
    assert call(3, ok[0], None) == E.ERR_INVALID and call(3, *ok, out=None) == E.ERR_INVALID
    for m in (0, 344, 2 ** 32 - 1):
        assert call(m, *ok) == E.ERR_INVALID and b"m must be" in L.dsi_last_error()
    assert call(343, *ok) == E.OK
    bound = 2 * 3073
    assert call(3, [bound, 0, 0], [bound * 3073, 0, 0, 0, 0, 0]) == E.OK
    for s, ss in (([bound + 1, 0, 0], [bound * 3073, 0, 0, 0, 0, 0]), ([0, -bound - 1, 0], ok[1]), ([0, 0, 0], [bound * 3073 + 1, 0, 0, 0, 0, 0]),
                  ([0, 0, 0], [100, -bound * 3073 - 1, 0, 100, 0, 100]), ([0, 0, 0], [100, 0, 0, -1, 0, 100]),
                  ([2 ** 62, 0, 0], ok[1]), ([0, 0, 0], [0, 0, 0, 0, 0, -2 ** 63])):
        assert call(3, s, ss) == E.ERR_INVALID and b"moments beyond" in L.dsi_last_error(), (s, ss)
    assert call(1, [0, 0, 0], [1, 0, 0, 0, 0, 0]) == E.ERR_INVALID               # m = 1 has no neighbour to sum
    assert call(3, [20, 0, 0], [100, 0, 0, 100, 0, 100]) == E.ERR_INVALID and b"m * ss < s^2" in L.dsi_last_error()   # 300 < 400
    for q in (0.0, -1.0, float("nan"), float("inf")):
        assert call(3, *ok, quantum=q) == E.ERR_INVALID and b"quantum" in L.dsi_last_error()
    assert call(3, *ok, orient=2) == E.ERR_INVALID and b"orient" in L.dsi_last_error()
    assert call(3, *ok, orient=1) == E.ERR_INVALID and b"orient needs" in L.dsi_last_error()
    assert call(3, *ok, orient=1, vp=(0, 0, float("nan")), p=(0, 0, 0)) == E.ERR_INVALID and b"finite" in L.dsi_last_error()
    assert call(3, *ok, orient=1, vp=(0, 0, 1), p=(float("inf"), 0, 0)) == E.ERR_INVALID
    assert call(3, *ok, orient=1, vp=(0, 0, 1), p=(0, 0, 0)) == E.OK


def angle_between(a, b):
    """the angle between two lines in radians, by atan2: exact enough near 0, where acos is not"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(axis=-1)))


def test_solve_against_numpy_eigh(built):
    """Where lambda1 - lambda0 >= lambda2 / 8 the normal lies within 1e-9 rad of numpy.linalg.eigh's eigenvector of C (float64),
    and the tangent likewise where lambda2 - lambda1 >= lambda2 / 8: both solvers are backward stable to about 1e-15 at that
    gap, so 1e-9 leaves five orders of magnitude and still catches a wrong column, a missing sweep or a transposed update.
    Of the solved scene rows of all settings together at least half meet each gap condition: the test does not pass on
    nothing.  (At reach 1 most neighbourhoods are two or three cells on a line, which have no normal.)"""
    total = met_normal = met_tangent = 0
    for k, radius in SCENE_SETTINGS:
        sp = pr.scene_pass(k, radius)
        rows = np.flatnonzero(~sp["sparse"])
        got = solve_rows(sp["members"][rows], sp["moments"][rows], False, None)
        Cm = pr.solve(sp["members"][rows], sp["moments"][rows, :3], sp["moments"][rows, 3:], QUANTUM)["C"].astype(np.float64)
        M = np.empty((len(rows), 3, 3))
        for i, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            M[:, a, b] = M[:, b, a] = Cm[:, i]
        w, v = np.linalg.eigh(M)                                                # ascending
        lam = np.array([g["lambda"] for g in got])
        assert np.abs(lam - np.maximum(w, 0.0)).max() <= 1e-12 * w[:, 2].max()
        normal_ok, tangent_ok = w[:, 1] - w[:, 0] >= w[:, 2] / 8.0, w[:, 2] - w[:, 1] >= w[:, 2] / 8.0
        an = angle_between(np.array([g["normal_d"] for g in got]), v[:, :, 0])
        at = angle_between(np.array([g["tangent_d"] for g in got]), v[:, :, 2])
        print("k=%d r=%g: %d rows, normal gap met by %d (worst %.3g rad), tangent gap met by %d (worst %.3g rad)" %
              (k, radius, len(rows), normal_ok.sum(), an[normal_ok].max(initial=0), tangent_ok.sum(), at[tangent_ok].max(initial=0)))
        assert an[normal_ok].max(initial=0) <= 1e-9 and at[tangent_ok].max(initial=0) <= 1e-9
        unit = np.array([np.linalg.norm(g["normal_d"]) for g in got] + [np.linalg.norm(g["tangent_d"]) for g in got])
        assert np.abs(unit - 1.0).max() < 4e-15 and len(rows) >= 500
        total, met_normal, met_tangent = total + len(rows), met_normal + int(normal_ok.sum()), met_tangent + int(tangent_ok.sum())
    assert 2 * met_normal >= total and 2 * met_tangent >= total, (total, met_normal, met_tangent)


# ---- the host solver under the host sanitizers ----
def test_host_solver_under_the_sanitizers(tmp_path):
    """tests/cpp/pca_solve_sanitize.cpp: dsi_pca_host.hpp alone, host code only, in a program of its own built with
    -fsanitize=address,undefined (any finding aborts it) -- scene rows, the hand-made moments, the largest ones and the
    refusals, compared with the restatement bit for bit.  Nothing is loaded into Python."""
    exe = str(tmp_path / "pca_solve_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "pca_solve_sanitize.cpp"), "-o", exe])
    sp = pr.scene_pass(0, 0.15, 2, True)
    pick = np.arange(0, len(sp["keys"]), 7)
    m = np.concatenate([sp["members"][pick].astype(np.int64), [c[1] for c in HAND]])
    mom = np.concatenate([sp["moments"][pick], np.array([c[2] + c[3] for c in HAND], np.int64)])
    p = np.concatenate([sp["xyz"][pick].astype(np.float64), np.tile([[0.5, 0.25, 1.0]], (len(HAND), 1))])
    bad = [(0, [0] * 9, 1), (344, [0] * 9, 1), (3, [2 * 3073 + 1] + [0] * 8, 2), (3, [0, 0, 0, -1, 0, 0, 0, 0, 0], 2),
           (3, [20, 0, 0, 100, 0, 0, 100, 0, 100], 3), (2, [-2 ** 63] + [0] * 8, 2), (2, [0, 0, 0, 2 ** 63 - 1, 0, 0, 0, 0, 0], 2)]
    hexes = lambda v: " ".join(float(x).hex() for x in v)
    lines = ["%d %s %s 1 %s %s" % (m[i], " ".join(str(int(x)) for x in mom[i]), QUANTUM.hex(), hexes(pr.VIEWPOINT), hexes(p[i])) for i in range(len(m))]
    lines += ["%d %s %s 0 0x0p+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0" % (mm, " ".join(str(x) for x in row), QUANTUM.hex()) for mm, row, _ in bad]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = r.stdout.strip().split("\n")
    assert len(out) == len(lines)
    want = pr.solve(m, mom[:, :3], mom[:, 3:], QUANTUM, True, pr.VIEWPOINT, p)
    for i in range(len(m)):
        f = out[i].split()
        vals = np.array([float.fromhex(x) for x in f[3:]])
        assert [int(x) for x in f[:3]] == [0, want["label"][i], want["flags"][i]], (i, out[i])
        assert np.array_equal(vals[:9].view(np.uint64), np.concatenate([want["normal_d"][i], want["tangent_d"][i], want["lambda"][i]]).view(np.uint64)), i
        assert np.array_equal(pr.bits(vals[9:]), np.concatenate([pr.bits(want["normal"][i]), pr.bits(want["tangent"][i]), pr.bits(want["eval"][i])])), i
    for (_, _, code), row in zip(bad, out[len(m):]):
        assert int(row.split()[0]) == code, row


# ---- argument checks with a handle that is never dereferenced ----
def test_abi_argument_checks_need_no_gpu(built):
    """Every bound of "the rule" that needs no map.  reach = ceil(radius / leaf) needs the map's leaf: a reach of 4 is refused
    in test_gpu_map_pca.py, with a map at hand."""
    L = d.load_library()
    INV = E.ERR_INVALID
    fake = C.c_void_p(0x1000)                                                   # never dereferenced: the checks come first
    info, sinfo = E._MapPcaInfo(), E._MapPcaSelectInfo()

    def opts(k=8, min_found=2, radius=0.1, orient=0, keep_moments=0, viewpoint=(0.0, 0.0, 0.0), min_points=1, min_windows=1):
        return E._MapPcaOpts(min_points, min_windows, k, min_found, radius, orient, keep_moments, (C.c_double * 3)(*viewpoint))
    bad = [(dict(k=-1), b"k must be"), (dict(k=17), b"k must be"), (dict(k=4, min_found=5), b"min_found"), (dict(k=4, min_found=1), b"min_found"),
           (dict(k=1, min_found=3), b"min_found"), (dict(k=0, min_found=343), b"min_found"), (dict(k=0, min_found=1), b"min_found"),
           (dict(radius=0.0), b"radius"), (dict(radius=-0.1), b"radius"), (dict(radius=float("nan")), b"radius"),
           (dict(radius=float("inf")), b"radius"), (dict(orient=2), b"orient"), (dict(orient=-1), b"orient"), (dict(keep_moments=2), b"keep_moments"),
           (dict(viewpoint=(0.0, float("nan"), 0.0)), b"viewpoint"), (dict(orient=1, viewpoint=(float("inf"), 0.0, 0.0)), b"viewpoint")]
    assert L.dsx_map_pca(fake, None, C.byref(info)) == INV and b"opts is null" in L.dsi_last_error()
    assert L.dsx_map_pca(None, None, None) == INV and b"opts is null" in L.dsi_last_error()
    for kw, word in bad:
        o = opts(**kw)
        for handle in (None, fake):
            assert L.dsx_map_pca(handle, C.byref(o), C.byref(info)) == INV, kw
            assert word in L.dsi_last_error(), (kw, L.dsi_last_error())
    for o in (opts(0, 342, 1e-300, min_points=0, min_windows=0), opts(16, 16, 1e300, 1, 1, (1e300, -1e300, 0.0), 2 ** 32 - 1, 2 ** 32 - 1),
              opts(1, 2), opts(2, 2), opts(0, 2)):                              # legal so far
        assert L.dsx_map_pca(None, C.byref(o), None) == INV and b"map is null" in L.dsi_last_error()
    for fn in (L.dsx_map_pca_select, L.dsx_map_prune_pca):
        assert fn(fake, None, C.byref(sinfo)) == INV and b"sel is null" in L.dsi_last_error()
        assert fn(None, None, None) == INV and b"sel is null" in L.dsi_last_error()
        for sel, word in ((E._MapPcaSelection(0, 1, 0), b"keep_labels"), (E._MapPcaSelection(8, 1, 0), b"keep_labels"),
                          (E._MapPcaSelection(3, 2, 0), b"remove_sparse"), (E._MapPcaSelection(3, -1, 0), b"remove_sparse"),
                          (E._MapPcaSelection(3, 1, 2), b"shrink"), (E._MapPcaSelection(3, 1, -1), b"shrink")):
            for handle in (None, fake):
                assert fn(handle, C.byref(sel), C.byref(sinfo)) == INV and word in L.dsi_last_error(), L.dsi_last_error()
        for sel in (E._MapPcaSelection(1, 0, 0), E._MapPcaSelection(7, 1, 1)):
            assert fn(None, C.byref(sel), None) == INV and b"map is null" in L.dsi_last_error()
    n = C.c_size_t()
    none = (None,) * 9
    assert L.dsx_map_pca_fetch(None, *none, 0, C.byref(n)) == INV and b"null" in L.dsi_last_error()
    assert L.dsx_map_pca_fetch(fake, *none, 0, None) == INV and b"null" in L.dsi_last_error()
    assert L.dsi_abi_version() == 10
    with pytest.raises(ValueError):
        E.shape_mask(("flat",))
    assert [E.shape_mask(k) for k in (("linear",), "planar", ("scattered", "linear"), 7, ())] == [1, 2, 5, 7, 0]


# ---- symbols ----
def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    core = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", core))) == 176 and "dsx_" not in core
    header = open(os.path.join(ROOT, "include", "dsi_map_pca.h")).read()
    assert sorted(re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header)) == sorted(NEW)
    for other in ("dsi_map_eval.h", "dsi_map_prune.h", "dsi_map_merge.h", "dsi_map_align.h", "dsi_map_components.h", "dsi_map_knn.h"):
        assert "pca" not in open(os.path.join(ROOT, "include", other)).read()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name                      # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "dsi_map_pca.h" in readme and all(name in readme for name in NEW)
    assert "dsi_map_pca.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Local shape" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("pca", "fetchPca", "selectShapes", "pruneShapes"):
        assert hasattr(d.WorldMap, name), name
    assert callable(E.pca_solve)
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for name in ("MapPcaOptions", "MapPcaSelection", "MapPcaInfo pca(", "MapShapes fetchPca(", "pruneShapes(", "pca_solve(", "dsi_map_pca.h"):
        assert name in hpp, name
    host = open(os.path.join(ROOT, "dvs_mcemvs_amd", "csrc", "dsi_pca_host.hpp")).read()
    assert not any(word in host for word in ("#include <hip", "__device__", "__global__", "hipLaunch", "threadIdx"))   # plain C++
    from dvs_mcemvs_amd import build, io as dio, process as proc
    assert inspect.signature(proc.full_sequence).parameters["world_map_shapes"].default is None
    assert any(h.endswith("dsi_map_pca.h") for h in build.HEADERS) and "dsi_pca_host.hpp" in build.HEADERS
    assert callable(dio.save_pcd_normals_ascii) and callable(dio.load_pcd_normals_ascii) and callable(dio.save_pcd_ascii)
    assert os.path.exists(os.path.join(ROOT, "tools", "map_pca_bench.py"))


def test_struct_sizes_equal_the_headers(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dsi_map_pca.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(dsx_map_pca_opts_t), sizeof(dsx_map_pca_info_t), sizeof(dsx_pca_row_t), sizeof(dsx_map_pca_selection_t), "
                   "sizeof(dsx_map_pca_select_info_t), offsetof(dsx_map_pca_opts_t, viewpoint), offsetof(dsx_pca_row_t, label), "
                   "offsetof(dsx_map_pca_info_t, reach)); return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert sizes == [C.sizeof(E._MapPcaOpts), C.sizeof(E._MapPcaInfo), C.sizeof(E._PcaRow), C.sizeof(E._MapPcaSelection),
                     C.sizeof(E._MapPcaSelectInfo), E._MapPcaOpts.viewpoint.offset, E._PcaRow.label.offset, E._MapPcaInfo.reach.offset]


def test_process_refuses_bad_shape_options():
    from dvs_mcemvs_amd import process as proc
    for kw, word in ((dict(world_map_shapes={"k": 4, "radius": 0.1}), "needs world_map"),
                     (dict(world_map=object(), world_map_shapes={"k": 4, "radius": 0.1, "every": 0}), "every"),
                     (dict(world_map=object(), world_map_shapes={"k": 4, "radius": 0.1, "every": 1.5}), "every"),
                     (dict(world_map=object(), world_map_shapes={"k": 4, "radius": 0.1, "std_mult": 1}), "unknown keys"),
                     (dict(world_map=object(), world_map_shapes={"k": 4, "radius": 0.1, "keep": ()}), "at least one"),
                     (dict(world_map=object(), world_map_shapes={"k": 4, "radius": 0.1, "keep": ("flat",)}), "unknown shape"),
                     (dict(world_map=object(), world_map_shapes={"radius": 0.1}), "needs k and radius")):
        with pytest.raises(ValueError, match=word):
            next(proc.full_sequence(None, None, None, None, None, 0.0, 1.0, 0.1, 1, **kw))


def test_pcd_with_normals_round_trips_without_a_gpu(tmp_path):
    from dvs_mcemvs_amd import io as dio
    sp = pr.scene_pass(0, 0.15, 2, True)
    cur = dio.pcd_curvature(sp["eval"])
    e = sp["eval"].astype(np.float64)
    assert np.array_equal(cur, e[:, 0] / ((e[:, 0] + e[:, 1]) + e[:, 2])) and sp["n_sparse"] == 0
    assert np.isnan(dio.pcd_curvature([[np.inf] * 3, [0, 0, 0]])).all()
    path = str(tmp_path / "n.pcd")
    assert dio.save_pcd_normals_ascii(path, sp["xyz"], sp["normal"], cur) == len(cur)
    back = dio.load_pcd_normals_ascii(path)
    assert np.array_equal(pr.bits(back["points"]), pr.bits(sp["xyz"])) and np.array_equal(pr.bits(back["normals"]), pr.bits(sp["normal"]))
    assert np.array_equal(back["curvature"], cur.astype(np.float32))
    plain = str(tmp_path / "p.pcd")
    dio.save_pcd_ascii(plain, np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        dio.load_pcd_normals_ascii(plain)
    with pytest.raises(ValueError):
        dio.save_pcd_normals_ascii(path, sp["xyz"], sp["normal"][:-1], cur)


# ---- the new kernels' resources, from the compiler's remarks ----
@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_new_kernels_use_no_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage for every k_map_pca* instantiation: no scratch and no spilled register -- the
    Jacobi state and the running top-k stay in registers for every K -- and the table that DESIGN.md quotes."""
    p = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-x", "hip", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "dvs_mcemvs_amd", "csrc", "dsi_kernels.hip"), "-o", str(tmp_path / "k.s")],
                       stderr=subprocess.PIPE, text=True, check=True)
    seen = {}
    for block in p.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        m = re.search(r"\d+(k_map_pca(?:_[a-z]+)?)(?:ILi(\d+)EEE|E)", name)
        if not m:
            continue
        val = lambda key: int(re.search(re.escape(key) + r"[^:]*: (\d+)", block).group(1))
        short = m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")
        seen[short] = (val("VGPRs"), val("TotalSGPRs"), val("Occupancy"), val("LDS Size"))
        assert val("ScratchSize") == 0 and val("VGPRs Spill") == 0, (short, block)
    print(seen)
    asm = open(str(tmp_path / "k.s")).read()
    meta = re.findall(r"\.name:\s+(\S*k_map_pca\S*)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", asm)
    assert len(meta) == len(INSTANCES) + 2, meta                                # the code objects' own metadata says the same
    for name, fixed, spill in meta:
        assert int(fixed) == 0 and int(spill) == 0, name
    want = {"k_map_pca_select", "k_map_pca_gather"} | {"k_map_pca<%d>" % K for K in INSTANCES}
    assert set(seen) == want, seen
    assert all(v[2] >= 2 and v[3] <= 64 for v in seen.values()), seen        # at least two waves per SIMD; a few counters in LDS
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for short, v in seen.items():                                               # DESIGN.md's table is this build's
        assert "| `%s` | %d | %d | %d |" % (short, v[0], v[1], v[2]) in design, (short, v)


# ---- the layout cases ----
def test_layout_cases_reach_the_second_round_and_the_tables_end():
    """What test_gpu_map_pca.py's layout tests rely on: the dense table never grows from 2^19 slots, so queries with a home in
    the second round exist and are solved there with every label; the chain's cells sit in a run across the table's end and
    the pass looks up present and absent keys."""
    rm = lc.dense_reference()
    assert lc.grown_from(lc.dense_calls(), lc.LEAF, lc.BIG_LOG2) == 1 << lc.BIG_LOG2 and len(rm.keys) > lc.ROUND
    sp = pr.dense_pass()
    first, second = lc.halves(sp["keys"])
    assert sp["reach"] == 1 and first.sum() >= 100_000 and second.sum() >= 100_000
    for half in (first, second):
        assert np.bincount(sp["label"][half], minlength=4).min() >= 10_000      # sparse, linear, planar and scattered cells in both rounds
        assert (sp["flags"][half] == 3).sum() >= 50_000
    assert sp["n_sparse"] + sum(sp["n_label"]) == len(rm.keys)
    for name in lc.CHAINS:
        ch = lc.chain(name)
        occ, run = lc.chain_run(name)
        assert run is not None and run[1] >= len(ch["cells"])
        crm = pr.reference_of([ch["first"], ch["again"]], lc.CHAIN_LEAF)
        for k in (0, 4):
            csp = pr.shape_pass(crm, k, lc.CHAIN_RADIUS)
            assert csp["reach"] == 2 and (csp["found"] > 0).sum() >= 30 and csp["n_sparse"] >= 100
    small = pr.shape_pass(pr.reference_of([lc.chain("2^8")["first"], lc.chain("2^8")["again"]], lc.CHAIN_LEAF), 4, lc.CHAIN_RADIUS)
    assert sum(small["n_label"]) >= 20                                          # the small chain's cells are solved too
