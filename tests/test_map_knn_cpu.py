"""The world map's k nearest cells and statistical outliers without a GPU (include/dsi_map_knn.h; DESIGN.md 7j "Neighbours
and statistical outliers"): the restatement's box rule (tests/map_knn_reference.py) against a brute-force all-pairs k-NN and
scipy's cKDTree on every scene the GPU tests use, the conditions those scenes must meet, dsx_map_knn_threshold against exact
Python arithmetic, the argument checks and symbols of the six dsx_* entry points, and the new kernels' resources."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
from scipy.spatial import cKDTree

import dvs_mcemvs_amd as d
import map_knn_reference as kref
import map_layout_cases as lc
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E
from kernel_asm import _hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_map_knn_points", "dsx_map_knn", "dsx_map_knn_threshold", "dsx_map_knn_select", "dsx_map_knn_fetch", "dsx_map_prune_knn")
INSTANCES = (1, 2, 4, 8, 16)


# ---- the box rule against brute force and cKDTree, on the scenes of the GPU tests ----
def scenes():
    """(name, restatement map, query points float32 or None, k, radius)"""
    lattice = kref.reference_of(kref.lattice_calls(), kref.LEAF)
    out = [("lattice r=%g k=%d" % (r, k), lattice, kref.lattice_queries(), k, r) for r in kref.LATTICE_RADII for k in (3, 16)]
    out.append(("sparse", kref.reference_of(kref.sparse_calls(), kref.LEAF), kref.sparse_queries(), kref.SPARSE_K, kref.SPARSE_RADIUS))
    out.append(("faces", kref.reference_of(kref.face_calls(), kref.FACE_LEAF), None, 4, kref.FACE_LEAF))
    out.append(("patch", kref.reference_of(kref.patch_calls()[0], kref.PATCH_LEAF), None, 4, kref.PATCH_RADIUS))
    out.append(("edge", kref.reference_of(kref.edge_calls(), kref.EDGE_LEAF), None, 4, 1.2))
    return out


@pytest.mark.parametrize("scene", scenes(), ids=lambda s: s[0])
def test_box_rule_equals_brute_force_and_kdtree(scene):
    """The float32 rounding of a centroid may move it across a face of its cell, out of the box around the query's index: on
    these inputs it does not cost a neighbour -- the box rule finds what all pairs find."""
    name, rm, queries, k, radius = scene
    cells = rm.extract()
    own = cells["xyz"].astype(np.float64)
    got = kref.neighbours(own, cells, rm.leaf, radius, k, exclude=cells["keys"])                # the self query's rows
    want = kref.brute_force(own, cells, radius, k, exclude=cells["keys"])
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["found"], want["found"]), name
    assert np.array_equal(got["d"].view(np.uint64), want["d"].view(np.uint64)), name
    print(name, "self: found histogram", np.bincount(got["found"], minlength=k + 1).tolist())
    if queries is None:
        return
    p = queries[:, :3].astype(np.float64)
    got = kref.neighbours(p, cells, rm.leaf, radius, k)
    want = kref.brute_force(p, cells, radius, k)
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["found"], want["found"]), name
    assert np.array_equal(got["d"].view(np.uint64), want["d"].view(np.uint64)), name
    # cKDTree sums the squares in its own order and compares against the bound in its own way: equal up to a few ulp, and a
    # neighbour within 1e-9 of the radius may fall on either side
    td, _ = cKDTree(own).query(p, k=k)
    td = td.reshape(len(p), k)
    clear = np.abs(td - radius) > 1e-9
    td = np.where(td <= radius, td, np.inf)
    same = np.isclose(got["d"], td, rtol=1e-12, atol=1e-15) | (np.isinf(got["d"]) & np.isinf(td))
    assert (same | ~clear).all(), name
    assert (got["found"] == np.isfinite(td).sum(axis=1))[clear.all(axis=1)].all(), name


def test_the_lattice_has_ties_that_the_key_decides():
    rm = kref.reference_of(kref.lattice_calls(), kref.LEAF)
    assert len(rm.keys) == 2028
    for radius, reach in zip(kref.LATTICE_RADII, (1, 2, 3)):
        sq = kref.self_query(rm, 16, radius)
        assert sq["reach"] == reach
        d2, keys = sq["rows"]["d2"], sq["rows"]["keys"]
        tie = (d2[:, 1:] == d2[:, :-1]) & np.isfinite(d2[:, 1:])
        assert (keys[:, 1:][tie] > keys[:, :-1][tie]).all()
        print("radius", radius, "tied neighbours", int(tie.sum()), "of", int(np.isfinite(d2).sum()))
        assert tie.sum() >= 2000
    pq = kref.query(rm, kref.lattice_queries(), 3, 0.05)
    cut = kref.neighbours(kref.lattice_queries()[:, :3].astype(np.float64), rm.extract(), rm.leaf, 0.05, 4)
    assert ((cut["d2"][:, 2] == cut["d2"][:, 3]) & (cut["found"] == 4)).sum() >= 50   # a tie ACROSS the cut at k = 3
    assert set(np.unique(pq["found"]).tolist()) >= {0, 3}


def test_the_sparse_scene_meets_every_count():
    rm = kref.reference_of(kref.sparse_calls(), kref.LEAF)
    sq = kref.self_query(rm, kref.SPARSE_K, kref.SPARSE_RADIUS, min_found=2)
    adm = sq["rows"]["admitted"]
    assert (adm == 0).any() and (adm < kref.SPARSE_K).sum() >= 100 and (adm == kref.SPARSE_K).any() and (adm > kref.SPARSE_K).sum() >= 20
    assert sq["n_isolated"] >= 5 and sq["n_scored"] >= 400 and sq["reach"] == 3
    two = kref.self_query(rm, kref.SPARSE_K, kref.SPARSE_RADIUS, min_windows=2)
    assert two["n_unqueried"] >= 100 and two["n_cells"] >= 100
    sel = kref.select(rm, sq, 1.0)
    assert min(sel["n_removed"][1:]) >= 5 and sel["n_kept"] >= 300


def test_a_face_cell_floors_into_its_neighbour():
    rm = kref.reference_of(kref.face_calls(), kref.FACE_LEAF)
    moved = kref.moved_cells(rm)
    print("cells whose centroid lies in another index:", int(moved.sum()), "of", len(moved))
    assert moved.sum() >= 1                                                     # (around 0, where the fraction rounds to 1)
    # such a cell finds the cell it floors into, not itself: excluded by key, offset 0 holds another cell
    sq = kref.self_query(rm, 4, kref.FACE_LEAF)
    own = np.repeat(sq["keys"][:, None], 4, axis=1)
    assert not (sq["rows"]["keys"] == own).any()
    cells = rm.extract()
    c = np.floor(cells["xyz"].astype(np.float64) / kref.FACE_LEAF).astype(np.int64)
    there = np.isin(ref.pack_key(c[moved]), rm.keys)
    assert there.any()                                                          # offset 0 of the query is an occupied OTHER cell
    naive = kref.neighbours(cells["xyz"].astype(np.float64), cells, rm.leaf, kref.FACE_LEAF, 4)   # no exclusion: differs
    assert not np.array_equal(naive["keys"], sq["rows"]["keys"])


def test_the_edge_scene_skips_offsets():
    rm = kref.reference_of(kref.edge_calls(), kref.EDGE_LEAF)
    assert len(rm.keys) == 9 and np.abs(ref.unpack_key(rm.keys)).max() == ref.CELL_MAX
    sq = kref.self_query(rm, 4, 1.2)
    assert sq["reach"] == 3 and sq["found"].tolist() == [2] * 9                 # three cells at each of three corners of the key range


def test_first_principles_patch():
    calls, n_patch = kref.patch_calls()
    rm = kref.reference_of(calls, kref.PATCH_LEAF)
    assert len(rm.keys) == n_patch + 6 + 5
    sq = kref.self_query(rm, 4, kref.PATCH_RADIUS)
    sel = kref.select(rm, sq, 1.0)
    assert sel["n_removed"] == [0, 5, 6] and sel["n_kept"] == n_patch


# ---- the threshold against exact arithmetic ----
def exact_threshold(N, sum_q, sum_q2, std_mult):
    """rationals up to the roundings the header names: the conversions to double by Fraction -> float (correctly rounded)"""
    if N == 0:
        return 0.0, 0.0, 1 << 30
    V = N * sum_q2 - sum_q * sum_q
    to_double = lambda n: float(Fraction(n))
    mu = to_double(sum_q) / to_double(N)
    sigma = math.sqrt(to_double(V) / (to_double(N) * to_double(N - 1))) if N >= 2 else 0.0
    T = mu + std_mult * sigma
    return mu, sigma, (1 << 30 if T >= 2.0 ** 30 else 0 if T < 0 else int(math.floor(T)))


def moments_of(qs):
    return len(qs), sum(qs), sum(q * q for q in qs)


THRESHOLD_CASES = [
    ("N = 0", (0, 0, 0), 1.0), ("N = 1", moments_of([7]), 2.0), ("N = 2", moments_of([3, 10]), 1.0),
    ("V = 0", moments_of([5, 5, 5]), 3.0),
    ("V above 2^64", (1 << 27, 1 << 56, 1 << 86), 0.5),                         # half the cells at 0, half at 2^30: V = 2^112
    ("V above 2^64, odd", moments_of([(i * 2654435761) % (1 << 30) for i in range(1, 2000)]), 1.5),
    ("halfway down", (2, 1, (1 << 52) + 1), 1.0),                               # V = 2^53 + 1 -> 2^53 (even)
    ("halfway up", (2, 1, (1 << 52) + 2), 1.0),                                 # V = 2^53 + 3 -> 2^53 + 4
    ("T >= 2^30", moments_of([0, 1 << 30]), 1.0), ("std_mult < 0", moments_of([0, 1 << 30]), -2.0),
    ("std_mult < 0, T > 0", moments_of([100, 200, 300, 1000]), -0.5), ("std_mult = 0", moments_of([100, 200, 301]), 0.0),
]


@pytest.mark.parametrize("case", THRESHOLD_CASES, ids=lambda c: c[0])
def test_threshold_equals_exact_arithmetic(built, case):
    name, (N, sum_q, sum_q2), std_mult = case
    got = E.knn_threshold(N, sum_q, sum_q2, std_mult)
    mu, sigma, T_q = exact_threshold(N, sum_q, sum_q2, std_mult)
    want = kref.threshold(N, sum_q, sum_q2, std_mult)
    print(name, got, "V =", want["V"])
    assert (got["mu"], got["sigma"], got["T_q"]) == (mu, sigma, T_q) == (want["mu"], want["sigma"], want["T_q"])
    V = want["V"]
    if name.startswith("V above"):
        assert V > 1 << 64
    if name == "halfway down":
        assert V == (1 << 53) + 1 and got["sigma"] == math.sqrt(2.0 ** 53 / 2.0)
    if name == "halfway up":
        assert V == (1 << 53) + 3 and got["sigma"] == math.sqrt((2.0 ** 53 + 4.0) / 2.0)
    if name == "T >= 2^30":
        assert got["T_q"] == 1 << 30 and got["mu"] + got["sigma"] > 2.0 ** 30
    if name == "std_mult < 0":
        assert got["T_q"] == 0
    if name == "V = 0":
        assert got["sigma"] == 0.0 and got["T_q"] == 5
    if name == "N = 0":
        assert got == {"mu": 0.0, "sigma": 0.0, "T_q": 1 << 30}


def test_threshold_refuses_what_no_query_returns(built):
    L = d.load_library()
    two = lambda v: (C.c_uint64 * 2)(v & (2 ** 64 - 1), v >> 64)
    mu, sigma, tq = C.c_double(), C.c_double(), C.c_uint64()
    out = (C.byref(mu), C.byref(sigma), C.byref(tq))
    assert L.dsx_map_knn_threshold(2, 3, None, 1.0, *out) == E.ERR_INVALID and b"sum_q2 is null" in L.dsi_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.dsx_map_knn_threshold(2, 3, two(5), bad, *out) == E.ERR_INVALID and b"std_mult" in L.dsi_last_error()
    assert L.dsx_map_knn_threshold(2, 4, two(1), 1.0, *out) == E.ERR_INVALID and b"sum_q^2" in L.dsi_last_error()      # V < 0
    assert L.dsx_map_knn_threshold((1 << 27) + 1, 0, two(0), 1.0, *out) == E.ERR_INVALID and b"N must be" in L.dsi_last_error()
    assert L.dsx_map_knn_threshold(2, (2 << 30) + 1, two(1 << 61), 1.0, *out) == E.ERR_INVALID and b"too large" in L.dsi_last_error()
    assert L.dsx_map_knn_threshold(2, 2, two((2 << 60) + 1), 1.0, *out) == E.ERR_INVALID and b"too large" in L.dsi_last_error()
    assert L.dsx_map_knn_threshold(2, 3, two(5), 1.0, None, None, None) == E.OK                                       # outputs may be NULL


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/knn_threshold_sanitize.cpp: the threshold and the 128-bit sum, host code only, in a program of its own built
    with -fsanitize=address,undefined (any finding aborts it) -- every case above, the refusals and the largest moments"""
    exe = str(tmp_path / "knn_threshold_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "knn_threshold_sanitize.cpp"), "-o", exe])
    top = 1 << 27
    cases = [(m, s) for _, m, s in THRESHOLD_CASES]
    cases += [((top, top << 30, top << 60), 1e308), ((top, top << 30, top << 60), -1e308), ((top, 0, top << 60), 3.0),
              ((top, 1, 1), 0.0), ((3, 6, 12), 1.0)]
    bad = [((top + 1, 0, 0), 1.0, 1), ((2, (2 << 30) + 1, 1 << 61), 1.0, 2), ((2, 2, (2 << 60) + 1), 1.0, 2), ((2, 4, 1), 1.0, 3),
           ((2 ** 64 - 1, 2 ** 64 - 1, 2 ** 128 - 1), 1.0, 1)]
    sums = [(0, 0), (2 ** 59, 2 ** 59), (2 ** 64 - 1, 2 ** 64 - 1), (2 ** 32 - 1, 1), (12345678901234567, 98765432109876543)]
    lines = ["%d %d %d %d %s" % (N, sq, s2 & (2 ** 64 - 1), s2 >> 64, float(sm).hex()) for (N, sq, s2), sm in cases]
    lines += ["%d %d %d %d %s" % (N, sq, s2 & (2 ** 64 - 1), s2 >> 64, float(sm).hex()) for (N, sq, s2), sm, _ in bad]
    lines += ["S %d %d" % lo_hi for lo_hi in sums]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = r.stdout.split("\n")
    for ((N, sq, s2), sm), row in zip(cases, out):
        e, mu, sigma, tq = row.split()
        want = kref.threshold(N, sq, s2, sm)
        assert (int(e), float.fromhex(mu), float.fromhex(sigma), int(tq)) == (0, want["mu"], want["sigma"], want["T_q"]), (N, sq, s2, sm, row)
    for (_, _, code), row in zip(bad, out[len(cases):]):
        assert int(row.split()[0]) == code, row
    for (lo, hi), row in zip(sums, out[len(cases) + len(bad):]):
        total = lo + (hi << 32)
        assert [int(v) for v in row.split()] == [total & (2 ** 64 - 1), total >> 64]


# ---- argument checks with a handle that is never dereferenced ----
def test_abi_argument_checks_need_no_gpu(built):
    """Every bound of "the rule" that needs no map.  reach = ceil(radius / leaf) needs the map's leaf: a reach of 4 is refused
    in test_gpu_map_knn.py, with a map at hand."""
    L = d.load_library()
    INV = E.ERR_INVALID
    fake = C.c_void_p(0x1000)                                                   # never dereferenced: the checks come first
    info, sinfo = E._MapKnnInfo(), E._MapKnnSelectInfo()
    pts = np.zeros((2, 3), np.float32)
    pp = pts.ctypes.data_as(C.POINTER(C.c_float))
    calls = (lambda h, o: L.dsx_map_knn(h, o, C.byref(info)), lambda h, o: L.dsx_map_knn_points(h, pp, 3, 2, o, None, None, None))
    bad = [(dict(k=0), b"k must be"), (dict(k=17), b"k must be"), (dict(k=-1), b"k must be"), (dict(k=4, min_found=5), b"min_found"),
           (dict(k=4, min_found=0), b"min_found"), (dict(radius=0.0), b"radius"), (dict(radius=-0.1), b"radius"),
           (dict(radius=float("nan")), b"radius"), (dict(radius=float("inf")), b"radius")]
    for call in calls:
        assert call(fake, None) == INV and b"opts is null" in L.dsi_last_error()
        assert call(None, None) == INV and b"opts is null" in L.dsi_last_error()
        for kw, word in bad:
            o = E._MapKnnOpts(1, 1, kw.get("k", 8), kw.get("min_found", 1), kw.get("radius", 0.1))
            for handle in (None, fake):
                assert call(handle, C.byref(o)) == INV, kw
                assert word in L.dsi_last_error(), (kw, L.dsi_last_error())
        for o in (E._MapKnnOpts(0, 0, 1, 1, 1e-300), E._MapKnnOpts(2 ** 32 - 1, 2 ** 32 - 1, 16, 16, 1e300)):   # legal so far
            assert call(None, C.byref(o)) == INV and b"map is null" in L.dsi_last_error()
    for fn in (L.dsx_map_knn_select, L.dsx_map_prune_knn):
        assert fn(fake, None, C.byref(sinfo)) == INV and b"sel is null" in L.dsi_last_error()
        assert fn(None, None, None) == INV and b"sel is null" in L.dsi_last_error()
        for sel, word in ((E._MapKnnSelection(float("nan"), 0), b"std_mult"), (E._MapKnnSelection(float("inf"), 0), b"std_mult"),
                          (E._MapKnnSelection(1.0, 2), b"shrink"), (E._MapKnnSelection(1.0, -1), b"shrink")):
            for handle in (None, fake):
                assert fn(handle, C.byref(sel), C.byref(sinfo)) == INV and word in L.dsi_last_error(), L.dsi_last_error()
        for sel in (E._MapKnnSelection(-1.0, 0), E._MapKnnSelection(1e300, 1)):
            assert fn(None, C.byref(sel), None) == INV and b"map is null" in L.dsi_last_error()
    n = C.c_size_t()
    assert L.dsx_map_knn_fetch(None, None, None, None, None, None, 0, C.byref(n)) == INV and b"null" in L.dsi_last_error()
    assert L.dsx_map_knn_fetch(fake, None, None, None, None, None, 0, None) == INV and b"null" in L.dsi_last_error()
    assert L.dsi_abi_version() == 10


# ---- symbols ----
def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    core = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", core))) == 176 and "dsx_" not in core
    header = open(os.path.join(ROOT, "include", "dsi_map_knn.h")).read()
    assert sorted(re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header)) == sorted(NEW)
    assert "float32" in header and "across a face" in header                  # the caveat is stated for the caller
    for other in ("dsi_map_eval.h", "dsi_map_prune.h", "dsi_map_merge.h", "dsi_map_align.h", "dsi_map_components.h"):
        assert "knn" not in open(os.path.join(ROOT, "include", other)).read()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name                      # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "dsi_map_knn.h" in readme and all(name in readme for name in NEW)
    assert "dsi_map_knn.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Neighbours and statistical outliers" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("query", "knn", "fetchKnn", "selectOutliers", "pruneOutliers"):
        assert hasattr(d.WorldMap, name), name
    assert callable(E.knn_threshold)
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for name in ("MapKnnOptions", "MapKnnSelection", "MapNeighbours query(", "MapKnnInfo knn(", "pruneOutliers(", "knn_threshold(",
                 "dsi_map_knn.h"):
        assert name in hpp, name
    from dvs_mcemvs_amd import build, process as proc
    assert inspect.signature(proc.full_sequence).parameters["world_map_outliers"].default is None
    assert any(h.endswith("dsi_map_knn.h") for h in build.HEADERS)
    assert os.path.exists(os.path.join(ROOT, "tools", "map_knn_bench.py"))


def test_struct_sizes_equal_the_headers(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dsi_map_knn.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(dsx_map_knn_opts_t), sizeof(dsx_map_knn_info_t), sizeof(dsx_map_knn_selection_t), "
                   "sizeof(dsx_map_knn_select_info_t), offsetof(dsx_map_knn_opts_t, radius), offsetof(dsx_map_knn_select_info_t, mu)); "
                   "return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert sizes == [C.sizeof(E._MapKnnOpts), C.sizeof(E._MapKnnInfo), C.sizeof(E._MapKnnSelection), C.sizeof(E._MapKnnSelectInfo),
                     E._MapKnnOpts.radius.offset, E._MapKnnSelectInfo.mu.offset]


def test_process_refuses_bad_outlier_options():
    from dvs_mcemvs_amd import process as proc
    for kw, word in ((dict(world_map_outliers={"k": 4, "radius": 0.1}), "needs world_map"),
                     (dict(world_map=object(), world_map_outliers={"k": 4, "radius": 0.1, "every": 0}), "every"),
                     (dict(world_map=object(), world_map_outliers={"k": 4, "radius": 0.1, "reach": 1}), "unknown keys"),
                     (dict(world_map=object(), world_map_outliers={"k": 4}), "needs k and radius")):
        with pytest.raises(ValueError, match=word):
            next(proc.full_sequence(None, None, None, None, None, 0.0, 1.0, 0.1, 1, **kw))


# ---- the new kernels' resources, from the compiler's remarks ----
@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_new_kernels_use_no_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage for every k_map_knn* instantiation: no scratch -- the running top-k stays in
    registers for every K -- and the table that DESIGN.md quotes."""
    p = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-x", "hip", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "dvs_mcemvs_amd", "csrc", "dsi_kernels.hip"), "-o", str(tmp_path / "k.s")],
                       stderr=subprocess.PIPE, text=True, check=True)
    seen = {}
    for block in p.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        m = re.search(r"\d+(k_map_knn_[a-z]+)(?:ILi(\d+)EEE|E)", name)
        if not m:
            continue
        val = lambda key: int(re.search(re.escape(key) + r"[^:]*: (\d+)", block).group(1))
        short = m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")
        seen[short] = (val("VGPRs"), val("TotalSGPRs"), val("Occupancy"), val("LDS Size"))
        assert val("ScratchSize") == 0, (short, block)
    print(seen)
    want = {"k_map_knn_select", "k_map_knn_gather"} | {"k_map_knn_%s<%d>" % (f, K) for f in ("points", "self") for K in INSTANCES}
    assert set(seen) == want, seen
    assert all(v[2] >= 2 and v[3] <= 64 for v in seen.values()), seen        # at least two waves per SIMD; a few counters in LDS
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for short, v in seen.items():                                               # DESIGN.md's table is this build's
        assert "| `%s` | %d | %d | %d |" % (short, v[0], v[1], v[2]) in design, (short, v)


# ---- the layout cases ----
def test_layout_cases_reach_the_second_round_and_the_tables_end():
    """What test_gpu_map_knn.py's layout tests rely on: the dense table never grows from 2^19 slots, so queries with a home in
    the second round exist and find neighbours there; the point query of its 300,007 centroids walks a second round too; the
    chain's cells sit in a run across the table's end and its self query looks up present and absent keys."""
    rm = lc.dense_reference()
    assert lc.grown_from(lc.dense_calls(), lc.LEAF, lc.BIG_LOG2) == 1 << lc.BIG_LOG2 and len(rm.keys) > lc.ROUND
    sq = kref.dense_self_query()
    first, second = lc.halves(sq["keys"])
    assert sq["reach"] == 1 and first.sum() >= 100_000 and second.sum() >= 100_000
    assert (sq["found"][second] >= 2).sum() >= 50_000 and len(np.unique(sq["found"][second])) >= 6
    assert sq["n_scored"] + sq["n_isolated"] == len(rm.keys) and sq["n_isolated"] >= 100
    assert sq["sum_q2"] > 1 << 64                                               # the 128-bit sum carries into its high word
    for name in lc.CHAINS:
        ch = lc.chain(name)
        occ, run = lc.chain_run(name)
        assert run is not None and run[1] >= len(ch["cells"])
        crm = kref.reference_of([ch["first"], ch["again"]], lc.CHAIN_LEAF)
        csq = kref.self_query(crm, 4, lc.CHAIN_RADIUS)
        assert csq["reach"] == 2 and (csq["found"] > 0).sum() >= 30 and (csq["rows"]["admitted"] < 124).all()
