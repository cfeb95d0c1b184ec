"""Pruning the world map without a GPU (include/dsi_map_prune.h; DESIGN.md 7j "Pruning"): the numpy restatement
(tests/map_prune_reference.py) against a brute-force classifier, the conditions the GPU tests' scene must meet, hand cases,
the argument checks and symbols of the three dsx_* entry points, and the new kernels' metadata."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_prune_reference as pref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_map_prune_classify", "dsx_map_prune_fetch", "dsx_map_prune")
NEW_KERNELS = ("k_map_prune_reason", "k_map_prune_support", "k_map_prune_rehash", "k_map_prune_gather")


def test_restatement_equals_brute_force_on_a_small_random_scene():
    rng = np.random.default_rng(21)
    rm = pref.PruneReferenceMap(0.05)
    for k, n in enumerate((260, 0, 90, 170)):
        pts = np.column_stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(0.0, 0.1, n)])
        if k == 3:
            pts = pts[pts[:, 0] > 0.0]
        rm.integrate(pts.astype(np.float32), pref.IDENTITY)
    assert 200 < len(rm.keys) < 400 and rm.calls == 4
    for opts in (dict(min_points=2, min_windows=2, max_age=0, box=((-0.25, -0.2, 0.0), (0.3, 0.3, 0.1)), reach=1, min_neighbors=3),
                 dict(reach=2, min_neighbors=20), dict(reach=1, min_neighbors=1), dict(max_age=1, reach=1, min_neighbors=8),
                 dict(min_windows=2), dict()):
        got = rm.classify(**opts)
        want = pref.brute_force(rm, **opts)
        assert np.array_equal(got["reason"], want), opts
        assert got["n_cells"] == len(rm.keys) == got["n_kept"] + sum(got["n_removed"])
        print(opts, got["n_kept"], got["n_removed"])
    got = rm.classify(min_points=2, min_windows=2, max_age=0, box=((-0.25, -0.2, 0.0), (0.3, 0.3, 0.1)), reach=1, min_neighbors=3)
    assert min(got["n_removed"]) >= 3 and got["n_kept"] >= 3                   # every branch of the brute force was taken
    assert rm.classify()["n_kept"] == len(rm.keys)                             # the defaults remove nothing


def test_random_scene_is_not_vacuous():
    """What the GPU tests on the shared scene rely on (floors, not tolerances): every reason and "kept" occurs, and some
    kept cell owes its support to cells that criterion 5 itself removes -- the one-pass rule is observable."""
    calls = pref.scene_calls()
    sizes = [len(p) for p, _ in calls]
    assert len(calls) == 8 and sizes.count(0) == 2 and 3000 <= sum(sizes) <= 6000 and len(set(sizes)) == 7
    rm = pref.scene_map()
    out = rm.classify(**pref.SCENE_OPTS)
    lone_support = pref.supported_only_by_removed(rm, **pref.SCENE_OPTS)
    print("cells %d, kept %d, removed %s, kept by removed supporters %d" % (out["n_cells"], out["n_kept"], out["n_removed"], lone_support))
    assert out["n_kept"] >= 20 and all(n >= 20 for n in out["n_removed"])
    assert lone_support >= 1
    # the prune itself: the kept cells with all their state, and a stamp that goes on counting
    before = {k: getattr(rm, k).copy() for k in ("keys", "n", "S", "windows", "stamp")}
    rm.prune(**pref.SCENE_OPTS)
    keep = out["reason"] == 0
    for k, v in before.items():
        assert np.array_equal(getattr(rm, k), v[keep]), k
    assert rm.calls == 8 and len(rm.keys) == out["n_kept"]
    assert rm.classify(**dict(pref.SCENE_OPTS, reach=0, min_neighbors=0))["n_kept"] == out["n_kept"]


@pytest.mark.parametrize("case", pref.hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(case):
    rm = pref.run_hand_case(case, pref.PruneReferenceMap)
    cells = rm.extract()
    want_xyz = ((ref.unpack_key(cells["keys"]) + 0.5) * case["leaf"]).astype(np.float32)
    if not case["name"].startswith("box"):
        assert np.array_equal(cells["xyz"], want_xyz)                          # every centroid is exact: the cell's centre
    out = rm.classify(**case["opts"])
    keys, reasons = pref.wanted_reasons(case)
    assert np.array_equal(out["keys"], keys) and np.array_equal(out["reason"], reasons), out["reason"]
    assert np.array_equal(pref.brute_force(rm, **case["opts"]), reasons)


def test_box_edges_are_exact_centroids():
    case = pref.hand_cases()[0]
    xyz = pref.run_hand_case(case, pref.PruneReferenceMap).extract()["xyz"]
    x = np.sort(xyz[:, 0])
    assert x[1] == np.float32(0.25) and x[2] == np.float32(0.75)
    assert x[0] == np.nextafter(np.float32(0.25), np.float32(0)) and x[3] == np.nextafter(np.float32(0.75), np.float32(1))


def test_shrunk_capacity():
    assert [pref.shrunk_capacity(k) for k in (0, 1, 192, 193, 384, 385, 20000)] == [256, 256, 256, 512, 512, 1024, 32768]


def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    core = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", core))) == 176 and "dsx_" not in core
    header = open(os.path.join(ROOT, "include", "dsi_map_prune.h")).read()
    declared = re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header)
    assert sorted(declared) == sorted(NEW)
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name                      # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    assert C.sizeof(E._MapPruneOpts) == 88 and C.sizeof(E._MapPruneInfo) == 64  # the header's layout
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "dsi_map_prune.h" in readme and all(name in readme for name in NEW)
    assert "dsi_map_prune.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("prune", "classifyPrune", "fetchPruneReasons"):
        assert hasattr(d.WorldMap, name), name
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for name in ("MapPruneOptions", "prune(", "classifyPrune(", "fetchPruneReasons(", "dsi_map_prune.h"):
        assert name in hpp, name
    import inspect
    from dvs_mcemvs_amd import build, process as proc
    assert inspect.signature(proc.full_sequence).parameters["world_map_prune"].default is None
    assert any(h.endswith("dsi_map_prune.h") for h in build.HEADERS)


def opts(**kw):
    o = E._MapPruneOpts()
    o.min_points = o.min_windows = 1
    o.max_age = -1
    for k, v in kw.items():
        if k in ("box_lo", "box_hi"):
            getattr(o, k)[:] = v
        else:
            setattr(o, k, v)
    return o


NAN, INF = float("nan"), float("inf")
BAD_OPTS = [(dict(use_box=2), b"use_box"), (dict(use_box=-1), b"use_box"),
            (dict(use_box=1, box_lo=[NAN, 0, 0], box_hi=[1, 1, 1]), b"box"), (dict(use_box=1, box_lo=[0, 0, 0], box_hi=[1, NAN, 1]), b"box"),
            (dict(use_box=1, box_lo=[0, 0, 2], box_hi=[1, 1, 1]), b"box"), (dict(use_box=1, box_lo=[INF, 0, 0], box_hi=[-INF, 1, 1]), b"box"),
            (dict(reach=-1), b"reach"), (dict(reach=3), b"reach"), (dict(reach=1, min_neighbors=0), b"min_neighbors"),
            (dict(reach=1, min_neighbors=27), b"min_neighbors"), (dict(reach=2, min_neighbors=125), b"min_neighbors"),
            (dict(reach=0, min_neighbors=1), b"min_neighbors"), (dict(shrink=2), b"shrink"), (dict(shrink=-1), b"shrink")]
GOOD_OPTS = [dict(), dict(reach=1, min_neighbors=1), dict(reach=1, min_neighbors=26), dict(reach=2, min_neighbors=124), dict(shrink=1),
             dict(use_box=1, box_lo=[-INF, 0, 0], box_hi=[INF, 0, 5]), dict(use_box=0, box_lo=[NAN, 2, 2], box_hi=[1, 1, NAN]),
             dict(min_points=0, min_windows=0, max_age=0), dict(min_points=2 ** 32 - 1, min_windows=2 ** 32 - 1, max_age=2 ** 62)]


def test_abi_argument_checks_need_no_gpu(built):
    L = d.load_library()
    INV = E.ERR_INVALID
    fake = C.c_void_p(0x1000)                                                   # never dereferenced: the checks come first
    info = E._MapPruneInfo()
    for fn in (L.dsx_map_prune_classify, L.dsx_map_prune):
        assert fn(fake, None, C.byref(info)) == INV and b"opts is null" in L.dsi_last_error()
        assert fn(None, None, None) == INV and b"opts is null" in L.dsi_last_error()
        # every bound of the options in turn: judged before the map is looked at
        for kw, word in BAD_OPTS:
            for handle in (None, fake):
                assert fn(handle, C.byref(opts(**kw)), C.byref(info)) == INV, kw
                assert word in L.dsi_last_error(), (kw, L.dsi_last_error())
        # the bounds themselves are legal: the complaint is then the missing map
        for kw in GOOD_OPTS:
            assert fn(None, C.byref(opts(**kw)), None) == INV and b"map is null" in L.dsi_last_error(), kw
    n = C.c_size_t()
    assert L.dsx_map_prune_fetch(None, None, None, 0, C.byref(n)) == INV and b"null" in L.dsi_last_error()
    assert L.dsx_map_prune_fetch(fake, None, None, 0, None) == INV and b"null" in L.dsi_last_error()
    assert L.dsi_abi_version() == 10


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    text = kernel_asm_text()
    seen = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = [k for k in NEW_KERNELS if re.search(r"\d+%sE" % k, name)]
        if not short:
            continue
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, name
        assert val("wavefront_size") == 64 and val("max_flat_workgroup_size") == 256, name
        seen[short[0]] = (val("vgpr_count"), val("sgpr_count"), val("group_segment_fixed_size"))
    print(seen)
    assert set(seen) == set(NEW_KERNELS), seen
    assert all(v[0] <= 64 and v[2] <= 64 for v in seen.values()), seen        # eight waves per SIMD; a few counters in LDS
    # the classification only reads the table: its atomics are its counters', never a compare-and-swap; the rebuild claims keys
    for k in ("k_map_prune_reason", "k_map_prune_support"):
        m = re.search(r"^(_ZN\w*\d+%sE\w*):.*?$(.*?)^\.Lfunc_end" % k, text, re.S | re.M)    # (the whole body, past any early exit)
        assert m and "atomic_cmpswap" not in m.group(2) and "global_atomic_add_x2" in m.group(2), k
    m = re.search(r"^(_ZN\w*\d+k_map_prune_rehashE\w*):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)
    assert m and "atomic_cmpswap" in m.group(2)
