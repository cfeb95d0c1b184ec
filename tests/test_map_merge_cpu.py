"""Merging world maps without a GPU (include/dsi_map_merge.h; DESIGN.md 7j "Merging"): the append property in the numpy
restatement (tests/map_merge_reference.py) at every cut of the shared scene, after a prune and round-robin, every refusal
of the restatement, the symbols and argument checks of the three dsx_* entry points, io.save_world_map / load_world_map,
and the new kernels' metadata.  Every comparison is array_equal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_merge_reference as mref
import map_prune_reference as pref
from dvs_mcemvs_amd import engine as E, io as dio
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_map_export", "dsx_map_import", "dsx_map_merge")
NEW_KERNELS = ("k_map_export", "k_map_import_build", "k_map_merge")
PRUNE = dict(min_points=2, reach=1, min_neighbors=2)


@pytest.fixture(scope="module")
def scene():
    calls = pref.scene_calls()
    return calls, mref.reference_of(calls).export_state()


def test_a_merge_appends_at_every_cut(scene):
    calls, whole = scene
    assert [len(p) for p, _ in calls] == [1010, 410, 0, 948, 210, 0, 756, 617] and len(whole["keys"]) == 1640
    for cut in range(len(calls) + 1):
        a, b = mref.reference_of(calls[:cut]), mref.reference_of(calls[cut:])
        b_before = b.export_state()
        info = a.merge(b)
        print(cut, info)
        mref.assert_states_equal(a.export_state(), whole)
        mref.assert_states_equal(b.export_state(), b_before)                   # the source is unchanged
        assert info["n_src_cells"] == len(b_before["keys"]) == info["n_new"] + info["n_common"]
        if 1 <= cut <= 7:
            assert info["n_new"] >= 100 and info["n_common"] >= 400, (cut, info)   # both branches of the rule are taken
    # the same through an exported state, and a restore into an empty map
    for cut in (0, 3, 8):
        a = mref.reference_of(calls[:cut])
        a.import_state(mref.reference_of(calls[cut:]).export_state())
        mref.assert_states_equal(a.export_state(), whole)


@pytest.mark.parametrize("cut", [3, 5])
def test_a_merge_appends_after_a_prune(scene, cut):
    calls, _ = scene
    a, want = mref.reference_of(calls[:cut]), mref.reference_of(calls[:cut])
    removed = a.prune(**PRUNE)
    want.prune(**PRUNE)
    assert sum(removed["n_removed"]) >= 100 and removed["n_kept"] >= 100
    for pts, T in calls[cut:]:
        want.integrate(pts, T)
    b = mref.reference_of(calls[cut:])
    back = int(np.isin(b.keys, removed["keys"][removed["reason"] != 0]).sum())
    assert back >= 10                                                          # removed cells come back, from zero
    a.merge(b)
    mref.assert_states_equal(a.export_state(), want.export_state())


def test_round_robin_agrees_in_all_but_the_stamps(scene):
    calls, whole = scene
    for ways, same in ((2, 790), (3, None)):
        maps = [mref.MergeReferenceMap(pref.LEAF) for _ in range(ways)]
        for k, (pts, T) in enumerate(calls):
            maps[k % ways].integrate(pts, T)
        for m in maps[1:]:
            maps[0].merge(m)
        got = maps[0].export_state()
        for k in ("keys", "n", "S", "windows"):
            assert np.array_equal(got[k], whole[k]), k
        assert all(got[k] == whole[k] for k in ("calls", "accepted", "rejected"))
        agree = int((got["stamp"] == whole["stamp"]).sum())
        print(ways, agree)
        assert 0 < agree < len(whole["keys"]) and (same is None or agree == same)
        # the stamps are the rule's: the last call of the LAST map that reached the cell, moved behind the maps before it
        assert (got["stamp"] >= 1).all() and (got["stamp"] <= got["calls"]).all() and (got["windows"] <= got["stamp"]).all()


def test_an_empty_source_ages_and_an_empty_destination_becomes_the_source(scene):
    calls, whole = scene
    a, empty = mref.reference_of(calls), mref.reference_of([calls[2]] * 3)
    assert len(empty.keys) == 0 and empty.calls == 3
    assert a.merge(empty) == {"n_src_cells": 0, "n_new": 0, "n_common": 0}
    got = a.export_state()
    assert got["calls"] == whole["calls"] + 3 and all(np.array_equal(got[k], whole[k]) for k in ("keys", "n", "S", "windows", "stamp"))
    assert a.classify(max_age=2)["n_kept"] == 0 and a.classify(max_age=3)["n_kept"] > 0
    b = mref.MergeReferenceMap(pref.LEAF)
    b.merge(mref.reference_of(calls))
    mref.assert_states_equal(b.export_state(), whole)


def test_every_refusal_of_the_restatement(scene):
    calls, whole = scene
    dst = mref.reference_of(calls[:3])
    before = dst.export_state()
    bad, good = mref.header_states(pref.LEAF, dst.calls, dst.accepted)
    for name, word, state in mref.bad_states(whole) + bad:
        with pytest.raises(mref.Refused) as e:
            dst.import_state(state)
        assert e.value.args[0] == word, (name, e.value.args)
        mref.assert_states_equal(dst.export_state(), before)
    with pytest.raises(mref.Refused):
        dst.merge(dst)
    with pytest.raises(mref.Refused):
        dst.merge(mref.MergeReferenceMap(float(np.nextafter(pref.LEAF, 1.0))))
    full = mref.MergeReferenceMap(pref.LEAF)
    full.calls = mref.U32_MAX
    with pytest.raises(mref.Refused):
        dst.merge(full)
    mref.assert_states_equal(dst.export_state(), before)
    dst.import_state(good[0])
    assert dst.calls == mref.U32_MAX and dst.accepted == mref.U32_MAX
    # S == n 2^32 exactly is legal (a point may count at the cell's upper face)
    ok = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in whole.items()}
    ok["S"][3, 1] = int(ok["n"][3]) << 32
    mref.MergeReferenceMap(pref.LEAF).import_state(ok)


def test_grown_capacity():
    assert mref.grown_capacity(256, 0, 192) == (256, 0) and mref.grown_capacity(256, 0, 193) == (512, 1)
    assert mref.grown_capacity(256, 100, 20000) == (1 << 15, 7) and mref.grown_capacity(1 << 16, 1000, 1000) == (1 << 16, 0)


def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    core = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", core))) == 176 and "dsx_" not in core
    header = open(os.path.join(ROOT, "include", "dsi_map_merge.h")).read()
    declared = re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header)
    assert sorted(declared) == sorted(NEW)
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name                      # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    assert C.sizeof(E._MapState) == 40 and C.sizeof(E._MapMergeInfo) == 40      # the header's layout
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "dsi_map_merge.h" in readme and all(name in readme for name in NEW)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "dsi_map_merge.h" in integration and all(name in integration for name in NEW)
    for name in ("merge", "exportState", "importState"):
        assert hasattr(d.WorldMap, name), name
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for name in ("MapState", "MapMergeInfo merge(", "exportState(", "importState(", "dsi_map_merge.h"):
        assert name in hpp, name
    from dvs_mcemvs_amd import build, process as proc
    assert callable(proc.merge_world_maps) and callable(dio.save_world_map) and callable(dio.load_world_map)
    assert any(h.endswith("dsi_map_merge.h") for h in build.HEADERS)


def test_abi_argument_checks_need_no_gpu(built):
    L = d.load_library()
    INV = E.ERR_INVALID
    fake, other = C.c_void_p(0x1000), C.c_void_p(0x2000)                        # never dereferenced: the checks come first
    info, n = E._MapMergeInfo(), C.c_size_t()
    assert L.dsx_map_merge(None, other, C.byref(info)) == INV and b"dst is null" in L.dsi_last_error()
    assert L.dsx_map_merge(fake, None, C.byref(info)) == INV and b"src is null" in L.dsi_last_error()
    assert L.dsx_map_merge(fake, fake, None) == INV and b"same map" in L.dsi_last_error()
    assert L.dsx_map_export(None, None, None, None, None, None, None, 0, C.byref(n)) == INV and b"null" in L.dsi_last_error()
    assert L.dsx_map_export(fake, None, None, None, None, None, None, 0, None) == INV and b"null" in L.dsi_last_error()
    st = E._MapState(0.05, 0, 0, 0, 0)
    assert L.dsx_map_import(None, C.byref(st), None, None, None, None, None, None) == INV and b"dst is null" in L.dsi_last_error()
    assert L.dsx_map_import(fake, None, None, None, None, None, None, None) == INV and b"state is null" in L.dsi_last_error()
    for leaf in (0.0, -1.0, float("nan"), float("inf")):
        assert L.dsx_map_import(fake, C.byref(E._MapState(leaf, 0, 0, 0, 0)), None, None, None, None, None, None) == INV
        assert b"leaf" in L.dsi_last_error()
    assert L.dsx_map_import(fake, C.byref(E._MapState(0.05, (1 << 27) + 1, 0, 0, 0)), None, None, None, None, None, None) == INV
    assert b"n_cells" in L.dsi_last_error()
    keys, cnt, S = np.ones(2, np.uint64), np.ones(2, np.uint32), np.ones(6, np.uint64)
    p = {"keys": keys.ctypes.data_as(C.POINTER(C.c_uint64)), "n": cnt.ctypes.data_as(C.POINTER(C.c_uint32)),
         "sums": S.ctypes.data_as(C.POINTER(C.c_uint64)), "windows": cnt.ctypes.data_as(C.POINTER(C.c_uint32)),
         "stamp": cnt.ctypes.data_as(C.POINTER(C.c_uint32))}
    st = E._MapState(0.05, 2, 1, 2, 0)
    for missing in p:                                                           # import needs all five arrays when n_cells > 0
        args = [None if k == missing else v for k, v in p.items()]
        assert L.dsx_map_import(fake, C.byref(st), *args, None) == INV
        assert missing.encode() + b" is null" in L.dsi_last_error(), (missing, L.dsi_last_error())
    assert L.dsi_abi_version() == 10


def test_world_map_files(scene, tmp_path):
    _, whole = scene
    path = str(tmp_path / "map.npz")
    dio.save_world_map(path, whole)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    back = dio.load_world_map(path)
    mref.assert_states_equal(back, whole)
    assert type(back["leaf"]) is float and all(type(back[k]) is int for k in ("calls", "accepted", "rejected"))
    empty = mref.MergeReferenceMap(0.5).export_state()
    dio.save_world_map(path, empty)
    mref.assert_states_equal(dio.load_world_map(path), empty)
    # refusals on the way out
    for k, v in (("n", whole["n"].astype(np.uint64)), ("keys", whole["keys"].astype(np.int64)), ("S", whole["S"].reshape(-1)),
                 ("stamp", whole["stamp"][:-1]), ("S", whole["S"][:, :2]), ("windows", whole["windows"].astype(np.float32))):
        with pytest.raises(ValueError):
            dio.save_world_map(path, dict(whole, **{k: v}))
    # refusals on the way in: files that numpy reads but that hold no map state
    raw = {k: np.asarray(v) for k, v in whole.items()}
    raw.update(leaf=np.float64(whole["leaf"]), calls=np.uint64(whole["calls"]), accepted=np.uint64(whole["accepted"]),
               rejected=np.uint64(whole["rejected"]))
    wrong = [{k: v for k, v in raw.items() if k != "stamp"}, dict(raw, n=raw["n"].astype(np.int32)), dict(raw, S=raw["S"].reshape(-1)),
             dict(raw, keys=raw["keys"][:-1]), dict(raw, leaf=np.float32(0.05)), dict(raw, calls=np.int64(8)),
             dict(raw, accepted=np.array([1, 2], np.uint64)), dict(raw, S=raw["S"].astype(np.float64))]
    for i, w in enumerate(wrong):
        bad = str(tmp_path / ("bad_%d.npz" % i))
        with open(bad, "wb") as f:
            np.savez(f, **w)
        with pytest.raises(ValueError):
            dio.load_world_map(bad)


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
