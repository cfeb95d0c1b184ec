"""The world map's connected components without a GPU (include/dsi_map_components.h; DESIGN.md 7j "Components"): the
restatement (tests/map_components_reference.py) against independent statements, the conditions the GPU tests' inputs must
meet, the selection's hand cases, the argument checks and symbols of the five dsx_* entry points, and the new kernels'
metadata."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import dvs_mcemvs_amd as d
import map_components_reference as cref
import map_layout_cases as lc
import map_prune_reference as pref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_map_components", "dsx_map_components_fetch", "dsx_map_components_list", "dsx_map_components_select",
       "dsx_map_prune_components")
NEW_KERNELS = ("k_map_comp_init", "k_map_comp_union", "k_map_comp_flatten", "k_map_comp_reduce", "k_map_comp_rank_cells",
               "k_map_comp_rank_label", "k_map_comp_count", "k_map_comp_select", "k_map_comp_gather", "k_map_comp_root_count",
               "k_map_comp_list")


# ---- the restatement against independent statements ----
def random_keys(seed, n, side):
    rng = np.random.default_rng(seed)
    cells = np.unique(rng.integers(-side, side, (n, 3)), axis=0)
    return np.sort(ref.pack_key(cells))


def test_offsets():
    for conn, half in zip(cref.CONNECTIVITIES, (3, 9, 13, 62)):
        offs, pos = cref.offsets(conn), cref.positive_half(conn)
        assert len(offs) == conn == len(set(offs)) and len(pos) == half
        assert set(pos) | {tuple(-v for v in o) for o in pos} == set(offs)


@pytest.mark.parametrize("connectivity", cref.CONNECTIVITIES)
def test_restatement_equals_breadth_first_search(connectivity):
    keys = random_keys(3, 500, {6: 5, 18: 6, 26: 7, 124: 18}[connectivity])  # sparse enough for several components
    got, want = cref.label_keys(keys, connectivity), cref.bfs_labels(keys, connectivity)
    sizes = np.unique(got, return_counts=True)[1]
    print(connectivity, len(keys), "cells,", len(sizes), "components, largest", sizes.max())
    assert np.array_equal(got, want) and len(sizes) >= 2 and sizes.max() >= 3


@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_restatement_equals_ndimage_label_on_dense_boxes(connectivity):
    rng = np.random.default_rng(connectivity)
    box = rng.random((14, 12, 10)) < 0.22
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    lab, count = ndimage.label(box, structure=structure)
    idx = np.argwhere(box)                                                     # (x, y, z)
    keys = ref.pack_key(idx - 5)
    order = np.argsort(keys)
    keys, ids = keys[order], lab[box][order]
    got = cref.label_keys(keys, connectivity)
    low = np.full(count + 1, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(low, ids, keys)
    assert count >= 5 and np.array_equal(got, low[ids])


def test_restatement_equals_a_brute_force_chebyshev_graph_at_124():
    keys = random_keys(9, 400, 12)
    got = cref.label_keys(keys, 124)
    assert np.array_equal(got, cref.chebyshev_labels(keys, 2)) and 5 <= len(np.unique(got)) < len(keys)
    assert np.array_equal(cref.label_keys(keys, 26), cref.chebyshev_labels(keys, 1))


def test_cells_at_the_index_bound():
    cells = cref.edge_pairs()
    keys = np.sort(ref.pack_key(cells))
    for conn in cref.CONNECTIVITIES:
        labels = cref.label_keys(keys, conn)
        assert len(np.unique(labels)) == 6 and np.array_equal(labels, cref.bfs_labels(keys, conn))


# ---- the GPU inputs are not vacuous ----
def test_random_scene_is_not_vacuous():
    rm = cref.scene_reference()
    parts = {}
    for conn in cref.CONNECTIVITIES:
        comp = cref.scene_components(1, 1, conn)
        cells = comp["list"]["cells"]
        print(conn, comp["info"])
        assert (cells >= 2).sum() >= 5 and comp["info"]["n_singletons"] >= 5 and comp["info"]["n_unlabelled"] == 0
        assert comp["info"]["n_cells"] == len(rm.keys) == int(cells.sum()) and int(comp["list"]["points"].sum()) == int(rm.n.sum())
        parts[conn] = cref.partition(comp)
    assert len(set(parts.values())) == 4                                       # pairwise different partitions
    for flt in ((2, 1), (1, 2)):
        info = cref.scene_components(*flt, 26)["info"]
        assert info["n_unlabelled"] >= 20 and info["n_cells"] >= 20 and info["n_cells"] + info["n_unlabelled"] == len(rm.keys)
    # the selection the GPU test makes has every reason
    comp = cref.scene_components(2, 1, 26)
    out = cref.select(rm, comp, **SCENE_SELECTION)
    print(out["n_kept"], out["n_removed"], out["n_components_kept"])
    assert out["n_kept"] >= 5 and min(out["n_removed"]) >= 1 and out["n_components_kept"] == SCENE_SELECTION["keep_largest"]


SCENE_SELECTION = dict(min_cells=2, min_component_points=6, keep_largest=3)


def test_snake_is_one_path_per_layer_in_both_rounds_of_the_table():
    cells = cref.snake_cells()
    per_layer = len(cells) // 3
    assert 39_000 <= per_layer <= 41_000 and len(np.unique(cells, axis=0)) == len(cells)
    one = cref.snake_layer(0)
    assert (np.abs(np.diff(one, axis=0)).sum(axis=1) == 1).all()                # a 6-connected path in path order
    keys = ref.pack_key(cells)
    low, high = lc.halves(keys, 1 << cref.SNAKE_LOG2)
    assert low.sum() >= 10_000 and high.sum() >= 10_000
    assert 4 * len(cells) <= 3 << cref.SNAKE_LOG2                               # the table never grows
    rm = cref.snake_reference()
    assert len(rm.keys) == len(cells)
    for conn, want in ((6, 3), (18, 3), (26, 3), (124, 2)):
        comp = cref.components(rm, connectivity=conn)
        assert comp["info"]["n_components"] == want and comp["info"]["n_singletons"] == 0
        assert comp["list"]["cells"].tolist() == ([per_layer] * 3 if want == 3 else [2 * per_layer, per_layer])
    # a row's neighbours two rows away are no neighbours below 124: only the connecting cells hold a layer together at 26
    cut = rm.keys[~np.isin(rm.keys, ref.pack_key(one[cref.SNAKE_ROW:cref.SNAKE_ROW + 1]))]
    assert len(np.unique(cref.label_keys(cut, 26))) == 4 and len(np.unique(cref.label_keys(cut, 124))) == 2


@pytest.mark.parametrize("name", list(lc.CHAINS))
def test_chain_cells_form_components(name):
    rm = lc.chain_reference(name)
    for conn in cref.CONNECTIVITIES:
        comp = cref.components(rm, connectivity=conn)
        multi = int((comp["list"]["cells"] >= 2).sum())                         # (`again` adds the +x neighbour of 30 cells)
        print(name, conn, comp["info"], multi)
        assert comp["info"]["n_components"] >= 2 and multi >= (1 if conn == 124 else 10), (name, conn, comp["info"])
    assert lc.chain_run(name)[1] is not None


# ---- the selection's hand cases ----
@pytest.mark.parametrize("case", cref.selection_hand_cases(), ids=lambda c: c["name"])
def test_selection_hand_cases(case):
    rm = cref.map_of(cref.selection_case_calls(case), cref.PAIR_LEAF)
    comp = cref.components(rm, connectivity=26)
    assert comp["info"]["n_components"] == len(case["comps"])
    out = cref.select(rm, comp, **case["sel"])
    labels = [int(ref.pack_key(np.asarray(c)).min()) for c in case["comps"]]
    kept = sorted(np.unique(comp["labels"][out["node_reason"] == 0]).tolist())
    assert kept == sorted(labels[i] for i in case["want_kept"]) and out["n_components_kept"] == len(case["want_kept"])
    if "want_reasons" in case:
        for label, want in zip(labels, case["want_reasons"]):
            assert set(out["node_reason"][comp["labels"] == np.uint64(label)].tolist()) == {want}, case["name"]


def test_a_tie_is_a_tie_of_cells():
    case = cref.selection_hand_cases()[0]
    comp = cref.components(cref.map_of(cref.selection_case_calls(case), cref.PAIR_LEAF))
    assert comp["list"]["cells"].tolist() == [3, 3, 2] and comp["list"]["labels"][0] < comp["list"]["labels"][1]


@pytest.mark.parametrize("offset", list(cref.PAIR_OFFSETS), ids=str)
def test_pairs(offset):
    keys = np.sort(ref.pack_key(cref.pair_cells(offset)))
    for conn in cref.CONNECTIVITIES:
        assert len(np.unique(cref.label_keys(keys, conn))) == (1 if conn in cref.PAIR_OFFSETS[offset] else 2)


# ---- symbols ----
def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    core = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", core))) == 176 and "dsx_" not in core
    header = open(os.path.join(ROOT, "include", "dsi_map_components.h")).read()
    declared = re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header)
    assert sorted(declared) == sorted(NEW)
    for other in ("dsi_map_eval.h", "dsi_map_prune.h", "dsi_map_merge.h", "dsi_map_align.h"):
        assert "components" not in open(os.path.join(ROOT, "include", other)).read()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name                      # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    assert C.sizeof(E._MapComponentsOpts) == 12 and C.sizeof(E._MapComponentsInfo) == 56  # the header's layout
    assert C.sizeof(E._MapComponentsSelection) == 24 and C.sizeof(E._MapComponentsSelectInfo) == 64
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "dsi_map_components.h" in readme and all(name in readme for name in NEW)
    assert "dsi_map_components.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("components", "fetchComponents", "listComponents", "selectComponents", "pruneComponents"):
        assert hasattr(d.WorldMap, name), name
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for name in ("MapComponentsOptions", "MapComponentsSelection", "components(", "fetchComponents(", "listComponents(", "selectComponents(",
                 "pruneComponents(", "dsi_map_components.h"):
        assert name in hpp, name
    from dvs_mcemvs_amd import build, process as proc
    assert inspect.signature(proc.full_sequence).parameters["world_map_components"].default is None
    assert any(h.endswith("dsi_map_components.h") for h in build.HEADERS)


def test_struct_sizes_equal_the_headers(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include "dsi_map_components.h"\nint main() { std::printf("%zu %zu %zu %zu\\n", '
                   "sizeof(dsx_map_components_opts_t), sizeof(dsx_map_components_info_t), sizeof(dsx_map_components_selection_t), "
                   "sizeof(dsx_map_components_select_info_t)); return 0; }\n")
    import subprocess
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert sizes == [C.sizeof(E._MapComponentsOpts), C.sizeof(E._MapComponentsInfo), C.sizeof(E._MapComponentsSelection),
                     C.sizeof(E._MapComponentsSelectInfo)]


# ---- argument checks with a handle that is never dereferenced ----
def test_abi_argument_checks_need_no_gpu(built):
    L = d.load_library()
    INV = E.ERR_INVALID
    fake = C.c_void_p(0x1000)                                                   # never dereferenced: the checks come first
    info, sinfo = E._MapComponentsInfo(), E._MapComponentsSelectInfo()
    assert L.dsx_map_components(fake, None, C.byref(info)) == INV and b"opts is null" in L.dsi_last_error()
    assert L.dsx_map_components(None, None, None) == INV and b"opts is null" in L.dsi_last_error()
    for conn in (0, 7, 27, 125, -26):
        for handle in (None, fake):
            assert L.dsx_map_components(handle, C.byref(E._MapComponentsOpts(1, 1, conn)), C.byref(info)) == INV, conn
            assert b"connectivity" in L.dsi_last_error()
    for conn in cref.CONNECTIVITIES:                                            # legal: the complaint is then the missing map
        assert L.dsx_map_components(None, C.byref(E._MapComponentsOpts(0, 2 ** 32 - 1, conn)), None) == INV
        assert b"map is null" in L.dsi_last_error()
    for fn in (L.dsx_map_components_select, L.dsx_map_prune_components):
        assert fn(fake, None, C.byref(sinfo)) == INV and b"sel is null" in L.dsi_last_error()
        assert fn(None, None, None) == INV and b"sel is null" in L.dsi_last_error()
        for kw, word in ((dict(keep_largest=17), b"keep_largest"), (dict(keep_largest=-1), b"keep_largest"), (dict(shrink=2), b"shrink"),
                         (dict(shrink=-1), b"shrink")):
            for handle in (None, fake):
                sel = E._MapComponentsSelection(1, 1, kw.get("keep_largest", 0), kw.get("shrink", 0))
                assert fn(handle, C.byref(sel), C.byref(sinfo)) == INV, kw
                assert word in L.dsi_last_error(), (kw, L.dsi_last_error())
        for sel in (E._MapComponentsSelection(0, 0, 0, 0), E._MapComponentsSelection(2 ** 64 - 1, 2 ** 64 - 1, 16, 1)):
            assert fn(None, C.byref(sel), None) == INV and b"map is null" in L.dsi_last_error()
    n = C.c_size_t()
    for fn, nulls in ((L.dsx_map_components_fetch, (None, None, None)), (L.dsx_map_components_list, (None, None, None))):
        assert fn(None, *nulls, 0, C.byref(n)) == INV and b"null" in L.dsi_last_error()
        assert fn(fake, *nulls, 0, None) == INV and b"null" in L.dsi_last_error()
    assert L.dsi_abi_version() == 10


# ---- the new kernels' resources ----
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
