"""One stage's mutator against another stage's result: after ANY call that changes (or may change) a world map, EVERY
fetch of EVERY derived pass refuses with DSI_ERR_INVALID -- the render, the compare, the classification, the alignment
step, the labelling, the self query and the local-shape pass, with and without their selections' reasons.  Each stage's
own test pins its own pair; this one pins the cross product, on one long-lived map of 2^8 slots.

The map: leaf 1, eleven cells in a row (x = 0..10) and one two cells further (x = 12), from two integrate calls.  The
lone cell is what each prune removes when it is asked to remove one cell: it lies outside the box, it is a component of one
cell, it has no neighbour within 1.5 and only one within 2.5.
"""
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
from dvs_mcemvs_amd import engine as E

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(4)[:3]
ROW = np.array([[x + 0.5, 0.5, 0.5] for x in range(11)], np.float32)
LONE = np.array([[12.5, 0.5, 0.5]], np.float32)
CALLS = (ROW, np.concatenate([LONE, ROW[:4]]))  # twelve cells, four of them seen twice
ROOM = 64  # every fetch gets room for more rows than the map has cells: a fetch that wrongly goes through stays in bounds
UNTOUCHED = 0x5A5A5A5A


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _fill(wm):
    wm.reset()
    for pts in CALLS:
        assert wm.integrate(pts, IDENTITY) == 0
    assert wm.info()["occupied"] == 12 and wm.info()["capacity"] == 256


def _run_passes(wm, other, knn_radius=2.5, pca_radius=2.5):
    """every derived pass once, the three selections included"""
    wm.render(IDENTITY, 8, 8, 4.0, 4.0, 4.0, 4.0, 0.1, 10.0, fetch=False)
    wm.compare(other, 1.5)
    wm.classifyPrune()
    wm.alignStep(other, 1.5)
    wm.components()
    wm.selectComponents()
    wm.knn(2, knn_radius)
    wm.selectOutliers(std_mult=-1.0)
    wm.pca(0, pca_radius, min_found=2)
    wm.selectShapes(keep=("linear", "planar", "scattered"), remove_sparse=False)


def _readers(wm):
    """name -> (call, count): every fetch of every stage through the C entry points, the ones that ask for reasons apart,
    and the selections, which read their pass too.  count is the size_t the call would write (None: it has none)."""
    L, h = d.load_library(), wm._h
    u64 = [np.zeros(ROOM, np.uint64) for _ in range(3)]
    f32 = [np.zeros(3 * ROOM, np.float32) for _ in range(4)]
    u32 = [np.zeros(ROOM, np.uint32) for _ in range(2)]
    u16, u8 = np.zeros(ROOM, np.uint16), [np.zeros(ROOM, np.uint8) for _ in range(4)]
    k0, k1, k2 = (_p(a, C.c_uint64) for a in u64)
    fl = [_p(a, C.c_float) for a in f32]
    b = [_p(a, C.c_uint8) for a in u8]
    out = {}

    def counted(name, call):
        n = C.c_size_t(UNTOUCHED)
        out[name] = (lambda: call(n), n)

    out["render_fetch"] = (lambda: L.dsi_map_render_fetch(h, fl[0], _p(u32[0], C.c_uint32), _p(u32[1], C.c_uint32), b[0]), None)
    counted("compare_fetch", lambda n: L.dsx_map_compare_fetch(h, fl[0], k0, ROOM, C.byref(n)))
    counted("prune_fetch", lambda n: L.dsx_map_prune_fetch(h, b[0], k0, ROOM, C.byref(n)))
    counted("align_fetch", lambda n: L.dsx_map_align_fetch(h, k0, k1, fl[0], ROOM, C.byref(n)))
    counted("components_fetch", lambda n: L.dsx_map_components_fetch(h, k0, k1, None, ROOM, C.byref(n)))
    counted("components_fetch+reasons", lambda n: L.dsx_map_components_fetch(h, k0, k1, b[0], ROOM, C.byref(n)))
    counted("components_list", lambda n: L.dsx_map_components_list(h, k0, k1, k2, ROOM, C.byref(n)))
    counted("knn_fetch", lambda n: L.dsx_map_knn_fetch(h, k0, b[0], fl[0], _p(u32[0], C.c_uint32), None, ROOM, C.byref(n)))
    counted("knn_fetch+reasons", lambda n: L.dsx_map_knn_fetch(h, k0, b[0], fl[0], _p(u32[0], C.c_uint32), b[1], ROOM, C.byref(n)))
    counted("pca_fetch", lambda n: L.dsx_map_pca_fetch(h, k0, fl[0], fl[1], fl[2], _p(u16, C.c_uint16), b[0], b[1], None, None, ROOM,
                                                       C.byref(n)))
    counted("pca_fetch+reasons", lambda n: L.dsx_map_pca_fetch(h, k0, fl[0], fl[1], fl[2], _p(u16, C.c_uint16), b[0], b[1], None, b[2],
                                                               ROOM, C.byref(n)))
    sel_c, sel_k, sel_p = E._MapComponentsSelection(1, 1, 0, 0), E._MapKnnSelection(-1.0, 0), E._MapPcaSelection(7, 0, 0)
    out["components_select"] = (lambda: L.dsx_map_components_select(h, C.byref(sel_c), None), None)
    out["knn_select"] = (lambda: L.dsx_map_knn_select(h, C.byref(sel_k), None), None)
    out["pca_select"] = (lambda: L.dsx_map_pca_select(h, C.byref(sel_p), None), None)
    out["_keep"] = (u64, f32, u32, u16, u8)  # (the buffers live as long as the calls)
    return out


def _all_go_through(wm):
    readers = _readers(wm)
    for name, entry in readers.items():
        if name != "_keep":
            assert entry[0]() == E.OK, name


def _all_refuse(wm, after):
    readers = _readers(wm)
    for name, entry in readers.items():
        if name == "_keep":
            continue
        call, n = entry
        rc = call()
        msg = (d.load_library().dsi_last_error() or b"").decode()
        assert rc == E.ERR_INVALID and msg.startswith("no "), "%s after %s: rc %d, '%s'" % (name, after, rc, msg)
        assert n is None or n.value == UNTOUCHED, "%s after %s wrote a count" % (name, after)


def _removed(info, want):
    assert sum(info["n_removed"]) == want and info["n_kept"] == 12 - want, info


def _mutators(other):
    """name -> (options of the passes, the call): every entry point that changes a map, each prune once with options that
    remove nothing and once with options that remove the lone cell"""
    state = other.exportState()
    box = ((-1.0, -1.0, -1.0), (11.9, 2.0, 2.0))
    return [
        ("dsi_map_integrate", {}, lambda wm: wm.integrate(ROW[:1], IDENTITY)),
        ("dsi_map_integrate of no points", {}, lambda wm: wm.integrate(np.zeros((0, 3), np.float32), IDENTITY)),
        ("dsx_map_integrate_map", {}, lambda wm: wm.integrateMap(other)),
        ("dsx_map_merge", {}, lambda wm: wm.merge(other)),
        ("dsx_map_import", {}, lambda wm: wm.importState(state)),
        ("dsi_map_reset", {}, lambda wm: wm.reset()),
        ("dsx_map_prune of nothing", {}, lambda wm: _removed(wm.prune(), 0)),
        ("dsx_map_prune of one cell", {}, lambda wm: _removed(wm.prune(box=box), 1)),
        ("dsx_map_prune_components of nothing", {}, lambda wm: _removed(wm.pruneComponents(), 0)),
        ("dsx_map_prune_components of one cell", {}, lambda wm: _removed(wm.pruneComponents(min_cells=2), 1)),
        ("dsx_map_prune_knn of nothing", {}, lambda wm: _removed(wm.pruneOutliers(std_mult=-1.0), 0)),
        ("dsx_map_prune_knn of one cell", {"knn_radius": 1.5}, lambda wm: _removed(wm.pruneOutliers(std_mult=-1.0), 1)),
        ("dsx_map_prune_pca of nothing", {},
         lambda wm: _removed(wm.pruneShapes(keep=("linear", "planar", "scattered"), remove_sparse=False), 0)),
        ("dsx_map_prune_pca of one cell", {},
         lambda wm: _removed(wm.pruneShapes(keep=("linear", "planar", "scattered"), remove_sparse=True), 1)),
    ]


def test_every_mutator_invalidates_every_result(ctx):
    wm, other = d.WorldMap(ctx, 1.0, 8), d.WorldMap(ctx, 1.0, 8)
    try:
        assert other.integrate(ROW[2:6] + np.float32(0.125), IDENTITY) == 0
        for name, passes, mutate in _mutators(other):
            _fill(wm)
            _run_passes(wm, other, **passes)
            _all_go_through(wm)  # (so that a refusal below is the mutator's doing)
            mutate(wm)
            _all_refuse(wm, name)
    finally:
        wm.close()
        other.close()
