"""The world map's kernels past one stride and across the table's end, on the MI355X against the existing
numpy restatements.  tests/map_layout_cases.py holds the inputs and tests/test_map_layouts_cpu.py proves, without a GPU,
the properties these tests rely on.  Every comparison is array_equal; floats are compared on their bit patterns.

    part A   tables of 2^19 slots that never grow (and lists of more than 2^18 items or pixels): every workgroup of
             k_map_render, k_map_render_finish, k_map_compare, k_map_export, k_map_import_build and k_map_merge walks a
             second round, with members of every counted class on both sides of slot 2^18
    part B   a run of occupied slots that crosses slot capacity - 1 -> 0, at 2^8 and at 2^19 slots: everything that inserts
             (map_slot) or looks up (map_find) goes through it
    part C   one call list in five layouts of the table: every read operation gives the restatement's bits in each
"""
import ctypes as C
import re

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_align_reference as ar
import map_eval_reference as eref
import map_layout_cases as lc
import map_merge_reference as mref
import map_prune_reference as pref
import world_map_reference as ref
import world_map_render_reference as rref
from dvs_mcemvs_amd import engine as E

pytestmark = pytest.mark.gpu

IDENTITY = lc.IDENTITY


def build(ctx, calls, leaf, log2):
    """the calls through a WorldMap; every call rejects nothing"""
    wm = d.WorldMap(ctx, leaf, log2)
    for pts, T in calls:
        assert wm.integrate(pts, T) == 0
    return wm


def never_grew(wm, log2):
    info = wm.info()
    return info["growths"] == 0 and info["capacity"] == 1 << log2


def check_state(wm, rm):
    """the map's counters and its exported state equal the restatement's"""
    info = wm.info()
    assert (info["occupied"], info["calls"], info["accepted"], info["rejected"]) == (len(rm.keys), rm.calls, rm.accepted, rm.rejected)
    mref.assert_states_equal(wm.exportState(), rm.export_state())


def check_merge_info(info, want, before, after):
    """a merge's or an import's counts equal the restatement's; growths and capacity are the 3/4 rule's"""
    assert {k: info[k] for k in want} == want, (info, want)
    cap, g = mref.grown_capacity(before["capacity"], before["occupied"], want["n_src_cells"])
    assert (info["capacity"], info["growths"]) == (cap, g) and after["capacity"] == cap and after["growths"] == before["growths"] + g
    assert after["occupied"] == before["occupied"] + want["n_new"]
    return g


def check_classify(wm, want):
    info = wm.classifyPrune(**want["opts"])
    assert (info["n_cells"], info["n_kept"], info["n_removed"]) == (want["n_cells"], want["n_kept"], want["n_removed"]), info
    got = wm.fetchPruneReasons()
    assert got["reason"].dtype == np.uint8 and np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["reason"], want["reason"])


def classified(rm, **opts):
    return dict(rm.classify(**opts), opts=opts)


def refusal(fn, word):
    """the engine refuses fn() with DSI_ERR_INVALID and names `word`; returns the count the message gives, if it gives one"""
    with pytest.raises(d.DsiError) as e:
        fn()
    assert e.value.code == E.ERR_INVALID and word + ": " in str(e.value), (e.value.code, str(e.value))
    m = re.search(re.escape(word) + r": (\d+) ", str(e.value))
    return int(m.group(1)) if m else None


def guarded_fetch(wm, shape):
    """dsi_map_render_fetch into the middle of guard-patterned arrays: (images, guards intact)"""
    n, pad = shape[0] * shape[1], 4096
    bufs = {"depth": np.full(n + 2 * pad, -77.0, np.float32), "windows": np.full(n + 2 * pad, 0xA5A5A5A5, np.uint32),
            "hits": np.full(n + 2 * pad, 0x5A5A5A5A, np.uint32), "mask": np.full(n + 2 * pad, 0xC3, np.uint8)}
    before = {k: v.copy() for k, v in bufs.items()}
    mid = {k: v[pad:pad + n] for k, v in bufs.items()}
    types = {"depth": C.c_float, "windows": C.c_uint32, "hits": C.c_uint32, "mask": C.c_uint8}
    assert d.load_library().dsi_map_render_fetch(wm._h, *(mid[k].ctypes.data_as(C.POINTER(types[k])) for k in types)) == E.OK
    intact = all(np.array_equal(bufs[k][:pad], before[k][:pad]) and np.array_equal(bufs[k][pad + n:], before[k][pad + n:])
                 for k in bufs)
    return {k: v.reshape(shape).copy() for k, v in mid.items()}, intact


# ---- part A: the second round of every strided kernel ----

@pytest.fixture(scope="module")
def sparse19(ctx):
    wm = build(ctx, lc.sparse_calls(), lc.LEAF, lc.BIG_LOG2)
    assert never_grew(wm, lc.BIG_LOG2)
    ref.assert_maps_equal(wm.extract(), lc.sparse_reference().extract())
    yield wm
    wm.close()


@pytest.fixture(scope="module")
def dense19(ctx):
    wm = build(ctx, lc.dense_calls(), lc.LEAF, lc.BIG_LOG2)
    assert never_grew(wm, lc.BIG_LOG2) and wm.info()["occupied"] == lc.DENSE_CELLS
    yield wm
    wm.close()


@pytest.fixture(scope="module")
def other(ctx):
    """the map of leaf 0.04 that the sparse scene is compared and aligned with, in a table that grows from 2^8 slots"""
    wm = build(ctx, lc.other_calls(), lc.LEAF_B, 8)
    ref.assert_maps_equal(wm.extract(), lc.other_reference().extract())
    yield wm
    wm.close()


@pytest.mark.parametrize("splat,min_windows", lc.RENDER_CASES)
def test_render_walks_two_rounds(sparse19, splat, min_windows):
    got = sparse19.render(*lc.SMALL_VIEW, splat=splat, min_windows=min_windows)
    want = lc.sparse_render("small", splat, min_windows)
    assert min(want["n_drawn"], want["n_clipped"], want["n_outside"]) >= 100
    rref.assert_renders_equal(got, want)
    assert never_grew(sparse19, lc.BIG_LOG2)


def test_render_finish_walks_two_rounds_and_a_partial_workgroup(sparse19):
    counts = sparse19.render(*lc.WIDE_VIEW, splat=2, fetch=False)
    want = lc.sparse_render("wide", 2, 1)
    assert (counts["width"], counts["height"]) == (lc.WIDE_W, lc.WIDE_H) and lc.WIDE_W * lc.WIDE_H > lc.ROUND
    images, intact = guarded_fetch(sparse19, (lc.WIDE_H, lc.WIDE_W))
    assert intact
    assert want["mask"].reshape(-1)[lc.ROUND:].any() and want["mask"].reshape(-1)[-157:].any()
    rref.assert_renders_equal(dict(counts, **images), want)


@pytest.mark.parametrize("radius", eref.RADII)
def test_compare_walks_two_rounds(sparse19, other, radius):
    """the big table walked (forward), and the big table looked up (backward)"""
    got = sparse19.compare(other, radius, eref.N_BINS, distances=True)
    eref.assert_compares_equal(got, lc.sparse_compare(True, radius))
    assert got["n_matched"] >= 100 and got["n_unmatched"] >= 100
    back = other.compare(sparse19, radius, eref.N_BINS, distances=True)
    eref.assert_compares_equal(back, lc.sparse_compare(False, radius))
    assert back["n_matched"] >= 100 and back["n_unmatched"] >= 100


def test_export_walks_two_rounds(dense19):
    got, want = dense19.exportState(), lc.dense_reference().export_state()
    assert len(got["keys"]) == lc.DENSE_CELLS
    mref.assert_states_equal(got, want)
    raw, cells = dense19.exportState(sort=False), dense19.extract(0, 0, sort=False)      # the table's order is the extraction's
    assert np.array_equal(raw["keys"], cells["keys"]) and np.array_equal(raw["n"], cells["n"])
    order = np.argsort(raw["keys"], kind="stable")
    assert all(np.array_equal(raw[k][order], want[k]) for k in ("keys", "n", "S", "windows", "stamp"))
    assert never_grew(dense19, lc.BIG_LOG2)


def test_import_walks_two_rounds(ctx):
    state = lc.dense_reference().export_state()
    assert len(state["keys"]) == lc.DENSE_CELLS > lc.ROUND and lc.DENSE_CELLS % 256
    # into an empty map: the state comes back
    wm, rm = d.WorldMap(ctx, lc.LEAF, 8), mref.MergeReferenceMap(lc.LEAF)
    before = wm.info()
    info = wm.importState(state)
    assert check_merge_info(info, rm.import_state(state), before, wm.info()) == 11 and info["n_new"] == lc.DENSE_CELLS
    mref.assert_states_equal(wm.exportState(), state)
    check_state(wm, rm)
    wm.close()
    # into a map that holds other cells, some of them the state's
    wm, rm = build(ctx, lc.sparse_calls(), lc.LEAF, 8), lc.fresh(lc.sparse_reference())
    before = wm.info()
    info = wm.importState(state)
    check_merge_info(info, rm.import_state(state), before, wm.info())
    assert info["n_common"] >= 2000 and info["n_new"] >= lc.ROUND
    check_state(wm, rm)
    wm.close()


def test_import_refuses_bad_cells_of_the_second_round(ctx):
    whole = lc.dense_reference().export_state()
    dst = build(ctx, lc.sparse_calls()[:1], lc.LEAF, 8)
    rd = mref.reference_of(lc.sparse_calls()[:1], lc.LEAF)
    before, info_before = dst.exportState(), dst.info()
    states = lc.second_round_bad_states(whole)
    assert [c for c, _, _ in states] == [0, 1, 2, 3, 4, 5]
    for counter, word, state in states:
        assert refusal(lambda: dst.importState(state), word) == len(lc.BAD_INDICES), counter
        with pytest.raises(mref.Refused) as e:
            rd.import_state(state)
        assert e.value.args[0] == word, counter
        assert dst.info() == info_before
        mref.assert_states_equal(dst.exportState(), before)
    check_state(dst, rd)
    dst.close()


def test_merge_walks_two_rounds(ctx, dense19):
    dense_ref = lc.dense_reference()
    # a small map into the dense one: one round over the source, every find-or-claim in the big table
    small, rs = build(ctx, lc.sparse_calls(), lc.LEAF, 8), lc.fresh(lc.sparse_reference())
    big, rb = build(ctx, lc.dense_calls(), lc.LEAF, lc.BIG_LOG2), lc.fresh(dense_ref)
    before = big.info()
    info = big.merge(small)
    assert check_merge_info(info, rb.merge(rs), before, big.info()) == 0 and never_grew(big, lc.BIG_LOG2)
    assert info["n_common"] >= 2000 and info["n_new"] >= 2000
    check_state(big, rb)
    big.close()
    # the dense map into the small one, which grows: two rounds over the source
    before = small.info()
    info = small.merge(dense19)
    assert check_merge_info(info, rs.merge(dense_ref), before, small.info()) >= 4
    assert info["n_common"] >= 2000 and info["n_new"] >= lc.ROUND and info["n_src_cells"] == lc.DENSE_CELLS
    check_state(small, rs)
    mref.assert_states_equal(dense19.exportState(), dense_ref.export_state())           # the source is unchanged
    small.close()


# ---- part B: probe runs that cross the table's end ----

def chain_map(ctx, name, calls=("first", "again")):
    """the chain on the device and in the restatement; the table has not grown, so the run of test_map_layouts_cpu.py exists"""
    ch = lc.chain(name)
    wm, rm = d.WorldMap(ctx, lc.CHAIN_LEAF, ch["log2"]), mref.MergeReferenceMap(lc.CHAIN_LEAF)
    for k in calls:
        assert wm.integrate(*ch[k]) == rm.integrate(*ch[k]) == 0
        assert never_grew(wm, ch["log2"])
    return ch, wm, rm


def small_map(ctx, calls, log2=8):
    wm, rm = d.WorldMap(ctx, lc.CHAIN_LEAF, log2), mref.MergeReferenceMap(lc.CHAIN_LEAF)
    for pts, T in calls:
        assert wm.integrate(pts, T) == rm.integrate(pts, T) == 0
    return wm, rm


CHAIN_NAMES = list(lc.CHAINS)


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_integrate_extract_and_count(ctx, name):
    ch, wm, rm = chain_map(ctx, name, ("first",))
    assert wm.info()["occupied"] == len(ch["cells"])
    ref.assert_maps_equal(wm.extract(), rm.extract())
    # the second call finds 40 of the cells again, far along the run, and claims the slots after it for new ones
    assert wm.integrate(*ch["again"]) == rm.integrate(*ch["again"]) == 0
    assert never_grew(wm, ch["log2"])
    for mp, mw in ((0, 0), (1, 1), (2, 1), (2, 2), (3, 1)):
        want = rm.extract(mp, mw)
        ref.assert_maps_equal(wm.extract(mp, mw), want)
        assert wm.count(mp, mw) == len(want["keys"])
    assert wm.count(2, 2) >= 40
    check_state(wm, rm)
    wm.close()


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_compare(ctx, name):
    ch, wm, rm = chain_map(ctx, name)
    shifted, rs = small_map(ctx, ch["other_calls"])
    mine, theirs = rm.extract(), rs.extract()
    itself = wm.compare(wm, lc.CHAIN_RADIUS, eref.N_BINS, distances=True)
    eref.assert_compares_equal(itself, eref.compare(mine, mine, lc.CHAIN_LEAF, lc.CHAIN_RADIUS, eref.N_BINS))
    assert itself["n_matched"] == len(mine["keys"]) and not itself["dist"].any()
    for a, b, ca, cb in ((shifted, wm, theirs, mine), (wm, shifted, mine, theirs)):
        for radius, filters in ((lc.CHAIN_RADIUS, {}), (0.5, dict(min_points_other=2))):
            got = a.compare(b, radius, eref.N_BINS, distances=True, **filters)
            cb_f = cb if not filters else (rm if b is wm else rs).extract(2, 1)
            eref.assert_compares_equal(got, eref.compare(ca, cb_f, lc.CHAIN_LEAF, radius, eref.N_BINS))
            if a is shifted and not filters:                                    # (what test_map_layouts_cpu.py looked into)
                assert got["n_matched"] >= 30 and got["n_unmatched"] >= 30
    assert never_grew(wm, ch["log2"])
    wm.close()
    shifted.close()


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_prune(ctx, name):
    ch, wm, rm = chain_map(ctx, name)
    want = classified(rm, **lc.CHAIN_PRUNE)
    assert want["n_kept"] >= 30 and want["n_removed"][4] >= 20
    check_classify(wm, want)
    check_classify(wm, classified(rm, min_points=2, reach=2, min_neighbors=2))
    ref.assert_maps_equal(wm.extract(), rm.extract())                          # a dry run changes nothing
    # the prune rebuilds the table at its size: the kept cells of the chain form a run across the end again
    twin, rt = chain_map(ctx, name)[1:]
    for m, r, shrink in ((wm, rm, False), (twin, rt, True)):
        before = m.info()
        info, out = m.prune(shrink=shrink, **lc.CHAIN_PRUNE), r.prune(**lc.CHAIN_PRUNE)
        assert (info["n_cells"], info["n_kept"], info["n_removed"]) == (out["n_cells"], out["n_kept"], out["n_removed"])
        assert info["capacity"] == m.info()["capacity"] == (pref.shrunk_capacity(info["n_kept"]) if shrink else before["capacity"])
        assert m.info()["growths"] == 0
        check_state(m, r)
        check_classify(m, classified(r, **lc.CHAIN_PRUNE))                      # and support is looked up in the rebuilt table
        m.close()


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_align_step(ctx, name):
    ch, wm, rm = chain_map(ctx, name)
    shifted, rs = small_map(ctx, ch["other_calls"])
    mine, theirs = rm.extract(), rs.extract()
    T = np.array([1, 0, 0, 0.05, 0, 1, 0, -0.03, 0, 0, 1, 0.02], np.float64)
    for a, b, ca, cb in ((shifted, wm, theirs, mine), (wm, shifted, mine, theirs), (wm, wm, mine, mine)):
        got = a.alignStep(b, lc.CHAIN_RADIUS, T, correspondences=True)
        ar.assert_steps_equal(got, ar.step(ca, cb, lc.CHAIN_LEAF, lc.CHAIN_RADIUS, T))
        fetched = a.fetchAlignment()
        assert all(np.array_equal(fetched[k].view(np.uint32), got[k].view(np.uint32)) for k in fetched)
        assert got["n_matched"] >= 10 and (a is not b or got["n_matched"] == len(mine["keys"]))
    wm.close()
    shifted.close()


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_integrate_map(ctx, name):
    ch, wm, rm = chain_map(ctx, name)
    guest, rg = small_map(ctx, ch["guest_calls"])
    # out of the chain: into a fresh map that grows, and into a fresh table of the chain's size (a run across the end again)
    for log2 in (8, ch["log2"]):
        dst, rd = small_map(ctx, [ch["guest_calls"][1]], log2)
        for mp, mw in ((1, 1), (2, 1)):
            n, rej = dst.integrateMap(wm, IDENTITY, mp, mw)
            assert (n, rej) == ar.integrate_map(rd, rm, IDENTITY, mp, mw) and n == wm.count(mp, mw) > 0 and rej == 0
        check_state(dst, rd)
        dst.close()
    # into the chain: cells it holds are found along the run, new ones with a home in the tail are claimed at its end
    n, rej = wm.integrateMap(guest, IDENTITY)
    assert (n, rej) == ar.integrate_map(rm, rg, IDENTITY) and n == len(rg.keys) and rej == 0
    assert never_grew(wm, ch["log2"])
    check_state(wm, rm)
    ref.assert_maps_equal(wm.extract(), rm.extract())
    wm.close()
    guest.close()


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_merge(ctx, name):
    ch, wm, rm = chain_map(ctx, name)
    guest, rg = small_map(ctx, ch["guest_calls"])
    # out of the chain: into an empty table of the chain's size, and into a map that shares cells with it and grows
    for dst, rd in ((d.WorldMap(ctx, lc.CHAIN_LEAF, ch["log2"]), mref.MergeReferenceMap(lc.CHAIN_LEAF)),
                    small_map(ctx, ch["other_calls"][:1] + ch["guest_calls"])):
        before = dst.info()
        info = dst.merge(wm)
        check_merge_info(info, rd.merge(rm), before, dst.info())
        assert info["n_new"] >= 50
        check_state(dst, rd)
        dst.close()
    # into the chain
    before = wm.info()
    info = wm.merge(guest)
    assert check_merge_info(info, rm.merge(rg), before, wm.info()) == 0 and never_grew(wm, ch["log2"])
    assert info["n_common"] >= 20 and info["n_new"] == 10
    check_state(wm, rm)
    ref.assert_maps_equal(wm.extract(), rm.extract())
    wm.close()
    guest.close()


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_export_and_import(ctx, name):
    ch, wm, rm = chain_map(ctx, name)
    state = wm.exportState()
    mref.assert_states_equal(state, rm.export_state())
    raw = wm.exportState(sort=False)
    assert np.array_equal(raw["keys"], wm.extract(0, 0, sort=False)["keys"])
    # the state into an empty table of the chain's size: the run is built once more, by the import and by its merge
    back, rb = d.WorldMap(ctx, lc.CHAIN_LEAF, ch["log2"]), mref.MergeReferenceMap(lc.CHAIN_LEAF)
    before = back.info()
    info = back.importState(raw)
    assert check_merge_info(info, rb.import_state(raw), before, back.info()) == 0
    mref.assert_states_equal(back.exportState(), state)
    # a guest's state into the chain itself
    guest = mref.reference_of(ch["guest_calls"], lc.CHAIN_LEAF).export_state()
    before = wm.info()
    info = wm.importState(guest)
    assert check_merge_info(info, rm.import_state(guest), before, wm.info()) == 0 and info["n_common"] >= 20
    check_state(wm, rm)
    # a state that repeats keys of the chain: the second map_slot finds the first far along the run and counts it.  The
    # import builds its own table of 2^8 slots, so this run is the 2^8 chain's: of any 30 of its cells at most 16 lie in the
    # 16 slots before the table's end
    chain_keys = ref.pack_key(ch["cells"])
    before_state, before_info = back.exportState(), back.info()
    for take in (1, 30):
        bad = lc.duplicated(state, chain_keys, take)
        assert len(bad["keys"]) * 4 <= 3 * 256                                  # the import's own table is 2^8 slots
        for dst, rdst in ((d.WorldMap(ctx, lc.CHAIN_LEAF, 8), mref.MergeReferenceMap(lc.CHAIN_LEAF)), (back, rb)):
            assert refusal(lambda: dst.importState(bad), "keys") == take
            with pytest.raises(mref.Refused) as e:
                rdst.import_state(bad)
            assert e.value.args[0] == "keys"
            if dst is not back:
                assert dst.info()["occupied"] == 0
                dst.close()
    assert back.info() == before_info
    mref.assert_states_equal(back.exportState(), before_state)
    back.close()
    wm.close()


# ---- part C: one map, five layouts ----

@pytest.fixture(scope="module")
def layouts(ctx):
    """the sparse scene's five calls in five tables"""
    calls, cells = lc.sparse_calls(), len(lc.sparse_reference().keys)
    maps = {"grown from 2^8": build(ctx, calls, lc.LEAF, 8), "2^16": build(ctx, calls, lc.LEAF, 16),
            "2^19": build(ctx, calls, lc.LEAF, 19), "2^20": build(ctx, calls, lc.LEAF, 20), "2^19 shrunk": build(ctx, calls, lc.LEAF, 19)}
    assert tuple(maps) == lc.LAYOUTS
    info = maps["2^19 shrunk"].prune(shrink=True)                               # the defaults remove nothing
    assert info["n_kept"] == cells and info["capacity"] == pref.shrunk_capacity(cells) < 1 << 16
    capacities = [m.info()["capacity"] for m in maps.values()]
    assert capacities == [lc.grown_from(calls, lc.LEAF, 8), 1 << 16, 1 << 19, 1 << 20, pref.shrunk_capacity(cells)]
    assert maps["grown from 2^8"].info()["growths"] >= 5 and all(maps[k].info()["growths"] == 0 for k in lc.LAYOUTS[1:])
    yield maps
    for m in maps.values():
        m.close()


_wanted = {}


def wanted(what, make):
    """a restatement's result, computed once and shared by the five layouts (never changed)"""
    if what not in _wanted:
        _wanted[what] = make()
    return _wanted[what]


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_layout_extract_count_and_export(layouts, layout):
    wm, rm = layouts[layout], lc.sparse_reference()
    for mp, mw in lc.EXTRACT_FILTERS:
        want = wanted(("extract", mp, mw), lambda: rm.extract(mp, mw))
        ref.assert_maps_equal(wm.extract(mp, mw), want)
        assert wm.count(mp, mw) == len(want["keys"]) > 0
    check_state(wm, rm)
    raw = wm.exportState(sort=False)
    assert np.array_equal(raw["keys"], wm.extract(0, 0, sort=False)["keys"])


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_layout_render(layouts, layout):
    for splat, mw in lc.RENDER_CASES[1:3]:
        rref.assert_renders_equal(layouts[layout].render(*lc.SMALL_VIEW, splat=splat, min_windows=mw), lc.sparse_render("small", splat, mw))


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_layout_compare_both_ways(layouts, other, layout):
    wm, radius = layouts[layout], eref.RADII[1]
    eref.assert_compares_equal(wm.compare(other, radius, eref.N_BINS, distances=True), lc.sparse_compare(True, radius))
    eref.assert_compares_equal(other.compare(wm, radius, eref.N_BINS, distances=True), lc.sparse_compare(False, radius))
    filtered = wanted("compare filtered", lambda: eref.compare(lc.sparse_reference().extract(2, 2), lc.other_reference().extract(1, 2),
                                                                lc.LEAF_B, radius, eref.N_BINS))
    got = wm.compare(other, radius, eref.N_BINS, min_points=2, min_windows=2, min_windows_other=2, distances=True)
    eref.assert_compares_equal(got, filtered)


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_layout_prune_classify(layouts, layout):
    want = wanted("classify", lambda: classified(lc.sparse_reference(), **lc.SPARSE_PRUNE))
    assert want["n_kept"] >= 100 and min(want["n_removed"]) >= 100
    check_classify(layouts[layout], want)


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_layout_align_step(layouts, other, layout):
    wm = layouts[layout]
    mine, theirs = wanted(("extract", 1, 1), lambda: lc.sparse_reference().extract()), lc.other_reference().extract()
    fwd = wanted("align forward", lambda: ar.step(mine, theirs, lc.LEAF_B, lc.ALIGN_RADIUS, lc.ALIGN_POSE))
    bwd = wanted("align backward", lambda: ar.step(theirs, mine, lc.LEAF, lc.ALIGN_RADIUS, lc.ALIGN_POSE))
    assert min(fwd["n_matched"], fwd["n_unmatched"], bwd["n_matched"], bwd["n_unmatched"]) >= 100
    ar.assert_steps_equal(wm.alignStep(other, lc.ALIGN_RADIUS, lc.ALIGN_POSE, correspondences=True), fwd)
    ar.assert_steps_equal(other.alignStep(wm, lc.ALIGN_RADIUS, lc.ALIGN_POSE, correspondences=True), bwd)


def _integrated():
    rd = mref.MergeReferenceMap(lc.LEAF_B)
    counts = [ar.integrate_map(rd, lc.sparse_reference(), T, mp, mw) for T, mp, mw in ((lc.ALIGN_POSE, 1, 1), (IDENTITY, 2, 2))]
    return counts, rd


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_layout_integrate_map_into_a_fresh_map(ctx, layouts, layout):
    counts, rd = wanted("integrate map", _integrated)
    dst = d.WorldMap(ctx, lc.LEAF_B, 8)
    got = [dst.integrateMap(layouts[layout], T, mp, mw) for T, mp, mw in ((lc.ALIGN_POSE, 1, 1), (IDENTITY, 2, 2))]
    assert got == counts and counts[0][0] > counts[1][0] > 100
    check_state(dst, rd)
    dst.close()
