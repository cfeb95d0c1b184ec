"""Merging world maps and moving their state (dsx_map_export / import / merge, engine.WorldMap.exportState / importState /
merge, process.merge_world_maps; DESIGN.md 7j "Merging") on the MI355X against the numpy restatement of
tests/map_merge_reference.py.  Every comparison is array_equal: the cells through world_map_reference.assert_maps_equal,
the counters through info(), the stamps through classifyPrune(max_age=a) at every age that occurs, and the raw state --
which only the export shows -- array by array."""
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_merge_reference as mref
import map_prune_reference as pref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = pref.IDENTITY
PRUNE = dict(min_points=2, reach=1, min_neighbors=2)
VIEW = (E.pose_matrix([0, 0, 2.0, 0, 0, 0, 1]), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 6.0)


@pytest.fixture(scope="module")
def scene():
    calls = pref.scene_calls()
    return calls, mref.reference_of(calls)


def both(ctx, calls, capacity_log2=10, leaf=pref.LEAF):
    """the calls through a WorldMap and through the restatement: (map, reference map)"""
    wm, rm = d.WorldMap(ctx, leaf, capacity_log2), mref.MergeReferenceMap(leaf)
    for pts, T in calls:
        assert wm.integrate(pts, T) == rm.integrate(pts, T)
    return wm, rm


def check_stamps(wm, rm):
    """the stamps through criterion 3 of the prune at every age that occurs (test_gpu_map_prune.check_stamps)"""
    for age in range(int(rm.calls) + 1):
        info, want = wm.classifyPrune(max_age=age), rm.classify(max_age=age)
        assert (info["n_kept"], info["n_removed"]) == (want["n_kept"], want["n_removed"]), age
        got = wm.fetchPruneReasons()
        assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["reason"], want["reason"]), age


def check_map(wm, rm, stamps=True):
    """cells, counters, raw state and stamps of the device map equal the restatement's"""
    ref.assert_maps_equal(wm.extract(), rm.extract())
    info = wm.info()
    assert (info["occupied"], info["calls"], info["accepted"], info["rejected"]) == (len(rm.keys), rm.calls, rm.accepted, rm.rejected)
    mref.assert_states_equal(wm.exportState(), rm.export_state())
    if stamps:
        check_stamps(wm, rm)


def check_info(info, want, before, after):
    """a merge's counts equal the restatement's; growths and capacity are the 3/4 rule's"""
    assert {k: info[k] for k in want} == want, (info, want)
    cap, g = mref.grown_capacity(before["capacity"], before["occupied"], want["n_src_cells"])
    assert (info["capacity"], info["growths"]) == (cap, g) and after["capacity"] == cap and after["growths"] == before["growths"] + g
    assert after["occupied"] == before["occupied"] + want["n_new"]


def merged(dst, dst_ref, src, src_ref, how="merge"):
    before = dst.info()
    info = dst.merge(src) if how == "merge" else dst.importState(src.exportState(sort=how == "sorted"))
    check_info(info, dst_ref.merge(src_ref), before, dst.info())
    return info


def refused(fn, code=E.ERR_INVALID, word=None):
    with pytest.raises(d.DsiError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert word is None or word + ": " in str(e.value), (word, str(e.value))   # the message begins with the offending thing
    return True


@pytest.mark.parametrize("cut", [0, 3, 5, 8])
def test_append(ctx, scene, cut):
    calls, whole_ref = scene
    whole, _ = both(ctx, calls)
    a, ra = both(ctx, calls[:cut])
    b, rb = both(ctx, calls[cut:])
    b_before = b.exportState()
    info = merged(a, ra, b, rb)
    if 0 < cut < 8:
        assert info["n_new"] >= 100 and info["n_common"] >= 400
    check_map(a, ra)                                                           # equals the restatement ...
    mref.assert_states_equal(a.exportState(), whole_ref.export_state())        # ... which equals the single map's
    mref.assert_states_equal(a.exportState(), whole.exportState())             # ... as does the device's single map
    ref.assert_maps_equal(a.extract(), whole.extract())
    mref.assert_states_equal(b.exportState(), b_before)                        # the source is unchanged
    for m in (whole, a, b):
        m.close()


def test_export(ctx, scene):
    calls, whole_ref = scene
    wm, rm = both(ctx, calls)
    r0 = wm.render(*VIEW)
    c0 = wm.compare(wm, 0.05, distances=True)
    p0 = wm.classifyPrune(**pref.SCENE_OPTS)
    v0 = wm.fetchPruneReasons()
    before = wm.info()
    got, want = wm.exportState(), rm.export_state()
    assert len(got["keys"]) == 1640 and got["S"].shape == (1640, 3)
    for k in ("keys", "n", "S", "windows", "stamp"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert (got["leaf"], got["calls"], got["accepted"], got["rejected"]) == (pref.LEAF, 8, rm.accepted, rm.rejected)
    assert got["stamp"].min() >= 1 and len(np.unique(got["stamp"])) >= 4 and got["S"].max() > 1 << 32
    # the table's order is extract(sort=False)'s
    raw, cells = wm.exportState(sort=False), wm.extract(0, 0, sort=False)
    assert np.array_equal(raw["keys"], cells["keys"]) and np.array_equal(raw["n"], cells["n"]) and not np.array_equal(raw["keys"], got["keys"])
    # nothing changed, nothing was invalidated
    assert wm.info() == before
    r1, c1, v1 = wm.fetchRender(), wm.fetchDistances(), wm.fetchPruneReasons()
    assert all(np.array_equal(r0[k], r1[k]) for k in r1) and all(np.array_equal(c0[k], c1[k]) for k in c1)
    assert all(np.array_equal(v0[k], v1[k]) for k in v1) and p0["n_cells"] == 1640
    # the capacity protocol: too small writes nothing and names the count; any array may be NULL
    L = d.load_library()
    m = 1640
    keys, n, S = np.full(m, 99, np.uint64), np.full(m, 77, np.uint32), np.full((m, 3), 55, np.uint64)
    st, cnt = E._MapState(), C.c_size_t()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = L.dsx_map_export(wm._h, C.byref(st), p(keys, C.c_uint64), p(n, C.c_uint32), p(S, C.c_uint64), None, None, m - 1, C.byref(cnt))
    assert rc == E.ERR_INVALID and cnt.value == m and (keys == 99).all() and (n == 77).all() and (S == 55).all()
    assert (st.leaf, st.n_cells, st.calls, st.accepted, st.rejected) == (pref.LEAF, m, 8, rm.accepted, rm.rejected)   # always filled
    assert L.dsx_map_export(wm._h, None, None, None, p(S, C.c_uint64), None, None, m, C.byref(cnt)) == E.OK
    assert (keys == 99).all() and np.array_equal(S, raw["S"])
    stamp = np.zeros(m + 5, np.uint32)
    assert L.dsx_map_export(wm._h, None, None, None, None, None, p(stamp, C.c_uint32), m + 5, C.byref(cnt)) == E.OK and cnt.value == m
    assert np.array_equal(stamp[:m], raw["stamp"]) and (stamp[m:] == 0).all()
    # an empty map
    empty = d.WorldMap(ctx, 0.5, 8)
    e = empty.exportState()
    assert len(e["keys"]) == 0 and e["S"].shape == (0, 3) and (e["calls"], e["accepted"], e["rejected"]) == (0, 0, 0)
    empty.close()
    wm.close()


@pytest.mark.parametrize("capacity_log2", [8, 16])
def test_round_trip(ctx, scene, capacity_log2):
    calls, whole_ref = scene
    src, rs = both(ctx, calls)
    state = src.exportState()
    wm, rm = d.WorldMap(ctx, pref.LEAF, capacity_log2), mref.MergeReferenceMap(pref.LEAF)
    before = wm.info()
    info = wm.importState(state)
    check_info(info, rm.import_state(state), before, wm.info())
    assert info["n_new"] == 1640 and info["growths"] == (4 if capacity_log2 == 8 else 0)
    mref.assert_states_equal(wm.exportState(), state)
    check_map(wm, rs)
    pts = calls[0][0][::-1]                                                    # an integrate call goes on exactly as on the source
    assert wm.integrate(pts, IDENTITY) == src.integrate(pts, IDENTITY) == rs.integrate(pts, IDENTITY)
    check_map(wm, rs)
    mref.assert_states_equal(wm.exportState(), src.exportState())
    src.close()
    wm.close()


def test_table_and_order_freedom(ctx, scene):
    calls, whole_ref = scene
    rng = np.random.default_rng(9)
    states = []
    for dst_log2 in (8, 16):
        for src_log2 in (8, 16):
            shuffled = [(p[rng.permutation(len(p))], T) for p, T in calls]
            a, ra = both(ctx, shuffled[:3], capacity_log2=dst_log2)
            b, rb = both(ctx, shuffled[3:], capacity_log2=src_log2)
            info = merged(a, ra, b, rb)
            assert info["capacity"] == (1 << 16 if dst_log2 == 16 else 1 << 12), info     # 1,640 cells: 2^12 slots at 3/4 load
            states.append(a.exportState())
            mref.assert_states_equal(states[-1], whole_ref.export_state())
            c, rc = both(ctx, shuffled[:3], capacity_log2=dst_log2)            # the same through the host arrays, unsorted
            merged(c, rc, b, rb, how="unsorted")
            mref.assert_states_equal(c.exportState(), states[0])
            for m in (a, b, c):
                m.close()
    assert all(np.array_equal(s[k], states[0][k]) for s in states for k in ("keys", "n", "S", "windows", "stamp"))


def test_two_contexts_on_one_gpu(ctx, scene):
    calls, whole_ref = scene
    other = d.Context(0)
    a, ra = both(ctx, calls[:5])
    b, rb = both(other, calls[5:], capacity_log2=8)
    before = a.exportState()
    refused(lambda: a.merge(b), E.ERR_CONTEXT, "contexts")
    mref.assert_states_equal(a.exportState(), before)
    infos = proc.merge_world_maps(a, [b])                                      # export -> import
    same, rsame = both(ctx, calls[:5])
    on_ctx, _ = both(ctx, calls[5:])
    assert proc.merge_world_maps(same, [on_ctx])[0]["n_new"] == infos[0]["n_new"] > 100   # the device merge
    mref.assert_states_equal(a.exportState(), same.exportState())
    ra.merge(rb)
    check_map(a, ra)
    mref.assert_states_equal(a.exportState(), whole_ref.export_state())
    for m in (a, b, same, on_ctx):
        m.close()
    other.close()


def test_round_robin_over_three_maps(ctx, scene):
    calls, whole_ref = scene
    maps = [d.WorldMap(ctx, pref.LEAF, 8 + 4 * k) for k in range(3)]
    refs = [mref.MergeReferenceMap(pref.LEAF) for _ in range(3)]
    for k, (pts, T) in enumerate(calls):
        assert maps[k % 3].integrate(pts, T) == refs[k % 3].integrate(pts, T)
    infos = proc.merge_world_maps(maps[0], maps[1:])
    for info, r in zip(infos, refs[1:]):
        want = refs[0].merge(r)
        assert {k: info[k] for k in want} == want
    check_map(maps[0], refs[0])
    got, want = maps[0].exportState(), whole_ref.export_state()
    assert all(np.array_equal(got[k], want[k]) for k in ("keys", "n", "S", "windows"))      # the single map's, but for the stamps
    assert all(got[k] == want[k] for k in ("calls", "accepted", "rejected")) and not np.array_equal(got["stamp"], want["stamp"])
    ref.assert_maps_equal(maps[0].extract(), whole_ref.extract())
    for m in maps:
        m.close()


def test_pruned_maps(ctx, scene):
    calls, _ = scene
    a, ra = both(ctx, calls[:3])
    b, rb = both(ctx, calls[3:6])
    for m, r in ((a, ra), (b, rb)):
        info, want = m.prune(shrink=True, **PRUNE), r.prune(**PRUNE)
        assert info["n_kept"] == want["n_kept"] >= 100 and sum(info["n_removed"]) >= 100
    merged(a, ra, b, rb)
    check_map(a, ra)
    # a pruned dst followed by the merge of an unpruned src equals the pruned map followed by src's calls
    c, rc = both(ctx, calls[:3])
    c.prune(**PRUNE), rc.prune(**PRUNE)
    follow = mref.reference_of(calls[:3])
    follow.prune(**PRUNE)
    for pts, T in calls[3:6]:
        follow.integrate(pts, T)
    e, re_ = both(ctx, calls[3:6])
    merged(c, rc, e, re_)
    mref.assert_states_equal(c.exportState(), follow.export_state())
    for pts, T in calls[6:]:                                                   # a further integrate call
        assert a.integrate(pts, T) == ra.integrate(pts, T)
    check_map(a, ra)
    for m in (a, b, c, e):
        m.close()


def test_empty_maps(ctx, scene):
    calls, whole_ref = scene
    a, ra = both(ctx, calls)
    empty, rempty = both(ctx, [calls[2]] * 3, capacity_log2=8)
    assert empty.info()["occupied"] == 0 and empty.info()["calls"] == 3
    info = merged(a, ra, empty, rempty)
    assert (info["n_src_cells"], info["n_new"], info["n_common"], info["growths"]) == (0, 0, 0, 0)
    assert a.info()["calls"] == 11 and a.classifyPrune(max_age=2)["n_kept"] == 0 and a.classifyPrune(max_age=3)["n_kept"] > 0
    check_map(a, ra)                                                           # every cell is three calls older
    fresh, rfresh = d.WorldMap(ctx, pref.LEAF, 8), mref.MergeReferenceMap(pref.LEAF)
    merged(fresh, rfresh, a, ra)                                               # an empty dst becomes src
    mref.assert_states_equal(fresh.exportState(), a.exportState())
    check_map(fresh, ra, stamps=False)
    nothing, rnothing = d.WorldMap(ctx, pref.LEAF, 8), mref.MergeReferenceMap(pref.LEAF)
    merged(nothing, rnothing, d.WorldMap(ctx, pref.LEAF, 8), mref.MergeReferenceMap(pref.LEAF))
    check_map(nothing, rnothing)
    for m in (a, empty, fresh, nothing):
        m.close()


def test_refusals(ctx, scene):
    calls, whole_ref = scene
    whole = whole_ref.export_state()
    dst, rd = both(ctx, calls[:3], capacity_log2=8)
    before, info_before = dst.exportState(), dst.info()
    dst.render(*VIEW)

    def unchanged():
        assert dst.info() == info_before
        mref.assert_states_equal(dst.exportState(), before)
        dst.fetchRender()                                                      # not even invalidated

    bad, good = mref.header_states(pref.LEAF, rd.calls, rd.accepted)
    for name, word, state in mref.bad_states(whole) + bad:
        refused(lambda: dst.importState(state), E.ERR_INVALID, word)
        with pytest.raises(mref.Refused) as e:
            rd.import_state(state)
        assert e.value.args[0] == word, name
        unchanged()
    refused(lambda: dst.merge(dst), E.ERR_INVALID, "same map")
    other_leaf = d.WorldMap(ctx, float(np.nextafter(pref.LEAF, 1.0)), 8)
    refused(lambda: dst.merge(other_leaf), E.ERR_INVALID, "leaf")
    unchanged()
    with pytest.raises(ValueError):
        dst.importState(dict(whole, n=whole["n"][:-1]))
    # the counter bounds of a device merge, reached through a map that imported a large header
    full = d.WorldMap(ctx, pref.LEAF, 8)
    full.importState(dict(good[0], calls=mref.U32_MAX - rd.calls + 1, accepted=0))
    refused(lambda: dst.merge(full), E.ERR_INVALID, "calls")
    full.reset()
    full.importState(dict(good[0], calls=0, accepted=mref.U32_MAX - rd.accepted + 1))
    refused(lambda: dst.merge(full), E.ERR_INVALID, "accepted")
    unchanged()
    check_map(dst, rd)
    # the bounds themselves are legal: 2^32 - 1 calls and accepted points, after which an integrate call is refused
    dst.importState(good[0])
    rd.import_state(good[0])
    check_map(dst, rd, stamps=False)
    assert dst.info()["calls"] == mref.U32_MAX == dst.info()["accepted"]
    refused(lambda: dst.integrate(calls[0][0], IDENTITY))
    for m in (dst, other_leaf, full):
        m.close()


def test_invalidation(ctx, scene):
    calls, _ = scene
    a, ra = both(ctx, calls[:4])
    b, rb = both(ctx, calls[4:])
    for m in (a, b):
        m.render(*VIEW)
        m.compare(m, 0.05, distances=True)
        m.classifyPrune(**PRUNE)
    kept = (b.fetchRender(), b.fetchDistances(), b.fetchPruneReasons())
    merged(a, ra, b, rb)
    assert refused(a.fetchRender) and refused(a.fetchDistances) and refused(a.fetchPruneReasons)
    for was, now in zip(kept, (b.fetchRender(), b.fetchDistances(), b.fetchPruneReasons())):
        assert all(np.array_equal(was[k], now[k]) for k in was)
    a.render(*VIEW)                                                            # and an import invalidates as a merge does
    a.importState(b.exportState())
    assert refused(a.fetchRender)
    a.close()
    b.close()


def test_growth_at_scale(ctx):
    n = 20000
    idx = np.arange(n)
    cells = np.stack([idx % 40 - 20, (idx // 40) % 40 - 20, idx // 1600 - 6], axis=1)
    rng = np.random.default_rng(3)
    pts = ((cells + rng.uniform(0.1, 0.9, (n, 3))) * 0.5).astype(np.float32)
    pts = pts[rng.permutation(n)]
    dst, rd = both(ctx, [(pts[:100], IDENTITY)], capacity_log2=8, leaf=0.5)
    src, rs = both(ctx, [(pts[50:12000], IDENTITY), (pts[8000:], IDENTITY)], capacity_log2=8, leaf=0.5)
    assert src.info()["occupied"] == n - 50 and src.info()["capacity"] == 1 << 15
    info = merged(dst, rd, src, rs)
    assert (info["n_new"], info["n_common"], info["capacity"], info["growths"]) == (n - 100, 50, 1 << 15, 7)
    check_map(dst, rd)
    back = d.WorldMap(ctx, 0.5, 8)                                             # and through the host arrays, from 2^8 slots
    assert back.importState(dst.exportState(sort=False))["growths"] == 7
    mref.assert_states_equal(back.exportState(), rd.export_state())
    for m in (dst, src, back):
        m.close()


def test_two_streams_merged_equal_the_whole_run(ctx):
    """full_sequence(..., world_map=) on the rig of test_gpu_world_map's stream test: the first two windows into one map,
    the last two into a map on a second context; merged, they equal the map of the whole run, stamps included."""
    n_win, dur, t0 = 4, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    kw = dict(options_depth_map=d.OptionsDepthMap(), options_point_cloud=d.OptionsPointCloud(2.0, 1))
    stop = t0 + n_win * dur + 1e-9
    bounds = proc.window_bounds(t0, stop, dur, dur)
    assert len(bounds) == n_win
    mid = bounds[2][0]                                                         # the third window's start, as the loop computes it
    other = d.Context(0)
    whole, first, rest = d.WorldMap(ctx, 0.5, 8), d.WorldMap(ctx, 0.5, 8), d.WorldMap(other, 0.5, 8)
    run = lambda c, a, b, wm: list(proc.full_sequence(c, (cam, cam), shape, rig["events"], rig["trajectories"], a, b, dur, dur,
                                                      world_map=wm, **kw))
    all_w, w1, w2 = run(ctx, t0, stop, whole), run(ctx, t0, mid + 1e-9, first), run(other, mid, stop, rest)
    assert [w[0] for w in w1 + w2] == [w[0] for w in all_w] and len(w1) == len(w2) == 2
    for a, b in zip(w1 + w2, all_w):
        assert np.array_equal(a[4].view(np.uint8), b[4].view(np.uint8))        # the same clouds went in
    assert first.info()["calls"] == rest.info()["calls"] == 2 and rest.info()["occupied"] > 20
    info = proc.merge_world_maps(first, [rest])[0]
    assert info["n_src_cells"] == rest.info()["occupied"] and info["n_common"] >= 1
    mref.assert_states_equal(first.exportState(), whole.exportState())
    ref.assert_maps_equal(first.extract(), whole.extract())
    assert all(first.info()[k] == whole.info()[k] for k in ("occupied", "calls", "accepted", "rejected"))
    for age in range(n_win + 1):
        assert first.classifyPrune(max_age=age) == dict(whole.classifyPrune(max_age=age), capacity=first.info()["capacity"])
        x, y = first.fetchPruneReasons(), whole.fetchPruneReasons()
        assert np.array_equal(x["keys"], y["keys"]) and np.array_equal(x["reason"], y["reason"])
    for m in (whole, first, rest):
        m.close()
    other.close()
