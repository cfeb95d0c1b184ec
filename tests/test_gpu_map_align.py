"""Aligning world maps on the device (include/dsi_map_align.h; DESIGN.md 7j "Aligning") against the restatement in
tests/map_align_reference.py: the exact integer moments and the correspondences of a pass, hand cases on a lattice, the
ICP loop round by round, one map integrated into another, the fetch protocol and process.score_world_map_3d(align=).
Every comparison is for equality; the distances and poses are compared by their bits.
NOT tested, here or in test_map_align_cpu.py: the refusal of a map whose table overflowed in an earlier call.  That state
follows only a table-full count from a kernel, which the host's sizing of the table rules out (it is reported as an engine
bug), and dsx_map_import validates what it takes: no public call sequence reaches it."""
import ctypes as C
import math

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_align_reference as ar
import map_eval_reference as mref
import map_merge_reference as merge_ref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = ar.IDENTITY


def code_of(fn):
    try:
        fn()
    except d.DsiError as e:
        return e.code
    return E.OK


def build(ctx, leaf, calls, log2=16):
    wm, rm = d.WorldMap(ctx, leaf, log2), merge_ref.MergeReferenceMap(leaf)
    for pts in calls:
        assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY) == 0
    return wm, rm


def check(first, first_cells, second, second_cells, leaf_second, radius, T=IDENTITY, **filters):
    got = first.alignStep(second, radius, T, correspondences=True, **filters)
    want = ar.step(first_cells, second_cells, leaf_second, radius, T)
    ar.assert_steps_equal(got, want)
    return got


@pytest.fixture(scope="module")
def scene1(ctx):
    """(map a, its cells, map b, its cells): leaf 0.05 against leaf 0.04; a's table starts at 2^8 slots"""
    ca, cb = ar.scene1_calls()
    a, ra = build(ctx, ar.LEAF_A, ca, log2=8)
    b, rb = build(ctx, ar.LEAF_B, cb, log2=14)
    ea, eb = ra.extract(), rb.extract()
    ref.assert_maps_equal(a.extract(), ea)
    ref.assert_maps_equal(b.extract(), eb)
    assert (len(ea["keys"]), len(eb["keys"])) == ar.SCENE1_CELLS
    yield a, ea, b, eb
    a.close()
    b.close()


@pytest.mark.parametrize("radius", ar.SCENE1_RADII)
@pytest.mark.parametrize("pose", ["identity", "2 degrees and 0.6 leaf", "far"])
def test_scene_1(scene1, radius, pose):
    a, ea, b, eb = scene1
    T = {"identity": IDENTITY, "2 degrees and 0.6 leaf": ar.T_TRUE_1, "far": ar.T_FAR}[pose]
    got = check(a, ea, b, eb, ar.LEAF_B, radius, T)
    assert got["reach"] == ar.SCENE1_RADII.index(radius) + 1 and got["n_cells"] == len(ea["keys"])
    if pose == "far":
        assert got["n_matched"] == 0 and got["e2"] == 0 and not any(got["su"] + got["sv"] + got["suv_hi"] + got["suv_lo"])
        assert not got["keys_other"].any() and np.isposinf(got["dist"]).all()
    else:
        assert got["n_matched"] >= 1500 and got["n_unmatched"] >= 500


def test_scene_2_many_workgroups_and_products_of_both_signs(ctx):
    """20,000 cells in tables that grow from 2^8 to 2^15 slots: 128 workgroups, one stride each (the second stride is
    test_the_strided_walk's), on both sides of the origin"""
    ca, cb = ar.scene2_calls()
    a, ra = build(ctx, ar.LEAF_A, ca, log2=8)
    b, rb = build(ctx, ar.LEAF_B, cb, log2=8)
    ea, eb = ra.extract(), rb.extract()
    assert len(ea["keys"]) > 19000 and a.info()["capacity"] >= 1 << 15 and a.info()["growths"] >= 7
    for T in (IDENTITY, ar.T_TRUE_2):
        got = a.alignStep(b, 0.08, T, correspondences=True)
        want = ar.step(ea, eb, ar.LEAF_B, 0.08, T)
        ar.assert_steps_equal(got, want)
        assert got["n_matched"] > 19000
        # products of both signs in every entry: the high words of the negative ones are negative (an arithmetic shift),
        # the low words never are, and the two sums put the exact sum together
        P = want["U"][:, :, None] * want["V"][:, None, :]
        assert (P > 0).any(axis=0).all() and (P < 0).any(axis=0).all()
        assert min(got["suv_hi"]) < 0 and min(got["suv_lo"]) > 0 and min(got["su"]) < 0 < max(got["su"])
        total = [hi * (1 << 32) + lo for hi, lo in zip(got["suv_hi"], got["suv_lo"])]
        assert total == [int(v) for v in P.sum(axis=0).reshape(9)] and min(total) < 0 < max(total)
    a.close()
    b.close()


def test_a_map_against_itself(scene1):
    a, ea, _, _ = scene1
    got = check(a, ea, a, ea, ar.LEAF_A, ar.LEAF_A)
    assert got["n_matched"] == got["n_cells"] == len(ea["keys"]) and got["e2"] == 0 and not got["dist"].any()
    assert got["su"] == got["sv"] and np.array_equal(got["keys"], got["keys_other"])
    for k in ("suv_hi", "suv_lo"):
        assert np.array_equal(np.array(got[k], object).reshape(3, 3), np.array(got[k], object).reshape(3, 3).T), k


def test_the_same_maps_built_another_way(ctx, scene1):
    a, ea, b, eb = scene1
    ca, cb = ar.scene1_calls()
    a2, _ = build(ctx, ar.LEAF_A, [np.concatenate(ca[::-1])[::-1]], log2=13)
    b2, _ = build(ctx, ar.LEAF_B, cb[::-1], log2=8)
    for k in ("keys", "xyz", "n"):                                  # (the windows differ: a2 is one call)
        assert np.array_equal(a2.extract()[k], ea[k]), k
    want = a.alignStep(b, 0.08, ar.T_TRUE_1, correspondences=True)
    for first, second in ((a2, b), (a, b2), (a2, b2)):
        ar.assert_steps_equal(first.alignStep(second, 0.08, ar.T_TRUE_1, correspondences=True), want)
    a2.close()
    b2.close()


def test_the_strided_walk(ctx, scene1):
    """2^19 slots are 2048 tiles for at most 1024 workgroups: every workgroup of k_map_align_step and of
    k_map_integrate_map walks two strides (at 2^18 and below, one), so the sums carried in registers over the strides and
    the counts carried over them are compared with the restatement's.  The cells are scene 1's, in a table that never grows."""
    a, ea, b, eb = scene1
    ca, cb = ar.scene1_calls()
    wide, _ = build(ctx, ar.LEAF_A, ca, log2=19)
    assert wide.info()["capacity"] == 1 << 19 and wide.info()["growths"] == 0
    ref.assert_maps_equal(wide.extract(), ea)
    for radius, T in ((0.08, ar.T_TRUE_1), (0.12, IDENTITY), (0.04, ar.T_TRUE_2)):
        got = check(wide, ea, b, eb, ar.LEAF_B, radius, T)
        assert got["n_matched"] >= 1500 and got["n_unmatched"] >= 500
        ar.assert_steps_equal(got, a.alignStep(b, radius, T, correspondences=True))
    # a filter on the walked map, and the wide table as the second map (looked up, not walked)
    want = ar.step(ar.reference_map(ca, ar.LEAF_A).extract(1, 2), eb, ar.LEAF_B, 0.08, ar.T_TRUE_1)
    ar.assert_steps_equal(wide.alignStep(b, 0.08, ar.T_TRUE_1, min_windows=2, correspondences=True), want)
    ar.assert_steps_equal(b.alignStep(wide, 0.1, correspondences=True), ar.step(eb, ea, ar.LEAF_A, 0.1))
    # the loop on it: the same pose and info as on the small table
    T, info = wide.align(b, **ar.SCENE1_LOOP)
    T_small, info_small = a.align(b, **ar.SCENE1_LOOP)
    assert np.array_equal(T, T_small) and info == info_small
    # integrateMap FROM the wide table: the strided walk of k_map_integrate_map
    src_ref = ar.reference_map(ca, ar.LEAF_A)
    for mp, mw, T in ((1, 1, ar.T_TRUE_1), (2, 1, IDENTITY)):
        dst, dst_ref = build(ctx, ar.LEAF_B, [np.float32([[0.01, 0.02, 0.03]])], log2=8)
        n, rej = dst.integrateMap(wide, T, mp, mw)
        assert (n, rej) == ar.integrate_map(dst_ref, src_ref, T, mp, mw) and n == wide.count(mp, mw) and rej == 0
        merge_ref.assert_states_equal(dst.exportState(), dst_ref.export_state())
        dst.close()
    far = IDENTITY.copy()
    far[3] = 1e9
    dst = d.WorldMap(ctx, ar.LEAF_B, 8)
    assert dst.integrateMap(wide, far) == (len(ea["keys"]), len(ea["keys"])) and dst.count() == 0     # the rejected count over two strides
    dst.close()
    wide.close()


def lattice(ctx, leaf, points):
    """a map of single points that are their cells' centroids exactly, and its cells"""
    wm, rm = build(ctx, leaf, [np.float32(points)], log2=8)
    cells = rm.extract()
    assert len(cells["keys"]) == len(points)
    return wm, cells


def test_hand_cases_on_a_lattice(ctx):
    made = []

    def maps(leaf, pa, pb):
        a, ea = lattice(ctx, leaf, pa)
        b, eb = lattice(ctx, leaf, pb)
        made.extend([a, b])
        return a, ea, b, eb

    # p' equidistant from two of b's centroids, and from four: the smaller key wins
    a, ea, b, eb = maps(0.5, [[0.75, 0.25, 0.25]], [[0.25, 0.25, 0.25], [1.25, 0.25, 0.25]])
    r = check(a, ea, b, eb, 0.5, 0.5)
    assert r["n_matched"] == 1 and r["dist"][0] == np.float32(0.5) and r["keys_other"][0] == eb["keys"].min()
    a, ea, b, eb = maps(0.5, [[-0.25, -0.25, 0.25]], [[x, y, 0.25] for x in (-0.75, 0.25) for y in (-0.75, 0.25)])
    r = check(a, ea, b, eb, 0.5, 0.75)
    assert r["reach"] == 2 and r["n_matched"] == 1 and r["dist"][0] == np.float32(math.sqrt(0.5)) and r["keys_other"][0] == eb["keys"].min()
    # the same through a pose: a quarter turn about z and a shift, exact in binary, carry another centroid onto the tie
    quarter = np.array([0, -1, 0, 1.0, 1, 0, 0, -1.0, 0, 0, 1, 0], np.float64)
    a2, ea2 = lattice(ctx, 0.5, [[0.75, 1.25, 0.25]])
    made.append(a2)
    assert ref.world_positions(ea2["xyz"], quarter).tolist() == [[-0.25, -0.25, 0.25]]
    r = check(a2, ea2, b, eb, 0.5, 0.75, quarter)
    assert r["n_matched"] == 1 and r["dist"][0] == np.float32(math.sqrt(0.5)) and r["keys_other"][0] == eb["keys"].min()
    assert check(a2, ea2, b, eb, 0.5, 0.75)["n_matched"] == 0                  # (where it lies it has no partner)
    # d exactly the radius is matched; a radius one ulp below d is not
    a, ea, b, eb = maps(0.5, [[0.25, 0.25, 0.25]], [[0.75, 0.25, 0.25]])
    r = check(a, ea, b, eb, 0.5, 0.5)
    assert r["n_matched"] == 1 and r["e2"] == 1024 ** 2 and r["su"] == [512, 512, 512] and r["sv"] == [1536, 512, 512]
    r = check(a, ea, b, eb, 0.5, float(np.nextafter(0.5, 0.0)))
    assert r["n_matched"] == 0 and r["n_unmatched"] == 1 and np.isposinf(r["dist"][0]) and r["keys_other"][0] == 0
    # a centroid at the edge of the key range: the sweep skips, never wraps, the cells beyond it
    top = float(ref.CELL_MAX)
    hi, ehi, nb, enb = maps(1.0, [[top + 0.5, 0.5, 0.5]], [[top - 0.5, 0.5, 0.5], [-top + 0.5, 0.5, 0.5]])
    r = check(hi, ehi, nb, enb, 1.0, 1.0)
    assert r["n_matched"] == 1 and r["sv"][0] == (ref.CELL_MAX - 1) * 1024 + 512 and r["su"][0] == ref.CELL_MAX * 1024 + 512
    r = check(nb, enb, hi, ehi, 1.0, 3.0)
    assert r["n_matched"] == 1 and r["n_unmatched"] == 1
    assert check(nb, enb, nb, enb, 1.0, 3.0)["n_matched"] == 2
    # a finite pose that sends some p' to +inf, -inf and NaN: those cells are unmatched, the others as before
    pts = [[0.25, 0.0, 0.0], [0.25, 2.0, 0.0], [0.25, 2.0, 2.0], [0.25, -2.0, 0.0]]
    a, ea, b, eb = maps(0.5, pts, pts)
    T = IDENTITY.copy()
    T[1], T[2] = 1e308, -1e308
    px = ref.world_positions(ea["xyz"], T)[:, 0]
    assert sorted(map(str, px.tolist())) == ["-inf", "0.25", "inf", "nan"]
    r = check(a, ea, b, eb, 0.5, 0.5, T)
    assert r["n_matched"] == 1 and r["n_unmatched"] == 3 and r["su"] == r["sv"] == [512, 0, 0] and r["e2"] == 0
    assert check(a, ea, b, eb, 0.5, 0.5)["n_matched"] == 4
    # filters that leave a or b empty
    a, ea, b, eb = maps(0.5, pts, pts)
    r = a.alignStep(b, 0.5, min_points=2, correspondences=True)
    assert r["n_cells"] == 0 and r["n_matched"] == 0 and len(r["keys"]) == 0
    r = a.alignStep(b, 0.5, min_windows_other=2, correspondences=True)
    assert r["n_cells"] == 4 and r["n_matched"] == 0 and not r["keys_other"].any()
    # the bounds that need a map
    assert code_of(lambda: a.alignStep(b, 1.5 + 1e-9)) == E.ERR_INVALID and a.alignStep(b, 1.5)["reach"] == 3
    other = d.Context(0)
    foreign = d.WorldMap(other, 0.5, 8)
    assert code_of(lambda: a.alignStep(foreign, 0.5)) == E.ERR_CONTEXT and code_of(lambda: foreign.align(a, 0.5)) == E.ERR_CONTEXT
    assert code_of(lambda: a.integrateMap(foreign)) == E.ERR_CONTEXT and code_of(lambda: a.integrateMap(a)) == E.ERR_INVALID
    for o in [foreign] + made:
        o.close()
    other.close()


def test_the_loop_round_by_round(scene1):
    a, ea, b, eb = scene1
    o = ar.SCENE1_LOOP
    T_want, info_want, history = ar.align(ea, eb, ar.LEAF_B, solver=d.solve_alignment, composer=d.compose_pose, **o)
    T, info = a.align(b, **o)
    assert np.array_equal(T, T_want) and info == info_want, (info, info_want)
    want = ar.SCENE1_LOOP_RESULT                                        # what test_map_align_cpu.py recorded
    assert ar.pose_error(T, ar.T_TRUE_1) == want["pose_error"]
    assert all(info[k] == want[k] for k in ("iterations", "converged", "n_matched_first", "n_matched_last", "rms_first", "rms_last"))
    # the correspondences that stay are the last pass's
    last = a.fetchAlignment()
    m = history[-1][0]
    assert np.array_equal(last["keys_other"], m["keys_other"]) and np.array_equal(last["dist"].view(np.uint32), m["dist"].view(np.uint32))
    # round by round: k rounds give the restatement's pose after round k
    for k in range(1, info_want["iterations"] + 1):
        Tk, ik = a.align(b, **dict(o, max_iterations=k))
        assert np.array_equal(Tk, history[k - 1][2]) and ik["iterations"] == k and ik["n_matched_last"] == history[k - 1][0]["n_matched"], k
    # one round is one step, one solve and one compose; from another start too
    for T0 in (IDENTITY, history[2][2]):
        m = a.alignStep(b, o["radius"], T0)
        T_delta, si = d.solve_alignment(m)
        T1, i1 = a.align(b, T_init=T0, **dict(o, max_iterations=1))
        assert np.array_equal(T1, d.compose_pose(T_delta, T0)) and i1["rms_first"] == i1["rms_last"] == si["rms"]
        assert i1["angle_last"] == si["angle"] and i1["trans_last"] == si["trans"]
    # generous tolerances end the loop early, converged
    Tc, ic = a.align(b, **dict(o, eps_rot=1e-3, eps_trans=1e-3))
    k = ic["iterations"]
    assert ic["converged"] == 1 and 1 < k < 12 and np.array_equal(Tc, history[k - 1][2])


def test_the_loop_refuses_too_few_matches_with_the_last_good_pose(scene1):
    a, ea, b, eb = scene1
    with pytest.raises(d.DsiError) as e:
        a.align(b, 0.08, min_matched=len(ea["keys"]) + 1, max_iterations=5)
    assert e.value.code == E.ERR_INVALID and np.array_equal(e.value.T, IDENTITY)
    assert e.value.info["stopped"] == 1 and e.value.info["iterations"] == 1 and e.value.info["n_matched_first"] == 2241
    # after good rounds the pose that comes back is the last good one: the first round that matches fewer cells than every
    # round before it is refused by a min_matched one above its count
    o = ar.SCENE1_LOOP
    _, _, history = ar.align(ea, eb, ar.LEAF_B, solver=d.solve_alignment, composer=d.compose_pose, **o)
    counts = [h[0]["n_matched"] for h in history]
    k = next(k for k in range(1, len(counts)) if counts[k] < min(counts[:k]))
    assert k >= 2
    with pytest.raises(d.DsiError) as e:
        a.align(b, **dict(o, min_matched=counts[k] + 1))
    assert e.value.code == E.ERR_INVALID and np.array_equal(e.value.T, history[k - 1][2])
    assert e.value.info["stopped"] == 1 and e.value.info["iterations"] == k + 1 and e.value.info["n_matched_last"] == counts[k]
    assert e.value.info["converged"] == 0 and e.value.info["rms_last"] == d.solve_alignment(history[k - 1][0])[1]["rms"]
    with pytest.raises(ar.Refused) as r:                             # the restatement's loop stops at the same place
        ar.align(ea, eb, ar.LEAF_B, solver=d.solve_alignment, composer=d.compose_pose, **dict(o, min_matched=counts[k] + 1))
    assert np.array_equal(r.value.T, e.value.T) and r.value.info == e.value.info
    # out of b nothing matches: refused in the first round, the pose given comes back
    with pytest.raises(d.DsiError) as e:
        a.align(b, 0.08, T_init=ar.T_FAR, min_matched=1)
    assert np.array_equal(e.value.T, ar.T_FAR) and e.value.info["n_matched_last"] == 0
    with pytest.raises(d.DsiError) as e:                             # min_matched 0: the solver refuses instead
        a.align(b, 0.08, T_init=ar.T_FAR, min_matched=0)
    assert e.value.info["stopped"] == 2 and np.array_equal(e.value.T, ar.T_FAR)


@pytest.mark.parametrize("leaf_dst", [ar.LEAF_A, ar.LEAF_B])
def test_integrate_map_equals_integrate_of_the_extraction(ctx, scene1, leaf_dst):
    src, _, _, _ = scene1
    ca, _ = ar.scene1_calls()
    src_ref = ar.reference_map(ca, ar.LEAF_A)
    for mp, mw, T in ((1, 1, ar.T_TRUE_1), (2, 1, IDENTITY), (1, 2, ar.T_TRUE_2)):
        dst, dst_ref = build(ctx, leaf_dst, [np.float32([[0.01, 0.02, 0.03]])], log2=8)     # grows from 2^8 slots
        twin, _ = build(ctx, leaf_dst, [np.float32([[0.01, 0.02, 0.03]])], log2=16)
        cells = src.extract(mp, mw, sort=False)
        assert 0 < len(cells["keys"]) and (mp == mw == 1 or len(cells["keys"]) < src.count())
        n, rej = dst.integrateMap(src, T, mp, mw)
        assert (n, rej) == (len(cells["keys"]), 0) == ar.integrate_map(dst_ref, src_ref, T, mp, mw)
        assert twin.integrate(cells["xyz"], T) == 0
        merge_ref.assert_states_equal(dst.exportState(), twin.exportState())
        merge_ref.assert_states_equal(dst.exportState(), dst_ref.export_state())
        assert dst.info()["growths"] >= 2 and dst.info()["calls"] == 2
        # a second call: one more window per touched cell, the points twice
        before = dst.exportState()
        dst.integrateMap(src, T, mp, mw)
        after = dst.exportState()
        touched = after["n"] > before["n"]
        assert np.array_equal(after["keys"], before["keys"]) and touched.sum() >= len(before["keys"]) - 1
        assert np.array_equal(after["windows"], before["windows"] + touched) and (after["stamp"][touched] == 3).all()
        assert code_of(lambda: dst.integrateMap(dst, T)) == E.ERR_INVALID
        merge_ref.assert_states_equal(dst.exportState(), after)                               # a refusal changes nothing
        dst.close()
        twin.close()
    # points that leave the key range are counted as rejected
    far = IDENTITY.copy()
    far[3] = 1e9
    dst = d.WorldMap(ctx, leaf_dst, 8)
    assert dst.integrateMap(src, far) == (src.count(), src.count()) and dst.count() == 0 and dst.info()["calls"] == 1
    dst.close()


def test_fetch_protocol_guards_and_invalidation(ctx, scene1):
    a, ea, b, eb = scene1
    L = d.load_library()
    ca, cb = ar.scene1_calls()
    mine, mine_ref = build(ctx, ar.LEAF_A, ca[::2], log2=8)
    assert code_of(mine.fetchAlignment) == E.ERR_INVALID             # before the first step
    want = ar.step(mine_ref.extract(1, 2), eb, ar.LEAF_B, 0.08, ar.T_TRUE_1)
    got = mine.alignStep(b, 0.08, ar.T_TRUE_1, min_windows=2)
    m = got["n_cells"]
    assert m == want["n_cells"] and 0 < m < mine.count()
    n = C.c_size_t()
    pad = 1024
    GUARD = 0xA5A5A5A5A5A5A5A5
    dist = np.full(m + 2 * pad, -77.0, np.float32)
    ka, kb = np.full(m + 2 * pad, GUARD, np.uint64), np.full(m + 2 * pad, GUARD, np.uint64)
    fptr = lambda x: x[pad:].ctypes.data_as(C.POINTER(C.c_float))
    kptr = lambda x: x[pad:].ctypes.data_as(C.POINTER(C.c_uint64))
    # too small a capacity: nothing is written, the size needed comes back
    assert L.dsx_map_align_fetch(mine._h, kptr(ka), kptr(kb), fptr(dist), m - 1, C.byref(n)) == E.ERR_INVALID and n.value == m
    assert (dist == -77.0).all() and (ka == GUARD).all() and (kb == GUARD).all()
    assert L.dsx_map_align_fetch(mine._h, kptr(ka), kptr(kb), fptr(dist), m, C.byref(n)) == E.OK and n.value == m
    for buf, guard in ((dist, np.float32(-77.0)), (ka, np.uint64(GUARD)), (kb, np.uint64(GUARD))):
        assert (buf[:pad] == guard).all() and (buf[pad + m:] == guard).all()
    order = np.argsort(ka[pad:pad + m], kind="stable")
    assert np.array_equal(ka[pad:pad + m][order], want["keys"]) and np.array_equal(kb[pad:pad + m][order], want["keys_other"])
    assert np.array_equal(dist[pad:pad + m][order].view(np.uint32), want["dist"].view(np.uint32))
    # the order is dsi_map_extract's for the same filter; any output may be left out
    assert np.array_equal(ka[pad:pad + m], mine.extract(1, 2, sort=False)["keys"])
    only = np.empty(m, np.uint64)
    assert L.dsx_map_align_fetch(mine._h, None, only.ctypes.data_as(C.POINTER(C.c_uint64)), None, m, C.byref(n)) == E.OK
    assert np.array_equal(only, kb[pad:pad + m])
    # a change to the second map does not invalidate the result; a render, a compare or an export of the first does not either
    other, _ = build(ctx, ar.LEAF_B, cb[:1], log2=8)
    mine.alignStep(other, 0.08)
    before = mine.fetchAlignment()
    other.integrate(np.float32([[0, 0, 2]]), IDENTITY)
    other.reset()
    mine.render(IDENTITY, 7, 5, 1.0, 1.0, 3.0, 2.0, 0.5, 100.0, fetch=False)
    mine.compare(b, 0.08, 16)
    mine.exportState()
    after = mine.fetchAlignment()
    assert all(np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)) for k in ("keys", "keys_other", "dist"))
    # any integrate call on the first map does, even an empty one; so do integrateMap, a merge, a prune and a reset
    empty = d.WorldMap(ctx, ar.LEAF_A, 8)
    changes = [lambda: mine.integrate(np.zeros((0, 3), np.float32), IDENTITY), lambda: mine.integrateMap(other),
               lambda: mine.merge(empty), lambda: mine.prune(min_points=2), mine.reset]
    for change in changes:
        mine.alignStep(b, 0.08)
        assert len(mine.fetchAlignment()["keys"]) == mine.count()
        change()
        assert code_of(mine.fetchAlignment) == E.ERR_INVALID
    # a refused step leaves the last result standing (the map is empty now); integrating FROM a map keeps its result
    mine.alignStep(b, 0.08)
    assert code_of(lambda: mine.alignStep(b, 1.0)) == E.ERR_INVALID
    assert len(mine.fetchAlignment()["keys"]) == 0
    other.integrateMap(mine)
    assert len(mine.fetchAlignment()["keys"]) == 0
    for o in (mine, other, empty):
        o.close()


def test_score_world_map_3d_aligned(ctx):
    """The run of test_gpu_map_eval.py's last test, scored against a ground-truth map displaced by a known motion of about
    half a leaf: registering first undoes the displacement, so F1 at the finest threshold rises.  Every figure equals the
    restatement's, which is run here on the two maps' extractions."""
    n_win, dur, t0 = 3, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    opts_dm, opts_pc = d.OptionsDepthMap(), d.OptionsPointCloud(2.0, 1)
    leaf, radius, n_bins = 0.5, 0.5, 8
    M = ar.axis_angle_pose((0.2, -1.0, 0.3), math.radians(0.4), (0.15, -0.12, 0.16))      # |t| = 0.25: half a leaf
    wm = d.WorldMap(ctx, leaf, 8)
    frames = []
    for w in proc.full_sequence(ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur,
                                options_depth_map=opts_dm, options_point_cloud=opts_pc, world_map=wm):
        T_w_rv = d.invert_pose(proc.reference_view_process1(rig["trajectories"][0], w[0]))
        frames.append((np.where(w[3] > 0, w[1], 0.0).astype(np.float32), d.compose_pose(M, T_w_rv)))
    gt = proc.ground_truth_map(ctx, frames, cam, leaf, 4.0, 50.0, capacity_log2=8)
    before = wm.exportState()
    plain = proc.score_world_map_3d(wm, gt, radius, n_bins)
    direct = E.map_f_score(wm, gt, radius, n_bins)
    for k in ("thresholds", "precision", "recall", "f1"):
        assert np.array_equal(plain[k], direct[k]), k                    # align=None: exactly what it returned before
    assert set(plain) == set(direct) and "T" not in plain
    opts = dict(radius=1.0, max_iterations=15, min_matched=10, eps_rot=1e-7, eps_trans=1e-7)
    s = proc.score_world_map_3d(wm, gt, radius, n_bins, align=opts)
    merge_ref.assert_states_equal(wm.exportState(), before)              # the estimate itself is not changed
    # the restatement on the two maps' cells
    ew, eg = wm.extract(), gt.extract()
    T_want, info_want, _ = ar.align(ew, eg, leaf, solver=d.solve_alignment, composer=d.compose_pose, **opts)
    assert np.array_equal(s["T"], T_want) and s["align"] == info_want
    moved = ref.ReferenceMap(leaf)
    moved.integrate(ew["xyz"], T_want)
    fwd = mref.compare(moved.extract(), eg, leaf, radius, n_bins)
    bwd = mref.compare(eg, moved.extract(), leaf, radius, n_bins)
    want = mref.f_score(fwd, bwd, radius, n_bins)
    for k in ("thresholds", "precision", "recall", "f1"):
        assert np.array_equal(s[k], want[k]), k
    err = ar.pose_error(s["T"], M)
    print("cells %d / %d; F1 at %.4f: %.2f -> %.2f; rounds %d, rms %.4f -> %.4f, pose error %.2e rad %.2e" %
          (len(ew["keys"]), len(eg["keys"]), s["thresholds"][0], plain["f1"][0], s["f1"][0], s["align"]["iterations"],
           s["align"]["rms_first"], s["align"]["rms_last"], err[0], err[1]))
    assert s["f1"][0] > plain["f1"][0]
    assert s["align"]["rms_last"] < s["align"]["rms_first"]
    gt.close()
    wm.close()
