"""Reused mappers: any sequence of calls on long-lived mappers equals fresh mappers, bit for bit.

A mapper's device scratch is grown, never cleared, and shared by entry points with different table layouts; the product
keeps mappers alive for a whole run.  Here one set of mappers goes through the call sequences of mapper_sequence_cases.py
(every ordered pair of the eight state classes, band plans, packet counts that shrink after growing, accumulate steps,
kernel timing on and off) and through sequences of the output mapper's entry points (fused vote, GM tree, Alg. 2, filters,
point cloud, tie resolver, refused calls); after every call the result is held to the exact reference
(oracle.fill_voxel_grid_q31 + q31_to_float, OracleMapper(exact=True) + fuse2 + collapse_max_z, filters_reference.py,
pointcloud_reference.py) with array_equal and to fresh mappers given only that call.  Production library only.
"""
import numpy as np
import pytest

import dvs_mcemvs_amd as d
import filters_reference as fr
import mapper_sequence_cases as msc
import pointcloud_reference as pcr
import test_gpu_exact_voxels as ev
from dvs_mcemvs_amd import engine, process as proc, synthetic as syn
from oracle import oracle as orc
from oracle_pipeline import OracleMapper

pytestmark = pytest.mark.gpu


# ---- a. voting sequences ---------------------------------------------------------------------------------------------
def _new_mapper(ctx, shape):
    return d.MapperEMVS(ctx, msc.camera(shape), d.ShapeDSI(0, 0, shape[2], msc.MIN_DEPTH, msc.MAX_DEPTH, 0.0))


def _empty_batch(ctx):
    return d.EventBatch(ctx, np.zeros(0, np.uint16), np.zeros(0, np.uint16), np.zeros((0, 12), np.float32),
                        np.zeros(0, np.uint32))


def _run_step(ctx, trio, step, inputs):
    """One step on (camera 0, camera 1, output mapper): what the engine left, fetched."""
    m, cam1, out = trio
    got = {}
    if step.cls == "F":
        # (the fused path reads its knobs from the OUTPUT mapper of the call)
        out.set_packed_lanes(step.mapping)
        out.set_band_params(step.band[0] if step.band else 0, 0, 0)
        out.set_kernel_timing(step.timing)
        batches = [d.EventBatch(ctx, x, y, Rt) for x, y, Rt in inputs]
        out.computeDepthMapOfEvents([m, cam1], batches, step.op)
        got["depth"], got["conf"], got["idx"] = out.fetchDepthMap()
        got["launches"] = out.vote_kernel_time()[1]
        for b in batches:
            b.close()
    else:
        m.set_vote_algo(d.VOTE_GLOBAL_ATOMIC if step.cls == "A" else d.VOTE_LDS_BANDS)
        m.set_band_params(*(step.band or (0, 0, 0)))
        m.set_packed_lanes(-1 if step.mapping is None else step.mapping)
        m.set_inline_cuts(0 if step.cls == "Vi" else -1)
        m.set_kernel_timing(step.timing)
        if step.cls == "Z":
            b = _empty_batch(ctx)
            m.evaluateDSI_batch(b)
            b.close()
        else:
            m.dsi_.resetGrid()
            for xy, centers in inputs:
                m.fillVoxelGrid(xy, centers)
        got["launches"] = m.vote_kernel_time()[1]
    got["dsi"] = m.dsi_.download()
    got["info"] = m.last_vote_info()
    return got


def _check_step(shape, step, e, got, held, what):
    info = got["info"]
    assert info["n_packets"] == step.n_packets, (what, info)
    if step.cls == "F":
        assert info["algo"] == d.VOTE_FUSED_ARGMAX and info["packed"] == step.mapping and info["chunks"] == 1, (what, info)
        if step.band:
            assert info["band_rows"] == step.band[0] and info["bands"] == -(-shape[1] // step.band[0]), (what, info)
        assert np.array_equal(got["idx"], e.idx), "%s: index differs at %d pixels" % (what, int((got["idx"] != e.idx).sum()))
        ev.assert_bits(got["conf"], e.conf, what + ", confidence")
        assert np.array_equal(got["depth"], msc.grid(shape)[0][e.idx]), what
        ev.assert_bits(got["dsi"], held, what + ": the fused kernel touched camera 0's DSI")
        assert got["launches"] == (1 if step.timing else 0), (what, got["launches"])
        return
    if step.cls == "A":
        assert info["algo"] == d.VOTE_GLOBAL_ATOMIC, (what, info)
        ev.assert_within_fp32_summation(got["dsi"], e.acc, e.count, what)
        assert np.all((e.count > 0) | (got["dsi"] == 0)), what
    else:
        assert info["algo"] == d.VOTE_LDS_BANDS, (what, info)
        if step.cls != "Z":
            assert info["packed"] == step.mapping, (what, info)
        if step.band:
            assert (info["band_rows"], info["chunks"], info["block_threads"]) == step.band, (what, info)
        ev.assert_bits(got["dsi"], e.dsi, what)
    votes = 0 if step.cls == "Z" else (2 if step.accumulate else 1)
    assert got["launches"] == (votes if step.timing else 0), (what, got["launches"])


def _run_sequence(ctx, seq):
    """`seq` on ONE set of mappers; every step against the exact reference and a fresh set."""
    inputs, expected = msc.inputs_and_expected(seq.name)
    trio = [_new_mapper(ctx, seq.shape) for _ in range(3)]
    planes, Kv = msc.grid(seq.shape)
    assert np.array_equal(trio[0].raw_depths_vec_, planes) and np.array_equal(np.array(trio[0].virtual_cam_, np.float32), Kv)
    held = np.zeros(trio[0].dsi_.shape, np.float32)        # what camera 0's DSI holds
    for k, (step, e) in enumerate(zip(seq.steps, expected)):
        what = "%s step %d %r" % (seq.name, k, tuple(step))
        got = _run_step(ctx, trio, step, inputs[k])
        _check_step(seq.shape, step, e, got, held, what)
        fresh = [_new_mapper(ctx, seq.shape) for _ in range(3)]
        alone = _run_step(ctx, fresh, step, inputs[k])
        _check_step(seq.shape, step, e, alone, np.zeros_like(held), what + " (fresh mappers)")
        for o in fresh:
            o.close()
        if step.cls == "F":
            for key in ("depth", "conf", "idx"):
                assert np.array_equal(got[key], alone[key]), (what, key)
        elif step.cls != "A":
            ev.assert_bits(got["dsi"], alone["dsi"], what + " against fresh mappers")
        if step.cls != "F":
            held = got["dsi"]
    for o in trio:
        o.close()


def test_the_band_plans_are_those_of_the_single_call_tests():
    assert msc.BANDS == ev.BANDS


@pytest.mark.parametrize("seq", msc.TRANSITIONS, ids=lambda q: q.name)
def test_every_transition_between_state_classes_on_one_mapper(ctx, seq):
    """a: every ordered pair "class X, then class Y on the same mapper" (96 x 72 x 12)."""
    _run_sequence(ctx, seq)


@pytest.mark.parametrize("seq", msc.RANDOM, ids=lambda q: q.name)
def test_random_call_sequences_on_one_mapper(ctx, seq):
    """a: seeded random sequences over the same vocabulary (131 x 97 x 7: odd width, ragged last band)."""
    _run_sequence(ctx, seq)


@pytest.mark.parametrize("seq", msc.CYCLES, ids=lambda q: q.name)
def test_one_class_walks_the_packet_counts_on_one_mapper(ctx, seq):
    """a: one banded class alone, 40 1 13 70 5 64 2 packets and back: tables of ONE layout that shrink after they grew;
    under Vi the transposed row table's stride goes 64 -> 128 -> 64."""
    _run_sequence(ctx, seq)


# ---- b. output-mapper sequences ----------------------------------------------------------------------------------------
SHAPE_B = (96, 72, 16)
DEPTHS_B = (4.0, 150.0)
RIG_EVENTS = (60_000, 20_000, 3_000, 900)


class _Rig:
    """One synthetic four-camera window: its batches on the device, and the exact volumes of its cameras (made once)."""

    def __init__(self, ctx, n_events, seed):
        nx, ny, nz = SHAPE_B
        self.ctx, self.n_events = ctx, n_events
        self.rig = syn.stereo_rig(n_events, width=nx, height=ny, duration=0.3, seed=seed, n_points=700, n_cams=4)
        self.cam = self.rig["cam"]
        self.packets, self.batches = [], []
        for c in range(4):
            ev_c = self.rig["events"][c]
            pk = d.packetize(ev_c[2], self.rig["trajectories"][c], self.rig["T_rv_w"])
            first, Rt = pk if pk is not None else (np.zeros(0, np.uint32), np.zeros((0, 12), np.float32))
            self.packets.append((first, Rt))
            self.batches.append(d.EventBatch(ctx, ev_c[0], ev_c[1], Rt, first))
        self._vols = {}
        self._alg2 = {}

    def vol(self, c):
        if c not in self._vols:
            nz = SHAPE_B[2]
            r = OracleMapper(self.cam, dimZ=nz, min_depth=DEPTHS_B[0], max_depth=DEPTHS_B[1], exact=True)
            first, Rt = self.packets[c]
            if len(first):
                r.evaluate_packets(self.rig["events"][c][0], self.rig["events"][c][1], first.astype(np.int64), Rt)
            self._vols[c] = r.dsi
        return self._vols[c]

    def alg2_batches(self, n_sub):
        if n_sub not in self._alg2:
            self._alg2[n_sub] = proc.alg2_window_batches(self.ctx, self.rig["events"][:2], self.rig["trajectories"][:2],
                                                         self.rig["t0"] + 0.2, n_sub)
        return self._alg2[n_sub]

    def close(self):
        for b in self.batches + [b for bs in self._alg2.values() for b in bs]:
            b.close()


@pytest.fixture(scope="module")
def rigs(ctx):
    made = {n: _Rig(ctx, n, 40 + k) for k, n in enumerate(RIG_EVENTS)}
    assert made[900].batches[0].n_packets == 0 and made[3_000].batches[0].n_packets == 2
    yield made
    for r in made.values():
        r.close()


def _mapper_b(ctx, rig):
    return d.MapperEMVS(ctx, rig.cam, d.ShapeDSI(0, 0, SHAPE_B[2], DEPTHS_B[0], DEPTHS_B[1], 0.0))


class _Set:
    """An output mapper (+ the camera_time one of Alg. 2) and four camera mappers."""

    def __init__(self, ctx, rig):
        self.out, self.out_ct = _mapper_b(ctx, rig), _mapper_b(ctx, rig)
        self.cams = [_mapper_b(ctx, rig) for _ in range(4)]

    def close(self):
        for m in [self.out, self.out_ct] + self.cams:
            m.close()


def _oracle_two(vol0, vol1, op, planes):
    conf, idx = orc.collapse_max_z(orc.fuse2(orc.accumulate(np.zeros_like(vol0), vol0, 0), vol1, op))
    return planes[idx], conf, idx


def _compute(s, rigs, call, band_rows):
    """Queue one call of section b on the set s; -> the exact oracle's maps where the call has them (two cameras)."""
    kind, n, arg = call
    rig = rigs[n]
    s.out.set_band_params(band_rows, 0, 0)
    planes = s.out.raw_depths_vec_
    if kind == "two":
        s.out.computeDepthMapOfEvents(s.cams[:2], rig.batches[:2], arg)
        return _oracle_two(rig.vol(0), rig.vol(1), arg, planes)
    if kind == "one":
        s.out.computeDepthMapOfEvents(s.cams[:1], rig.batches[:1], 0)
        conf, idx = orc.collapse_max_z(rig.vol(0))
        return planes[idx], conf, idx
    if kind == "four":
        s.out.computeDepthMapOfEventsN(s.cams, rig.batches)
        conf, idx = orc.collapse_max_z(orc.fuse_gm_tree([rig.vol(c) for c in range(4)]))
        return planes[idx], conf, idx
    if kind == "alg2":
        s.out.computeDepthMapOfEventsAlg2(s.out_ct, s.cams[:2], rig.alg2_batches(arg), arg, d.FUSE_HM, d.FUSE_HM)
        return None
    empty = rigs[900]
    zero = np.zeros_like(rig.vol(0))
    if kind == "empty-second":
        s.out.computeDepthMapOfEvents(s.cams[:2], [rig.batches[0], empty.batches[1]], arg)
        return _oracle_two(rig.vol(0), zero, arg, planes)
    assert kind == "empty-first"
    s.out.computeDepthMapOfEvents(s.cams[:2], [empty.batches[0], rig.batches[1]], arg)
    return _oracle_two(zero, rig.vol(1), arg, planes)


CALLS_B = [("two", 60_000, 1), ("two", 3_000, 2), ("two", 20_000, 3), ("two", 900, 4), ("two", 60_000, 5), ("two", 3_000, 6),
           ("one", 20_000, 0), ("four", 60_000, 0), ("four", 3_000, 0), ("alg2", 60_000, 2), ("two", 3_000, 2),
           ("alg2", 20_000, 5), ("empty-second", 60_000, 6), ("empty-first", 20_000, 6), ("four", 900, 0), ("two", 60_000, 2)]
BAND_ROWS_B = (0, 7, 5)


def _assert_maps(got, want, what):
    for g, w, name in zip(got, want, ("depth", "confidence", "index")):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s: %s differs at %d pixels" % (
            what, name, int((g != w).sum()))


def test_output_mapper_call_sequence(ctx, rigs):
    """b: fused vote with every fusion op, one / four cameras, Alg. 2, empty cameras and band rows 0 / 7 / 5 in turn on ONE
    output mapper and ONE set of camera mappers, rigs of 60,000 / 20,000 / 3,000 / 900 events alternating; every call
    equals fresh mappers given only that call and (two cameras, one, four) the exact oracle's maps.  Every fourth call
    is fetched asynchronously and the NEXT call queued before the wait (those next calls have band rows 7, 5, 0 and 7):
    the arrays hold the earlier call's maps."""
    s = _Set(ctx, rigs[60_000])
    ny, nx = SHAPE_B[1], SHAPE_B[0]
    pins = [d.PinnedArray((ny, nx), t) for t in (np.float32, np.float32, np.uint8)]
    pending = None                                          # (the maps the pinned arrays must hold after the wait, what)
    for k, call in enumerate(CALLS_B):
        what = "call %d %r, band rows %d" % (k, call, BAND_ROWS_B[k % 3])
        oracle = _compute(s, rigs, call, BAND_ROWS_B[k % 3])
        if pending is not None:                             # the earlier call's fetch was queued BEFORE this compute
            s.out.fetchWait()
            _assert_maps([p.a for p in pins], pending[0], pending[1] + ": asynchronous fetch overtaken by the next call")
            pending = None
        got = s.out.fetchDepthMap()
        got_ct = s.out_ct.fetchDepthMap() if call[0] == "alg2" else None
        fresh = _Set(ctx, rigs[60_000])
        _compute(fresh, rigs, call, BAND_ROWS_B[k % 3])
        _assert_maps(got, fresh.out.fetchDepthMap(), what + " against fresh mappers")
        if got_ct is not None:
            _assert_maps(got_ct, fresh.out_ct.fetchDepthMap(), what + " (camera_time) against fresh mappers")
            assert got[1].max() > 0 and got_ct[1].max() > 0
        fresh.close()
        if oracle is not None:
            _assert_maps(got, oracle, what + " against the exact oracle")
        info = s.cams[0].last_vote_info()
        if call[0] != "alg2":
            assert info["algo"] == d.VOTE_FUSED_ARGMAX, (what, info)
            if BAND_ROWS_B[k % 3]:
                assert info["band_rows"] == BAND_ROWS_B[k % 3], (what, info)
        if k % 4 == 0 and k + 1 < len(CALLS_B):
            for p in pins:
                p.a[...] = 0
            s.out.fetchDepthMapAsync(*[p.a for p in pins])
            pending = (got, what)
    for p in pins:
        p.close()
    s.close()


def test_vote_statistics_and_kernel_timing_between_calls(ctx, rigs):
    """b: vote_statistics (its first pass votes with unit multiplicities) between two votes of a camera mapper leaves the
    next vote -- banded and fused -- the exact oracle's; vote_kernel_time reports exactly the voting launches made while
    timing was on."""
    s = _Set(ctx, rigs[60_000])
    big, small = rigs[60_000], rigs[3_000]
    planes = s.out.raw_depths_vec_
    cam = s.cams[0]
    cam.set_kernel_timing(True)
    cam.evaluateDSI_batch(big.batches[0])
    ev.assert_bits(cam.dsi_.download(), big.vol(0), "first vote")
    stats = cam.vote_statistics(small.batches[0])
    ev.assert_bits(cam.dsi_.download(), small.vol(0), "the DSI vote_statistics leaves")
    assert stats[0] == pytest.approx(float(small.vol(0).astype(np.float64).sum()), rel=1e-6) and 0 < stats[1] <= stats[0]
    cam.evaluateDSI_batch(big.batches[0])
    ev.assert_bits(cam.dsi_.download(), big.vol(0), "the vote after vote_statistics")
    assert cam.vote_kernel_time()[1] == 4                   # two votes + the two passes of vote_statistics
    cam.set_kernel_timing(False)
    again = cam.vote_statistics(big.batches[0])
    fresh = _mapper_b(ctx, big)
    assert fresh.vote_statistics(big.batches[0]) == again
    fresh.close()
    # the fused kernel with this camera right after: its packet sort must not see unit multiplicities either
    s.out.set_kernel_timing(True)
    for op in (d.FUSE_HM, d.FUSE_AM):
        s.out.computeDepthMapOfEvents(s.cams[:2], big.batches[:2], op)
        _assert_maps(s.out.fetchDepthMap(), _oracle_two(big.vol(0), big.vol(1), op, planes), "fused after vote_statistics")
    s.out.computeDepthMapOfEventsN(s.cams, small.batches)
    s.out.set_kernel_timing(False)
    s.out.computeDepthMapOfEvents(s.cams[:2], small.batches[:2], d.FUSE_HM)         # not timed
    _assert_maps(s.out.fetchDepthMap(), _oracle_two(small.vol(0), small.vol(1), d.FUSE_HM, planes), "after timing")
    assert s.out.vote_kernel_time()[1] == 3 and cam.vote_kernel_time()[1] == 0
    assert s.out.vote_kernel_time()[1] == 0                 # read once
    s.close()


def test_direct_band_flush_between_other_calls(ctx, rigs):
    """b: evaluateDSI_batch with ONE chunk writes the bands' fp32 sums straight into the grid (no partial volumes, no
    accumulation; stage A inside the packet sort) -- the path fillVoxelGrid never takes.  One camera mapper alternates
    it, with every lane mapping, with several chunks, with being a camera of the fused kernel and with empty windows,
    over rigs that shrink and grow; every DSI is the exact oracle's."""
    s = _Set(ctx, rigs[60_000])
    cam, planes = s.cams[0], s.out.raw_depths_vec_
    cam.set_vote_algo(d.VOTE_LDS_BANDS)
    plan = [(7, 60_000, 1), (5, 3_000, 1), (0, 20_000, 3), (2, 900, 1), (6, 60_000, 1), (3, 3_000, 4), (4, 20_000, 1),
            (1, 60_000, 1), (5, 900, 2), (7, 3_000, 1)]
    for k, (mapping, n, chunks) in enumerate(plan):
        rig = rigs[n]
        what = "round %d: mapping %d, %d events, %d chunks" % (k, mapping, n, chunks)
        cam.set_packed_lanes(mapping)
        cam.set_band_params(BAND_ROWS_B[k % 3], chunks, 0)
        cam.set_inline_cuts(0 if k % 4 == 1 else -1)
        cam.evaluateDSI_batch(rig.batches[0])
        info = cam.last_vote_info()
        assert info["n_packets"] == rig.batches[0].n_packets and info["algo"] == d.VOTE_LDS_BANDS, (what, info)
        if info["n_packets"]:
            assert info["packed"] == mapping and info["chunks"] == chunks, (what, info)
        ev.assert_bits(cam.dsi_.download(), rig.vol(0), what)
        if k % 2 == 0:                                      # the camera's tables rebuilt with halo rows in between
            other = rigs[RIG_EVENTS[(k // 2) % 4]]
            s.out.computeDepthMapOfEvents(s.cams[:2], other.batches[:2], d.FUSE_HM)
            _assert_maps(s.out.fetchDepthMap(), _oracle_two(other.vol(0), other.vol(1), d.FUSE_HM, planes), what + ", fused")
            ev.assert_bits(cam.dsi_.download(), rig.vol(0), what + ": the fused kernel touched the camera's DSI")
    s.close()


# ---- c. post-arg-max scratch on one mapper ---------------------------------------------------------------------------
FILTER_OPTIONS = [(3, 0.0, 1), (63, -2.0, 31), (5, 3.0, 3)]


def _raw_map(s, rig, op=d.FUSE_HM):
    s.out.computeDepthMapOfEvents(s.cams[:2], rig.batches[:2], op)
    return s.out.fetchDepthMap()


def _filter_and_check(s, raw, options, what):
    ksize, C_, med = options
    _, conf, idx = raw
    max_conf = 0.5 * float(conf.max())
    depth, fconf, mask = s.out.filterDepthMap(d.OptionsDepthMap(ksize, C_, med, max_conf))
    got = {"depth": depth, "confidence": fconf, "mask": mask, "idx_filtered": s.out.depth_cell_indices_filtered}
    want = fr.depth_map_filters(conf, idx, s.out.raw_depths_vec_, ksize, C_, med, max_conf)
    for key in ("confidence", "mask", "idx_filtered", "depth"):
        assert np.array_equal(got[key], want[key]), "%s: %s differs at %d pixels" % (what, key, int((got[key] != want[key]).sum()))
    return depth, mask


def test_filters_on_one_mapper_with_changing_options_and_rigs(ctx, rigs):
    """c: filterDepthMap with (kernel size, C, median size) cycling (3, 0, 1), (63, -2, 31), (5, 3, 3) over maps of the
    60,000-, 3,000- and 20,000-event rigs and back: conf8, mask, idx_filtered and minmax of ONE output mapper."""
    s = _Set(ctx, rigs[60_000])
    order = [60_000, 3_000, 20_000, 3_000, 60_000, 20_000, 60_000]
    some = 0
    for k, n in enumerate(order):
        raw = _raw_map(s, rigs[n], d.FUSE_HM if k % 2 == 0 else d.FUSE_AM)
        _, mask = _filter_and_check(s, raw, FILTER_OPTIONS[k % 3], "round %d, %d events, options %r" % (k, n, FILTER_OPTIONS[k % 3]))
        some += int(mask.sum() > 0)
    assert some >= 4
    s.close()


def _cloud_reference(m, depth, mask, radius, k):
    pts = pcr.backproject(depth, mask, *m.virtual_cam_)
    if not len(pts):
        return pts, 0
    keep = pcr.keep_bruteforce if radius > 100.0 else pcr.keep_kdtree      # (all pairs lie within the large radius)
    return pts[keep(pts, radius, k)], len(pts)


def test_pointcloud_dense_sparse_empty_dense_on_one_mapper(ctx, rigs):
    """c: getPointcloud resident (dense window), with host maps of a denser mask, resident again after a sparser window,
    after an empty one and after the dense one again; radii that keep nothing, a part and everything."""
    s = _Set(ctx, rigs[60_000])
    m = s.out
    clouds = {}

    def resident(n, options, cases, what):
        raw = _raw_map(s, rigs[n], d.FUSE_AM)
        depth, mask = _filter_and_check(s, raw, options, what)
        for radius, k in cases:
            want, n0 = _cloud_reference(m, depth, mask, radius, k)
            got = m.getPointcloud(options_pc=d.OptionsPointCloud(radius, k))
            assert m.n_unfiltered_ == n0 == int((mask > 0).sum()), (what, radius, k)
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, radius, k)
            clouds[(what, radius, k)] = len(got)
        return raw, depth, mask

    cases = [(1.0, 3), (1e-6, 1), (1e4, 3), (3.0, 1)]
    raw, depth, mask = resident(60_000, (3, 0.0, 1), cases, "dense")
    assert clouds[("dense", 1e-6, 1)] == 0 and clouds[("dense", 1e4, 3)] == int((mask > 0).sum()) > 100
    # host maps, a denser mask: every pixel with a vote, at its raw depth
    dense_mask = (raw[1] > 0).astype(np.uint8)
    assert dense_mask.sum() > 2 * (mask > 0).sum()
    for radius, k in cases:
        want, n0 = _cloud_reference(m, raw[0], dense_mask, radius, k)
        got = m.getPointcloud(raw[0], dense_mask, d.OptionsPointCloud(radius, k))
        assert m.n_unfiltered_ == n0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("host maps", radius, k)
    _, _, sparse_mask = resident(3_000, (63, -2.0, 31), cases, "sparse")
    assert 0 < (sparse_mask > 0).sum() < (mask > 0).sum()
    _, _, empty_mask = resident(900, (5, 3.0, 3), cases, "empty")
    assert not empty_mask.any()
    resident(60_000, (3, 0.0, 1), cases, "dense again")
    for radius, k in cases:
        assert clouds[("dense again", radius, k)] == clouds[("dense", radius, k)]
    print("points kept (window, radius, min_neighbors): %r" % (clouds,))
    s.close()


RESOLVE_KEYS = ("rel_gap", "near_tie_pixels", "candidate_voxels", "candidate_planes", "votes", "changed_pixels",
                "max_rel_bound", "max_order_diff", "gap_widenings", "premise_ok", "columns_bounded")


def _resolve(s, rig, rel_gap):
    for m, b in zip(s.cams[:2], rig.batches[:2]):
        m.evaluateDSI_batch(b)
    s.out.computeDepthMapOfFusion(s.cams[0].dsi_, s.cams[1].dsi_, d.FUSE_HM)
    info = s.out.resolveNearTies(s.cams[:2], rig.batches[:2], d.FUSE_HM, rel_gap=rel_gap)
    return {k: info[k] for k in RESOLVE_KEYS}, s.out.fetchDepthMap()


def _exact_ties(rig):
    """(columns, voxels) of the fused volume in which two or more planes EQUAL a positive maximum: what no rel_gap, however
    small, takes from the resolver's candidates (it keeps `second >= best - rel_gap * best`)."""
    fused = orc.fuse2(orc.accumulate(np.zeros_like(rig.vol(0)), rig.vol(0), 0), rig.vol(1), d.FUSE_HM)
    best = fused.max(axis=0)
    n = (fused == best).sum(axis=0)
    cols = (best > 0) & (n >= 2)
    return int(cols.sum()), int(n[cols].sum())


def test_tie_resolver_scratch_on_one_output_mapper(ctx, rigs):
    """c: resolveNearTies after a rig with thousands of contenders, one with few, a gap so small (1e-30: rel_gap * best
    vanishes against best in fp32) that only EXACT ties remain -- a gap with no contender at all does not exist, an exact
    tie always contends; their columns and voxels are counted from the exact volumes (none in this rig) -- then the first again:
    statistics and resolved maps equal those of a fresh set of mappers."""
    s = _Set(ctx, rigs[60_000])
    seen = []
    for n, rel_gap in ((60_000, 0.05), (3_000, 0.0), (60_000, 1e-30), (60_000, 0.05)):
        info, maps = _resolve(s, rigs[n], rel_gap)
        fresh = _Set(ctx, rigs[60_000])
        finfo, fmaps = _resolve(fresh, rigs[n], rel_gap)
        fresh.close()
        assert info == finfo, (n, rel_gap, info, finfo)
        _assert_maps(maps, fmaps, "resolved maps, %d events, rel_gap %g" % (n, rel_gap))
        seen.append(info)
    print("contending voxels: %r" % ([i["candidate_voxels"] for i in seen],))
    assert seen[0]["candidate_voxels"] > 2000 > seen[1]["candidate_voxels"] > 0
    assert seen[2]["candidate_voxels"] < seen[0]["candidate_voxels"] // 4
    assert (seen[2]["near_tie_pixels"], seen[2]["candidate_voxels"]) == _exact_ties(rigs[60_000])
    assert seen[3] == seen[0]
    s.close()


# ---- d. refused calls leave no trace ---------------------------------------------------------------------------------
def test_refused_calls_leave_no_trace(ctx, rigs):
    """d: argument errors only (nothing here provokes a device fault): each is refused with its documented code, and the
    next good call -- fused vote and banded vote -- equals the exact oracle as if nothing had happened."""
    big, small = rigs[60_000], rigs[3_000]
    s = _Set(ctx, big)
    planes = s.out.raw_depths_vec_
    other = d.MapperEMVS(ctx, big.cam, d.ShapeDSI(0, 0, SHAPE_B[2] + 1, DEPTHS_B[0], DEPTHS_B[1], 0.0))

    def good(rig, op, what):
        s.out.computeDepthMapOfEvents(s.cams[:2], rig.batches[:2], op)
        _assert_maps(s.out.fetchDepthMap(), _oracle_two(rig.vol(0), rig.vol(1), op, planes), what)
        s.cams[0].evaluateDSI_batch(rig.batches[0])
        ev.assert_bits(s.cams[0].dsi_.download(), rig.vol(0), what + ", banded vote")

    def refused(code, fn, *args, **kw):
        with pytest.raises(d.DsiError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))

    good(big, d.FUSE_HM, "before")
    refused(engine.ERR_SHAPE, s.out.computeDepthMapOfEvents, [s.cams[0], other], big.batches[:2], d.FUSE_HM)
    good(small, d.FUSE_MIN, "after a camera mapper of another shape")
    refused(engine.ERR_INVALID, s.out.computeDepthMapOfEvents, [s.cams[0], s.cams[0]], big.batches[:2], d.FUSE_HM)
    good(big, d.FUSE_GM, "after the same mapper twice")
    s.out.computeDepthMapOfEvents(s.cams[:2], small.batches[:2], d.FUSE_AM)
    raw = s.out.fetchDepthMap()
    _filter_and_check(s, raw, (5, 3.0, 3), "first filter")
    refused(engine.ERR_INVALID, s.out.filterDepthMap, d.OptionsDepthMap(5, 3.0, 3))
    good(big, d.FUSE_AM, "after filterDepthMap twice in a row")
    refused(engine.ERR_INVALID, s.out.getPointcloud, options_pc=d.OptionsPointCloud(0.5, 3))   # a raw map, no filtered one
    good(small, d.FUSE_RMS, "after getPointcloud without a filtered map")
    refused(engine.ERR_INVALID, s.cams[0].set_band_params, 5, 2, 384)
    refused(engine.ERR_INVALID, s.out.set_band_params, 5, 2, 384)
    good(big, d.FUSE_MAX, "after set_band_params with a block size the kernel does not have")
    assert s.cams[0].last_vote_info()["block_threads"] == 1024
    refused(engine.ERR_BAD_OP, s.out.computeDepthMapOfEventsN, s.cams, big.batches, engine.ACC_MIN)
    good(small, d.FUSE_HM, "after four cameras with a mode other than the GM tree")
    s.out.computeDepthMapOfEventsN(s.cams, big.batches)
    conf, idx = orc.collapse_max_z(orc.fuse_gm_tree([big.vol(c) for c in range(4)]))
    _assert_maps(s.out.fetchDepthMap(), (planes[idx], conf, idx), "four cameras after the refused call")
    other.close()
    s.close()
