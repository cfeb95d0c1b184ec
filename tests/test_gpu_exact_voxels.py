"""Every voxel of the exact voting paths against the exact reference, bit for bit.

DESIGN.md ("GPU vs oracle"): a voxel built by the banded kernels (lane mappings 0-7), the fused vote -> fusion ->
arg-max kernel and every band / chunk decomposition is fl32(sum trunc(fl32(w) * 2^31) * 2^-31) -- the exact integer
sum of the truncated Q.31 weights, rounded to fp32 once.  The reference of that statement is the C oracle's
fill_voxel_grid_q31 + q31_to_float (pinned to a numpy restatement and to rational arithmetic by
test_exact_reference.py), and every comparison here is array_equal on the uint32 views.  The two non-exact paths
(lane mapping 8, VOTE_GLOBAL_ATOMIC) are held to bounds derived from their arithmetic.
"""
import numpy as np
import pytest

import dvs_mcemvs_amd as d
from dvs_mcemvs_amd import synthetic as syn
from oracle import oracle as orc
from oracle_pipeline import OracleMapper
from test_exact_reference import WITNESS, exact_case
from test_gpu_parity import make_mapper

pytestmark = pytest.mark.gpu


def assert_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError("%s: %d values differ; first at %s: gpu %r, exact %r" % (
            what, bad.shape[0], i, float(got[i]), float(want[i])))


def exact_fill(m, xy, centers):
    nx, ny, _ = m.dsi_.getDimensions()
    acc, count = orc.fill_voxel_grid_q31(xy, centers, m.raw_depths_vec_, np.array(m.virtual_cam_, np.float32), nx, ny)
    return acc, count, orc.q31_to_float(acc)


SHAPES = [(2, 2, 1), (9, 2, 3), (131, 97, 7), (40, 30, 1), (24, 16, 256), (5000, 3, 2), (3, 4000, 2)]
BANDS = [None, (5, 1, 256), (7, 3, 512), (16, 8, 1024)]


def _run_fill(ctx, shape, packed, band=None, inline_cuts=None, algo=d.VOTE_LDS_BANDS, n_packets=12, seed=0):
    nx, ny, nz = shape
    rng = np.random.default_rng(5000 + 7 * nx + ny + nz + seed)
    cam = (nx, ny, 0.8 * max(nx, 4), 0.8 * max(nx, 4), 0.5 * nx, 0.5 * ny)
    m = make_mapper(ctx, cam, nz, 1.0, 6.5, algo, band=band, packed=packed, inline_cuts=inline_cuts)
    xy, centers = exact_case(rng, nx, ny, n_packets, m.raw_depths_vec_)
    acc, count, want = exact_fill(m, xy, centers)
    m.fillVoxelGrid(xy, centers)
    got = m.dsi_.download()
    info = m.last_vote_info()
    m.close()
    return got, want, acc, count, info


@pytest.mark.parametrize("packed", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_fill_voxel_grid_is_the_exact_sum_on_every_shape(ctx, packed, shape):
    """3a: every exact lane mapping on 2 x 2 x 1, odd widths, one plane, 256 planes, 5000 x 3 and 3 x 4000; the
    special coordinates and centres, duplicate bursts up to multiplicity 1024, dead and one-row packets."""
    got, want, acc, _, info = _run_fill(ctx, shape, packed)
    assert info["packed"] == packed
    assert_bits(got, want, "mapping %d, %r" % (packed, shape))
    assert acc.any()


@pytest.mark.parametrize("packed", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("band", BANDS)
def test_fill_voxel_grid_is_the_exact_sum_for_every_band_plan(ctx, packed, band):
    """3a: band heights, chunk counts and block sizes (ragged last band, more chunks than packets); the grouped
    mappings 2 and 4 sort several packets together here (group_packets > 1); 5 and 6 also with the runs derived in
    the kernel (set_inline_cuts(0)) instead of the cut table."""
    for inline in ((None, 0) if packed in (5, 6) else (None,)):
        got, want, _, _, info = _run_fill(ctx, (96, 72, 12), packed, band=band, inline_cuts=inline, n_packets=20)
        assert info["packed"] == packed and info["algo"] == d.VOTE_LDS_BANDS
        if band is not None:
            assert info["band_rows"] == band[0]
        if packed in (2, 4) and band == (5, 1, 256):
            assert info["group_packets"] > 1
        assert_bits(got, want, "mapping %d, band %r, inline cuts %r" % (packed, band, inline))


@pytest.mark.parametrize("shape", SHAPES + [(346, 260, 20)])
def test_vote_auto_is_the_exact_sum(ctx, shape):
    got, want, _, _, info = _run_fill(ctx, shape, None, algo=d.VOTE_AUTO)
    if info["algo"] == d.VOTE_LDS_BANDS:
        assert_bits(got, want, "VOTE_AUTO %r" % (shape,))
    else:
        assert shape == (5000, 3, 2), "VOTE_AUTO left the exact path on %r" % (shape,)


@pytest.mark.parametrize("packed", [-1, 1, 3, 5])
@pytest.mark.parametrize("band", [(9, 1, 1024), (9, 4, 1024)])
def test_fill_voxel_grid_accumulates_in_fp32(ctx, packed, band):
    """3b: fillVoxelGrid adds to the grid (k_reduce_partials with accumulate): after a second call with other packets
    every voxel is fl32(old + fl32(exact sum of the new votes)) -- one chunk and several."""
    nx, ny, nz = 70, 48, 9
    rng = np.random.default_rng(61)
    cam = (nx, ny, 60.0, 60.0, 35.0, 24.0)
    m = make_mapper(ctx, cam, nz, 0.5, 4.0, d.VOTE_LDS_BANDS, band=band, packed=packed)
    xa, ca = exact_case(rng, nx, ny, 10, m.raw_depths_vec_)
    xb, cb = exact_case(rng, nx, ny, 13, m.raw_depths_vec_)
    _, _, wa = exact_fill(m, xa, ca)
    _, _, wb = exact_fill(m, xb, cb)
    m.fillVoxelGrid(xa, ca)
    assert m.last_vote_info()["chunks"] == band[1]
    assert_bits(m.dsi_.download(), wa, "first call")
    m.fillVoxelGrid(xb, cb)
    assert_bits(m.dsi_.download(), wa + wb, "second call")      # numpy fp32 +: one IEEE rounding
    m.close()


def _rig_exact(cam, c, rig, kw):
    r = OracleMapper(cam, exact=True, **kw)
    assert r.evaluateDSI(rig["events"][c], rig["trajectories"][c], rig["T_rv_w"])
    return r


@pytest.mark.parametrize("variant", ["plain", "lut", "inverse_depth", "fov_dims"])
def test_evaluate_dsi_is_the_exact_sum(ctx, variant):
    """3c: the four variants of test_evaluate_dsi_matches_oracle (host packetisation and pose interpolation, device
    stage A and B) against OracleMapper(exact=True): stage A's coordinates are the oracle's bit for bit, so the DSIs are.
    Default plan, one chunk (the band flush writes fp32 straight into the grid) and several chunks (k_reduce_partials);
    the global-atomic path within its fp32 summation bound (3g)."""
    rig = syn.stereo_rig(30000, width=96, height=72, duration=0.3, seed=21)
    cam = rig["cam"]
    lut, inverse, dimX, dimY, fov = None, False, 0, 0, 0.0
    if variant == "lut":
        lut = syn.radial_lut(cam)
    elif variant == "inverse_depth":
        inverse = True
    elif variant == "fov_dims":
        dimX, dimY, fov = 80, 64, 60.0
    kw = dict(dimX=dimX, dimY=dimY, fov=fov, lut=lut, inverse_depth=inverse, dimZ=24, min_depth=4.0, max_depth=200.0)
    for c in range(2):
        r = _rig_exact(cam, c, rig, kw)
        for algo, band in ((d.VOTE_LDS_BANDS, None), (d.VOTE_LDS_BANDS, (0, 1, 1024)), (d.VOTE_LDS_BANDS, (5, 3, 512)),
                           (d.VOTE_AUTO, None), (d.VOTE_GLOBAL_ATOMIC, None)):
            m = make_mapper(ctx, cam, 24, 4.0, 200.0, algo, dimX=dimX, dimY=dimY, fov=fov, lut=lut, inverse=inverse,
                            band=band)
            assert m.evaluateDSI(rig["events"][c], rig["trajectories"][c], rig["T_rv_w"])
            got = m.dsi_.download()
            if m.last_vote_info()["algo"] == d.VOTE_GLOBAL_ATOMIC:
                assert_within_fp32_summation(got, r.acc, r.count, "global atomic, %s" % variant)
            else:
                if band == (0, 1, 1024):
                    assert m.last_vote_info()["chunks"] == 1
                assert_bits(got, r.dsi, "%s camera %d band %r" % (variant, c, band))
            m.close()
        assert r.dsi.max() > 10.0


def assert_within_fp32_summation(got, acc, count, what):
    """3g, VOTE_GLOBAL_ATOMIC: fp32 atomics in any order.  The real sum S of a voxel's n fp32 weights lies in
    [E, E + n 2^-31) (E = acc 2^-31: each weight truncated to the 2^-31 grid loses less than 2^-31), and any fp32
    summation order of n non-negative terms is within gamma_(n-1) S of S, gamma_k = k u / (1 - k u), u = 2^-24."""
    E = acc.astype(np.float64) * 2.0 ** -31
    n = count.astype(np.float64)
    u = 2.0 ** -24
    g = np.where(n > 1, (n - 1) * u / (1 - (n - 1) * u), 0.0)
    lo = E * (1 - g)
    hi = (E + n * 2.0 ** -31) * (1 + g)
    x = got.astype(np.float64)
    bad = (x < lo) | (x > hi)
    assert not bad.any(), "%s: %d voxels outside the fp32 summation bound, first %s" % (what, int(bad.sum()),
                                                                                      tuple(np.argwhere(bad)[0]))


def test_configs1_both_cameras_equal_the_exact_reference_at_full_size(ctx):
    """3d: BASELINE configs[1] (stereo, 10 M events per camera, 346 x 260 x 100): both cameras' DSIs equal the C
    exact reference bit for bit, all 8,996,000 voxels each."""
    rig = syn.stereo_rig(10_000_000, seed=1234)
    cam = rig["cam"]
    for c in range(2):
        m = make_mapper(ctx, cam, 100, 4.0, 200.0, d.VOTE_LDS_BANDS)
        assert m.evaluateDSI(rig["events"][c], rig["trajectories"][c], rig["T_rv_w"])
        got = m.dsi_.download()
        m.close()
        r = _rig_exact(cam, c, rig, dict(dimZ=100, min_depth=4.0, max_depth=200.0))
        assert_bits(got, r.dsi, "configs[1] camera %d" % c)
        assert int(r.count.max()) > 1000


# ---- the fused kernel ------------------------------------------------------------------------------------------------
def _batches(ctx, rig, n):
    out = []
    for c in range(n):
        first, Rt = d.packetize(rig["events"][c][2], rig["trajectories"][c], rig["T_rv_w"])
        out.append((d.EventBatch(ctx, rig["events"][c][0], rig["events"][c][1], Rt, first), first, Rt))
    return out


def _exact_volume(cam, ev, first, Rt, nz, lut=None):
    r = OracleMapper(cam, dimZ=nz, min_depth=4.0, max_depth=150.0, lut=lut, exact=True)
    r.evaluate_packets(ev[0], ev[1], first.astype(np.int64), Rt)
    return r


def _fused_reference(vols, op):
    """process1.cpp:126-191 (fused = 0; += dsi0; op(dsi1); min / HM(., 3) / max with dsi2), the GM tree of four."""
    if len(vols) == 1:
        return vols[0]
    if len(vols) == 4:
        return orc.fuse_gm_tree(vols)
    fused = orc.fuse2(orc.accumulate(np.zeros_like(vols[0]), vols[0], 0), vols[1], op)
    if len(vols) == 3:
        if op == 1:
            fused = orc.fuse2(fused, vols[2], 1)
        elif op == 2:
            fused = orc.fuse_hm_n(fused, vols[2], 3)
        elif op == 6:
            fused = orc.fuse2(fused, vols[2], 6)
    return fused


@pytest.mark.parametrize("packed,band_rows", [(1, 0), (3, 0), (3, 5), (5, 0), (6, 7), (1, 4)])
def test_fused_kernel_equals_the_exact_reference(ctx, packed, band_rows):
    """3e: k_vote_fuse_argmax with 1, 2, 3 and 4 cameras (mappings 1 / 3 with small bands take the two-workgroups-per-CU
    variant): confidence and index equal the oracle's fusion ops and collapse_max_z applied to the EXACT reference volumes."""
    nx, ny, nz = 96, 72, 24
    rig = syn.stereo_rig(40_000, width=nx, height=ny, duration=0.3, seed=17, n_points=700, n_cams=4)
    rig["events"][2] = tuple(a[:29_000] for a in rig["events"][2])
    sh = d.ShapeDSI(0, 0, nz, 4.0, 150.0, 0.0)
    bs = _batches(ctx, rig, 4)
    vols = [_exact_volume(rig["cam"], rig["events"][c], bs[c][1], bs[c][2], nz).dsi for c in range(4)]
    ms = [d.MapperEMVS(ctx, rig["cam"], sh) for _ in range(5)]
    for m in ms:
        m.set_packed_lanes(packed)
        m.set_band_params(band_rows, 0, 0)
    planes = ms[0].raw_depths_vec_
    batches = [b[0] for b in bs]

    def check(n, op, what):
        conf, idx = orc.collapse_max_z(_fused_reference(vols[:n], op))
        depth, gconf, gidx = ms[4].fetchDepthMap()
        assert ms[0].last_vote_info()["algo"] == d.VOTE_FUSED_ARGMAX
        assert np.array_equal(gidx, idx), "%s: index differs at %d pixels" % (what, int((gidx != idx).sum()))
        assert_bits(gconf, conf, what)
        assert np.array_equal(depth, planes[idx])

    ms[4].computeDepthMapOfEvents(ms[:1], batches[:1], 0)
    check(1, 0, "one camera")
    for op in (1, 2, 3, 4, 5, 6):
        ms[4].computeDepthMapOfEvents(ms[:2], batches[:2], op)
        check(2, op, "two cameras, op %d" % op)
    for op in (1, 2, 3, 6):
        ms[4].computeDepthMapOfEvents(ms[:3], batches[:3], op)
        check(3, op, "three cameras, op %d" % op)
    ms[4].computeDepthMapOfEventsN(ms[:4], batches)
    check(4, 3, "four cameras, GM tree")
    for o in ms + batches:
        o.close()


# ---- sums of 2^52 and more (3f) --------------------------------------------------------------------------------------
BIG_CAM = (8, 6, 8.0, 8.0, 4.0, 3.0)     # f = 8, c = (4, 3), z0 = 4: H = I / 4 and X = x0 exactly (centres at 0)


def big_sum_events():
    """Pixels of an 8 x 6 sensor with a LUT that sends each to one z0 location; one plane at depth 4 and the camera at
    the origin, so X = x0 and Y = y0.  Voxels (x, y) of the DSI:
      (1, 3): 4096 packets at (1, 3) + one packet with (1.5, 3), ((2^24 - 1) 2^-26, 3) and (31 2^-31, 3):
              2^53 + 2^30 + 2^29 - 1 -- fl32 = 4194304.5, through a double 4194305.0
      (3, 1): 2^21 full votes = 2^52;  (5, 1): 2^21 - 1 full votes = 2^52 - 2^31
      (5, 4): 3 2^20 full votes + a few fractional ones (between 2^52 and 2^53)
    and a few small voxels (the rest of the mixed packets) in the same wave of cells."""
    lut = np.full((6 * 8, 2), -4.0, np.float32)                     # off the grid unless set
    locs = [(1.0, 3.0), (1.5, 3.0), ((2 ** 24 - 1) * 2.0 ** -26, 3.0), (31 * 2.0 ** -31, 3.0), (3.0, 1.0),
            (5.0, 1.0), (5.0, 4.0), (4.7, 4.0), (6.25, 2.5), (2.5, 4.75)]
    for p, loc in enumerate(locs):
        lut[p] = loc
    off = len(locs)                                                  # a pixel that votes nowhere
    seq = [(0, 4096 * 1024), (1, 1), (2, 1), (3, 1), (8, 1021),
           (4, 2 ** 21), (5, 2 ** 21 - 1), (6, 3 * 2 ** 20), (7, 3), (9, 5)]
    pix = np.concatenate([np.full(n, p, np.int64) for p, n in seq])
    pix = np.concatenate([pix, np.full(-pix.size % 1024, off, np.int64)])
    return lut, (pix % 8).astype(np.uint16), (pix // 8).astype(np.uint16)


def _big_expected(xy, m):
    acc, _, want = exact_fill(m, xy, np.zeros((xy.shape[0] // 1024, 3), np.float32))
    a = acc[0]
    assert int(a[3, 1]) == WITNESS and int(a[1, 3]) == 2 ** 52 and int(a[1, 5]) == 2 ** 52 - 2 ** 31
    assert 2 ** 52 < int(a[4, 5]) < 2 ** 53 and 0 < int(a[2, 6]) < 2 ** 40
    assert float(want[0, 3, 1]) == 4194304.5
    return acc, want


def test_large_sums_are_rounded_once(ctx):
    """3f: voxels of 2^52 and more (the general conversion of fix_to_float and of the fused kernel's read-back) are
    fl32 of the exact sum: the banded path with one chunk and with several (fillVoxelGrid: k_reduce_partials),
    evaluateDSI's direct band flush (one chunk), and the fused kernel, on a wave that mixes big and small voxels."""
    lut, ex, ey = big_sum_events()
    n_packets = ex.size // 1024
    Rt = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (n_packets, 1))
    xy = lut[ey.astype(np.int64) * 8 + ex]
    shape = d.ShapeDSI(0, 0, 1, 4.0, 8.0, 0.0)
    probe = d.MapperEMVS(ctx, BIG_CAM, shape, lut=lut)
    assert np.array_equal(np.array(probe.virtual_cam_, np.float32), np.array([8, 8, 4, 3], np.float32))
    acc, want = _big_expected(xy, probe)
    # the oracle's stage A (events + LUT + identity pose) gives the same z0 locations
    r = _exact_volume(BIG_CAM, (ex, ey), np.arange(n_packets, dtype=np.int64) * 1024, Rt, 1, lut=lut)
    assert np.array_equal(r.acc, acc)
    probe.close()
    batch = d.EventBatch(ctx, ex, ey, Rt)
    for packed in (-1, 1, 3, 5):
        for chunks in (1, 4):
            m = d.MapperEMVS(ctx, BIG_CAM, shape, lut=lut)
            m.set_vote_algo(d.VOTE_LDS_BANDS)
            m.set_packed_lanes(packed)
            m.set_band_params(0, chunks, 1024)
            m.fillVoxelGrid(xy, np.zeros((n_packets, 3), np.float32))
            assert m.last_vote_info()["chunks"] == chunks
            assert_bits(m.dsi_.download(), want, "fillVoxelGrid, mapping %d, %d chunks" % (packed, chunks))
            m.evaluateDSI_batch(batch)
            assert_bits(m.dsi_.download(), want, "evaluateDSI, mapping %d, %d chunks" % (packed, chunks))
            m.close()
    for packed in (1, 3, 5, 6):
        ms = [d.MapperEMVS(ctx, BIG_CAM, shape, lut=lut) for _ in range(2)]
        for m in ms:
            m.set_packed_lanes(packed)
        ms[1].computeDepthMapOfEvents(ms[:1], [batch], 0)
        depth, conf, idx = ms[1].fetchDepthMap()
        assert not idx.any()
        assert_bits(conf, want[0], "fused kernel, mapping %d" % packed)
        for m in ms:
            m.close()
    batch.close()


# ---- the non-exact paths (3g) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,band", [((64, 48, 16), None), ((131, 97, 7), (5, 3, 1024)), ((41, 30, 6), (9, 1, 1024)),
                                        ((346, 260, 12), None)])
def test_paired_cells_within_their_rounding_of_the_exact_sum(ctx, shape, band):
    """Lane mapping 8 sums ROUNDED Q.19 weights (v_cvt_rpi of the scaled products): per vote at most 2^-20 from the
    fp32 weight, plus 2^-22 for its own fp32 products (S - S fx instead of fl(1 - fx)), plus the 2^-31 truncation of
    the exact sum; then both sums are rounded to fp32 once (half an ulp each)."""
    nx, ny, nz = shape
    rng = np.random.default_rng(830 + nx)
    cam = (nx, ny, 0.8 * nx, 0.8 * nx, 0.5 * nx, 0.5 * ny)
    m = make_mapper(ctx, cam, nz, 1.0, 6.5, d.VOTE_LDS_BANDS, band=band, packed=8)
    xy, centers = exact_case(rng, nx, ny, 40, m.raw_depths_vec_)
    acc, count, want = exact_fill(m, xy, centers)
    m.fillVoxelGrid(xy, centers)
    assert m.last_vote_info()["packed"] == 8 and not m.paired_overflow()
    got = m.dsi_.download().astype(np.float64)
    w = want.astype(np.float64)
    bound = count * (2.0 ** -20 + 2.0 ** -22 + 2.0 ** -31) + 2.0 ** -24 * (np.abs(got) + np.abs(w))
    err = np.abs(got - w)
    assert np.all(err <= bound), "%d voxels outside, worst %g of %g" % (int((err > bound).sum()), err.max(),
                                                                       bound[np.unravel_index(err.argmax(), err.shape)])
    assert np.all((count > 0) | (got == 0))
    m.close()


@pytest.mark.parametrize("shape", [(64, 48, 16), (131, 97, 7), (2, 2, 1), (5000, 3, 2)])
def test_global_atomic_within_the_fp32_summation_bound(ctx, shape):
    got, _, acc, count, info = _run_fill(ctx, shape, None, algo=d.VOTE_GLOBAL_ATOMIC, n_packets=30)
    assert info["algo"] == d.VOTE_GLOBAL_ATOMIC
    assert_within_fp32_summation(got, acc, count, "global atomic %r" % (shape,))
