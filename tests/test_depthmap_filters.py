"""Post-arg-max part of MapperEMVS::getDepthMapFromDSI (mapper_emvs_stereo.cpp:390-436):
confidence normalisation, Gaussian adaptive threshold, masked Huang median, border removal,
index -> depth.  CPU: known answers for the oracle's restatement; GPU: HIP == oracle, bit exact
(everything is integer or exactly representable float work), and HIP == oracle == tests/filters_reference.py (a
second restatement, itself pinned to exact arithmetic by test_filters_reference_cpu.py) over the matrix of
tests/filters_cases.py, for every entry point that ends in the filters, and for their state handling."""
import numpy as np
import pytest

from oracle import oracle as orc


def test_uniform_confidence_gives_empty_mask():
    conf = np.full((20, 30), 3.0, np.float32)
    idx = np.full((20, 30), 7, np.uint8)
    planes = orc.depth_planes(1.0, 5.0, 16)
    r = orc.depth_map_filters(conf, idx, planes, 5, 5.0, 5, max_confidence=0.0)
    # (0,0) <- max_confidence = 0 is the minimum, everything else maps to 255; (0,0) -> 0
    assert r["confidence"][0, 0] == 0.0
    assert r["conf8"][0, 0] == 0 and (r["conf8"].reshape(-1)[1:] == 255).all()
    # nothing exceeds its neighbourhood mean by C -- except next to the zeroed pixel (0,0), whose
    # neighbours see a lowered mean (a quirk of :393-396), and those lie in the removed border
    assert not r["mask"].any()
    assert not r["idx_filtered"][6:, :].any() and not r["idx_filtered"][:, 6:].any()
    assert r["idx_filtered"][1, 1] == 7             # the median ran on the mask BEFORE border removal
    assert (r["depth"][6:, 6:] == planes[0]).all()  # empty windows -> median 0 (median_filtering.cpp:7-18)


def test_isolated_peak_is_selected_and_border_removed():
    conf = np.zeros((21, 21), np.float32)
    conf[10, 10] = 100.0
    conf[1, 10] = 100.0                              # inside the removed boundary (border = 2)
    idx = np.full((21, 21), 3, np.uint8)
    idx[10, 10] = 9
    planes = orc.depth_planes(1.0, 5.0, 16)
    r = orc.depth_map_filters(conf, idx, planes, 5, 4.0, 5, max_confidence=100.0)
    assert r["conf8"][10, 10] == 255 and r["conf8"][0, 0] == 0
    # mean at the peak = 255 * 0.375^2 = 35.86 -> 36; 255 - 36 > 4
    assert r["mask"][10, 10] == 1 and r["mask"].sum() == 1
    assert r["mask"][1, 10] == 0                     # x<=2 | y<=2 | ... cleared (:316-329)
    # the median used the mask BEFORE the border removal: windows containing (1,10) or (10,10)
    assert r["idx_filtered"][10, 10] == 9 and r["idx_filtered"][12, 12] == 9
    assert r["idx_filtered"][1, 10] == 3 and r["idx_filtered"][20, 20] == 0
    assert r["depth"][10, 10] == planes[9]


def test_median_definition_even_count():
    """compute_median_histogram: smallest v with cumulative count >= (num+1)/2 (lower median)."""
    conf = np.zeros((9, 9), np.float32)
    idx = np.zeros((9, 9), np.uint8)
    for (y, x, c, v) in [(4, 3, 50, 10), (4, 4, 60, 20), (4, 5, 70, 30), (3, 4, 80, 40)]:
        conf[y, x], idx[y, x] = c, v
    r = orc.depth_map_filters(conf, idx, orc.depth_planes(1, 5, 64), 3, 1.0, 3, max_confidence=80.0)
    assert r["mask"][4, 3] == r["mask"][4, 4] == r["mask"][4, 5] == r["mask"][3, 4] == 1
    assert r["idx_filtered"][4, 4] == 20             # values {10,20,30,40}: middle = 2 -> 20


def test_max_confidence_caps_the_range():
    rng = np.random.default_rng(2)
    conf = rng.gamma(1.0, 3.0, (30, 40)).astype(np.float32)
    idx = rng.integers(0, 50, (30, 40)).astype(np.uint8)
    lo = orc.depth_map_filters(conf, idx, orc.depth_planes(1, 5, 64), 5, 4.0, 5, max_confidence=0.0)
    hi = orc.depth_map_filters(conf, idx, orc.depth_planes(1, 5, 64), 5, 4.0, 5, max_confidence=10 * conf.max())
    assert hi["conf8"].max() <= 26                   # 255 / 10
    assert hi["mask"].sum() < lo["mask"].sum()       # "pixels with few votes" no longer look confident


@pytest.mark.gpu
@pytest.mark.parametrize("ksize,C_,med", [(5, 4.0, 5), (3, 2.0, 3), (7, 5.0, 9), (5, 4.5, 1), (9, 3.0, 5)])
def test_hip_filters_match_oracle(ctx, ksize, C_, med):
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import synthetic as syn
    rig = syn.stereo_rig(60000, width=120, height=90, duration=0.3, seed=5)
    m = d.MapperEMVS(ctx, rig["cam"], d.ShapeDSI(0, 0, 40, 4.0, 200.0, 0.0))
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    _, conf, idx = m.getDepthMapFromDSI()
    for max_conf in (0.0, 60.0):
        ref = orc.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf)
        depth, conf2, mask = m.getDepthMapFromDSI(options_depth_map=d.OptionsDepthMap(ksize, C_, med, max_conf))
        assert np.array_equal(conf2, ref["confidence"])
        assert np.array_equal(mask, ref["mask"]), "mask differs at %d pixels" % (mask != ref["mask"]).sum()
        assert np.array_equal(m.depth_cell_indices_filtered, ref["idx_filtered"])
        assert np.array_equal(depth, ref["depth"])
        if ksize <= 7:
            assert mask.sum() > 0
    with pytest.raises(d.DsiError):
        m.getDepthMapFromDSI(options_depth_map=d.OptionsDepthMap(4, 4.0, 5, 0.0))   # even kernel
    m.close()


# ---------------------------------------------------------------------------------------------------------------------
# The kernels against BOTH references at the shapes, options and ties of tests/filters_cases.py (the matrix that
# test_filters_reference_cpu.py runs on the CPU), through the existing ABI: an arbitrary (confidence, index) image is
# the arg-max of a volume that is zero except v[idx[y, x], y, x] = conf[y, x].
import filters_cases as fc          # noqa: E402
import filters_reference as fr      # noqa: E402

OUTPUTS = ("confidence", "mask", "idx_filtered", "depth")


def _mapper(ctx, shape, nz=256):
    import dvs_mcemvs_amd as d
    ny, nx = shape
    cam = (nx, ny, 100.0, 100.0, 0.5 * (nx + 1), 0.5 * (ny + 1))
    return d.MapperEMVS(ctx, cam, d.ShapeDSI(nx, ny, nz, 1.0, 5.0, 0.0))


def _plant(m, conf, idx, volume=None):
    """Upload the volume whose arg-max is (conf, idx) into the mapper's DSI and check that it is."""
    assert ((conf > 0) | (idx == 0)).all()
    if volume is None:
        volume = np.zeros(m.dsi_.shape, np.float32)
    else:
        volume.fill(0)
    assert int(idx.max()) < volume.shape[0]
    np.put_along_axis(volume, idx[None].astype(np.intp), conf[None], axis=0)
    m.dsi_.upload(volume)
    depth, raw_conf, raw_idx = m.getDepthMapFromDSI()
    assert np.array_equal(raw_conf, conf) and np.array_equal(raw_idx, idx)
    assert np.array_equal(depth, m.raw_depths_vec_[idx])
    return volume


def _filtered(m, opts, through_filter=False):
    """The engine's filtered outputs as the references' dict."""
    if through_filter:
        depth, conf, mask = m.filterDepthMap(opts)
    else:
        depth, conf, mask = m.getDepthMapFromDSI(options_depth_map=opts)
    return {"depth": depth, "confidence": conf, "mask": mask, "idx_filtered": m.depth_cell_indices_filtered}


def _assert_same(got, ref, where, what):
    for key in OUTPUTS:
        assert np.array_equal(got[key], ref[key]), "%s: %s differs from the %s at %d pixels" % (
            where, key, what, (got[key] != ref[key]).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_hip_filters_match_both_references(ctx, shape):
    """Every case of the CPU matrix: the kernels == the oracle == the restatement (with mean (a)), bit for bit, on
    confidence, mask, filtered indices and depth.  The float64 comparison of mean (a) needs no GPU and stays in
    test_filters_reference_cpu.py."""
    import dvs_mcemvs_amd as d
    m = _mapper(ctx, shape)
    volume, n = None, 0
    for name, conf, idx, options in fc.cases(shape):
        volume = _plant(m, conf, idx, volume)
        for ksize, C_, med, max_conf in options:
            where = "%s %s ksize=%d C=%g median=%d max_confidence=%g" % (shape, name, ksize, C_, med, max_conf)
            got = _filtered(m, d.OptionsDepthMap(ksize, C_, med, max_conf))
            _assert_same(got, orc.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf), where, "oracle")
            _assert_same(got, fr.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf, walk=False),
                         where, "restatement")
            n += 1
    m.close()
    print("%s: %d cases" % (shape, n))


@pytest.mark.gpu
@pytest.mark.parametrize("side,ksize,med", [(1024, 5, 5), (512, 9, 9)])
def test_hip_filters_large_images(ctx, side, ksize, med):
    """Grid-size arithmetic: many tiles in both directions (16 planes keep the planted volume small)."""
    import dvs_mcemvs_amd as d
    m = _mapper(ctx, (side, side), nz=16)
    rng = np.random.default_rng(side)
    conf = rng.gamma(1.0, 3.0, (side, side)).astype(np.float32)
    idx = rng.integers(0, 16, (side, side)).astype(np.uint8)
    idx[conf == 0] = 0
    _plant(m, conf, idx)
    for C_, max_conf in ((5.0, 0.0), (4.5, 20.0)):
        where = "%d x %d ksize=%d C=%g" % (side, side, ksize, C_)
        got = _filtered(m, d.OptionsDepthMap(ksize, C_, med, max_conf))
        assert got["mask"].sum() > 1000
        _assert_same(got, orc.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf), where, "oracle")
        _assert_same(got, fr.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf, walk=False),
                     where, "restatement")
    m.close()


@pytest.fixture(scope="module")
def stereo(ctx):
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import synthetic as syn
    rig = syn.stereo_rig(40000, width=96, height=72, duration=0.3, seed=11, n_points=800)
    shape = d.ShapeDSI(0, 0, 32, 4.0, 150.0, 0.0)
    mappers, batches = [], []
    for c in range(2):
        first, Rt = d.packetize(rig["events"][c][2], rig["trajectories"][c], rig["T_rv_w"])
        batches.append(d.EventBatch(ctx, rig["events"][c][0], rig["events"][c][1], Rt, first))
        mappers.append(d.MapperEMVS(ctx, rig["cam"], shape))
        mappers[c].evaluateDSI_batch(batches[c])
    yield rig, shape, mappers, batches
    for o in mappers + batches:
        o.close()


def _check_entry_point(m, where, ksize=9, C_=4.5, med=3):
    """m holds a raw map: filterDepthMap with a non-default option set == the restatement (and the oracle) applied to
    that raw map."""
    import dvs_mcemvs_amd as d
    _, conf, idx = m.fetchDepthMap()
    max_conf = 0.5 * float(conf.max())
    assert max_conf > 0
    got = _filtered(m, d.OptionsDepthMap(ksize, C_, med, max_conf), through_filter=True)
    assert got["confidence"][0, 0] == np.float32(max_conf)
    assert got["mask"].sum() > 0, where
    _assert_same(got, fr.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf), where, "restatement")
    _assert_same(got, orc.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf), where, "oracle")


@pytest.mark.gpu
def test_filter_after_compute_depth_map(ctx, stereo):
    rig, shape, mappers, batches = stereo
    mappers[0].computeDepthMap()
    _check_entry_point(mappers[0], "computeDepthMap")
    mappers[1].computeDepthMap(mappers[0].dsi_)                       # another mapper's grid
    _check_entry_point(mappers[1], "computeDepthMap(grid)", 15, 0.999, 9)


@pytest.mark.gpu
def test_filter_after_compute_depth_map_of_fusion(ctx, stereo):
    import dvs_mcemvs_amd as d
    rig, shape, mappers, batches = stereo
    out = d.MapperEMVS(ctx, rig["cam"], shape)
    out.computeDepthMapOfFusion(mappers[0].dsi_, mappers[1].dsi_, d.FUSE_HM)
    _check_entry_point(out, "computeDepthMapOfFusion")
    out.close()


@pytest.mark.gpu
def test_filter_after_compute_depth_map_of_events(ctx, stereo):
    import dvs_mcemvs_amd as d
    rig, shape, mappers, batches = stereo
    out = d.MapperEMVS(ctx, rig["cam"], shape)
    out.computeDepthMapOfEvents(mappers, batches, d.FUSE_HM)
    _check_entry_point(out, "computeDepthMapOfEvents")
    out.close()


@pytest.mark.gpu
def test_filter_after_compute_depth_map_of_events_alg2(ctx, stereo):
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import process
    rig, shape, _, _ = stereo
    cams = [d.MapperEMVS(ctx, rig["cam"], shape) for _ in range(2)]
    out_tc, out_ct = d.MapperEMVS(ctx, rig["cam"], shape), d.MapperEMVS(ctx, rig["cam"], shape)
    batches = process.alg2_window_batches(ctx, rig["events"], rig["trajectories"], rig["t0"] + 0.2, 2)
    out_tc.computeDepthMapOfEventsAlg2(out_ct, cams, batches, 2, d.FUSE_HM, d.FUSE_HM)
    _check_entry_point(out_tc, "computeDepthMapOfEventsAlg2 time_camera")
    _check_entry_point(out_ct, "computeDepthMapOfEventsAlg2 camera_time", 7, 0.999, 5)
    for o in batches + cams + [out_tc, out_ct]:
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4])
def test_focus_methods_with_options(ctx, stereo, method):
    """getDepthMapFromDSI(method, options) == the restatement applied to getDepthMapFromDSI(method)'s raw map."""
    import dvs_mcemvs_amd as d
    rig, shape, mappers, batches = stereo
    m = mappers[0]
    _, conf, idx = m.getDepthMapFromDSI(method=method)
    assert np.isfinite(conf).all()
    ksize, C_, med, max_conf = 9, 4.5, 3, 0.5 * float(conf.max())
    depth, conf2, mask = m.getDepthMapFromDSI(options_depth_map=d.OptionsDepthMap(ksize, C_, med, max_conf), method=method)
    got = {"depth": depth, "confidence": conf2, "mask": mask, "idx_filtered": m.depth_cell_indices_filtered}
    assert mask.sum() > 0
    _assert_same(got, fr.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf), "method %d" % method,
                 "restatement")
    _assert_same(got, orc.depth_map_filters(conf, idx, m.raw_depths_vec_, ksize, C_, med, max_conf), "method %d" % method,
                 "oracle")


@pytest.mark.gpu
def test_filter_state_handling(ctx, stereo):
    """An asynchronous fetch of the raw map followed at once by the filters still delivers the RAW confidence; the
    filters consume the raw map; they leave the DSI alone."""
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import engine
    rig, shape, mappers, batches = stereo
    m = mappers[0]
    before = m.dsi_.download()
    m.computeDepthMap()
    raw = m.fetchDepthMap()
    pins = [d.PinnedArray(raw[0].shape, t) for t in (np.float32, np.float32, np.uint8)]
    for p in pins:
        p.a[...] = 0
    opts = d.OptionsDepthMap(9, 4.5, 3, 0.5 * float(raw[1].max()))
    m.fetchDepthMapAsync(*[p.a for p in pins])
    depth, conf, mask = m.filterDepthMap(opts)                          # at once: no fetchWait in between
    m.fetchWait()
    for p, w in zip(pins, raw):
        assert np.array_equal(p.a, w)                                   # (0,0) of the confidence is NOT max_confidence
    assert conf[0, 0] == np.float32(opts.max_confidence) != raw[1][0, 0]
    with pytest.raises(d.DsiError) as e:                                # no new raw map: refused
        m.filterDepthMap(opts)
    assert e.value.code == engine.ERR_INVALID
    assert np.array_equal(m.dsi_.download(), before)
    m.computeDepthMap()                                                 # a new raw map: the same answer again
    again = m.filterDepthMap(opts)
    for g, w in zip(again, (depth, conf, mask)):
        assert np.array_equal(g, w)
    for p in pins:
        p.close()


@pytest.mark.gpu
def test_option_checks_at_the_abi(ctx):
    """Even, 0, negative and too large sizes are refused with DSI_ERR_INVALID, through both entry points.  ksize 1 is
    accepted: the mean is the pixel itself, so the mask before the border removal is (0 > -ceil(-C)) everywhere."""
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import engine
    shape = (12, 20)
    m = _mapper(ctx, shape)
    conf, idx = fc.image("gamma", shape)
    _plant(m, conf, idx)
    bad = [(4, 5), (0, 5), (-3, 5), (65, 5), (5, 4), (5, 0), (5, -3), (5, 33)]
    for ksize, med in bad:
        for call in (lambda o: m.getDepthMapFromDSI(options_depth_map=o), m.filterDepthMap):
            m.computeDepthMap()
            with pytest.raises(d.DsiError) as e:
                call(d.OptionsDepthMap(ksize, 5.0, med, 0.0))
            assert e.value.code == engine.ERR_INVALID, (ksize, med)
    m.computeDepthMap()
    m.filterDepthMap(d.OptionsDepthMap(63, 5.0, 31, 0.0))               # the largest sizes are accepted
    interior = np.zeros(shape, np.uint8)
    interior[2:-1, 2:-1] = 1                                            # border max(1 // 2, 1) = 1 clears x <= 1 and x >= nx - 1
    for C_, value in ((-2.0, 1), (-0.5, 1), (0.0, 0), (5.0, 0)):
        got = _filtered(m, d.OptionsDepthMap(1, C_, 1, 0.0))
        assert np.array_equal(got["mask"], interior * value), C_
        # median 1 on an all-one mask is the identity; on an empty mask it is 0
        assert np.array_equal(got["idx_filtered"], idx if value else np.zeros_like(idx))
        _assert_same(got, fr.depth_map_filters(conf, idx, m.raw_depths_vec_, 1, C_, 1, 0.0), "ksize 1", "restatement")
    m.close()


@pytest.mark.gpu
def test_argmax_never_selects_a_nan(ctx):
    """The collapse compares with a strict `best < v` from plane 0 on (std::max_element, cartesian3dgrid.cpp:132): a NaN
    in any later plane is never selected, so the filters never see one from there.  (A NaN in plane 0 is the initial
    `best`, beats nothing and loses to nothing, and comes out -- exactly like std::max_element.)"""
    m = _mapper(ctx, (6, 70), nz=8)
    rng = np.random.default_rng(8)
    v = rng.random(m.dsi_.shape).astype(np.float32)
    holes = rng.random(v.shape) < 0.3
    holes[0] = False
    m.dsi_.upload(np.where(holes, np.nan, v).astype(np.float32))
    _, conf, idx = m.getDepthMapFromDSI()
    clean = np.where(holes, -np.inf, v)
    assert not np.isnan(conf).any() and np.array_equal(idx, clean.argmax(axis=0)) and np.array_equal(conf, clean.max(axis=0))
    m.close()
