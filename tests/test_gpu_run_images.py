"""The run's pictures on the MI355X: the event image of accumulateEvents and the two images of saveDepthMaps,
engine against the numpy restatement of tests/run_images_reference.py, byte for byte; the batch, device-output and
device-resident forms against the host forms; the window stream with save_images; the reference-spelled C++ call sites."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import run_images_reference as rr
from dvs_mcemvs_amd import engine, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENSORS = ((70, 5), (346, 260))
MIN_DEPTH, MAX_DEPTH = 4.0, 200.0


def code_of(fn):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code


def batch_of(ctx, x, y):
    return d.EventBatch(ctx, x, y, np.zeros((0, 12), F))               # a batch without packets: the events are all it holds


def check_event_image(ctx, x, y, pol, width, height):
    """Host-array form and batch form against the restatement, with and without polarity; returns the polarity image."""
    x, y = np.asarray(x, np.uint16), np.asarray(y, np.uint16)
    b = batch_of(ctx, x, y)
    first = None
    for use_polarity in (True, False):
        want, want_dropped = rr.event_image(x, y, pol, width, height, use_polarity)
        got, dropped = d.accumulate_events(ctx, x, y, pol, width, height, use_polarity, return_dropped=True)
        assert got.shape == (height, width) and got.dtype == np.uint8
        assert np.array_equal(got, want), "use_polarity=%r: %d pixels differ" % (use_polarity, (got != want).sum())
        assert dropped == want_dropped
        got_b, dropped_b = b.event_image(pol, width, height, use_polarity, return_dropped=True)
        assert np.array_equal(got_b, want) and dropped_b == want_dropped
        first = got if first is None else first
    b.close()
    return first


# ------------------------------------------------------------------------------------------------ event images
@pytest.mark.parametrize("n", [0, 1, 1023, 100_000])
@pytest.mark.parametrize("sensor", SENSORS)
def test_event_image_random(ctx, sensor, n):
    """Random events, a few of them outside the sensor (n_dropped); n = 1023: 127 groups of eight and a tail of seven."""
    width, height = sensor
    rng = np.random.default_rng(100 + n + width)
    x = rng.integers(0, width + 3, n).astype(np.uint16)
    y = rng.integers(0, height + 1, n).astype(np.uint16)
    pol = rng.random(n) < 0.55
    img = check_event_image(ctx, x, y, pol, width, height)
    if n == 0:
        assert (img == 128).all()
    if n == 100_000:
        assert rr.event_image(x, y, pol, width, height)[1] > 0 and (img.min() == 0 or img.max() == 255)


@pytest.mark.parametrize("sensor", SENSORS)
def test_event_image_contention_on_16_pixels(ctx, sensor):
    """All 100,000 events on 16 pixels: 6,250 atomics per counter."""
    width, height = sensor
    rng = np.random.default_rng(3)
    px = rng.choice(width * height, 16, replace=False)
    pick = px[rng.integers(0, 16, 100_000)]
    x, y = (pick % width).astype(np.uint16), (pick // width).astype(np.uint16)
    img = check_event_image(ctx, x, y, rng.random(100_000) < 0.5, width, height)
    assert (img != 128).sum() <= 16
    img = check_event_image(ctx, x, y, np.ones(100_000, bool), width, height)     # 6,250 +- per pixel, all positive
    assert (img > 128).sum() == 16


@pytest.mark.parametrize("sensor", SENSORS)
def test_event_image_all_negative_and_cancelling(ctx, sensor):
    width, height = sensor
    rng = np.random.default_rng(4)
    x = rng.integers(0, width, 5000).astype(np.uint16)
    y = rng.integers(0, height, 5000).astype(np.uint16)
    x[(x == 0) & (y == 0)] = 1                                         # pixel (0, 0) stays untouched
    img = check_event_image(ctx, x, y, np.zeros(5000, bool), width, height)
    assert img.min() == 0 and img.max() == 128 and img[0, 0] == 128    # -half is 0, an untouched pixel stays 128
    # equal numbers of both polarities on every touched pixel: half == 0, 128 everywhere
    x2, y2 = np.concatenate([x, x]), np.concatenate([y, y])
    pol = np.concatenate([np.ones(5000, bool), np.zeros(5000, bool)])
    img = check_event_image(ctx, x2, y2, pol, width, height)
    assert (img == 128).all()


@pytest.mark.parametrize("sensor", SENSORS)
def test_event_image_rounding_ties(ctx, sensor):
    """256 positive events on one pixel: a = 0.5, so one event is 128.5 -> 128 and three are 129.5 -> 130."""
    width, height = sensor
    x = np.array([5] * 256 + [6] + [7] * 3, np.uint16)
    y = np.full(260, height - 1, np.uint16)
    img = check_event_image(ctx, x, y, np.ones(260, bool), width, height)
    assert list(img[height - 1, 5:8]) == [255, 128, 130]
    assert (np.delete(img.ravel(), (height - 1) * width + np.arange(5, 8)) == 128).all()


@pytest.mark.parametrize("sensor", SENSORS)
def test_event_image_dropped_events(ctx, sensor):
    width, height = sensor
    x = np.array([0, width, width - 1, 65535, 3, 3], np.uint16)
    y = np.array([0, 0, height, 65535, height - 1, height], np.uint16)
    pol = np.ones(6, bool)
    got, dropped = d.accumulate_events(ctx, x, y, pol, width, height, True, return_dropped=True)
    assert dropped == 4 and (got == 255).sum() == 2 and got[0, 0] == 255 and got[height - 1, 3] == 255
    check_event_image(ctx, x, y, pol, width, height)
    # every event outside: an empty image
    got, dropped = d.accumulate_events(ctx, x[[1, 3]], y[[1, 3]], pol[:2], width, height, True, return_dropped=True)
    assert dropped == 2 and (got == 128).all()


@pytest.mark.parametrize("sensor", SENSORS)
def test_event_image_without_polarity_wraps(ctx, sensor):
    """Pixels holding 255, 256 and 257 events read 255, 0 and 1 after the reference's uchar wrap."""
    width, height = sensor
    x = np.array([1] * 255 + [2] * 256 + [3] * 257, np.uint16)
    y = np.full(x.shape[0], 2, np.uint16)
    got = d.accumulate_events(ctx, x, y, None, width, height, False)
    assert list(got[2, 1:4]) == [255, 0, 1] and got.sum() == 256
    check_event_image(ctx, x, y, np.ones(x.shape[0], bool), width, height)


def test_event_image_dev_forms_match_host_form(ctx):
    """The device-output forms, written into the memory of a grid (zeroed when created); the count at byte 4096."""
    L = d.load_library()
    rng = np.random.default_rng(6)
    for width, height in ((70, 5), (71, 5)):                           # 350 bytes: 87 words and a tail of two; 355: tail of three
        n = 3001
        x = rng.integers(0, width + 2, n).astype(np.uint16)
        y = rng.integers(0, height, n).astype(np.uint16)
        pol = (rng.random(n) < 0.5).astype(np.uint8)
        out = d.Grid3D(ctx, 64, 8, 4)                                  # 8 KiB
        b = batch_of(ctx, x, y)
        for use_polarity in (1, 0):
            want, want_dropped = d.accumulate_events(ctx, x, y, pol, width, height, bool(use_polarity), return_dropped=True)
            assert want_dropped > 0
            calls = (lambda o, c: L.dsi_event_image_dev(ctx._h, engine._ptr(x, ctypes.c_uint16), engine._ptr(y, ctypes.c_uint16),
                                                        engine._ptr(pol, ctypes.c_uint8), n, width, height, use_polarity, o, c),
                     lambda o, c: L.dsi_batch_event_image_dev(b._h, engine._ptr(pol, ctypes.c_uint8), width, height,
                                                              use_polarity, o, c))
            for call in calls:
                out.resetGrid()
                engine._check(call(ctypes.c_void_p(out.device_ptr), ctypes.c_void_p(out.device_ptr + 4096)))
                ctx.synchronize()
                raw = out.download().view(np.uint8).ravel()
                assert np.array_equal(raw[:width * height].reshape(height, width), want)
                assert not raw[width * height:4096].any()              # nothing behind the image
                assert int(raw[4096:4100].view(np.uint32)[0]) == want_dropped
                engine._check(call(ctypes.c_void_p(out.device_ptr), None))       # the count is optional
                assert call(ctypes.c_void_p(out.device_ptr + 2), None) == engine.ERR_INVALID
                assert b"4-byte aligned" in L.dsi_last_error()
        ctx.synchronize()
        b.close()
        out.close()


def test_event_image_error_returns(ctx):
    L = d.load_library()
    x = np.zeros(4, np.uint16)
    pol = np.ones(4, np.uint8)
    out = np.zeros(64, np.uint8)
    xp, pp, op = engine._ptr(x, ctypes.c_uint16), engine._ptr(pol, ctypes.c_uint8), engine._ptr(out, ctypes.c_uint8)
    for width, height in ((0, 4), (4, 0), (-1, 4)):
        assert L.dsi_event_image(ctx._h, xp, xp, pp, 4, width, height, 1, op, None) == engine.ERR_INVALID
    assert L.dsi_event_image(ctx._h, xp, xp, None, 4, 4, 4, 1, op, None) == engine.ERR_INVALID     # polarity missing
    assert L.dsi_event_image(ctx._h, xp, xp, None, 4, 4, 4, 0, op, None) == engine.OK              # ... and not needed
    assert L.dsi_event_image(ctx._h, None, None, None, 4, 4, 4, 0, op, None) == engine.ERR_INVALID
    # an empty event list needs no array at all: 128 everywhere with polarity, 0 without
    for use_polarity, want in ((1, 128), (0, 0)):
        out[:] = 77
        assert L.dsi_event_image(ctx._h, None, None, None, 0, 4, 4, use_polarity, op, None) == engine.OK
        assert (out[:16] == want).all() and (out[16:] == 77).all()
        e = batch_of(ctx, x[:0], x[:0])
        out[:] = 77
        assert L.dsi_batch_event_image(e._h, None, 4, 4, use_polarity, op, None) == engine.OK
        assert (out[:16] == want).all()
        e.close()
    assert L.dsi_event_image(ctx._h, xp, xp, pp, 1 << 31, 4, 4, 1, op, None) == engine.ERR_INVALID     # more than 2^31 - 1 events
    assert L.dsi_event_image(ctx._h, xp, xp, pp, 4, 4, 4, 1, None, None) == engine.ERR_INVALID
    b = batch_of(ctx, x, x)
    assert L.dsi_batch_event_image(b._h, None, 4, 4, 1, op, None) == engine.ERR_INVALID
    assert L.dsi_batch_event_image(b._h, pp, 4, 0, 1, op, None) == engine.ERR_INVALID
    assert L.dsi_batch_event_image(b._h, None, 4, 4, 0, op, None) == engine.OK
    b.close()
    with pytest.raises(ValueError):
        d.accumulate_events(ctx, x, x, None, 4, 4, True)
    with pytest.raises(ValueError):
        d.accumulate_events(ctx, x, x, pol[:3], 4, 4, True)
    assert code_of(lambda: d.accumulate_events(ctx, x, x, pol, 0, 4)) == engine.ERR_INVALID


# ------------------------------------------------------------------------------------------------ depth images
@pytest.fixture(scope="module")
def planes100(ctx):
    m = d.MapperEMVS(ctx, (346, 260, 200.0, 200.0, 173.0, 130.0), d.ShapeDSI(0, 0, 100, MIN_DEPTH, MAX_DEPTH, 0.0))
    z = m.raw_depths_vec_.copy()
    m.close()
    assert z.shape == (100,) and z[0] == F(MIN_DEPTH)
    return z


def depth_case(shape, planes, seed):
    """(depth, conf, mask) with the special pixels of the issue; shape at least 9 x 70."""
    rows, cols = shape
    rng = np.random.default_rng(seed)
    depth = rng.uniform(MIN_DEPTH, MAX_DEPTH / 4, shape).astype(F)
    conf = rng.gamma(1.0, 3.0, shape).astype(F)
    mask = np.where(rng.random(shape) < 0.3, rng.choice(np.array([1, 255], np.uint8), shape), 0).astype(np.uint8)
    for r, c in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):    # a masked pixel in each corner
        mask[r, c] = 255 if (r + c) & 1 else 1
    # two adjacent masked pixels with different colours, alone in their neighbourhood
    mask[2:7, 8:14] = 0
    mask[4, 10], mask[4, 11] = 1, 255
    depth[4, 10], depth[4, 11] = MIN_DEPTH, MAX_DEPTH
    # depths at the limits, outside both, 0 and NaN (masked), and every plane of a 100-plane shape
    special = np.array([MIN_DEPTH, MAX_DEPTH, 3.0, 300.0, 0.0, np.nan, -5.0, np.inf, 1e-39], F)
    depth[1, 20:20 + special.size] = special
    mask[1, 20:20 + special.size] = 1
    depth[7:9, 10:60] = planes.reshape(2, 50)
    mask[7:9, 10:60] = 255
    return depth, conf, mask


@pytest.mark.parametrize("shape", [(9, 70), (260, 346)])
def test_depth_images_against_restatement(ctx, planes100, shape):
    rng = np.random.default_rng(11)
    depth, conf, mask = depth_case(shape, planes100, 12 + shape[0])
    random_lut = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    for lut in (None, random_lut):
        neg, bgr = d.depth_images(ctx, depth, conf, mask, MIN_DEPTH, MAX_DEPTH, lut)
        assert neg.shape == shape and bgr.shape == shape + (3,) and neg.dtype == bgr.dtype == np.uint8
        assert np.array_equal(neg, rr.conf_negated(conf))
        want = rr.inv_depth_colored_dilated(depth, mask, MIN_DEPTH, MAX_DEPTH, lut)
        assert np.array_equal(bgr, want), "%d pixels differ" % (bgr != want).any(axis=2).sum()
        table = rr.default_jet_lut() if lut is None else lut
        # the adjacent pair: both read the per-channel maximum of the two colours; their outer neighbours one colour each
        both = np.maximum(table[255], table[0])
        assert np.array_equal(bgr[4, 10], both) and np.array_equal(bgr[4, 11], both)
        assert np.array_equal(bgr[4, 9], table[255]) and np.array_equal(bgr[4, 12], table[0])
        assert np.array_equal(bgr[3, 10], table[255]) and np.array_equal(bgr[5, 11], table[0])
        assert not bgr[3, 12].any() and not bgr[5, 9].any()
        # a corner sees itself and its two neighbours inside the image
        undilated = rr.inv_depth_colored(depth, mask, MIN_DEPTH, MAX_DEPTH, lut)
        assert np.array_equal(bgr[0, 0], np.maximum(undilated[0, 0], np.maximum(undilated[0, 1], undilated[1, 0])))
        assert np.array_equal(bgr[-1, -1], np.maximum(undilated[-1, -1], np.maximum(undilated[-1, -2], undilated[-2, -1])))
    # every plane depth of the 100-plane shape indexes the table like the restatement (near plane 255, far side low)
    idx = rr.inv_depth_index(planes100, MIN_DEPTH, MAX_DEPTH)
    assert idx[0] == 255 and (np.diff(idx.astype(int)) <= 0).all() and idx[-1] <= 1
    # either output alone
    L = d.load_library()
    only = np.zeros(shape, np.uint8)
    engine._check(L.dsi_depth_images(ctx._h, None, engine._ptr(conf, ctypes.c_float), None, shape[0], shape[1], 0.0, 0.0, None,
                                     engine._ptr(only, ctypes.c_uint8), None))
    assert np.array_equal(only, rr.conf_negated(conf))
    only3 = np.zeros(shape + (3,), np.uint8)
    engine._check(L.dsi_depth_images(ctx._h, engine._ptr(depth, ctypes.c_float), None, engine._ptr(mask, ctypes.c_uint8), shape[0],
                                     shape[1], MIN_DEPTH, MAX_DEPTH, None, None, engine._ptr(only3, ctypes.c_uint8)))
    assert np.array_equal(only3, rr.inv_depth_colored_dilated(depth, mask, MIN_DEPTH, MAX_DEPTH))


@pytest.mark.parametrize("shape", [(9, 70), (260, 346)])
def test_conf_negated_constant_and_tie(ctx, planes100, shape):
    depth, _, mask = depth_case(shape, planes100, 5)
    neg, _ = d.depth_images(ctx, depth, np.full(shape, 7.5, F), mask, MIN_DEPTH, MAX_DEPTH)
    assert (neg == 255).all()                                          # a constant map: scale 0
    conf = np.zeros(shape, F)
    conf[0, :4] = (0.0, 2.0, 1.0, 0.5)                                 # 255 - (0, 255, 127.5, 63.75): the tie goes to 128
    conf[-1, -1] = 1.0
    neg, _ = d.depth_images(ctx, depth, conf, mask, MIN_DEPTH, MAX_DEPTH)
    assert list(neg[0, :4]) == [255, 0, 128, 191] and neg[-1, -1] == 128
    assert np.array_equal(neg, rr.conf_negated(conf))


def test_mapper_depth_images_equal_host_form(ctx):
    """After a real getDepthMapFromDSI (the synthetic DSI of the filter tests): the device-resident form gives the bytes
    of the host form fed with what that call returned, and of the restatement."""
    rig = syn.stereo_rig(60000, width=120, height=90, duration=0.3, seed=5)
    m = d.MapperEMVS(ctx, rig["cam"], d.ShapeDSI(0, 0, 40, MIN_DEPTH, MAX_DEPTH, 0.0))
    assert code_of(lambda: m.depthImages(MIN_DEPTH, MAX_DEPTH)) == engine.ERR_INVALID     # nothing computed yet
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    rng = np.random.default_rng(2)
    lut = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    for max_conf in (0.0, 60.0):
        depth, conf, mask = m.getDepthMapFromDSI(options_depth_map=d.OptionsDepthMap(5, 4.0, 5, max_conf))
        assert 0 < (mask > 0).sum() < mask.size
        for table in (None, lut):
            neg, bgr = m.depthImages(MIN_DEPTH, MAX_DEPTH, table)
            hneg, hbgr = d.depth_images(ctx, depth, conf, mask, MIN_DEPTH, MAX_DEPTH, table)
            assert np.array_equal(neg, hneg) and np.array_equal(bgr, hbgr)
            assert np.array_equal(neg, rr.conf_negated(conf))
            assert np.array_equal(bgr, rr.inv_depth_colored_dilated(depth, mask, MIN_DEPTH, MAX_DEPTH, table))
        assert bgr.any()
    # through filterDepthMap as well; a new raw depth map invalidates the maps
    m.computeDepthMap()
    assert code_of(lambda: m.depthImages(MIN_DEPTH, MAX_DEPTH)) == engine.ERR_INVALID
    depth, conf, mask = m.filterDepthMap(d.OptionsDepthMap(5, 4.0, 5, 0.0))
    neg, bgr = m.depthImages(MIN_DEPTH, MAX_DEPTH)
    hneg, hbgr = d.depth_images(ctx, depth, conf, mask, MIN_DEPTH, MAX_DEPTH)
    assert np.array_equal(neg, hneg) and np.array_equal(bgr, hbgr)
    m.close()


def test_depth_images_error_returns(ctx):
    L = d.load_library()
    f = np.ones((4, 4), F)
    u = np.ones((4, 4), np.uint8)
    o = np.zeros((4, 4, 3), np.uint8)
    fp, up, op = engine._ptr(f, ctypes.c_float), engine._ptr(u, ctypes.c_uint8), engine._ptr(o, ctypes.c_uint8)
    assert L.dsi_depth_images(ctx._h, fp, fp, up, 4, 4, 4.0, 200.0, None, op, op) == engine.OK
    for rows, cols in ((0, 4), (4, 0), (-1, 4)):
        assert L.dsi_depth_images(ctx._h, fp, fp, up, rows, cols, 4.0, 200.0, None, op, op) == engine.ERR_INVALID
    assert L.dsi_depth_images(ctx._h, fp, None, up, 4, 4, 4.0, 200.0, None, op, None) == engine.ERR_INVALID   # no confidence
    assert L.dsi_depth_images(ctx._h, None, fp, up, 4, 4, 4.0, 200.0, None, None, op) == engine.ERR_INVALID   # no depth
    assert L.dsi_depth_images(ctx._h, fp, fp, None, 4, 4, 4.0, 200.0, None, None, op) == engine.ERR_INVALID   # no mask
    for lo, hi in ((4.0, 4.0), (0.0, 200.0), (4.0, float("inf")), (float("nan"), 200.0), (-4.0, 200.0)):
        assert L.dsi_depth_images(ctx._h, fp, fp, up, 4, 4, lo, hi, None, None, op) == engine.ERR_INVALID
    assert L.dsi_depth_images(ctx._h, fp, fp, up, 4, 4, 4.0, 200.0, None, None, None) == engine.OK            # nothing asked
    with pytest.raises(ValueError):
        d.depth_images(ctx, f, f, u, 4.0, 200.0, lut=np.zeros((256, 4), np.uint8))
    with pytest.raises(ValueError):
        d.depth_images(ctx, f, f[:3], u, 4.0, 200.0)


# ------------------------------------------------------------------------------------------------ the window stream
def test_full_sequence_save_images(ctx, tmp_path):
    """Two windows of the small synthetic stream: each window's pictures equal the per-window host-form calls, the maps
    are those of a run without save_images, and the files carry the reference's names."""
    rig = syn.stereo_rig(60_000, width=96, height=72, t0=3.0, duration=0.6, seed=5)
    shape = d.ShapeDSI(0, 0, 24, 4.0, 100.0, 0.0)
    rng = np.random.default_rng(9)
    pols = [rng.random(rig["events"][c][0].shape[0]) < 0.5 for c in range(2)]
    cams = (rig["cam"],) * 2
    opts = d.OptionsDepthMap(5, 4.0, 5, 0.0)
    args = (ctx, cams, shape, rig["events"], rig["trajectories"], 3.0, 3.6, 0.3, 0.3)
    prefix = str(tmp_path / "run_")
    on = list(proc.full_sequence(*args, options_depth_map=opts, polarities=pols, save_images=True, out_path=prefix))
    off = list(proc.full_sequence(*args, options_depth_map=opts))
    assert len(on) == len(off) == 2
    names = set(os.listdir(str(tmp_path)))
    for w, p in zip(on, off):
        ts, depth, conf, mask, pics = w
        assert len(p) == 4 and ts == p[0]
        for a, b in zip(w[1:4], p[1:]):
            assert np.array_equal(a, b, equal_nan=True)
        assert sorted(pics) == ["confidence_negated", "event_images", "inv_depth_colored_dilated"]
        hneg, hbgr = d.depth_images(ctx, depth, conf, mask, 4.0, 100.0)
        assert np.array_equal(pics["confidence_negated"], hneg) and np.array_equal(pics["inv_depth_colored_dilated"], hbgr)
        assert np.array_equal(hneg, rr.conf_negated(conf))
        assert np.array_equal(hbgr, rr.inv_depth_colored_dilated(depth, mask, 4.0, 100.0)) and hbgr.any()
        assert len(pics["event_images"]) == 2
        for c in range(2):
            x, y, t = rig["events"][c]
            sel = slice(int(np.searchsorted(t, ts - 0.3, "left")), int(np.searchsorted(t, ts, "right")))
            wx, wy, _ = proc.window_events(rig["events"][c], ts - 0.3, ts)
            assert np.array_equal(wx, x[sel])
            host = d.accumulate_events(ctx, x[sel], y[sel], pols[c][sel], 96, 72, True)
            assert np.array_equal(pics["event_images"][c], host)
            assert np.array_equal(host, rr.event_image(x[sel], y[sel], pols[c][sel], 96, 72, True)[0])
            name = "run_" + "%f" % ts + "events_%d.png" % c
            assert name in names
            assert np.array_equal(rr.decode_png(open(str(tmp_path / name), "rb").read())[0], host)
        base = "run_" + "%013.9f" % ts
        for name in (base + "depth_points_fused_2.txt", base + "confidence_map_negated_fused_2.png",
                     base + "inv_depth_colored_dilated_fused_2.png"):
            assert name in names
        px, ctype = rr.decode_png(open(str(tmp_path / (base + "inv_depth_colored_dilated_fused_2.png")), "rb").read())
        assert ctype == 2 and np.array_equal(px, hbgr[:, :, ::-1])
    assert len(names) == 2 * 5
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, options_depth_map=opts, save_images=True))           # no polarities
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, polarities=pols, save_images=True))                  # no filtered maps


# ------------------------------------------------------------------------------------------------ C++ call sites
def test_cpp_call_sites(built, ctx, tmp_path):
    exe = str(tmp_path / "test_run_images")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_run_images.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    read = lambda name, dtype: np.fromfile(str(out / name), dtype)
    W, H = 70, 9
    x, y, p = read("events.x.u16", np.uint16), read("events.y.u16", np.uint16), read("events.p.u8", np.uint8)
    assert np.array_equal(read("event_image.u8", np.uint8).reshape(H, W), rr.event_image(x, y, p, W, H, True)[0])
    assert np.array_equal(read("event_image_nopol.u8", np.uint8).reshape(H, W), rr.event_image(x, y, p, W, H, False)[0])
    depth, conf = read("depth.f32", F).reshape(H, W), read("conf.f32", F).reshape(H, W)
    mask = read("mask.u8", np.uint8).reshape(H, W)
    neg, bgr = rr.conf_negated(conf), rr.inv_depth_colored_dilated(depth, mask, 4.0, 200.0)
    assert np.array_equal(read("neg.u8", np.uint8).reshape(H, W), neg)
    assert np.array_equal(read("bgr.u8", np.uint8).reshape(H, W, 3), bgr)
    for suffix in "abc":
        lines = open(str(out / ("depth_points_%s.txt" % suffix))).read().splitlines()
        rows, cols = np.nonzero(mask)
        assert lines == ["%d %d %g" % (c, r, depth[r, c]) for r, c in zip(rows, cols)]
        px, ctype = rr.decode_png(open(str(out / ("confidence_map_negated_%s.png" % suffix)), "rb").read())
        assert ctype == 0 and np.array_equal(px, neg)
        px, ctype = rr.decode_png(open(str(out / ("inv_depth_colored_dilated_%s.png" % suffix)), "rb").read())
        assert ctype == 2 and np.array_equal(px, bgr[:, :, ::-1])
