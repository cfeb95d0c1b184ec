"""Numpy restatement of the run's pictures, written from the reference's utils.cpp and the definitions of
include/dsi_engine.h, not from the engine's kernels:

  event_image            accumulateEvents                       utils.cpp:184-216
  conf_negated           saveDepthMaps, the negated confidence  utils.cpp:55-58
  inv_depth_colored      ... the coloured inverse depth         utils.cpp:82-90
  dilate_cross           cv::dilate with MORPH_ELLIPSE 3 x 3    utils.cpp:91-92
  default_jet_lut        the engine's default colour table (not OpenCV's COLORMAP_JET)

Every fp32 step is one numpy float32 operation (no fused multiply-add); scale and shift constants are formed in float64
and cast, as OpenCV's convertTo / normalize do."""
import struct
import zlib

import numpy as np

F = np.float32
DBL_EPSILON = 2.220446049250313e-16


def saturate_u8(v):
    """cv::saturate_cast<uchar>(float): round to nearest, ties to even, clamp to 0..255.  NaN is the caller's business."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        r = np.rint(v)
        r = np.where(r < 0, F(0), np.where(r > 255, F(255), r))
        return np.where(np.isnan(r), F(0), r).astype(np.uint8)


def event_counts(x, y, polarity, width, height, use_polarity):
    """(per-pixel integer image, number of events outside the sensor)."""
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    inside = (x < width) & (y < height)
    flat = (y * width + x)[inside]
    if use_polarity:
        w = np.where(np.asarray(polarity)[inside] != 0, 1, -1).astype(np.int64)
    else:
        w = np.ones(flat.shape[0], np.int64)
    c = np.zeros(width * height, np.int64)
    np.add.at(c, flat, w)
    return c.reshape(height, width), int((~inside).sum())


def normalize_minmax_coeffs(smin, smax):
    """cv::normalize(NORM_MINMAX, 0, 255): scale and shift in double, returned as the floats convertTo applies."""
    rng = float(smax) - float(smin)
    scale = 255.0 * (1.0 / rng if rng > DBL_EPSILON else 0.0)
    shift = 0.0 - float(smin) * scale
    return F(scale), F(shift)


def event_image(x, y, polarity, width, height, use_polarity=True):
    """(uint8 [height][width], n_dropped)."""
    c, dropped = event_counts(x, y, polarity, width, height, use_polarity)
    if use_polarity:
        half = max(abs(float(c.min())), abs(float(c.max())))
        if not half > 0:
            return np.full((height, width), 128, np.uint8), dropped
        a = F(128.0 / half)
        v = c.astype(F) * a
        v = v + F(128)
        return saturate_u8(v), dropped
    c8 = c % 256                                                       # uchar += 1 wraps
    a, b = normalize_minmax_coeffs(c8.min(), c8.max())
    v = c8.astype(F) * a
    v = v + b
    return saturate_u8(v), dropped


def conf_negated(conf):
    conf = np.asarray(conf, F)
    a, b = normalize_minmax_coeffs(conf.min(), conf.max())
    n = conf * a
    n = n + b
    return saturate_u8(F(255) - n)


def default_jet_lut():
    """256 x 3 uint8, B G R."""
    t = np.arange(256, dtype=np.float64) / 255.0
    ch = [1.5 - np.abs(4.0 * t - k) for k in (1.0, 2.0, 3.0)]          # b, g, r
    return np.stack([np.rint(np.clip(c, 0.0, 1.0) * 255.0) for c in ch], axis=1).astype(np.uint8)


def inv_depth_index(depth, min_depth, max_depth):
    s1 = 1.0 / float(F(max_depth))
    s2 = 1.0 / float(F(min_depth)) - s1
    k = 1.0 / s2
    a, b = F(k * 255.0), F(((-s1) * k) * 255.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F(1) / np.asarray(depth, F)
        v = inv * a
        v = v + b
    return np.where(np.isnan(v), np.uint8(0), saturate_u8(v))


def inv_depth_colored(depth, mask, min_depth, max_depth, lut=None):
    lut = default_jet_lut() if lut is None else np.asarray(lut, np.uint8).reshape(256, 3)
    img = lut[inv_depth_index(depth, min_depth, max_depth)]
    img[np.asarray(mask) == 0] = 0
    return img


def dilate_cross(img):
    """Per-channel maximum over the pixel and its 4-neighbours; nothing outside the image contributes."""
    img = np.asarray(img)
    out = img.copy()
    out[1:] = np.maximum(out[1:], img[:-1])
    out[:-1] = np.maximum(out[:-1], img[1:])
    out[:, 1:] = np.maximum(out[:, 1:], img[:, :-1])
    out[:, :-1] = np.maximum(out[:, :-1], img[:, 1:])
    return out


def inv_depth_colored_dilated(depth, mask, min_depth, max_depth, lut=None):
    return dilate_cross(inv_depth_colored(depth, mask, min_depth, max_depth, lut))


def decode_png(data):
    """(rows x cols [x 3] uint8, colour type) of an 8-bit PNG of colour type 0 or 2 whose scanlines all use filter 0."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(kind + body) & 0xffffffff)
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    cols, rows, depth, ctype, comp, flt, lace = hdr
    assert (depth, comp, flt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(rows, cols * ch + 1)
    assert not raw[:, 0].any()
    px = raw[:, 1:]
    return (px.reshape(rows, cols, 3) if ch == 3 else px.copy()), ctype
