"""A SECOND, independent restatement of the post-arg-max filters of MapperEMVS::getDepthMapFromDSI
(mapper_emvs_stereo.cpp:390-436), in numpy / scipy.  TEST INFRASTRUCTURE, like independent_numpy.py: it exists
so that a misreading would have to be made twice, in two differently shaped programs, to go unnoticed.  It is
written from what the OpenCV calls at :393-409 are documented to do (cv::normalize NORM_MINMAX, Mat::convertTo
with saturate_cast<uchar>, cv::adaptiveThreshold with ADAPTIVE_THRESH_GAUSSIAN_C / THRESH_BINARY,
cv::getGaussianKernel with sigma <= 0), from Huang, Yang and Tang's sliding-histogram median
(median_filtering.cpp:33-158) and from removeMaskBoundary (:316-329) -- and NOT from oracle/dsi_oracle.c, whose
shape (per-pixel loops, float accumulators, a saturate helper) it avoids on purpose:

  normalisation     whole-array fp32 operations, scale / shift as Python doubles
  Gaussian mean     ksize <= 7: INTEGER arithmetic on the integer tap tables (no float anywhere)
                    ksize >= 9: (a) the arithmetic the project defines, whole fp32 arrays accumulated tap by tap
                                (b) float64 separable correlation + the set of pixels (b) cannot decide
  threshold         Python / numpy integers
  median            (1) the definition: sort the window's masked values, take element (num + 1) // 2 - 1
                    (2) Huang's walk: one histogram, carried over the image in a serpentine scan
  border, depth     index grids and a table lookup

numpy float32 arithmetic is IEEE single with one rounding per operation; a product and a sum of whole arrays are
two separate passes, so no fused multiply-add can form.
"""
import math
import sys

import numpy as np
from scipy import ndimage

F = np.float32

# cv::getGaussianKernel's fixed tables for sigma <= 0 and ksize <= 7, as integers over a power of two
INT_TAPS = {1: ((1,), 1), 3: ((1, 2, 1), 4), 5: ((1, 4, 6, 4, 1), 16), 7: ((2, 7, 14, 18, 14, 7, 2), 64)}


def round_half_even_u8(v):
    """cvRound + saturate_cast<uchar> on a float array: nearest integer, ties to even, clamped to 0..255.  A NaN
    (0 * inf in the normalisation of an image holding +inf) becomes 0: cvRound's conversion instruction returns
    INT_MIN for it, which saturates to 0."""
    with np.errstate(invalid="ignore"):
        r = np.rint(v)                                   # ties to even
        r = np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0))
    return r.astype(np.uint8)


def scale_shift(conf, a, b):
    """conf * a + b as two separately rounded fp32 operations on whole arrays."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(conf, F) * F(a)).astype(F)       # one rounding
        return (v + F(b)).astype(F)                      # and another


def normalise(conf, max_confidence):
    """:393-397.  (confidence image with (0,0) overwritten, the u8 image, (a, b) as fp32 scalars)."""
    conf = np.array(conf, dtype=F, copy=True)
    conf[0, 0] = F(max_confidence)                       # :393
    smin, smax = float(np.min(conf)), float(np.max(conf))
    rng = smax - smin                                    # cv::normalize: doubles from here
    scale = 255.0 * ((1.0 / rng) if rng > sys.float_info.epsilon else 0.0)
    shift = 0.0 - smin * scale
    a, b = F(scale), F(shift)                            # convertTo applies them in the image's type
    v = scale_shift(conf, a, b)
    v[0, 0] = F(0)                                       # :396
    return conf, round_half_even_u8(v), (a, b)


def gaussian_taps(ksize):
    """cv::getGaussianKernel(ksize, sigma <= 0, CV_32F) for ksize >= 9: sigma from the size, exp in double,
    normalised by the reciprocal of the sum, rounded to fp32.  math.exp is the host's libm, which is what the
    engine and the oracle call."""
    sigma = 0.3 * ((ksize - 1) / 2 - 1) + 0.8
    s2 = -0.5 / (sigma * sigma)
    t = []
    for i in range(ksize):
        x = i - (ksize - 1) * 0.5
        t.append(math.exp(s2 * x * x))
    total = 0.0
    for v in t:
        total += v
    inv = 1.0 / total
    return np.array([F(v * inv) for v in t], dtype=F)


def gaussian_mean_int(conf8, ksize):
    """ksize in INT_TAPS: the 2-D weights are integers over den^2, the weighted sum of u8 values an integer below
    2^24 * den^2 / 4096 -- exact in any order, so one integer quotient rounded half to even IS the mean."""
    taps, den = INT_TAPS[ksize]
    r = ksize // 2
    w2 = np.outer(taps, taps).astype(np.int64)
    p = np.pad(conf8.astype(np.int64), r, mode="edge")   # BORDER_REPLICATE
    win = np.lib.stride_tricks.sliding_window_view(p, (ksize, ksize))
    s = np.einsum("yxij,ij->yx", win, w2)
    d = den * den
    q, rem = np.divmod(s, d)
    up = (2 * rem > d) | ((2 * rem == d) & (q % 2 == 1))
    return (q + up).astype(np.int64), s, d


def gaussian_mean_fp32(conf8, taps):
    """(a) the arithmetic the project defines: rows, then columns; taps in ascending order; per tap one rounded
    product and one rounded sum, on whole fp32 arrays; replicate border."""
    k = len(taps)
    r = k // 2
    ny, nx = conf8.shape
    p = np.pad(conf8.astype(F), ((0, 0), (r, r)), mode="edge")
    rows = np.zeros((ny, nx), F)
    for t in range(k):
        prod = (taps[t] * p[:, t:t + nx]).astype(F)
        rows = (rows + prod).astype(F)
    p = np.pad(rows, ((r, r), (0, 0)), mode="edge")
    acc = np.zeros((ny, nx), F)
    for t in range(k):
        prod = (taps[t] * p[t:t + ny, :]).astype(F)
        acc = (acc + prod).astype(F)
    return acc


def undecidable_bound(ksize):
    """Two sequential fp32 sums of ksize non-negative terms of magnitude <= 255: each product and each partial sum
    rounds once, relative 2^-24 of a value <= 255, so <= (ksize + 1) roundings per pass, two passes."""
    return 2.0 * (ksize + 1) * 2.0 ** -24 * 255.0


def gaussian_mean_f64(conf8, taps):
    """(b) float64 separable correlation with the fp32 taps; (mean, undecidable)."""
    w = taps.astype(np.float64)
    m = ndimage.correlate1d(conf8.astype(np.float64), w, axis=1, mode="nearest")
    m = ndimage.correlate1d(m, w, axis=0, mode="nearest")
    dist = np.abs(m - (np.floor(m) + 0.5))
    return m, dist <= undecidable_bound(len(taps))


def median_by_definition(idx, mask, size):
    """The masked in-image values of the size x size window, sorted; element (num + 1) // 2 - 1; 0 when num == 0."""
    p = size // 2
    v = np.where(mask > 0, idx.astype(np.int16), np.int16(256))
    v = np.pad(v, p, mode="constant", constant_values=256)   # outside the image: not a value
    win = np.lib.stride_tricks.sliding_window_view(v, (size, size))
    ny, nx = idx.shape
    out = np.zeros((ny, nx), np.uint8)
    for y0 in range(0, ny, 16):                              # (in slabs: the sorted copy is size^2 times the image)
        s = np.sort(win[y0:y0 + 16].reshape(-1, nx, size * size), axis=-1)
        num = (s < 256).sum(axis=-1)
        k = np.maximum((num + 1) // 2 - 1, 0)
        pick = np.take_along_axis(s, k[..., None], axis=-1)[..., 0]
        out[y0:y0 + 16] = np.where(num == 0, 0, pick).astype(np.uint8)
    return out


def median_by_histogram_walk(idx, mask, size):
    """Huang, Yang, Tang: ONE 256-bin histogram follows the window over the image -- right along the first row, down
    one row, left along the next, and so on; a step drops the strip that leaves and adds the strip that enters."""
    p = size // 2
    ny, nx = idx.shape
    v = np.where(mask > 0, idx.astype(np.int64), -1)
    hist = np.zeros(256, np.int64)

    def strip(y_lo, y_hi, x_lo, x_hi):                       # inclusive bounds, cut to the image
        y_lo, x_lo = max(y_lo, 0), max(x_lo, 0)
        y_hi, x_hi = min(y_hi, ny - 1), min(x_hi, nx - 1)
        if y_lo > y_hi or x_lo > x_hi:
            return np.zeros(256, np.int64)
        s = v[y_lo:y_hi + 1, x_lo:x_hi + 1].ravel()
        return np.bincount(s[s >= 0], minlength=256)

    def lower_median():
        num = int(hist.sum())
        return int(np.searchsorted(np.cumsum(hist), (num + 1) // 2, side="left"))   # first bin reaching the middle

    out = np.zeros((ny, nx), np.uint8)
    hist += strip(-p, p, -p, p)
    x, step = 0, 1
    for y in range(ny):
        while True:
            out[y, x] = lower_median()
            nxt = x + step
            if nxt < 0 or nxt >= nx:
                break
            leave = x - p if step > 0 else x + p
            enter = nxt + p if step > 0 else nxt - p
            hist -= strip(y - p, y + p, leave, leave)
            hist += strip(y - p, y + p, enter, enter)
            x = nxt
        if y + 1 < ny:
            hist -= strip(y - p, y - p, x - p, x + p)
            hist += strip(y + 1 + p, y + 1 + p, x - p, x + p)
            step = -step
    assert hist.min() >= 0
    return out


def depth_map_filters(conf, idx, raw_depths, ksize=5, C_=5.0, median_size=5, max_confidence=0.0, walk=True):
    """The dict of oracle.depth_map_filters (depth, confidence, mask, conf8, idx_filtered) plus mask_before_border,
    undecidable (all False for ksize <= 7), mean (the integer the threshold used) and, for ksize >= 9, mean64.
    walk=False skips the histogram walk (the two medians are otherwise asserted equal here)."""
    idx = np.ascontiguousarray(idx, np.uint8)
    confidence, conf8, _ = normalise(conf, max_confidence)
    out = {"confidence": confidence, "conf8": conf8}
    if ksize in INT_TAPS:
        mean, _, _ = gaussian_mean_int(conf8, ksize)
        out["undecidable"] = np.zeros(conf8.shape, bool)
    else:
        taps = gaussian_taps(ksize)
        mean = round_half_even_u8(gaussian_mean_fp32(conf8, taps)).astype(np.int64)
        out["mean64"], out["undecidable"] = gaussian_mean_f64(conf8, taps)
    out["mean"] = mean
    # cv::adaptiveThreshold(..., THRESH_BINARY, delta = -C): 1 where src - mean > -ceil(delta)
    idelta = math.ceil(-C_)
    before = (conf8.astype(np.int64) - mean > -idelta).astype(np.uint8)
    out["mask_before_border"] = before
    filt = median_by_definition(idx, before, median_size)     # :420-423, on the mask BEFORE the border removal
    if walk:
        assert np.array_equal(filt, median_by_histogram_walk(idx, before, median_size)), "the two medians differ"
    out["idx_filtered"] = filt
    border = max(ksize // 2, 1)                               # :426-427, removeMaskBoundary :316-329
    ny, nx = before.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    edge = (xx <= border) | (xx >= nx - border) | (yy <= border) | (yy >= ny - border)
    out["mask"] = np.where(edge, 0, before).astype(np.uint8)
    out["depth"] = np.asarray(raw_depths, F)[filt]            # :435
    return out
