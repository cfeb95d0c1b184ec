"""The case matrix of the depth-map filter tests (test_filters_reference_cpu.py on the CPU, test_depthmap_filters.py
on the GPU): shapes, option values, images built to sit on the filters' ties and edges, and the rule that picks
option sets.  TEST INFRASTRUCTURE.

Every image is a (confidence, index) pair that the arg-max of a volume can emit: confidence >= 0 and index 0
wherever the confidence is 0, so the GPU tests can plant it as v[idx[y, x], y, x] = conf[y, x].

The full product of the option values (8 x 7 x 6 x 4 per image, 13 images, 12 shapes) is about 210,000 filter runs; the
matrix below is a covering selection of it instead, fixed by seeds:
  * per shape, on the random-gamma image: EVERY (ksize, C) pair, with the median size and max_confidence cycling so
    that every median size and every max_confidence kind meets every ksize and every C;
  * per shape and per other image: a seeded draw of option sets from the product (6 below 5,000 pixels, 3 or 2 above);
  * per tie image: the option sets its tie needs, on every shape.
So every shape meets every ksize, C, median size and max_confidence kind, and every (ksize, C) pair."""
import zlib

import numpy as np
from scipy import ndimage

F = np.float32

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (4, 64), (5, 63), (4, 65), (9, 129), (5, 200), (97, 131), (260, 346)]
KSIZES = [1, 3, 5, 7, 9, 15, 31, 63]
CS = [5.0, 4.5, 0.999, 0.0, -2.0, 300.0, -300.0]
MEDIANS = [1, 3, 5, 9, 15, 31]
MEDIAN_31_BELOW = 5000          # pixels: the kernel's median is O(window^2) per pixel
MAXCONF_KINDS = ["zero", "below_min", "inside", "ten_times_max"]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _random_idx(rng, shape):
    idx = rng.integers(0, 256, shape).astype(np.uint8)
    flat = idx.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 8))] = 0       # both ends of the index range,
    flat[rng.integers(0, flat.size, max(1, flat.size // 8))] = 255     # often
    return idx


def _few_idx(rng, shape):
    """Few distinct values: equal values enter and leave the median window together, and even counts split them."""
    return rng.choice(np.array([0, 1, 2, 127, 128, 254, 255], np.uint8), shape)


def _board(shape, a, b):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    c = np.where((yy + xx) % 2 == 0, a, b).astype(F)
    c.reshape(-1)[-1] = 0            # a zero somewhere, so that with max_confidence 255 the u8 image IS the board
    return c


def _gamma(rng, shape):
    return rng.gamma(1.0, 3.0, shape).astype(F)


def _smoothed(rng, shape):
    return ndimage.gaussian_filter(rng.gamma(1.0, 3.0, shape), 2.0, mode="nearest").astype(F)


def _peak(rng, shape):
    c = np.zeros(shape, F)
    c[shape[0] // 2, shape[1] // 2] = 100.0
    return c


def _norm_ladder(rng, shape):
    """With max_confidence 63.75 and a zero in the image: range = 63.75, scale = 255 * (1 / 63.75) = 4 exactly, shift 0.
    The values (k + 0.5) / 4 are dyadic, so conf * 4 + 0 = k + 0.5 exactly: the conversion to u8 sits on a tie at
    every pixel, with k even and odd."""
    n = shape[0] * shape[1]
    k = rng.permutation(n) % 255
    c = ((k + 0.5) / 4.0).astype(F).reshape(shape)
    c.reshape(-1)[-1] = 0
    return c


BUMP_HEIGHTS = [7, 5, 6, 4, 16, 20, 30, 12, 25, 40]


def _bumps(rng, shape):
    """With max_confidence 255 and a zero in the image the u8 image is this one.  A flat background of 100 (diff = 0:
    the tie of C = 0 and 0.999) with isolated raised pixels, five apart so that no kernel up to 7 sees two of them.
    With w the centre weight and w' the weight next to the centre (k3: 1/4, 1/8; k5: 36/256, 24/256; k7: 324/4096,
    252/4096), diff = h - round(h * w) at a bump and -round(h * w') beside it:
      C = 5   (diff == 5):  k3 h = 7 (7 - 2), k5 h = 6 (6 - 1), k7 h = 5 (5 - 0)
      C = 4.5 (diff == 4):  k3 h = 5 (5 - 1), k5 h = 5 (5 - 1), k7 h = 4 (4 - 0)
      C = -2  (diff == -2): k3 h = 16 (2.0), k5 h = 20 (1.875), k7 h = 30 (1.85)"""
    c = np.full(shape, 100.0, F)
    i = 0
    for y in range(shape[0] // 2 % 5, shape[0], 5):
        for x in range(2, shape[1], 5):
            c[y, x] += BUMP_HEIGHTS[i % len(BUMP_HEIGHTS)]
            i += 1
    c.reshape(-1)[-1] = 0
    return c


def _inf_pixel(rng, shape):
    c = _gamma(rng, shape)
    c[shape[0] // 2, shape[1] // 2] = np.inf
    return c


def _wide_range(rng, shape):
    return (10.0 ** rng.uniform(-30.0, 30.0, shape)).astype(F)


# name -> (confidence builder, index builder, max_confidence kinds or explicit values)
IMAGES = {
    "gamma": (_gamma, _random_idx, MAXCONF_KINDS),
    "smoothed": (_smoothed, _few_idx, MAXCONF_KINDS),
    "constant": (lambda rng, s: np.full(s, 3.0, F), _random_idx, [3.0, 0.0, 30.0]),     # 3.0: range 0, scale 0
    "all_zero": (lambda rng, s: np.zeros(s, F), _random_idx, [0.0, 7.0]),               # 0.0: range 0, scale 0
    "peak": (_peak, _random_idx, ["zero", "inside", "ten_times_max"]),
    "board_0_2": (lambda rng, s: _board(s, 0, 2), _few_idx, [255.0]),
    "board_1_3": (lambda rng, s: _board(s, 1, 3), _few_idx, [255.0]),
    "board_0_1": (lambda rng, s: _board(s, 0, 1), _few_idx, [255.0]),
    "board_1_2": (lambda rng, s: _board(s, 1, 2), _random_idx, [255.0]),
    "norm_ladder": (_norm_ladder, _random_idx, [63.75]),
    "bumps": (_bumps, _few_idx, [255.0]),
    "inf_pixel": (_inf_pixel, _random_idx, ["zero", "inside"]),
    "wide_range": (_wide_range, _random_idx, ["zero", "inside", "ten_times_max"]),
}


def image(name, shape):
    """(confidence fp32, index u8) of that name and shape, from a seed fixed by both."""
    conf_fn, idx_fn, _ = IMAGES[name]
    rng = _rng(name, shape)
    conf = np.ascontiguousarray(conf_fn(rng, shape), F)
    idx = np.ascontiguousarray(idx_fn(rng, shape), np.uint8)
    idx[conf == 0] = 0                      # what an arg-max returns for an empty column
    return conf, idx


def max_confidence_value(kind, conf):
    if not isinstance(kind, str):
        return float(kind)
    finite = conf[np.isfinite(conf)]
    lo, hi = (float(finite.min()), float(finite.max())) if finite.size else (0.0, 0.0)
    return {"zero": 0.0, "below_min": lo - 1.0 if lo <= 0 else lo / 2, "inside": lo + 0.5 * (hi - lo),
            "ten_times_max": min(10.0 * hi, 3.0e38)}[kind]


def _medians_for(shape):
    return [m for m in MEDIANS if m < 31 or shape[0] * shape[1] < MEDIAN_31_BELOW]


def option_sets(name, shape):
    """The (ksize, C, median size, max_confidence kind) tuples of one image at one shape, in a fixed order."""
    meds, kinds = _medians_for(shape), IMAGES[name][2]
    out = []
    if name == "gamma":
        for ki, k in enumerate(KSIZES):
            for ci, c in enumerate(CS):
                out.append((k, c, meds[(ki + ci) % len(meds)], kinds[(ki + 2 * ci + ci // 4) % len(kinds)]))
        # every median size and every max_confidence kind once more, against the defaults
        out += [(5, 5.0, m, "zero") for m in meds] + [(5, 5.0, 5, kind) for kind in kinds]
        return out
    npix = shape[0] * shape[1]
    rng = _rng("options", name, shape)
    # (the 0/1 and 1/2 boards stay with the exact kernels: a mean of x.5 everywhere is by construction undecidable
    # for a float kernel, which is what the 1 % cap of the float64 comparison excludes)
    ksizes = [k for k in KSIZES if k <= 7] if name in ("board_0_1", "board_1_2") else KSIZES
    for _ in range(6 if npix < 5000 else 3 if npix < 50000 else 2):
        out.append((ksizes[rng.integers(len(ksizes))], CS[rng.integers(len(CS))], meds[rng.integers(len(meds))],
                    kinds[rng.integers(len(kinds))]))
    if name.startswith("board"):            # the mean ties: every exact kernel
        out += [(k, c, 3, 255.0) for k in (3, 5, 7) for c in (0.0, 0.999)]
    if name == "norm_ladder":
        out += [(3, 5.0, 3, 63.75), (9, 0.0, 5, 63.75)]
    if name == "bumps":                     # the threshold ties
        out += [(k, c, 3, 255.0) for k in (3, 5, 7) for c in (5.0, 4.5, 0.999, 0.0, -2.0)]
    return out


def cases(shape):
    """Every (image name, confidence, index, [(ksize, C, median, max_confidence value)]) of one shape."""
    for name in IMAGES:
        conf, idx = image(name, shape)
        yield name, conf, idx, [(k, c, m, max_confidence_value(kind, conf)) for k, c, m, kind in option_sets(name, shape)]
