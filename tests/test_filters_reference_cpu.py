"""The C oracle's post-arg-max filters (orc_depth_map_filters) against tests/filters_reference.py, a restatement
of mapper_emvs_stereo.cpp:390-436 that is structured differently on purpose, and that restatement against exact
arithmetic: integers for the Gaussian mean with ksize <= 7, fractions.Fraction for the fp32 normalisation, mpmath for
the Gaussian taps, float64 (outside a stated undecidable set) for the Gaussian mean with ksize >= 9.  No GPU: the HIP
kernels meet the same matrix in test_depthmap_filters.py.

Measured here (the figures DESIGN section 2 quotes; test_undecidable_share prints them): undecidable share of the
float64 comparison, the larger of the random-gamma and the smoothed image -- 97 x 131: ksize 9: 0.09 %, 15: 0.14 %,
31: 0.20 %, 63: 0.50 %;  260 x 346: 0.08 %, 0.10 %, 0.20 %, 0.40 %.  The cap the tests assert is 1 %.

The 0/2 and 1/3 checkerboards: with the k3 / k5 / k7 taps the weights on either colour sum to exactly 1/2, so in
the interior their mean is the INTEGER (a + b) / 2; they tie only where the replicated border breaks the balance,
and the zeroed pixel (0,0) often spoils that too.  They stay in the matrix as ordinary images.  The 0/1 and 1/2
boards are here for the ties: (a + b) / 2 = 0.5 in the interior (stays 0 under half-to-even, 1 under half-away)
and 1.5 (goes to 2).  test_tie_images_tie counts ties of both parities for every exact kernel.
"""
from fractions import Fraction
import math

import numpy as np
import pytest

from oracle import oracle as orc
import filters_cases as fc
import filters_reference as fr

PLANES = orc.depth_planes(1.0, 5.0, 256)
OUTPUTS = ("confidence", "conf8", "mask", "idx_filtered", "depth")
CAP = 0.01                      # undecidable share, asserted on every image of at least CAP_PIXELS pixels
CAP_PIXELS = 10000


def f32_round(x):
    """Fraction -> the nearest fp32 value as a Fraction (ties to even); None beyond the finite range."""
    if x == 0:
        return Fraction(0)
    e = math.floor(math.log2(abs(x)))
    while Fraction(2) ** e > abs(x):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(x):
        e += 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    r = round(x / quantum) * quantum            # round(Fraction) is half to even
    return r if abs(r) < Fraction(2) ** 128 else None


def check_against_float64(ref, ksize, where):
    """Mean (a) (fp32, the arithmetic the project defines) == half-to-even of mean (b) (float64) on every decidable
    pixel; returns the undecidable share."""
    und = ref["undecidable"]
    want = np.clip(np.rint(ref["mean64"]), 0, 255).astype(np.int64)
    bad = (ref["mean"] != want) & ~und
    assert not bad.any(), "%s: fp32 mean differs from float64 on %d decidable pixels" % (where, bad.sum())
    return und.mean()


@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_equals_restatement(shape):
    """All five outputs, bit for bit, at every ksize (with mean (a) the restatement is comparable everywhere); for
    ksize >= 9 mean (a) is also held to float64 on every decidable pixel, and on images of >= 10,000 pixels the
    undecidable share is capped at 1 %."""
    npix = shape[0] * shape[1]
    seen = {"ksize": set(), "C": set(), "median": set(), "empty_window": 0, "even_count": 0, "cases": 0}
    for name, conf, idx, options in fc.cases(shape):
        for n_opt, (ksize, C_, med, max_conf) in enumerate(options):
            where = "%s %s ksize=%d C=%g median=%d max_confidence=%g" % (shape, name, ksize, C_, med, max_conf)
            got = orc.depth_map_filters(conf, idx, PLANES, ksize, C_, med, max_conf)
            # (the histogram walk is pure Python: on the 90,000-pixel image it follows every image's first option set)
            ref = fr.depth_map_filters(conf, idx, PLANES, ksize, C_, med, max_conf, walk=npix < 50000 or n_opt == 0)
            for key in OUTPUTS:
                assert np.array_equal(got[key], ref[key]), "%s: %s differs at %d pixels" % (
                    where, key, (got[key] != ref[key]).sum())
            if ksize >= 9:
                share = check_against_float64(ref, ksize, where)
                if npix >= CAP_PIXELS:
                    assert share <= CAP, "%s: %.3f %% of the pixels are undecidable" % (where, 100 * share)
            seen["ksize"].add(ksize)
            seen["C"].add(C_)
            seen["median"].add(med)
            seen["cases"] += 1
            m = ref["mask_before_border"].astype(np.int64)
            count = np.lib.stride_tricks.sliding_window_view(np.pad(m, med // 2), (med, med)).sum(axis=(2, 3))
            seen["empty_window"] += int((count == 0).sum())
            seen["even_count"] += int(((count > 0) & (count % 2 == 0)).sum())
    assert seen["ksize"] == set(fc.KSIZES) and seen["C"] == set(fc.CS)
    assert seen["median"] == set(m for m in fc.MEDIANS if m < 31 or npix < fc.MEDIAN_31_BELOW)
    assert seen["empty_window"] > 0
    if npix >= 9:
        assert seen["even_count"] > 0, "no window with an even number of masked pixels"
    print("%s: %d cases" % (shape, seen["cases"]))


@pytest.mark.parametrize("shape", [s for s in fc.SHAPES if s[0] * s[1] >= CAP_PIXELS], ids=lambda s: "%dx%d" % s)
def test_undecidable_share(shape):
    """The cap of the float64 comparison on the images the issue measured it on, per ksize (printed: -s shows them)."""
    for name in ("gamma", "smoothed", "constant"):
        conf, idx = fc.image(name, shape)
        for ksize in (9, 15, 31, 63):
            for C_ in (5.0, 4.5, 0.0, -2.0):
                ref = fr.depth_map_filters(conf, idx, PLANES, ksize, C_, 1, 0.0, walk=False)
                share = check_against_float64(ref, ksize, "%s %s ksize=%d" % (shape, name, ksize))
                if C_ == 5.0:
                    print("undecidable %s %-8s ksize %2d: %.3f %%" % (shape, name, ksize, 100 * share))
                assert share <= CAP
                # outside the undecidable set the mask is the float64 mask
                want = (ref["conf8"].astype(np.int64) - np.rint(ref["mean64"]).astype(np.int64) > -math.ceil(-C_))
                assert np.array_equal(ref["mask_before_border"][~ref["undecidable"]] > 0, want[~ref["undecidable"]])


def test_fixed_taps_are_the_documented_tables():
    for ksize, (taps, den) in fr.INT_TAPS.items():
        assert len(taps) == ksize and sum(taps) == den and taps == taps[::-1]
    assert [t / 4 for t in fr.INT_TAPS[3][0]] == [0.25, 0.5, 0.25]
    assert [t / 16 for t in fr.INT_TAPS[5][0]] == [0.0625, 0.25, 0.375, 0.25, 0.0625]
    assert [t / 64 for t in fr.INT_TAPS[7][0]] == [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]


def test_computed_taps_match_mpmath():
    """Every odd ksize in 9..63 against a 50-digit evaluation: within 1 ulp of fp32 (the engine, the oracle and the
    restatement all call the host's exp and normalise by a rounded reciprocal, so the last bit is not promised).
    Taps that differ from the correctly rounded value on the machine this was written on: none."""
    import mpmath
    mpmath.mp.dps = 50
    differ = []
    for ksize in range(9, 64, 2):
        sigma = mpmath.mpf(3) / 10 * (mpmath.mpf(ksize - 1) / 2 - 1) + mpmath.mpf(8) / 10
        t = [mpmath.exp(-((i - mpmath.mpf(ksize - 1) / 2) ** 2) / (2 * sigma ** 2)) for i in range(ksize)]
        total = mpmath.fsum(t)
        taps = fr.gaussian_taps(ksize)
        assert taps.dtype == np.float32 and len(taps) == ksize
        for i in range(ksize):
            exact = t[i] / total
            ulp = float(np.spacing(taps[i]))
            assert abs(mpmath.mpf(float(taps[i])) - exact) <= ulp, (ksize, i)
            if np.float32(float(exact)) != taps[i]:      # (double rounding of `exact` itself is far below this)
                differ.append((ksize, i))
        assert abs(float(taps.astype(np.float64).sum()) - 1.0) < ksize * 2.0 ** -24
    print("taps that are not the correctly rounded value:", differ)


@pytest.mark.parametrize("name,max_conf", [("gamma", 0.0), ("gamma", 41.7), ("smoothed", 2.5), ("wide_range", 1e10),
                                           ("norm_ladder", 63.75), ("constant", 0.0)])
def test_normalisation_is_two_rounded_fp32_operations(name, max_conf):
    """float32(float32(conf * a) + b) against Fraction arithmetic with explicit rounding to fp32, and scale / shift
    against their definition in doubles."""
    conf, _ = fc.image(name, (9, 129))
    conf_out, conf8, (a, b) = fr.normalise(conf, max_conf)
    assert conf_out[0, 0] == np.float32(max_conf) and np.array_equal(conf_out.reshape(-1)[1:], conf.reshape(-1)[1:])
    smin, smax = float(conf_out.min()), float(conf_out.max())
    scale = 255.0 * (1.0 / (smax - smin))
    assert a == np.float32(scale) and b == np.float32(0.0 - smin * scale)
    v = fr.scale_shift(conf_out, a, b)
    fa, fb = Fraction(float(a)), Fraction(float(b))
    for i in np.random.default_rng(3).choice(conf.size, 200, replace=False):
        c = Fraction(float(conf_out.reshape(-1)[i]))
        want = f32_round(f32_round(c * fa) + fb)
        assert want is not None and Fraction(float(v.reshape(-1)[i])) == want, (i, float(c))
        if i:
            n, half = divmod(want, 1)
            u8 = int(n) + (1 if half > Fraction(1, 2) or (half == Fraction(1, 2) and n % 2 == 1) else 0)
            assert conf8.reshape(-1)[i] == min(max(u8, 0), 255)
    assert conf8[0, 0] == 0


def test_f32_round_helper():
    for x in (0.1, 1.0 / 3, 255.0 / 7, 1e-42, 3e38, 16777217.0):
        assert f32_round(Fraction(x)) == Fraction(float(np.float32(x)))
    assert f32_round(Fraction(16777217)) == 16777216 and f32_round(Fraction(16777219)) == 16777220   # ties to even


TIE_SHAPES = [s for s in fc.SHAPES if s[0] * s[1] >= 9 and s != (3, 3)]


@pytest.mark.parametrize("shape", TIE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_tie_images_tie(shape):
    """A tie image that has stopped tying fails here.  Counted in the restatement's exact arithmetic."""
    # the Gaussian mean on x.5: even x (stays) and odd x (goes up)
    for ksize in (3, 5, 7):
        stay = up = 0
        for name in ("board_0_1", "board_1_2", "board_0_2", "board_1_3"):
            conf, idx = fc.image(name, shape)
            _, conf8, _ = fr.normalise(conf, 255.0)
            assert np.array_equal(conf8.reshape(-1)[1:], conf.reshape(-1)[1:].astype(np.uint8))   # the board itself
            mean, s, d = fr.gaussian_mean_int(conf8, ksize)
            tie = 2 * (s % d) == d
            stay += int((tie & (s // d % 2 == 0)).sum())
            up += int((tie & (s // d % 2 == 1)).sum())
            assert np.array_equal(mean[tie], (s // d + s // d % 2)[tie])
            if name in ("board_0_1", "board_1_2"):
                npix = shape[0] * shape[1]       # (a 9-pixel line has one pixel whose k7 window is interior)
                assert tie.sum() >= (npix // 4 if npix >= 64 else 1), (name, ksize, int(tie.sum()))
        assert stay > 0 and up > 0, (ksize, stay, up)
    # conf * a + b on k + 0.5, k even and odd
    conf, idx = fc.image("norm_ladder", shape)
    conf_out, conf8, (a, b) = fr.normalise(conf, 63.75)
    assert a == 4.0 and b == 0.0
    v = [Fraction(float(c)) * 4 for c in conf_out.reshape(-1)[1:-1]]
    assert all(x % 1 == Fraction(1, 2) for x in v)
    floors = np.array([int(x // 1) for x in v])
    assert (floors % 2 == 0).any() and (floors % 2 == 1).any()
    assert np.array_equal(conf8.reshape(-1)[1:-1], floors + floors % 2)
    # conf8 - mean == -idelta: the mask must be 0 there
    if shape[0] * shape[1] >= 256:
        conf, idx = fc.image("bumps", shape)
        for ksize in (3, 5, 7):
            for C_ in (5.0, 4.5, 0.999, 0.0, -2.0):
                ref = fr.depth_map_filters(conf, idx, PLANES, ksize, C_, 3, 255.0, walk=False)
                tie = ref["conf8"].astype(np.int64) - ref["mean"] == -math.ceil(-C_)
                assert tie.sum() > 0, "no threshold tie: ksize %d C %g" % (ksize, C_)
                assert not ref["mask_before_border"][tie].any()
                assert ref["mask_before_border"].any() or C_ > 0


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 7), (17, 23), (40, 33)])
def test_the_two_medians_agree(shape):
    """The definition (sort, element (num + 1) // 2 - 1) against the sliding-histogram walk, on masks of every density."""
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for size in (1, 3, 5, 9, 31):
        for density in (0.0, 0.1, 0.6, 1.0):
            for idx in (rng.integers(0, 256, shape).astype(np.uint8), rng.choice(np.array([0, 7, 255], np.uint8), shape)):
                mask = (rng.random(shape) < density).astype(np.uint8)
                a = fr.median_by_definition(idx, mask, size)
                b = fr.median_by_histogram_walk(idx, mask, size)
                assert np.array_equal(a, b), (shape, size, density)
                if density == 0.0:
                    assert not a.any()
                if size == 1:
                    assert np.array_equal(a, np.where(mask > 0, idx, 0))


def test_known_answers_of_the_restatement():
    """Hand-computed: lower median of an even count; 2.5 and 3.5 both round to even; ceil(-C) for a fractional C."""
    idx = np.array([[10, 20, 30, 40]], np.uint8)
    assert fr.median_by_definition(idx, np.ones((1, 4), np.uint8), 31)[0, 0] == 20       # {10,20,30,40} -> 20
    assert fr.median_by_definition(idx, np.array([[1, 0, 1, 0]], np.uint8), 31)[0, 3] == 10
    assert list(fr.round_half_even_u8(np.array([0.5, 1.5, 2.5, 3.5, -0.5, 254.5, 255.5, 300, -7, np.nan], np.float32))) == [
        0, 2, 2, 4, 0, 254, 255, 255, 0, 0]
    # a 1 x 3 image (0, 4, 0) -> u8 (0, 255, 0) with max_confidence 0; k3 means 255 * (1, 2, 1) / 4 = 63.75, 127.5, 63.75
    r = fr.depth_map_filters(np.array([[0, 4, 0]], np.float32), np.zeros((1, 3), np.uint8), PLANES, 3, 127.5, 1, 0.0)
    assert list(r["mean"][0]) == [64, 128, 64]                                          # 127.5 -> 128 (even)
    assert list(r["mask_before_border"][0]) == [0, 0, 0]                                # 127 > 127 is false (ceil(-127.5) = -127)
    r = fr.depth_map_filters(np.array([[0, 4, 0]], np.float32), np.zeros((1, 3), np.uint8), PLANES, 3, 126.5, 1, 0.0)
    assert list(r["mask_before_border"][0]) == [0, 1, 0] and not r["mask"].any()        # 127 > 126; the border clears it
