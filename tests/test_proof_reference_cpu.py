"""No GPU: pins proof_reference.py (the restatement test_gpu_proof_verdicts.py compares the proof kernels with) and the inputs
of proof_cases.py.  The bound of tie_reference_interval against exact integer arithmetic; the 8 u and (2 n + 2) u fusion slacks
against 100-bit real values; the monotonicity flip_value's bisection rests on; hand-made columns with verdicts written by
hand; and the fault list: every listed mistake changes a verdict on the steered columns, so the GPU test can see it."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import proof_cases as pc
import proof_reference as pr

F32 = np.float32
U = Fraction(1, 2 ** 24)


# ---- the bound itself ----
def _fl32(fr):
    """A non-negative Fraction with a power-of-two denominator, rounded ONCE to fp32 (nearest, ties to even), by integers."""
    num, den = fr.numerator, fr.denominator
    assert den & (den - 1) == 0
    if num == 0:
        return F32(0)
    shift = max(0, num.bit_length() - 24)
    q, r = divmod(num, 1 << shift)
    if shift and (2 * r > (1 << shift) or (2 * r == (1 << shift) and q & 1)):
        q += 1
    return F32(np.ldexp(float(q), shift - (den.bit_length() - 1)))          # q <= 2^24 and the result is normal: exact


def _sequences():
    rng = np.random.default_rng(12)
    uni = rng.random(5000, dtype=F32)
    yield "uniform", uni
    yield "heavy_tailed", (rng.random(20000) ** 8).astype(F32)
    yield "ones_then_tiny", np.concatenate([np.ones(3, F32), (2.0 ** -20 * (1 + rng.random(6000))).astype(F32)])
    yield "all_below_grid", (2.0 ** -31 * rng.random(3000) * 0.999).astype(F32)
    yield "descending", np.sort(uni)[::-1].copy()
    yield "ascending", np.sort(uni)
    yield "one_weight", np.array([0.37], F32)
    yield "one_tiny_weight", np.array([2.0 ** -31], F32)
    # a prototype's adversarial order: a large head, then weights of half an ulp of the running sum (each addition rounds)
    yield "half_ulps", np.concatenate([np.full(1, 256, F32), np.full(30000, 2.0 ** -16 * 1.0001, F32)])


SHARES = {}


@pytest.mark.parametrize("name,w", list(_sequences()), ids=[n for n, _ in _sequences()])
def test_the_interval_holds_the_sequential_fp32_sum(name, w):
    """R: the weights added one by one in fp32 (the reference); S: the exact integer sum of floor(w 2^31) (the engine's cells);
    E = fl32(S 2^-31) (the engine's one rounding).  lo <= R <= hi, and R > 0 whenever E > 0."""
    R = F32(0)
    for x in w:                                      # (sequential by construction: no pairwise summation)
        R = F32(R + x)
    S = sum(int(x) for x in np.floor(w.astype(np.float64) * 2.0 ** 31))      # Python ints: exact at any size
    E = _fl32(Fraction(S, 2 ** 31))
    lo, hi = pr.reference_interval(E, np.uint32(w.size))
    lo, hi = float(lo), float(hi)
    assert lo <= float(R) <= hi, (name, lo, float(R), hi)
    assert (E == 0) == (S == 0)
    if E > 0:
        assert R > 0 and lo >= 2.0 ** -33
    else:
        assert lo == 0.0 and w.size > 0 and hi > 0
    SHARES[name] = abs(float(R) - float(E)) / (hi - lo)
    print("interval share used by |R - E|, %s (n = %d): %.4f" % (name, w.size, SHARES[name]))
    assert SHARES[name] < 1.0


def test_the_interval_of_no_vote_and_of_too_many():
    """n = 0: exactly zero.  The unbounded branch is `(n - 1) u >= 1/2`: it starts at n = 2^23 + 1, one vote later than the
    kernel's comment says; at n = 2^23 gamma is still finite (just below 1) and the interval is a real, if useless, bound."""
    assert pr.reference_interval(F32(5), np.uint32(0)) == (0.0, 0.0)
    lo, hi = pr.reference_interval(F32(5), np.uint32(2 ** 23 + 1))
    assert lo == 0.0 and hi == np.inf
    lo, hi = pr.reference_interval(F32(5), np.uint32(2 ** 24))
    assert lo == 0.0 and hi == np.inf
    lo, hi = pr.reference_interval(F32(5), np.uint32(2 ** 23))
    nu = (2 ** 23 - 1) * 2.0 ** -24
    assert nu < 0.5 and np.isfinite(hi) and hi == (5.0 * (1 + 2.0 ** -23) + 2.0 ** -8) * (1 + nu / (1 - nu))
    assert lo == (5.0 * (1 - 2.0 ** -23) - 2.0 ** -8) * (1 - nu / (1 - nu)) and lo > 2.0 ** -33
    assert 0 <= lo <= 5.0 <= hi


def test_votes_of_borders():
    rng = np.random.default_rng(0)
    H = rng.integers(0, 9, (3, 5, 7)).astype(np.uint32)
    vol = pr.votes_volume(H)
    for y in range(5):
        for x in range(7):
            want = sum(H[:, yy, xx].astype(np.int64) for yy in (y - 1, y) for xx in (x - 1, x) if yy >= 0 and xx >= 0)
            assert np.array_equal(pr.votes_of(H, x, y), want), (x, y)
            assert np.array_equal(vol[:, y, x], want)


# ---- the fusion slack ----
def _pairs():
    rng = np.random.default_rng(5)
    a = (2.0 ** rng.uniform(-33, 26, 1500)).astype(F32)
    g = (2.0 ** rng.uniform(-33, 26, 1500)).astype(F32)
    ends = np.array([2.0 ** -33, 2.0 ** 26], F32)
    mid = (2.0 ** rng.uniform(-33, 26, 40)).astype(F32)
    extra_a = np.concatenate([np.zeros(40, F32), mid, np.repeat(ends, 40), np.tile(mid, 2), ends, ends])
    extra_g = np.concatenate([mid, mid, np.tile(mid, 2), np.repeat(ends, 40), ends, ends[::-1]])
    return np.concatenate([a, extra_a]), np.concatenate([g, extra_g])


def _real2(op, a, g):
    a, g = mpmath.mpf(float(a)), mpmath.mpf(float(g))
    if op == 0:
        return a
    if op == 1:
        return min(a, g)
    if op == 2:
        return 2 * a * g / (a + g + mpmath.mpf(float(F32(0.1))))
    if op == 3:
        return mpmath.sqrt(a * g)
    if op == 4:
        return (a + g) / 2
    if op == 5:
        return mpmath.sqrt((a * a + g * g) / 2)
    return max(a, g)


def _real_n(mode, v):
    v = [mpmath.mpf(float(x)) for x in v]
    if mode == pr.MIN:
        return min(v)
    if mode == pr.MAX:
        return max(v)
    if mode == pr.SUM:
        return mpmath.fsum(v) / len(v)
    while len(v) > 1:
        v = [mpmath.sqrt(v[i] * v[i + 1]) for i in range(0, len(v), 2)]
    return v[0]


@pytest.mark.parametrize("op", range(7))
def test_the_two_camera_ops_stay_within_8u_of_the_real_function(op):
    """The comment at tie_fuse_real: `the fp32 chains of fuse_op stay within 8 u of it`.  Also: the double restatement is the
    real function to within a few double roundings, and a real value of 0 means an engine value of 0."""
    mpmath.mp.prec = 100
    a, g = _pairs()
    eng = pr.engine_value(op, a, g)
    dbl = pr.fuse_real(op, a.astype(np.float64), g.astype(np.float64))
    worst = mpmath.mpf(0)
    for i in range(a.size):
        real = _real2(op, a[i], g[i])
        if real == 0:
            assert eng[i] == 0
            continue
        err = abs(mpmath.mpf(float(eng[i])) - real) / real
        worst = max(worst, err)
        assert err <= 8 * mpmath.mpf(2) ** -24, (op, a[i], g[i], eng[i])
        assert abs(mpmath.mpf(float(dbl[i])) - real) <= 8 * mpmath.mpf(2) ** -53 * real
    print("share of the 8 u slack used by op %d: %.4f" % (op, float(worst / (8 * mpmath.mpf(2) ** -24))))


@pytest.mark.parametrize("mode,n", [(m, n) for m in (pr.SUM, pr.MIN, pr.MAX) for n in range(1, 9)] + [(pr.GM_TREE, n) for n in (2, 4, 8)])
def test_the_n_camera_modes_stay_within_their_slack(mode, n):
    """The comment at ProveSources: `at most 2 n + 2 roundings`."""
    mpmath.mp.prec = 100
    rng = np.random.default_rng(100 * mode + n)
    v = [(2.0 ** rng.uniform(-33, 26, 400)).astype(F32) for _ in range(n)]
    v[0][:20] = 0
    for c in range(n):
        v[c][20:40] = v[0][20:40]                    # all equal
        v[c][40:50], v[c][50:60] = F32(2.0 ** -33), F32(2.0 ** 26)
    v[n - 1][40:50] = F32(2.0 ** 26)
    eng = pr.engine_value_n(mode, v)
    slack = (2 * n + 2) * mpmath.mpf(2) ** -24
    worst = mpmath.mpf(0)
    for i in range(400):
        real = _real_n(mode, [x[i] for x in v])
        if real == 0:
            assert eng[i] == 0
            continue
        err = abs(mpmath.mpf(float(eng[i])) - real) / real
        worst = max(worst, err)
        assert err <= slack, (mode, n, [x[i] for x in v], eng[i])
    print("share of the (2 n + 2) u slack used by mode %d, n = %d: %.4f" % (mode, n, float(worst / slack)))


# ---- monotonicity: what flip_value's bisection rests on ----
VALUES = np.unique(np.concatenate([[0.0], 2.0 ** np.arange(-40, 30, 0.5), 1 + 2.0 ** -23 * np.arange(0, 64)]).astype(F32))
COUNTS = np.array([0, 1, 2, 3, 17, 400, 6000, 2 ** 20, 2 ** 23, 2 ** 23 + 1], np.uint32)


def _nondecreasing(x, axis):
    with np.errstate(invalid="ignore"):
        d = np.diff(x, axis=axis)
    return np.all((d >= 0) | np.isnan(d))               # (inf - inf: both unbounded)


def test_the_interval_is_monotone_in_the_value():
    lo, hi = pr.reference_interval(VALUES[:, None], COUNTS[None, 1:])
    assert _nondecreasing(hi, 0) and _nondecreasing(lo, 0)
    # in the count: hi grows (q and gamma grow), from one vote on (no vote is exactly zero)
    assert _nondecreasing(hi, 1)


@pytest.mark.parametrize("op", range(7))
def test_upper_and_winner_lo_are_monotone_two(op):
    for n_other in (1, 400):
        for other in (F32(0), F32(0.3), F32(5)):
            lo, hi = pr.reference_interval(VALUES[:, None], COUNTS[None, 1:])
            lo1, hi1 = pr.reference_interval(other, np.uint32(n_other))
            for steer in (0, 1):
                up = pr.fuse_real(op, hi, hi1) if steer == 0 else pr.fuse_real(op, hi1 if op else hi, hi)
                wl = pr.fuse_real(op, lo, lo1) if steer == 0 else pr.fuse_real(op, lo1 if op else lo, lo)
                if op != 2:
                    assert _nondecreasing(up * (1 + pr.C8), 0) and _nondecreasing(up * (1 + pr.C8), 1)
                    assert _nondecreasing(wl * (1 - pr.C8), 0)
                    continue
                # the harmonic mean is a QUOTIENT of two sums that both grow: monotone as a real function, in double only up
                # to the quotient's rounding (seen where one operand is 10^17 times the other: one ulp of the double).  That is
                # 2^-29 of the 8 u slack and cannot prove anything wrongly; flip_value needs monotonicity only where the steered
                # columns live (operands within a factor of 64 of each other), and there it is exact:
                for x, axes in ((up * (1 + pr.C8), (0, 1)), (wl * (1 - pr.C8), (0,))):
                    with np.errstate(invalid="ignore"):
                        for axis in axes:
                            d = np.diff(x, axis=axis)
                            before = x[:-1] if axis == 0 else x[:, :-1]
                            assert np.all((d >= -2.0 ** -51 * before) | np.isnan(d))
                near = (VALUES >= other / 64) & (VALUES <= max(other, F32(2.0 ** -20)) * 64)
                assert _nondecreasing((up * (1 + pr.C8))[near], 0) and _nondecreasing((wl * (1 - pr.C8))[near], 0)


@pytest.mark.parametrize("mode,n", [(pr.SUM, 3), (pr.SUM, 4), (pr.MIN, 4), (pr.MAX, 4), (pr.GM_TREE, 2), (pr.GM_TREE, 4), (pr.GM_TREE, 8)])
def test_upper_and_winner_lo_are_monotone_n(mode, n):
    lo, hi = pr.reference_interval(VALUES[:, None], COUNTS[None, 1:])
    for other in (F32(0.3), F32(5)):
        lo1, hi1 = pr.reference_interval(other, np.uint32(17))
        for steer in range(n):
            up = pr.fuse_real_n(mode, [hi if c == steer else hi1 for c in range(n)])
            wl = pr.fuse_real_n(mode, [lo if c == steer else lo1 for c in range(n)])
            assert _nondecreasing(up, 0) and _nondecreasing(up, 1) and _nondecreasing(wl, 0)


def test_flip_value_is_the_first_open_value():
    n_w, n_c = np.array([1, 40, 6000], np.uint32), np.array([3, 3, 900], np.uint32)
    W = np.array([1.0, 2.5, 7.75], F32)
    v = pr.flip_two(0, (W, None), (n_w, None), (n_c, None))
    wl = pr.reference_interval(W, n_w)[0] * (1 - pr.C8)
    up = lambda x: pr.reference_interval(x, n_c)[1] * (1 + pr.C8)
    below = pr.from_bits(pr.bits(v) - np.uint32(1))
    assert np.all(~(up(v) < wl)) and np.all(up(below) < wl)
    assert np.all(v < W) and np.all(v > W * F32(0.99))
    assert pr.flip_value(lambda x: np.zeros(x.shape, bool), (2,)).tolist() == [np.inf, np.inf]
    assert pr.flip_value(lambda x: np.ones(x.shape, bool), (2,)).tolist() == [0.0, 0.0]


# ---- round_down / round_up ----
def test_round_down_and_round_up_enclose_and_are_tight():
    rng = np.random.default_rng(4)
    # (negative values stay within fp32's range: round_up of a finite v below -FLT_MAX is -inf in the kernel's helper, which
    # only ever sees non-negative bounds)
    v = np.concatenate([2.0 ** rng.uniform(-160, 130, 3000), -2.0 ** rng.uniform(-160, 127, 1000),
                        [0.0, -0.0, 1.0, 1 + 2.0 ** -30, 1 - 2.0 ** -30, 2.0 ** -149, 2.0 ** -150, 2.0 ** -151, float(pr.FLT_MAX),
                         float(pr.FLT_MAX) * (1 + 2.0 ** -30), 1e300, np.inf, -np.inf, np.nan]])
    dn, up = pr.round_down(v), pr.round_up(v)
    assert dn.dtype == F32 and up.dtype == F32
    ok = np.isfinite(v)
    with np.errstate(over="ignore"):
        exact = v.astype(F32).astype(np.float64) == v
    assert np.all(dn[ok].astype(np.float64) <= v[ok]) and np.all(up[ok].astype(np.float64) >= v[ok])
    assert np.array_equal(pr.bits(dn[exact]), pr.bits(v[exact].astype(F32))) and np.array_equal(pr.bits(up[exact]), pr.bits(dn[exact]))
    inexact = ok & ~exact & (np.abs(v) < float(pr.FLT_MAX))
    assert np.array_equal(np.nextafter(dn[inexact], F32(np.inf)), up[inexact])       # neighbours: nothing tighter exists
    assert pr.bits(pr.round_down(0.0)) == 0 and pr.bits(pr.round_down(-0.0)) == 0x80000000
    assert pr.round_down(1e300) == pr.FLT_MAX and pr.round_up(1e300) == np.inf        # finite beyond FLT_MAX
    assert pr.round_down(np.inf) == np.inf and np.isnan(pr.round_down(np.nan)) and np.isnan(pr.round_up(np.nan))
    assert pr.bits(pr.round_up(2.0 ** -151)) == 1 and pr.bits(pr.round_down(2.0 ** -151)) == 0
    lo, hi = pr.widen(np.array([0.0, -0.0, 1e-45, 1.0, pr.FLT_MAX, np.inf], F32), np.array([0.0, -0.0, 1e-45, 1.0, pr.FLT_MAX, np.inf], F32), 8)
    assert pr.bits(lo).tolist() == [0, 0, 0, 0x3F7FFFF8, pr.bits(pr.FLT_MAX) - 8, 0x7F800000]
    assert pr.bits(hi).tolist() == [0, 0x80000000, 2, 0x3F800004, 0x7F800000, 0x7F800000]


# ---- hand-made columns ----
@pytest.mark.parametrize("nz", [1, 2, 3, 4, 5])
def test_hand_made_columns_of_interval_grids(nz):
    rel_gap = 2.5e-4
    cols = pc.hand_columns(nz, rel_gap)
    assert len(cols) == {1: 2, 2: 12}.get(nz, 14)
    f, lo, hi = (np.array([c[i] for c in cols]).T for i in (1, 2, 3))
    v = pr.prove_columns(f, lo, hi, rel_gap)
    for j, (kind, _, _, _, proven, need) in enumerate(cols):
        assert bool(v["proven"][j]) == proven, kind
        assert pr.bits(v["need"][j]) == pr.bits(F32(0) if proven else need), kind
    assert pr.summary(v)["max_votes"] == 0


@pytest.mark.parametrize("nz", [1, 2, 3, 4, 5])
def test_hand_made_columns_of_counted_votes(nz):
    """The same kinds through k_tie_prove's rule (one camera), the bounds made from counts."""
    W = F32(3.0)
    rel_gap = 1e-7
    thr = F32(W - F32(rel_gap) * W)
    dn = lambda f: pr.from_bits(pr.bits(F32(f)) - np.uint32(1)).reshape(-1)[0]
    last = nz - 1

    def run(E, n):
        v = pr.prove_two(np.array(E, F32)[:, None], None, np.array(n, np.uint32)[:, None], None, 0, rel_gap)
        return bool(v["proven"][0]), v["need"][0], int(v["most"][0]), int(v["zbest"][0]), v["open"][:, 0].tolist()

    assert run([0] * nz, [7] * nz)[:3] == (True, 0, 0)                     # all zero: proven, and no count looked at
    if nz == 1:
        assert run([W], [9])[:3] == (True, 0, 9)
        return
    E, n = [0] * nz, [0] * nz
    E[0], E[last], n[0], n[last] = W, W, 4, 4000                           # equal maxima: the first wins, the other is skipped
    assert run(E, n) == (True, 0, 4, 0, [False] * nz)
    flip = pr.flip_two(0, (W, None), (np.uint32(4), None), (np.uint32(9), None))[()]
    wl = pr.reference_interval(W, np.uint32(4))[0] * (1 - pr.C8)
    assert pr.reference_interval(flip, np.uint32(9))[1] * (1 + pr.C8) >= wl > pr.reference_interval(dn(flip), np.uint32(9))[1] * (1 + pr.C8)
    E[last], n[last] = flip, 9                                             # the first value that cannot be excluded
    proven, need, most, zbest, open_ = run(E, n)
    assert (proven, most, zbest, open_[last]) == (False, 9, 0, True) and pr.bits(need) == pr.bits(F32((W - flip) / W))
    E[last] = dn(flip)
    assert run(E, n)[:3] == (True, 0, 9)
    E[last], n[last] = thr, 2 ** 23 + 1                                    # v == thr: skipped, whatever its bound; not in `most`
    assert run(E, n)[:3] == (True, 0, 4)
    E[last] = dn(thr)                                                      # one fp32 below: bounded (here: without a bound)
    proven, need, most, _, _ = run(E, n)
    assert (proven, most) == (False, 2 ** 23 + 1) and pr.bits(need) == pr.bits(F32((W - dn(thr)) / W))
    tiny = F32(2.0 ** -31)
    E, n = [0] * nz, [0] * nz
    E[last], n[last] = tiny, 5                                             # the 2^-33 floor excludes planes nobody voted for ...
    assert run(E, n)[:2] == (True, 0)
    if nz >= 3:
        n[1] = 3                                                           # ... but not a zero plane WITH votes
        proven, need, most, _, open_ = run(E, n)
        assert (proven, need, most) == (False, 1.0, 5) and open_ == [z == 1 for z in range(nz)]


# ---- the faults the GPU test must be able to see ----
RULES = [("op%d" % op, lambda op=op: pc.TwoRule(op)) for op in range(7)] + \
        [("mode%d_n%d" % (m, n), lambda m=m, n=n: pc.NRule(m, n)) for m, n in ((pr.SUM, 4), (pr.MIN, 4), (pr.MAX, 3), (pr.GM_TREE, 4))]


@pytest.mark.parametrize("name,make", RULES, ids=[n for n, _ in RULES])
def test_every_listed_fault_changes_a_steered_verdict(name, make):
    """The steered columns of part C, built here from synthetic count volumes (counts 0, 1, a few, thousands; border and
    interior columns; both sides of the workgroup boundary): the plan's own preconditions hold, and every fault of the list,
    applied to the restatement, changes a verdict, a gap or the vote maximum -- with either camera steered."""
    rule = make()
    rel_gap = 1e-7
    counts = pc.synthetic_counts(rule.k)
    rng = np.random.default_rng(1)
    natural = [(rng.random(counts[0].shape, dtype=F32) * np.minimum(counts[c], 50)).astype(F32) for c in range(rule.k)]
    for steer in range(min(rule.k, 2)):
        vols, plan = pc.steer(rule, natural, counts, rel_gap, steer=steer, seed=3 + steer)
        truth = rule.prove(vols, counts, rel_gap)
        kinds = pc.check_plan(rule, plan, vols, truth)
        assert kinds["flip"] >= 32 and kinds["below"] >= 32 and min(kinds.values()) >= 1, kinds
        assert set(pc.required_pixels(32, 9)) <= set(plan["pixels"].tolist())
        for fault in rule.faults:
            assert pc.detects(rule, vols, counts, rel_gap, truth, fault), "%s, camera %d steered: %s goes unseen" % (name, steer, fault)
        # and the faults move the flip value itself, where they touch the bounds
        j = np.flatnonzero(plan["kinds"] == "flip")
        assert np.array_equal(pr.bits(plan["value"][j]), pr.bits(plan["flip"][j]))


def test_hand_made_grids_place_every_kind_at_every_anchor():
    cols = pc.hand_columns(5, 2.5e-4)
    seen = set()
    for r in range(len(cols)):
        f, lo, hi, expect = pc.hand_grid(37, 11, 5, 2.5e-4, seed=r, rotate=r)
        assert sorted(expect) == [0, 255, 256, 406]
        v = pr.prove_columns(f, lo, hi, 2.5e-4)
        for p, (kind, proven, need) in expect.items():
            seen.add((p, kind))
            assert bool(v["proven"].reshape(-1)[p]) == proven and pr.bits(v["need"].reshape(-1)[p]) == pr.bits(F32(0) if proven else need)
    assert len(seen) == 4 * len(cols)
    # the two faults k_prove_columns could have that the hand-made kinds exist for
    f, lo, hi, _ = pc.hand_grid(37, 11, 5, 2.5e-4, seed=1, rotate=3)
    truth = pr.prove_columns(f, lo, hi, 2.5e-4)
    for fault in ("le", "last_maximum", "skip_last_plane", "thr_double", "need_min"):
        bad = False
        for r in range(len(cols)):
            g = pc.hand_grid(37, 11, 5, 2.5e-4, seed=r, rotate=r)
            bad |= not pc.same_verdict(pr.prove_columns(*g[:3], 2.5e-4), pr.prove_columns(*g[:3], 2.5e-4, fault=fault))
        assert bad, fault
    assert truth["proven"].sum() > 100 and (~truth["proven"]).sum() > 20
