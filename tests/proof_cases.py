"""The steered columns of test_gpu_proof_verdicts.py (part C), and what test_proof_reference_cpu.py proves of them without a
GPU.  Natural DSIs use at most half of a reference interval's width, so a proof kernel that proves a little too much agrees
with a correct one on them; here chosen columns are overwritten so that a verdict hangs on ONE fp32 step of one value:

    flip       a winner (every camera >= 1) and one challenger whose steered camera holds proof_reference.flip_*: the smallest
               fp32 for which the challenger cannot be excluded.  Unproven, and `need` is that challenger's gap exactly
    below      the same with the next fp32 below: proven
    tie        `below`, and a later plane with more votes repeats the winner's values: the first maximum's counts decide
    two        `flip`, and a third plane just below the threshold: two open planes, `need` is the larger gap
    thr_at     the challenger's fused value is the first that is >= thr: skipped (the resolver re-sums it), proven
    thr_below  the last fused value below thr: bounded, open
    zero       the winner and the challenger (half its value) on planes without a vote: both bounds are 0, and 0 < 0 does not
               exclude.  The planes before the winner hold a little less than it (open either way, a small gap), those
               behind it its value again (skipped), so `need` is the challenger's gap
    floor      every plane voted by all cameras holds 2^-31, the others (without any vote) 0: only the 2^-33 floor excludes
               them

Every other plane of a steered column is 0; the other columns keep the values given.  Counts are never changed: on the GPU
they are the events'.  `detects` runs one fault of proof_reference.FAULTS over the steered volumes and says whether any
verdict, gap or vote maximum changes -- the precondition both test files assert."""
import numpy as np

import proof_reference as pr

F32 = np.float32
KINDS = ("flip", "below", "tie", "two", "thr_at", "thr_below", "zero", "floor")
TINY = F32(2.0 ** -31)


class TwoRule:
    """k_tie_prove<OP>: one camera (op 0) or two cameras fused by op 1..6."""

    def __init__(self, op):
        self.op, self.k, self.faults = op, (1 if op == 0 else 2), pr.FAULTS

    def engine(self, vals):
        return pr.engine_value(self.op, vals[0], vals[1] if self.k == 2 else None)

    def fixed(self, winner):
        if self.op == 1:
            return [F32(1.25) * np.maximum(winner[0], winner[1])] * 2          # min: the steered camera decides
        if self.op == 6:
            return [F32(0.5) * np.minimum(winner[0], winner[1])] * 2           # max: likewise
        return list(winner)

    def flip(self, winner, n_w, n_c, fixed, steer, fault=None):
        pad = lambda v: (list(v) + [None])[:2]
        return pr.flip_two(self.op, pad(winner), pad(n_w), pad(n_c), fixed=None if self.k == 1 else fixed[1 - steer],
                           steer=steer, fault=fault)

    def prove(self, vols, counts, rel_gap, fault=None, fused=None):
        two = self.k == 2
        return pr.prove_two(vols[0], vols[1] if two else None, counts[0], counts[1] if two else None, self.op, rel_gap, fault)


class NRule:
    """k_tie_prove_n<MODE>: k cameras fused by an n-ary mode."""

    def __init__(self, mode, k):
        self.mode, self.k, self.faults = mode, k, pr.FAULTS_N

    def engine(self, vals):
        return pr.engine_value_n(self.mode, vals)

    def fixed(self, winner):
        if self.mode == pr.MIN:
            return [F32(1.25) * np.maximum.reduce(winner)] * self.k
        if self.mode == pr.MAX:
            return [F32(0.5) * np.minimum.reduce(winner)] * self.k
        return list(winner)

    def flip(self, winner, n_w, n_c, fixed, steer, fault=None):
        return pr.flip_n(self.mode, winner, n_w, n_c, fixed, steer=steer, fault=fault)

    def prove(self, vols, counts, rel_gap, fault=None, fused=None):
        return pr.prove_n(self.engine(vols) if fused is None else fused, vols, counts, self.mode, rel_gap, fault)


def required_pixels(nx, ny):
    """Pixel 0, a column in row 0, one in column 0, either side of the first workgroup boundary, the last pixel."""
    return [0, 5, 3 * nx, 255, 256, nx * ny - 1]


def _pick_planes(kind, j, cnt, voted, empty, nz):
    """(zw, zc, z3) of one column: the winner's, the challenger's and a third plane (-1: none)."""
    vp = np.flatnonzero(voted)
    if kind == "zero":
        ep = np.flatnonzero(empty)
        return int(ep[0]), int(ep[-1] if j % 2 else ep[1]), -1
    if kind == "floor":
        return int(vp[0]), -1, -1
    if kind == "tie":
        zw = int(vp[0])
        z2 = int(vp[1:][np.argmax(cnt[vp[1:]])])
        zc = int([z for z in vp if z not in (zw, z2)][-1])
        return zw, zc, z2
    few, many = int(vp[np.argmin(cnt[vp])]), int(vp[len(vp) - 1 - np.argmax(cnt[vp][::-1])])
    if few == many:
        few, many = int(vp[0]), int(vp[-1])
    zw, zc = (few, many) if j % 2 else (many, few)
    if kind in ("thr_at", "thr_below") and zc < zw:
        zw, zc = zc, zw                                         # (a challenger AT thr may equal the maximum: it must come later)
    if kind == "flip" and j % 4 == 0 and voted[nz - 1] and zw != nz - 1:
        zc = nz - 1                                             # a challenger on the last plane
    rest = [z for z in vp if z not in (zw, zc)]
    return zw, zc, (int(rest[len(rest) // 2]) if rest else -1)


def steer(rule, vols, counts, rel_gap, steer=0, seed=0, per_kind=(40, 40, 8, 8, 8, 8, 8, 8)):
    """-> (steered volumes, plan).  vols / counts: rule.k arrays [nz, ny, nx]; steer: the camera that carries the value sought.
    The plan lists, per steered column, its pixel, kind, planes and the challenger's steered value."""
    k = rule.k
    nz, ny, nx = vols[0].shape
    npix = nx * ny
    cn = [np.asarray(c, np.uint32).reshape(nz, npix) for c in counts]
    voted = np.logical_and.reduce([c > 0 for c in cn])
    empty = np.logical_and.reduce([c == 0 for c in cn])
    nv, ne = voted.sum(0), empty.sum(0)
    rng = np.random.default_rng(seed)
    req = required_pixels(nx, ny)
    assert np.all(nv[req] >= 2), "a required column has fewer than two planes voted by every camera: %r" % (nv[req],)
    taken = np.zeros(npix, bool)
    taken[req] = True
    pixels, kinds = list(req), ["flip", "below"] * (len(req) // 2)
    for kind, want in zip(KINDS, per_kind):
        ok = {"zero": ne >= 2, "floor": (ne >= 1) & (nv >= 1) & (ne + nv == nz)}.get(kind, nv >= 3) & ~taken
        pool = np.flatnonzero(ok)
        if kind in ("flip", "below"):
            assert pool.size >= want, "%s: only %d columns with three voted planes" % (kind, pool.size)
        got = rng.choice(pool, min(want, pool.size), replace=False)
        taken[got] = True
        pixels += [int(p) for p in got]
        kinds += [kind] * got.size
    pixels, kinds = np.array(pixels), np.array(kinds)
    m = pixels.size
    zw, zc, z3 = (np.zeros(m, np.int64) for _ in range(3))
    for j in range(m):
        zw[j], zc[j], z3[j] = _pick_planes(kinds[j], j, cn[steer][:, pixels[j]], voted[:, pixels[j]], empty[:, pixels[j]], nz)
    at = lambda c, z: cn[c][np.maximum(z, 0), pixels]
    winner = [(F32(1) + F32(7) * rng.random(m, dtype=F32)).astype(F32) for _ in range(k)]
    # thr = best - fl(rel_gap * best) differs from the double's best (1 - rel_gap) by a fraction of an ulp; with rel_gap = 1e-7
    # a maximum in [7.2, 8) puts the fp32 thr BELOW the double's, so that a challenger at thr is skipped by the rule and
    # bounded by a kernel that computes thr in double
    at_thr = np.isin(kinds, ("thr_at", "thr_below"))
    for c in range(k):
        winner[c] = np.where(at_thr, F32(7.3) + F32(0.65) * rng.random(m, dtype=F32), winner[c]).astype(F32)
    fixed = rule.fixed(winner)
    n_w, n_c = ([at(c, z) for c in range(k)] for z in (zw, zc))
    flip = rule.flip(winner, n_w, n_c, fixed, steer)
    below = pr.from_bits(np.maximum(pr.bits(flip).astype(np.int64) - 1, 0).astype(np.uint32))
    best = rule.engine(winner)
    thr = best - F32(rel_gap) * best
    with_v = lambda v: [v if c == steer else fixed[c] for c in range(k)]
    thr_at = pr.flip_value(lambda v: rule.engine(with_v(v)) >= thr, (m,), top=64.0)   # (the engine's ops are monotone, too)
    thr_below = pr.from_bits(np.maximum(pr.bits(thr_at).astype(np.int64) - 1, 0).astype(np.uint32))
    value = np.select([kinds == "flip", kinds == "below", kinds == "tie", kinds == "two", kinds == "thr_at", kinds == "thr_below"],
                      [flip, below, below, flip, thr_at, thr_below], F32(0)).astype(F32)
    out = [np.array(v, F32).reshape(nz, npix) for v in vols]
    for c in range(k):
        out[c][:, pixels] = 0
        chal = value if c == steer else fixed[c]
        for kind in KINDS:
            s = kinds == kind
            if not s.any():
                continue
            if kind == "floor":
                out[c][:, pixels[s]] = np.where(voted[:, pixels[s]], TINY, F32(0))
                continue
            if kind == "zero":
                before = np.arange(nz)[:, None] < zw[s][None]
                out[c][:, pixels[s]] = np.where(before, F32(1 - 2.0 ** -10) * winner[c][s], winner[c][s])
            out[c][zw[s], pixels[s]] = winner[c][s]
            out[c][zc[s], pixels[s]] = F32(0.5) * winner[c][s] if kind == "zero" else chal[s]
            if kind == "tie":
                out[c][z3[s], pixels[s]] = winner[c][s]
            if kind == "two":
                out[c][z3[s], pixels[s]] = (thr_below if c == steer else fixed[c])[s]
    plan = dict(pixels=pixels, kinds=kinds, zw=zw, zc=zc, z3=z3, value=value, flip=flip, steer=steer)
    return [v.reshape(nz, ny, nx) for v in out], plan


def check_plan(rule, plan, vols, verdict):
    """What the rule (a verdict of proof_reference on the steered volumes) must say of the steered columns: the plan's own
    preconditions.  verdict: rule.prove(vols, counts, rel_gap)."""
    nz = vols[0].shape[0]
    vol = lambda a: np.asarray(a).reshape(nz, -1)
    flat = lambda a: np.asarray(a).reshape(-1)
    px, kinds, zw, zc = plan["pixels"], plan["kinds"], plan["zw"], plan["zc"]
    proven, need, zbest, best = (flat(verdict[key])[px] for key in ("proven", "need", "zbest", "best"))
    below, open_ = vol(verdict["below"]), vol(verdict["open"])
    has_winner = kinds != "floor"
    assert np.array_equal(zbest[has_winner], zw[has_winner]), "a steered winner is not its column's first maximum"
    steered = np.isin(kinds, ("flip", "below", "tie", "two"))
    assert np.all(np.isfinite(plan["flip"][steered])) and np.all(plan["flip"][steered] > 0), "a flip value does not exist"
    assert np.all(below[zc[steered], px[steered]]), "a flip value does not lie below thr"
    fused = vol(rule.engine([vol(v) for v in vols]))
    for kind in ("flip", "zero"):
        s = kinds == kind
        gap = ((best[s] - fused[zc[s], px[s]]) / best[s]).astype(F32)
        assert not proven[s].any(), "%s: a column is proven" % kind
        assert np.array_equal(pr.bits(need[s]), pr.bits(gap)), "%s: need is not the challenger's gap" % kind
    for kind in ("below", "tie", "thr_at"):
        assert proven[kinds == kind].all(), "%s: a column is unproven" % kind
    s = kinds == "thr_at"
    assert not below[zc[s], px[s]].any(), "thr_at: bounded"
    for kind in ("thr_below", "two"):
        s = kinds == kind
        z = zc[s] if kind == "thr_below" else plan["z3"][s]
        assert below[z, px[s]].all() and open_[z, px[s]].all() and not proven[s].any(), kind
    s = kinds == "two"
    assert np.all(open_[:, px[s]].sum(0) == 2), "two: not two open planes"
    return {kind: int((kinds == kind).sum()) for kind in KINDS}


def same_verdict(a, b):
    """Whether two verdicts agree in everything the GPU test compares."""
    return (np.array_equal(a["proven"], b["proven"]) and np.array_equal(pr.bits(a["need"]), pr.bits(b["need"]))
            and int(a["most"].max()) == int(b["most"].max()))


def detects(rule, vols, counts, rel_gap, truth, fault, fused=None):
    return not same_verdict(truth, rule.prove(vols, counts, rel_gap, fault=fault, fused=fused))


def synthetic_counts(k, nz=12, ny=9, nx=32, seed=0):
    """Count volumes for the CPU test (made like the device's: cell counters H, then votes_volume): cells with 0, 1, a few and
    thousands of votes; whole planes without a vote in some columns; 288 columns, so pixel 255 | 256 exist."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(k):
        H = rng.choice(np.array([0, 0, 1, 3, 17, 400, 6000], np.uint32), size=(nz, ny, nx), p=[.3, .2, .15, .15, .1, .05, .05])
        H[:, ny - 1, :] = 0                                    # the accept test keeps votes off the last row and column
        H[:, :, nx - 1] = 0
        H[:, :2, :6] = np.maximum(H[:, :2, :6], 1 + c)         # the required border columns are voted
        H[:, 2:4, 0] = np.maximum(H[:, 2:4, 0], 2)
        H[:, 7, 0] = np.maximum(H[:, 7, 0], 4)
        H[:, 7:9, 30:32] = 0
        H[:, 7, 30] = 5
        H[:, 6:8, 28:31] = np.maximum(H[:, 6:8, 28:31], 3)
        H[::2, 4:7, 8:24] = 0                                   # planes without a vote, shared by the cameras
        H[1::2, 4:7, 8:24] = np.maximum(H[1::2, 4:7, 8:24], 1)
        out.append(pr.votes_volume(H))
    return out


# ---- hand-made columns for k_prove_columns (part A of the GPU test; the CPU test holds the restatement to `expect`) ----
def hand_columns(nz, rel_gap):
    """-> [(kind, fused[nz], lo[nz], hi[nz], proven, need)]: every kind that fits into nz planes, its verdict written by hand.
    Planes not named hold fused 0, lo 0, hi 0 (excluded by any positive lower bound of the winner)."""
    W, L = F32(3.0), F32(2.5)
    thr = F32(W - F32(rel_gap) * W)
    dn = lambda f: pr.from_bits(pr.bits(F32(f)) - np.uint32(1)).reshape(-1)[0]
    half = F32((W - F32(1.5)) / W)
    cols = []

    def col(kind, planes, proven, need=0.0):
        f, lo, hi = (np.zeros(nz, F32) for _ in range(3))
        for z, (fv, lv, hv) in planes.items():
            f[z], lo[z], hi[z] = fv, lv, hv
        cols.append((kind, f, lo, hi, proven, F32(need)))

    last = nz - 1
    col("all_zero", {0: (0, 0, np.inf), last: (0, 0, np.nan)}, True)                       # an empty column is proven
    col("single_maximum", {last: (W, 0, np.inf)}, nz == 1, 1.0)                            # lo = 0: the zero planes stay open
    if nz >= 2:
        col("equal_maxima", {0: (W, L, W), 1: (W, 2 * W, W)}, True)                        # the second maximum is skipped
        col("hi_equals_winner_lo", {last: (W, L, W), 0: (1.5, 0, L)}, False, half)         # not (hi < lo): open
        col("hi_below_winner_lo", {last: (W, L, W), 0: (1.5, 0, dn(L))}, True)
        col("at_thr", {0: (W, L, W), last: (thr, 0, np.inf)}, True)                        # v == thr: the resolver's, skipped
        col("below_thr", {0: (W, L, W), last: (dn(thr), 0, np.inf)}, False, F32((W - dn(thr)) / W))
        col("hi_inf", {0: (W, L, W), last: (1.5, 0, np.inf)}, False, half)
        col("hi_nan", {last: (W, L, W), 0: (1.5, 0, np.nan)}, False, half)                 # NaN is never excluded
        col("lo_zero", {0: (W, 0, W), last: (1.5, 0, 1.0)}, False, 1.0 if nz > 2 else half)
        col("floor_no_votes", {0: (TINY, pr.FLOOR, 2 * TINY), last: (0, 0, 0)}, True)      # a plane nobody voted for: hi = 0
        col("floor_votes", {0: (TINY, pr.FLOOR, 2 * TINY), last: (0, 0, 3 * TINY)}, False, 1.0)
    if nz >= 3:
        # the FIRST of equal maxima decides: its lo leaves plane 2 open, the second's would exclude it
        col("first_of_equal_maxima", {0: (W, L, W), 1: (W, 2 * W, 2 * W), 2: (1.5, 0, W)}, False, half)
        # two open planes: the larger gap is needed
        col("two_open", {1: (W, L, W), 0: (1.5, 0, W), 2: (0.75, 0, W)}, False, F32((W - F32(0.75)) / W))
    return cols


def hand_grid(nx, ny, nz, rel_gap, seed=0, rotate=0):
    """(fused, lo, hi) [nz, ny, nx] with hand-made columns at pixel 0, at the last pixel of the first workgroup, at the first of
    the second and at the last of all (where the grid has them): kinds rotate, rotate + 1, ... of hand_columns, so that
    rotate = 0 .. len(hand_columns) - 1 puts every kind at every one of them.  Random columns elsewhere, some hi +inf or NaN,
    some lo 0.  `expect`: {pixel: (kind, proven, need)} of the hand-made ones."""
    rng = np.random.default_rng(seed)
    npix = nx * ny
    fused = (rng.random((nz, npix), dtype=F32) * (rng.random((nz, npix)) < 0.8)).astype(F32)
    fused[:, rng.random(npix) < 0.1] = 0
    far = rng.random((nz, npix)) < 0.7                                      # most planes well below the maximum, some near it
    fused = np.where(far, fused * F32(0.5), F32(0.5) + fused * F32(1e-3)).astype(F32)
    eps = (rng.random((nz, npix)) * 4e-4).astype(F32)
    lo = (fused * (1 - eps)).astype(F32)
    hi = (fused * (1 + eps)).astype(F32)
    odd = rng.random((nz, npix))
    hi[odd < 0.01] = np.inf
    hi[(odd >= 0.01) & (odd < 0.02)] = np.nan
    lo[odd > 0.98] = 0
    cols = hand_columns(nz, rel_gap)
    anchors = sorted({p for p in (0, 255, 256, npix - 1) if p < npix})
    expect = {}
    for j, p in enumerate(anchors):
        kind, f, l, h, proven, need = cols[(rotate + j) % len(cols)]
        fused[:, p], lo[:, p], hi[:, p] = f, l, h
        expect[p] = (kind, proven, need)
    shape = (nz, ny, nx)
    return fused.reshape(shape), lo.reshape(shape), hi.reshape(shape), expect
