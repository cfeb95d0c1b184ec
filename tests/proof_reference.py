"""The per-column proof (dsi_kernels.hip: tie_votes_of, tie_reference_interval, tie_fuse_real, tie_fuse_real_n, k_tie_prove,
k_tie_prove_n, k_prove_columns, k_interval_of_counts, k_interval_widen) restated in numpy, in the kernels' own operation order:
float64 where they use double, float32 where they use float.  The kernels are built without contraction and use IEEE
+ - * / sqrt fmin fmax only, so every figure here is meant to equal the device's bit for bit.  Nothing of the engine is imported;
the fp32 fused value (tie_value<OP>) is the oracle's fuse2, the function the engine's own fusion is pinned to.

Volumes are [nz, ...]: plane first, any pixel shape behind it.  `fault` names ONE deliberate mistake (FAULTS below) and exists
for test_proof_reference_cpu.py and the precondition asserts of test_gpu_proof_verdicts.py, which show that the steered inputs
tell every such mistake from the rule; fault=None is the rule."""
import numpy as np

from oracle import oracle as orc

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
Q31 = 2.0 ** -31
FLOOR = 2.0 ** -33
C8 = 8.0 * U
FLT_MAX = np.finfo(np.float32).max
SUM, MIN, MAX, GM_TREE = 0, 4, 5, 6          # dsi_acc_mode_t

# the mistakes the GPU test must be able to see (ISSUE list); SLACK_2N applies to the n-ary rule only
FAULTS = ("le", "no_winner_slack", "no_challenger_slack", "n_for_n_minus_1", "no_q", "no_floor", "skip_last_plane",
          "last_maximum", "thr_double", "need_min")
FAULTS_N = FAULTS + ("slack_2n",)


def bits(f):
    return np.ascontiguousarray(f, F32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(F32)


# ---- tie_votes_of ----
def votes_of(H, x, y):
    """The votes whose 2 x 2 footprint contains (x, y): H[..., y, x] and its left, upper and upper-left neighbours."""
    H = np.asarray(H)
    n = H[..., y, x].astype(np.uint32)
    if x > 0:
        n = n + H[..., y, x - 1]
    if y > 0:
        n = n + H[..., y - 1, x]
    if x > 0 and y > 0:
        n = n + H[..., y - 1, x - 1]
    return n.astype(np.uint32)


def votes_volume(H):
    """votes_of on every voxel of H [nz, ny, nx] at once (uint32 wrap-around like the kernel's)."""
    H = np.asarray(H, np.uint32)
    n = H.copy()
    n[..., :, 1:] += H[..., :, :-1]
    n[..., 1:, :] += H[..., :-1, :]
    n[..., 1:, 1:] += H[..., :-1, :-1]
    return n


# ---- tie_reference_interval ----
def reference_interval(E, n, fault=None):
    E = np.asarray(E, F32)
    n = np.asarray(n, np.uint32)
    E, n = np.broadcast_arrays(E, n)
    Ed, nd = E.astype(F64), n.astype(F64)
    q = nd * Q31 if fault != "no_q" else np.zeros_like(nd)
    nu = ((n - np.uint32(1)).astype(F64) if fault != "n_for_n_minus_1" else nd) * U       # (n - 1u: uint32, as the kernel)
    with np.errstate(all="ignore"):
        gamma = nu / (1.0 - nu)
        w_hi = Ed * (1.0 + 2.0 * U) + q
        w_lo = np.fmax(0.0, Ed * (1.0 - 2.0 * U) - q)
        hi = w_hi * (1.0 + gamma)
        lo = np.fmax(0.0, w_lo * (1.0 - gamma))
    if fault != "no_floor":
        lo = np.where(E > 0, np.fmax(lo, FLOOR), lo)
    unbounded = ~(nu < 0.5)
    lo = np.where(unbounded, 0.0, lo)
    hi = np.where(unbounded, np.inf, hi)
    none = n == 0
    return np.where(none, 0.0, lo), np.where(none, 0.0, hi)


# ---- tie_fuse_real / tie_fuse_real_n ----
def fuse_real(op, a, g):
    a = np.asarray(a, F64)
    if op == 0:
        return a
    g = np.asarray(g, F64)
    with np.errstate(all="ignore"):
        if op == 1:
            return np.fmin(a, g)
        if op == 2:
            return 2.0 * a * g / (a + g + F64(F32(0.1)))
        if op == 3:
            return np.sqrt(a * g)
        if op == 4:
            return 0.5 * (a + g)
        if op == 5:
            return np.sqrt(0.5 * (a * a + g * g))
        if op == 6:
            return np.fmax(a, g)
    raise ValueError("op %r" % (op,))


def fuse_real_n(mode, v):
    v = [np.asarray(x, F64) for x in v]
    with np.errstate(all="ignore"):
        if mode in (MIN, MAX):
            r = v[0]
            for x in v[1:]:
                r = np.fmin(r, x) if mode == MIN else np.fmax(r, x)
            return r
        if mode == SUM:
            r = np.zeros_like(v[0])
            for x in v:
                r = r + x
            return r / F64(len(v))
        if mode == GM_TREE:
            t = list(v)
            w = len(t)
            while w > 1:
                for c in range(w // 2):
                    t[c] = np.sqrt(t[2 * c] * t[2 * c + 1])
                w >>= 1
            return t[0]
    raise ValueError("mode %r" % (mode,))


# ---- the engine's fp32 values ----
def engine_value(op, a, b=None):
    """tie_value<OP>: camera 0's value, or the reference's 2-ary op on (0 + a, b) -- the oracle's, not written anew."""
    a = np.ascontiguousarray(a, F32)
    if op == 0:
        return a
    b = np.ascontiguousarray(b, F32)
    a, b = np.broadcast_arrays(a, b)
    return orc.fuse2(F32(0) + a, b, op).reshape(a.shape)


def engine_value_n(mode, v):
    v = [np.ascontiguousarray(x, F32) for x in v]
    if mode == GM_TREE:
        return orc.fuse_gm_tree(v).reshape(v[0].shape)
    return orc.fuse_nary(v, mode).reshape(v[0].shape)


# ---- the column rule shared by k_tie_prove, k_tie_prove_n and k_prove_columns ----
def _first_maximum(v, fault):
    best, zbest = v[0].copy(), np.zeros(v.shape[1:], np.int64)
    for z in range(1, v.shape[0]):
        take = best <= v[z] if fault == "last_maximum" else best < v[z]
        best = np.where(take, v[z], best)
        zbest = np.where(take, z, zbest)
    return best, zbest


def _at(vol, zbest):
    return np.take_along_axis(vol, zbest[None], axis=0)[0]


def _verdict(v, rel_gap, upper, winner_lo_of, counts, fault):
    """v: fused fp32 [nz, ...]; upper: every plane's upper bound; winner_lo_of(zbest): the winner's lower bound; counts: the
    count volumes that go into `most` (None: k_prove_columns keeps none)."""
    nz = v.shape[0]
    best, zbest = _first_maximum(v, fault)
    live = best > 0
    rel_gap = F32(rel_gap)
    with np.errstate(all="ignore"):
        if fault == "thr_double":
            below = v.astype(F64) < best.astype(F64) - F64(rel_gap) * best.astype(F64)
        else:
            below = v < best - rel_gap * best            # not (v >= thr): the planes the kernel goes on to bound
        gap = (best[None] - v) / best[None]              # fp32
    below &= live[None]
    if fault == "skip_last_plane":
        below[nz - 1] = False
    winner_lo = winner_lo_of(zbest)
    with np.errstate(invalid="ignore"):
        excluded = upper <= winner_lo[None] if fault == "le" else upper < winner_lo[None]
    open_ = below & ~excluded
    proven = ~open_.any(axis=0)
    if fault == "need_min":
        need = np.where(open_, gap, F32(np.inf)).min(axis=0)
        need = np.where(proven, F32(0), need).astype(F32)
    else:
        need = np.where(open_, gap, F32(0)).max(axis=0).astype(F32)   # fmaxf from 0: the gaps are not negative
    most = np.zeros(best.shape, np.uint32)
    for n in counts or ():
        n = np.asarray(n, np.uint32)
        seen = np.where(below, n, np.uint32(0)).max(axis=0)
        most = np.maximum(most, np.where(live, np.maximum(seen, _at(n, zbest)), np.uint32(0)))
    return dict(proven=proven, need=need, most=most, best=best, zbest=zbest, below=below, open=open_)


def prove_two(a, b, na, nb, op, rel_gap, fault=None):
    """k_tie_prove<OP>: a, b the cameras' DSIs (b, nb ignored for op 0), na, nb their counted votes per voxel."""
    a = np.ascontiguousarray(a, F32)
    v = engine_value(op, a, b)
    lo0, hi0 = reference_interval(a, na, fault)
    lo1 = hi1 = None
    if op != 0:
        lo1, hi1 = reference_interval(b, nb, fault)
    up = fuse_real(op, hi0, hi1)
    upper = up if fault == "no_challenger_slack" else up * (1.0 + C8)
    wl = fuse_real(op, lo0, lo1)
    wl = wl if fault == "no_winner_slack" else wl * (1.0 - C8)
    return _verdict(v, rel_gap, upper, lambda zb: _at(wl, zb), [na] if op == 0 else [na, nb], fault)


def prove_n(fused, e, n, mode, rel_gap, fault=None):
    """k_tie_prove_n<MODE>: fused the grid the columns are read from, e[c] / n[c] camera c's DSI and counted votes."""
    k = len(e)
    slack = F64(2 * k if fault == "slack_2n" else 2 * k + 2) * U
    iv = [reference_interval(e[c], n[c], fault) for c in range(k)]
    up = fuse_real_n(mode, [x[1] for x in iv])
    upper = up if fault == "no_challenger_slack" else up * (1.0 + slack)
    wl = fuse_real_n(mode, [x[0] for x in iv])
    wl = wl if fault == "no_winner_slack" else wl * (1.0 - slack)
    return _verdict(np.ascontiguousarray(fused, F32), rel_gap, upper, lambda zb: _at(wl, zb), list(n), fault)


def prove_columns(fused, lo, hi, rel_gap, fault=None):
    """k_prove_columns: all fp32; a plane below thr is open iff not (hi < lo of the winner's plane)."""
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    return _verdict(np.ascontiguousarray(fused, F32), rel_gap, hi, lambda zb: _at(lo, zb), None, fault)


def summary(verdict):
    """What the ABI reports of a verdict: the counters, gap_needed's float bits and the sorted (pixel, gap bits) pairs."""
    proven = verdict["proven"].reshape(-1)
    need = verdict["need"].reshape(-1)
    pix = np.flatnonzero(~proven).astype(np.uint32)
    gap_bits = bits(need)[pix]
    return dict(columns=proven.size, columns_proven=int(proven.sum()), columns_unproven=int(pix.size),
                gap_needed_bits=int(gap_bits.max()) if pix.size else 0, max_votes=int(verdict["most"].max()),
                pixels=pix, gap_bits=gap_bits)


def sorted_pairs(pixels, gaps):
    """(pixel, gap bits) pairs in pixel order: the device lists them in an atomic's order."""
    pixels = np.asarray(pixels, np.uint32)
    order = np.argsort(pixels, kind="stable")
    return pixels[order], bits(gaps)[order]


# ---- round_down / round_up / k_interval_of_counts / k_interval_widen ----
def _next_below(f):
    b = bits(f)
    return from_bits(np.where(f > 0, b - np.uint32(1), np.where(f < 0, b + np.uint32(1), np.uint32(0x80000001))))


def _next_above(f):
    b = bits(f)
    return from_bits(np.where(f > 0, b + np.uint32(1), np.where(f < 0, b - np.uint32(1), np.uint32(0x00000001))))


def round_down(v):
    v = np.asarray(v, F64)
    with np.errstate(all="ignore"):
        f = v.astype(F32)
    finite = (f == f) & (np.abs(f) < np.inf)
    out = np.where((f.astype(F64) > v) & finite, _next_below(f), f)
    return np.where((f == np.inf) & (v < np.inf), FLT_MAX, out).astype(F32)      # a finite v beyond FLT_MAX


def round_up(v):
    v = np.asarray(v, F64)
    with np.errstate(all="ignore"):
        f = v.astype(F32)
    finite = (f == f) & (np.abs(f) < np.inf)
    return np.where((f.astype(F64) < v) & finite, _next_above(f), f).astype(F32)


def _fmax0(x):
    """fmax(0.0, x) as the device gives it: x where x > 0, else +0 (for -0 and NaN too: v_max_f64 orders the zeros)."""
    return np.where(x > 0, x, 0.0)


def interval_grids(E, n):
    lo, hi = reference_interval(E, n)
    return round_down(lo), round_up(hi)


def widen(lo, hi, k):
    ku = F64(k) * U
    lo, hi = np.asarray(lo, F32).astype(F64), np.asarray(hi, F32).astype(F64)
    with np.errstate(all="ignore"):
        return round_down(_fmax0(lo * (1.0 - ku))), round_up(hi * (1.0 + ku))


# ---- the value at which a verdict flips ----
def flip_value(is_open, shape=(), top=np.inf):
    """The smallest non-negative fp32 v with is_open(v) -- is_open takes a float32 array of `shape` and says whether a
    challenger of that value is unexcluded; it must be monotone (upper is non-decreasing in v: a CPU test).  Bisection over
    the bit patterns 0 .. top; where even the fp32 below `top` stays excluded the answer is `top` ("no flip value" for +inf)."""
    lo = np.full(shape, -1, np.int64)                      # (-1: "below +0"; is_open(lo) is false by convention)
    hi = np.full(shape, int(bits(F32(top)).reshape(-1)[0]), np.int64)     # is_open(hi) taken as true
    while True:
        active = hi - lo > 1
        if not active.any():
            break
        mid = np.maximum((lo + hi) // 2, 0)
        o = np.asarray(is_open(from_bits(mid.astype(np.uint32)).reshape(shape)), bool)
        hi = np.where(active & o, mid, hi)
        lo = np.where(active & ~o, mid, lo)
    return from_bits(hi.astype(np.uint32)).reshape(shape)


def flip_two(op, winner, n_winner, n_chal, fixed=None, steer=0, fault=None):
    """flip_value for k_tie_prove<OP>: winner = (a, b) values and n_winner = (na, nb) counts at the winner's plane, n_chal the
    challenger's counts, `fixed` the value of the challenger's camera that is not steered (2-ary ops).  Arrays broadcast."""
    lo0, _ = reference_interval(winner[0], n_winner[0], fault)
    lo1 = None
    if op != 0:
        lo1, _ = reference_interval(winner[1], n_winner[1], fault)
    wl = fuse_real(op, lo0, lo1)
    wl = wl if fault == "no_winner_slack" else wl * (1.0 - C8)
    shape = np.broadcast(wl, *[np.asarray(x) for x in n_chal if x is not None]).shape

    def is_open(v):
        vals = [v, fixed] if steer == 0 else [fixed, v]
        h0 = reference_interval(vals[0], n_chal[0], fault)[1]
        h1 = reference_interval(vals[1], n_chal[1], fault)[1] if op != 0 else None
        up = fuse_real(op, h0, h1)
        up = up if fault == "no_challenger_slack" else up * (1.0 + C8)
        with np.errstate(invalid="ignore"):
            return ~(up < wl)
    return flip_value(is_open, shape)


def flip_n(mode, winner, n_winner, n_chal, fixed, steer=0, fault=None):
    """flip_value for k_tie_prove_n<MODE>: winner / n_winner / n_chal / fixed are lists over the cameras; camera `steer` of the
    challenger takes the value sought, the others `fixed[c]`."""
    k = len(winner)
    slack = F64(2 * k if fault == "slack_2n" else 2 * k + 2) * U
    wl = fuse_real_n(mode, [reference_interval(winner[c], n_winner[c], fault)[0] for c in range(k)])
    wl = wl if fault == "no_winner_slack" else wl * (1.0 - slack)
    shape = np.broadcast(wl, *[np.asarray(x) for x in n_chal]).shape

    def is_open(v):
        hs = [reference_interval(v if c == steer else fixed[c], n_chal[c], fault)[1] for c in range(k)]
        up = fuse_real_n(mode, hs)
        up = up if fault == "no_challenger_slack" else up * (1.0 + slack)
        with np.errstate(invalid="ignore"):
            return ~(up < wl)
    return flip_value(is_open, shape)
