"""Plain numpy restatement of DESIGN.md 7g: ground-truth depth from a disparity image as
scripts/evaluate_mcemvs_dsec.py:108-122 makes it, and the script's thicken_edges erosion (:75-79).  Element-wise float64
arithmetic in the written order (numpy's multiply and add are separate operations: nothing is contracted), no matrix
product and no fancy indexing: the scatter is a loop over the kept points in row-major order, so "the last write wins" is
spelled out.  Test infrastructure; tests/golden/make_dsec_ground_truth.py pins it against the script's own expressions."""
import numpy as np

AS_SCRIPT, DROP_OUTSIDE = 0, 1
F32, F64 = np.float32, np.float64


def disparity_from_png16(raw):
    """matplotlib's 16-bit rule, then the script's * 256"""
    return np.divide(np.asarray(raw, np.uint16), 65535, dtype=F32) * F32(256)


def points(d, Q, T, K):
    """steps 1-4 for every source pixel, flat in row-major order: dict of kept, outside (both bool), iu, iv (int64; valid
    where kept and not outside, before any wrap) and value (float32)"""
    d = np.asarray(d)
    assert d.dtype == F32 and d.ndim == 2
    Q, T, K = np.asarray(Q, F64), np.asarray(T, F64), np.asarray(K, F64)
    H, W = d.shape
    x = np.broadcast_to(np.arange(W, dtype=F64)[None, :], (H, W)).ravel()
    y = np.broadcast_to(np.arange(H, dtype=F64)[:, None], (H, W)).ravel()
    dd = d.astype(F64).ravel()
    with np.errstate(all="ignore"):
        h = [((Q[i, 0] * x + Q[i, 1] * y) + Q[i, 2] * dd) + Q[i, 3] for i in range(4)]
        X, Y, Z = ((h[i] / h[3]).astype(F32) for i in range(3))
        kept = Z < F32(np.inf)
        X, Y, Z = X.astype(F64), Y.astype(F64), Z.astype(F64)
        P = [((T[i, 0] * X + T[i, 1] * Y) + T[i, 2] * Z) + T[i, 3] for i in range(4)]
        p = [((K[i, 0] * P[0] + K[i, 1] * P[1]) + K[i, 2] * P[2]) + K[i, 3] * P[3] for i in range(3)]
        u, v = p[0] / p[2], p[1] / p[2]
        tu, tv = np.trunc(u), np.trunc(v)
        inside = np.isfinite(u) & np.isfinite(v) & (tu >= -W) & (tu < W) & (tv >= -H) & (tv < H)
        value = P[2].astype(F32)
    iu = np.where(inside, tu, 0.0).astype(np.int64)
    iv = np.where(inside, tv, 0.0).astype(np.int64)
    return {"kept": kept, "outside": kept & ~inside, "iu": iu, "iv": iv, "value": value}


def project(d, Q, T, K, mode=AS_SCRIPT):
    """(depth float32 [H][W], n_points, n_outside)"""
    assert mode in (AS_SCRIPT, DROP_OUTSIDE)
    H, W = np.shape(d)
    pt = points(d, Q, T, K)
    out = np.zeros((H, W), F32)
    n_points, n_outside = int(pt["kept"].sum()), int(pt["outside"].sum())
    if mode == AS_SCRIPT and n_outside:
        return out, n_points, n_outside
    kept, outside, iu, iv, value = (pt[k].tolist() if k != "value" else pt[k] for k in ("kept", "outside", "iu", "iv", "value"))
    for i in range(H * W):                                           # row-major source order: a later point overwrites
        if not kept[i] or outside[i]:
            continue
        a, b = iu[i], iv[i]
        if a < 0 or b < 0:
            if mode == DROP_OUTSIDE:
                continue
            a, b = (a + W if a < 0 else a), (b + H if b < 0 else b)
        out[b, a] = value[i]
    return out, n_points, n_outside


def erode_cross(depth, mask, no_estimate=255.0):
    """thicken_edges: (out_depth float32, out_mask uint8)"""
    depth, mask = np.asarray(depth, F32), np.asarray(mask)
    assert depth.ndim == 2 and depth.shape == mask.shape
    v = np.where(mask != 0, depth, F32(no_estimate)).astype(F32)
    e = v.copy()
    e[1:, :] = np.minimum(e[1:, :], v[:-1, :])
    e[:-1, :] = np.minimum(e[:-1, :], v[1:, :])
    e[:, 1:] = np.minimum(e[:, 1:], v[:, :-1])
    e[:, :-1] = np.minimum(e[:, :-1], v[:, 1:])
    return e, (e != F32(no_estimate)).astype(np.uint8)
