"""The world map's arithmetic restated in numpy (include/dsi_engine.h "the world map").

Elementwise float64 operations only -- every product and sum is rounded on its own, as the kernel's are (no FMA), so no
`@` / matmul / dot, whose summation order and contraction are the BLAS's business.  The sums are uint64 (np.add.at) and
the output is ordered by ascending key: the engine's extraction, sorted, is compared with array_equal.

    world position   X = ((r00 x + r01 y) + r02 z) + t0          (rows 1, 2 for Y, Z)
    cell, fraction   q = X / leaf, c = floor(q), f = q - c, F = uint64(floor(f * 2^32))
    rejected         X, Y or Z not finite, or some |c| > 2^20 - 2
    per cell         n, S[3] = sums of F, windows = calls that put a point into the cell
    centroid         Q = S // n, m = (c + Q * 2^-32) * leaf, float32(m)
    key              (cx + 2^20 - 1) | (cy + 2^20 - 1) << 21 | (cz + 2^20 - 1) << 42
"""
import numpy as np

CELL_MAX = (1 << 20) - 2
TWO32 = 4294967296.0


def invert_pose(T):
    """R' = R^T, t'_i = -((r0i t0 + r1i t1) + r2i t2); T and the result are 12 doubles, row-major [R | t]."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    out = np.empty((3, 4), np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return out.reshape(12)


def world_positions(xyz, T_w_rv):
    """(N, 3) float64 world positions of float32 points (N, >= 3)."""
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    T = np.asarray(T_w_rv, np.float64).reshape(3, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def cells(xyz, T_w_rv, leaf):
    """(accepted bool [N], c int64 [N][3], F uint64 [N][3]); c and F are 0 where the point is rejected."""
    W = world_positions(xyz, T_w_rv)
    leaf = np.float64(leaf)
    with np.errstate(all="ignore"):
        q = W / leaf
        cf = np.floor(q)
        ok = np.isfinite(W).all(axis=1) & (np.abs(cf) <= CELL_MAX).all(axis=1)     # (NaN compares false)
        cf = np.where(ok[:, None], cf, 0.0)
        f = np.where(ok[:, None], q - cf, 0.0)
        F = np.floor(f * TWO32).astype(np.uint64)
    return ok, cf.astype(np.int64), F


def pack_key(c):
    c = np.asarray(c, np.int64)
    b = (c + (CELL_MAX + 1)).astype(np.uint64)
    return b[..., 0] | (b[..., 1] << np.uint64(21)) | (b[..., 2] << np.uint64(42))


def unpack_key(keys):
    keys = np.asarray(keys, np.uint64)
    m = np.uint64(0x1FFFFF)
    return np.stack([((keys >> np.uint64(21 * a)) & m).astype(np.int64) - (CELL_MAX + 1) for a in range(3)], axis=-1)


class ReferenceMap:
    """The map's state as plain dictionaries' worth of arrays, rebuilt per call with np.unique / np.add.at."""

    def __init__(self, leaf):
        self.leaf = float(leaf)
        self.reset()

    def reset(self):
        self.keys = np.zeros(0, np.uint64)
        self.n = np.zeros(0, np.uint64)
        self.S = np.zeros((0, 3), np.uint64)
        self.windows = np.zeros(0, np.uint64)
        self.calls = self.accepted = self.rejected = 0

    def integrate(self, xyz, T_w_rv):
        """One call; returns the number of rejected points."""
        xyz = np.asarray(xyz, np.float32)
        if xyz.ndim != 2:
            xyz = xyz.reshape(-1, 3)
        self.calls += 1
        ok, c, F = cells(xyz, T_w_rv, self.leaf)
        rejected = int((~ok).sum())
        self.rejected += rejected
        self.accepted += int(ok.sum())
        k = pack_key(c[ok])
        allk = np.union1d(self.keys, k)                      # sorted, unique
        n = np.zeros(allk.shape[0], np.uint64)
        S = np.zeros((allk.shape[0], 3), np.uint64)
        w = np.zeros(allk.shape[0], np.uint64)
        old = np.searchsorted(allk, self.keys)
        n[old], S[old], w[old] = self.n, self.S, self.windows
        idx = np.searchsorted(allk, k)
        np.add.at(n, idx, np.uint64(1))
        for a in range(3):
            np.add.at(S[:, a], idx, F[ok][:, a])
        w[np.unique(idx)] += np.uint64(1)
        self.keys, self.n, self.S, self.windows = allk, n, S, w
        return rejected

    def extract(self, min_points=1, min_windows=1):
        """dict of xyz float32 (M, 3), n, windows uint32, keys uint64 -- by ascending key."""
        keep = (self.n >= np.uint64(min_points)) & (self.windows >= np.uint64(min_windows))
        keys, n, S, w = self.keys[keep], self.n[keep], self.S[keep], self.windows[keep]
        c = unpack_key(keys).astype(np.float64).reshape(-1, 3)
        Q = S // np.maximum(n, np.uint64(1))[:, None]
        m = (c + Q.astype(np.float64) * (1.0 / TWO32)) * np.float64(self.leaf)
        return {"xyz": m.astype(np.float32).reshape(-1, 3), "n": n.astype(np.uint32), "windows": w.astype(np.uint32), "keys": keys}


def assert_maps_equal(got, want):
    """array_equal on keys, n, windows and the float BITS of xyz."""
    for k in ("keys", "n", "windows"):
        assert np.array_equal(got[k], want[k]), k
    assert got["xyz"].dtype == np.float32 and want["xyz"].dtype == np.float32
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), "xyz bits"
