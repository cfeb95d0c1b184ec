"""The restatement of MapperEMVS::getPointcloud (mapper_emvs_stereo.cpp:440-480) that the point-cloud tests compare the
engine with, in numpy:

  backproject(depth, mask, fx, fy, cx, cy)   :455-464 in float64, in the reference's order -- projectPixelTo3dRay
                                             (geometry_utils.hpp:56-59: (u - cx) / fx with float members), Eigen's
                                             normalize() (n = (bx*bx + by*by) + bz*bz; / sqrt(n) when n > 0),
                                             b / b[2] * depth, stored as float32; intensity = float(1.0 / z_f32).
                                             Row-major pixel order (PCL's push_back order).
  keep_bruteforce(xyz, r, min_neighbors)     pcl::RadiusOutlierRemoval (radius_outlier_removal.hpp, dense cloud) as a
                                             count: i kept iff >= min_neighbors + 1 points j (j = i, duplicates
                                             included) have float64(d2_f32(i, j)) <= float64(r_f32) ** 2, with
                                             d2_f32 = ((dx*dx) + dy*dy) + dz*dz in float32 (FLANN's L2_Simple<float>
                                             over x, y, z).  Every pair, chunked.
  keep_kdtree(xyz, r, min_neighbors)         the same keep-set for large clouds: scipy's cKDTree pairs within
                                             r (1 + 1e-3) (a superset of what the fp32 test accepts), then the same
                                             exact float32 recheck of every candidate pair.
"""
import numpy as np


def backproject(depth, mask, fx, fy, cx, cy):
    depth = np.asarray(depth, np.float32)
    rows, cols = np.nonzero(np.asarray(mask) > 0)     # row-major
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    bx = (cols.astype(np.float64) - cx) / fx
    by = (rows.astype(np.float64) - cy) / fy
    bz = np.ones_like(bx)
    n = (bx * bx + by * by) + bz * bz
    s = np.sqrt(n)
    pos = n > 0
    bx = np.where(pos, bx / s, bx)
    by = np.where(pos, by / s, by)
    bz = np.where(pos, bz / s, bz)
    d = depth[rows, cols].astype(np.float64)
    x = ((bx / bz) * d).astype(np.float32)
    y = ((by / bz) * d).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ((bz / bz) * d).astype(np.float32)
        inten = (1.0 / z.astype(np.float64)).astype(np.float32)
    return np.stack([x, y, z, inten], axis=1)


def _d2_f32(a, b):
    """((dx*dx) + dy*dy) + dz*dz in float32, a (n, 3) against b (m, 3) -> (n, m); numpy rounds every operation."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = a[:, None, 0] - b[None, :, 0]
        dy = a[:, None, 1] - b[None, :, 1]
        dz = a[:, None, 2] - b[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def keep_bruteforce(xyz, r, min_neighbors, chunk=None):
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    n = xyz.shape[0]
    rr = float(np.float32(r)) ** 2                       # exact in float64 (48 bits)
    need = int(min_neighbors) + 1
    if n == 0:
        return np.zeros(0, bool)
    chunk = chunk or max(1, (1 << 24) // max(1, n))
    cnt = np.zeros(n, np.int64)
    for i0 in range(0, n, chunk):
        d2 = _d2_f32(xyz[i0:i0 + chunk], xyz)
        cnt[i0:i0 + chunk] = (d2.astype(np.float64) <= rr).sum(axis=1)
    return cnt >= need


def keep_kdtree(xyz, r, min_neighbors):
    return counts_kdtree(xyz, r) >= int(min_neighbors) + 1


def counts_kdtree(xyz, r):
    """Per point, the number of points j (itself included) the fp32 test accepts."""
    from scipy.spatial import cKDTree
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    n = xyz.shape[0]
    rr = float(np.float32(r)) ** 2
    if n == 0:
        return np.zeros(0, np.int64)
    finite = np.isfinite(xyz).all(axis=1)
    idx = np.nonzero(finite)[0]
    tree = cKDTree(xyz[idx].astype(np.float64))
    pairs = tree.query_pairs(float(np.float32(r)) * (1 + 1e-3), output_type="ndarray")
    cnt = np.zeros(n, np.int64)
    if pairs.size:
        a, b = idx[pairs[:, 0]], idx[pairs[:, 1]]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = xyz[a, 0] - xyz[b, 0]
            dy = xyz[a, 1] - xyz[b, 1]
            dz = xyz[a, 2] - xyz[b, 2]
            ok = ((dx * dx + dy * dy) + dz * dz).astype(np.float64) <= rr
        np.add.at(cnt, a[ok], 1)
        np.add.at(cnt, b[ok], 1)
    # the point itself: d2 = 0 <= r^2 for every finite point (a non-finite one never passes: NaN or inf - inf)
    cnt[finite] += 1
    return cnt


# ---- adversarial clouds (shared by the CPU and GPU tests) ----

def lattice(n=6, spacing=0.25, offset=(0.0, 0.0, 0.0)):
    """n^3 points on a cubic lattice: neighbour distances are exactly `spacing` in float32 (spacing a power of two)."""
    g = np.arange(n, dtype=np.float32) * np.float32(spacing)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1) + np.asarray(offset, np.float32)


def perturb_ulps(xyz, frac, seed):
    """Moves a fraction of the coordinates one float32 ulp up or down: d2 = r^2 exactly becomes one ulp either side."""
    rng = np.random.default_rng(seed)
    out = np.array(xyz, np.float32, copy=True)
    sel = rng.random(out.shape) < frac
    up = rng.random(out.shape) < 0.5
    out[sel & up] = np.nextafter(out[sel & up], np.float32(np.inf))
    out[sel & ~up] = np.nextafter(out[sel & ~up], np.float32(-np.inf))
    return out


_CELL_MAX = (1 << 20) - 2
_M64 = (1 << 64) - 1


def engine_buckets(n):
    """The engine's bucket count for n points (dsi::pc_buckets): a power of two >= 2 n, at least 64."""
    m = 64
    while m < 2 * n:
        m <<= 1
    return m


def engine_bucket(cx, cy, cz, buckets):
    """The bucket the engine hashes cell (cx, cy, cz) to (pc_key + pc_hash in dsi_kernels.hip; integer arrays) -- to
    BUILD clouds whose cells collide; the keep-set never depends on it."""
    off = _CELL_MAX + 1
    k = ((np.asarray(cx, np.int64) + off).astype(np.uint64) | ((np.asarray(cy, np.int64) + off).astype(np.uint64) << np.uint64(21)) |
         ((np.asarray(cz, np.int64) + off).astype(np.uint64) << np.uint64(42)))
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return (k & np.uint64(buckets - 1)).astype(np.int64)


def colliding_cloud(r, n_points, seed):
    """n_points points in cells that all hash to ONE bucket of the engine (cells chosen among a block of about 40 x the
    bucket count, so some of them are neighbours of each other and most are not): 1 - 4 points per cell, some on the
    cell's faces.  Returns (points, number of colliding cells)."""
    rng = np.random.default_rng(seed)
    h = float(np.float32(r)) * (1 + 2.0 ** -10)
    buckets = engine_buckets(n_points)
    span = int(np.ceil((40 * buckets) ** (1 / 3)))
    g = np.arange(-(span // 2), span - span // 2)
    cx, cy, cz = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    b = engine_bucket(cx, cy, cz, buckets)
    cells = np.stack([cx, cy, cz], axis=1)[b == b[0]]
    pts = []
    while len(pts) < n_points:
        c = cells[rng.integers(len(cells))]
        for _ in range(int(rng.integers(1, 5))):
            f = rng.random(3)
            f[rng.random(3) < 0.2] = 0.0                # on the cell's lower faces
            pts.append((c + f) * h)
    pts = np.asarray(pts[:n_points], np.float32)
    # keep only points whose float32 coordinates still fall in a colliding cell (rounding may move a face point out)
    cell = np.floor(pts.astype(np.float64) / h).astype(np.int64)
    ok = engine_bucket(cell[:, 0], cell[:, 1], cell[:, 2], buckets) == b[0]
    return pts[ok], len(cells)
