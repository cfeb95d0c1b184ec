"""The world map's local shape restated in numpy and Python ints (include/dsi_map_pca.h; DESIGN.md 7j "Local shape"): the
neighbourhoods (the box rule of map_knn_reference.py, every admitted cell or the first k by (d2, key)), the quantised
offsets and their integer moments, the Jacobi eigen-solve with its flags, signs and labels, the selection and the prune,
and the scenes that the GPU tests and the CPU tests share.  Every floating-point operation is a numpy float64 operation
rounded on its own, in the order the header states; the solve runs on all rows at once, a skipped rotation keeping the row's
old values."""
import functools
import itertools

import numpy as np

import map_knn_reference as kref
import world_map_reference as ref

IDENTITY = kref.IDENTITY
SWEEPS = 8
SEPARATION = 2.0 ** -26
QUANTUM_PER_LEAF = 2.0 ** -10
MAX_OFFSET = 3073
MAX_FOUND = 342
LABELS = {"linear": 1, "planar": 2, "scattered": 4}
COUNTS = ("n_cells", "n_unqueried", "n_sparse", "n_label", "n_normal_determined", "n_tangent_determined", "sum_members", "reach")


def quantum_of(leaf):
    return np.float64(leaf) * np.float64(QUANTUM_PER_LEAF)


def admitted_sets(cells, leaf, radius):
    """Steps 1-4 of dsi_map_knn.h for every cell of `cells` (a ReferenceMap.extract() already filtered, by ascending key) as
    its own query, itself excluded by key.  Returns (D2, KEY, J, reach): per query and per offset of the box d2 (+inf where
    no cell is admitted), the key (all ones there) and the candidate's row in `cells`."""
    radius, leaf = np.float64(radius), np.float64(leaf)
    reach = kref.reach_of(radius, leaf)
    assert 1 <= reach <= 3
    q_all = np.asarray(cells["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    keys_b = np.asarray(cells["keys"], np.uint64)
    p, N = q_all, q_all.shape[0]
    span = range(-reach, reach + 1)
    offsets = list(itertools.product(span, span, span))
    D2 = np.full((N, len(offsets)), np.inf)
    KEY = np.full((N, len(offsets)), ~np.uint64(0), np.uint64)
    J = np.zeros((N, len(offsets)), np.int64)
    if N:
        with np.errstate(all="ignore"):
            c = np.floor(p / leaf)
            for col, (oz, oy, ox) in enumerate(offsets):
                v = c + np.array([ox, oy, oz], np.float64)
                inside = (np.abs(v) <= ref.CELL_MAX).all(axis=1)
                key = ref.pack_key(np.where(inside[:, None], v, 0.0).astype(np.int64))
                j = np.minimum(np.searchsorted(keys_b, key), N - 1)
                hit = inside & (keys_b[j] == key) & (key != keys_b)
                q = q_all[j]
                dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
                d2 = ((dx * dx) + dy * dy) + dz * dz
                adm = hit & (np.sqrt(d2) <= radius)
                D2[:, col] = np.where(adm, d2, np.inf)
                KEY[:, col] = np.where(adm, key, ~np.uint64(0))
                J[:, col] = j
    return D2, KEY, J, reach


def moments(cells, leaf, radius, k):
    """Steps 1-3: dict of found int64 [N], s int64 (N, 3), ss int64 (N, 6), member (N, offsets) bool, KEY and reach"""
    assert 0 <= k <= kref.MAX_K
    D2, KEY, J, reach = admitted_sets(cells, leaf, radius)
    member = np.isfinite(D2)
    if k > 0:
        order = np.lexsort((KEY, D2), axis=1)                                      # by (d2, key): a total order
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.broadcast_to(np.arange(order.shape[1]), order.shape), axis=1)
        member &= rank < k
    xyz = np.asarray(cells["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    quantum = quantum_of(leaf)
    N = xyz.shape[0]
    s = np.zeros((N, 3), np.int64)
    ss = np.zeros((N, 6), np.int64)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for col in range(D2.shape[1]):
        on = member[:, col]
        if not on.any():
            continue
        D = np.rint((xyz[J[:, col]] - xyz) / quantum).astype(np.int64)             # IEEE subtract, divide, ties to even
        D = np.where(on[:, None], D, 0)
        assert np.abs(D).max() <= MAX_OFFSET
        s += D
        for i, (a, b) in enumerate(pairs):
            ss[:, i] += D[:, a] * D[:, b]
    return {"found": member.sum(axis=1).astype(np.int64), "s": s, "ss": ss, "member": member, "KEY": KEY, "reach": reach}


def _rotate(A, V, p, q):
    apq = A[p][q]
    skip = apq == 0.0
    with np.errstate(all="ignore"):
        theta = (A[q][q] - A[p][p]) / (2.0 * apq)
        t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        new = {}
        for k in range(3):
            akp, akq = A[k][p], A[k][q]
            new[(k, p)], new[(k, q)] = c * akp - s * akq, s * akp + c * akq
        for key, v in new.items():
            A[key[0]][key[1]] = np.where(skip, A[key[0]][key[1]], v)
        new = {}
        for k in range(3):
            apk, aqk = A[p][k], A[q][k]
            new[(p, k)], new[(q, k)] = c * apk - s * aqk, s * apk + c * aqk
        for key, v in new.items():
            A[key[0]][key[1]] = np.where(skip, A[key[0]][key[1]], v)
        new = {}
        for k in range(3):
            vkp, vkq = V[k][p], V[k][q]
            new[(k, p)], new[(k, q)] = c * vkp - s * vkq, s * vkp + c * vkq
        for key, v in new.items():
            V[key[0]][key[1]] = np.where(skip, V[key[0]][key[1]], v)


def _pick(a0, a1, a2, i):
    return np.where(i == 0, a0, np.where(i == 1, a1, a2))


def _unit_canonical(x, y, z):
    norm = np.sqrt(((x * x + y * y) + z * z))
    x, y, z = x / norm, y / norm, z / norm
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    lead = np.where((ax >= ay) & (ax >= az), x, np.where(ay >= az, y, z))
    flip = lead < 0.0
    return np.stack([np.where(flip, -x, x), np.where(flip, -y, y), np.where(flip, -z, z)], axis=1)


def solve(m, s, ss, quantum, orient=False, viewpoint=None, p=None):
    """Steps 3-7 and the row of step 8 on N rows at once: m int [N], s (N, 3), ss (N, 6) (Python-int exact: every product is
    below 2^41).  Returns dict of normal_d, tangent_d, lambda (float64 (N, 3)), normal, tangent, eval (float32 (N, 3)), label
    and flags (uint8 [N]) and C (the six centred integers)."""
    m = np.asarray(m, np.int64).reshape(-1)
    s = np.asarray(s, np.int64).reshape(-1, 3)
    ss = np.asarray(ss, np.int64).reshape(-1, 6)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    C = np.stack([m * ss[:, i] - s[:, a] * s[:, b] for i, (a, b) in enumerate(pairs)], axis=1)
    assert np.abs(C).max(initial=0) < 1 << 41
    Cd = C.astype(np.float64)                                                      # exact: below 2^53
    A = [[None] * 3 for _ in range(3)]
    for i, (a, b) in enumerate(pairs):
        A[a][b] = Cd[:, i].copy()
        A[b][a] = Cd[:, i].copy()
    one, zero = np.ones(len(m)), np.zeros(len(m))
    V = [[one.copy() if i == j else zero.copy() for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1)
        _rotate(A, V, 0, 2)
        _rotate(A, V, 1, 2)
    e = [np.where(A[i][i] < 0.0, 0.0, A[i][i]) for i in range(3)]
    i0 = np.where((e[0] <= e[1]) & (e[0] <= e[2]), 0, np.where(e[1] <= e[2], 1, 2))   # the first minimum
    ia, ib = np.where(i0 == 0, 1, 0), np.where(i0 == 2, 1, 2)
    i2 = np.where(_pick(*e, ia) >= _pick(*e, ib), ia, ib)                          # the first maximum among the other two
    i1 = 3 - i0 - i2
    l0, l1, l2 = _pick(*e, i0), _pick(*e, i1), _pick(*e, i2)
    normal = _unit_canonical(*[_pick(V[r][0], V[r][1], V[r][2], i0) for r in range(3)])
    tangent = _unit_canonical(*[_pick(V[r][0], V[r][1], V[r][2], i2) for r in range(3)])
    if orient:
        w = np.asarray(viewpoint, np.float64).reshape(1, 3) - np.asarray(p, np.float64).reshape(-1, 3)
        dot = ((normal[:, 0] * w[:, 0] + normal[:, 1] * w[:, 1]) + normal[:, 2] * w[:, 2])
        normal = np.where((dot < 0.0)[:, None], -normal, normal)
    size = (l0 + l1) + l2
    flags = ((l1 - l0 > SEPARATION * size).astype(np.uint8) | ((l2 - l1 > SEPARATION * size).astype(np.uint8) << 1)).astype(np.uint8)
    g0, g1, g2 = np.sqrt(l0), np.sqrt(l1), np.sqrt(l2)
    lin, pla = g2 - g1, g1 - g0
    label = np.where((lin >= pla) & (lin >= g0), 1, np.where(pla >= g0, 2, 3)).astype(np.uint8)
    md = m.astype(np.float64)
    mm, qq = md * md, np.float64(quantum) * np.float64(quantum)
    lam = np.stack([l0, l1, l2], axis=1)
    ev = ((lam / mm[:, None]) * qq).astype(np.float32)
    return {"normal_d": normal, "tangent_d": tangent, "lambda": lam, "normal": normal.astype(np.float32),
            "tangent": tangent.astype(np.float32), "eval": ev, "label": label, "flags": flags, "C": C}


def shape_pass(rm, k, radius, min_found=2, orient=False, viewpoint=None, keep_moments=True, min_points=1, min_windows=1):
    """WorldMap.pca and fetchPca(sort=True) in one dict: the counts, and per query keys, normal, tangent, eval, members, label,
    flags and moments (N, 9)"""
    assert 2 <= min_found <= (MAX_FOUND if k == 0 else max(k, 2))
    cells = rm.extract(min_points, min_windows)
    mo = moments(cells, rm.leaf, radius, k)
    found = mo["found"]
    N = len(found)
    m = found + 1
    p = cells["xyz"].astype(np.float64)
    sol = solve(m, mo["s"], mo["ss"], quantum_of(rm.leaf), orient, viewpoint, p)
    sparse = found < min_found
    out = {"keys": cells["keys"], "members": m.astype(np.uint16), "moments": np.concatenate([mo["s"], mo["ss"]], axis=1),
           "label": np.where(sparse, 0, sol["label"]).astype(np.uint8), "flags": np.where(sparse, 0, sol["flags"]).astype(np.uint8),
           "normal": np.where(sparse[:, None], np.float32(0), sol["normal"]), "tangent": np.where(sparse[:, None], np.float32(0), sol["tangent"]),
           "eval": np.where(sparse[:, None], np.float32(np.inf), sol["eval"]), "sparse": sparse, "solved": sol, "found": found,
           "xyz": cells["xyz"], "filter": (min_points, min_windows), "rows": mo}
    out.update({"n_cells": N, "n_unqueried": len(rm.keys) - N, "n_sparse": int(sparse.sum()),
                "n_label": [int((out["label"] == v).sum()) for v in (1, 2, 3)],
                "n_normal_determined": int((out["flags"] & 1).sum()), "n_tangent_determined": int(((out["flags"] >> 1) & 1).sum()),
                "sum_members": int(m.sum()), "reach": mo["reach"]})
    return out


def keep_mask(keep):
    return keep if isinstance(keep, int) else sum(LABELS[name] for name in set(keep))


def select(rm, sp, keep, remove_sparse):
    """WorldMap.selectShapes on the pass sp of rm: dict of the counts and per OCCUPIED cell (by ascending key) `all_reason`;
    `reason` is the queries' (fetchPca's)"""
    mask = keep_mask(keep)
    assert 1 <= mask <= 7
    lab = sp["label"].astype(np.int64)
    r = np.zeros(len(lab), np.uint8)
    kept_label = ((mask >> np.maximum(lab - 1, 0)) & 1).astype(bool)
    r[(lab > 0) & ~kept_label] = 3
    if remove_sparse:
        r[lab == 0] = 2
    every = np.ones(len(rm.keys), np.uint8)
    every[np.searchsorted(rm.keys, sp["keys"])] = r
    return {"n_cells": len(every), "n_kept": int((every == 0).sum()), "n_removed": [int((every == v).sum()) for v in (1, 2, 3)],
            "reason": r, "all_reason": every}


def capacity_after(kept, capacity, shrink):
    if not shrink:
        return capacity
    log2 = 8
    while kept * 4 > 3 << log2:
        log2 += 1
    return 1 << log2


class PcaReferenceMap(kref.KnnReferenceMap):
    def prune_shapes(self, sp, keep, remove_sparse):
        out = select(self, sp, keep, remove_sparse)
        ok = out["all_reason"] == 0
        self.keys, self.n, self.S = self.keys[ok], self.n[ok], self.S[ok]
        self.windows, self.stamp = self.windows[ok], self.stamp[ok]
        return out


def reference_of(calls, leaf):
    rm = PcaReferenceMap(leaf)
    for pts, T in calls:
        rm.integrate(pts, T)
    return rm


def brute_force_moments(cells, leaf, radius, k):
    """all pairs, no cells, Python ints: per query the other cells with sqrt(d2) <= radius, cut at the first k by (d2, key)
    when k > 0; found [N], moments (N, 9) as nested lists of ints"""
    xyz = np.asarray(cells["xyz"], np.float32).astype(np.float64)
    keys = np.asarray(cells["keys"], np.uint64)
    quantum = quantum_of(leaf)
    found, rows = [], []
    for i in range(len(xyz)):
        dx, dy, dz = xyz[i, 0] - xyz[:, 0], xyz[i, 1] - xyz[:, 1], xyz[i, 2] - xyz[:, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        idx = np.flatnonzero((np.sqrt(d2) <= np.float64(radius)) & (keys != keys[i]))
        if k > 0:
            idx = idx[np.lexsort((keys[idx], d2[idx]))][:k]
        D = [[int(v) for v in row] for row in np.rint((xyz[idx] - xyz[i]) / quantum)]
        s = [sum(d[a] for d in D) for a in range(3)]
        ss = [sum(d[a] * d[b] for d in D) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        found.append(len(idx))
        rows.append(s + ss)
    return np.array(found, np.int64), np.array(rows, np.int64).reshape(-1, 9)


# ---- the scenes ----
LEAF = 0.05
RADII = (0.05, 0.1, 0.15)                                                        # reach 1, 2, 3
KS = (0, 1, 3, 5, 8, 16)                                                         # every instantiation; 3 and 5 are truncated ones
VIEWPOINT = (0.3, -0.2, -2.0)


@functools.lru_cache(maxsize=None)
def scene_calls():
    """about 2,000 cells: a tilted, jittered plane patch, a jittered helix and uniform noise, apart from each other, seen by
    three calls (the third repeats about 40 % of the points: with min_windows = 2 the others leave)"""
    rng = np.random.default_rng(71)
    g = np.arange(34) * 0.05
    u, v = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    plane = np.stack([u, v, 0.35 * u - 0.2 * v + 1.0], axis=1) + rng.normal(0.0, 0.004, (len(u), 3))
    t = np.linspace(0.0, 8.0 * np.pi, 900)
    helix = np.stack([0.4 * np.cos(t) + 3.0, 0.4 * np.sin(t), 0.05 * t + 1.0], axis=1) + rng.normal(0.0, 0.003, (len(t), 3))
    noise = rng.uniform(0.0, 0.65, (800, 3)) + np.array([-3.0, 0.0, 1.0])
    pts = np.concatenate([plane, helix, noise])
    pts = pts[rng.permutation(len(pts))]
    again = pts[rng.random(len(pts)) < 0.4] + rng.normal(0.0, 0.0005, (1, 3))
    half = len(pts) // 2
    return ((pts[:half].astype(np.float32), IDENTITY), (pts[half:].astype(np.float32), IDENTITY), (again.astype(np.float32), IDENTITY))


@functools.lru_cache(maxsize=None)
def scene_reference():
    return reference_of(scene_calls(), LEAF)


@functools.lru_cache(maxsize=None)
def scene_pass(k, radius, min_found=2, orient=False, min_points=1, min_windows=1):
    """the restatement's pass over the scene, computed once per setting and shared"""
    return shape_pass(scene_reference(), k, radius, min_found, orient, VIEWPOINT if orient else None, True, min_points, min_windows)


@functools.lru_cache(maxsize=None)
def cloud_calls():
    """a random cloud for the brute-force check: 400 points of a cube of 12 leaves, one call"""
    rng = np.random.default_rng(72)
    return ((rng.uniform(-0.3, 0.3, (400, 3)).astype(np.float32), IDENTITY),)


SHAPE_LEAF = 0.5                                                                 # cell centres and their offsets are exact


def block_calls(nx, ny, nz):
    """one point at each cell centre of an nx x ny x nz block around the origin"""
    gx, gy, gz = (np.arange(n) - n // 2 for n in (nx, ny, nz))
    c = np.stack([a.ravel() for a in np.meshgrid(gx, gy, gz, indexing="ij")], axis=1)
    return (((c + 0.5) * SHAPE_LEAF).astype(np.float32), IDENTITY),


def centre_key(c):
    return int(ref.pack_key(np.array([c], np.int64))[0])


# ---- the layout cases (tests/map_layout_cases.py) ----
DENSE_K, DENSE_RADIUS = 8, 0.05                                                  # reach 1 at the layout cases' leaf


@functools.lru_cache(maxsize=None)
def dense_pass():
    """the pass over the layout cases' dense scene (300,007 cells in a table of 2^19 slots: two rounds of every stride)"""
    import map_layout_cases as lc
    return shape_pass(lc.dense_reference(), DENSE_K, DENSE_RADIUS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_passes_equal(info, rows, want, moments=True):
    """info: WorldMap.pca's dict; rows: fetchPca(sort=True)'s; want: shape_pass's.  array_equal on everything, the floats by
    their bits."""
    for f in COUNTS:
        assert info[f] == want[f], (f, info[f], want[f])
    for f in ("keys", "members", "label", "flags") + (("moments",) if moments else ()):
        assert rows[f].dtype == want[f].dtype and np.array_equal(rows[f], want[f]), f
    for f in ("normal", "tangent", "eval"):
        assert rows[f].dtype == np.float32 and np.array_equal(bits(rows[f]), bits(want[f])), f + " bits"
