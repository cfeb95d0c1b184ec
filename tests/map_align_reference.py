"""Aligning world maps restated from include/dsi_map_align.h (DESIGN.md 7j "Aligning"): numpy for the geometry, Python
ints for the moments, Python floats for the solver.  Elementwise float64 operations only, as world_map_reference.py: every
product and sum is rounded on its own, a dot product is ((a0 b0 + a1 b1) + a2 b2).

    step      p' = T p (rule 1); c = floor(p' / leaf_b); candidates as map_eval_reference.compare's, around p';
              the least (d2, key) wins; matched iff sqrt(d2) <= radius; quantum = leaf_b 2^-10;
              U = rint(p' / quantum), V = rint(q / quantum); su, sv, sum U[r] V[c] split into hi = P >> 32 and
              lo = P & 0xffffffff, e2 = sum (U - V)^2 -- all Python ints
    solve     centred in ints, scaled by quantum^2 / n^2, Horn's N, 16 sweeps of cyclic Jacobi, t = mean V - R mean U
    compose   R = A_R B_R, t = A_R B_t + A_t
    loop      step, solve, T <- compose(T_delta, T)
"""
import math

import numpy as np

import map_merge_reference as merge_ref
import world_map_reference as ref

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
MASK32 = (1 << 32) - 1
SWEEPS = 16
SEPARATION = 2.0 ** -26


class Refused(ValueError):
    """what the engine refuses with DSI_ERR_INVALID; args[0] names the cause"""


# ---- poses ----

def compose(A, B):
    A, B = np.asarray(A, np.float64).reshape(3, 4), np.asarray(B, np.float64).reshape(3, 4)
    out = np.empty((3, 4), np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
        out[i, 3] = ((A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3]) + A[i, 2] * B[2, 3]) + A[i, 3]
    return out.reshape(12)


def axis_angle_pose(axis, angle, t):
    """12 doubles [R | t] of a rotation by `angle` radians about `axis` and a translation: pose_matrix's expression of the
    unit quaternion, in Python floats (no BLAS: the same bits on every machine)"""
    ax, ay, az = (float(v) for v in axis)
    norm = math.sqrt((ax * ax + ay * ay) + az * az)
    s = math.sin(0.5 * angle) / norm
    w, x, y, z = math.cos(0.5 * angle), ax * s, ay * s, az * s
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return np.array([R[r] + [float(t[r])] for r in range(3)], np.float64).reshape(12)


def pose_error(T, T_true):
    """(angle in radians, norm of the translation difference) between two poses, in Python floats"""
    A, B = np.asarray(T, np.float64).reshape(3, 4).tolist(), np.asarray(T_true, np.float64).reshape(3, 4).tolist()
    trace = sum(A[r][c] * B[r][c] for r in range(3) for c in range(3))
    d = [A[r][3] - B[r][3] for r in range(3)]
    return math.acos(max(-1.0, min(1.0, (trace - 1.0) / 2.0))), math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


# ---- one correspondence pass ----

def quantise(x, quantum):
    """llrint(x / quantum): the IEEE divide, rounded to the nearest integer, ties to even"""
    return np.rint(np.asarray(x, np.float64) / np.float64(quantum)).astype(np.int64)


def moments_of(U, V, n_cells, quantum, reach):
    """the integer moments of matched pairs U, V (int64 (M, 3)), as Python ints"""
    U = [[int(v) for v in row] for row in np.asarray(U, np.int64).reshape(-1, 3)]
    V = [[int(v) for v in row] for row in np.asarray(V, np.int64).reshape(-1, 3)]
    m = {"n_cells": int(n_cells), "n_matched": len(U), "n_unmatched": int(n_cells) - len(U), "su": [0, 0, 0], "sv": [0, 0, 0],
         "suv_hi": [0] * 9, "suv_lo": [0] * 9, "e2": 0, "quantum": float(quantum), "reach": int(reach)}
    for u, v in zip(U, V):
        for r in range(3):
            m["su"][r] += u[r]
            m["sv"][r] += v[r]
            m["e2"] += (u[r] - v[r]) ** 2
            for c in range(3):
                P = u[r] * v[c]
                m["suv_hi"][3 * r + c] += P >> 32                                # (Python's >> floors, as an arithmetic shift)
                m["suv_lo"][3 * r + c] += P & MASK32
    return m


def step(cells_a, cells_b, leaf_b, radius, T=IDENTITY):
    """cells_a / cells_b: ReferenceMap.extract() (or WorldMap.extract()) of the two maps, already filtered, by ascending
    key.  Returns what WorldMap.alignStep(..., correspondences=True) returns: the moments, keys (a's), keys_other (0 where
    unmatched) and dist (float32, inf where unmatched); plus U, V (int64, the matched pairs) and matched (bool)."""
    radius, leaf_b = np.float64(radius), np.float64(leaf_b)
    reach = int(np.ceil(radius / leaf_b))
    assert 1 <= reach <= 3
    quantum = leaf_b * np.float64(2.0 ** -10)
    p = ref.world_positions(np.asarray(cells_a["xyz"], np.float32).reshape(-1, 3), T)
    q_all = np.asarray(cells_b["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    keys_b = np.asarray(cells_b["keys"], np.uint64)
    assert (keys_b[1:] > keys_b[:-1]).all()
    M = p.shape[0]
    best = np.full(M, np.inf)
    best_key = np.zeros(M, np.uint64)
    best_q = np.zeros((M, 3), np.float64)
    with np.errstate(all="ignore"):
        c = np.floor(p / leaf_b)
        for oz in range(-reach, reach + 1):
            for oy in range(-reach, reach + 1):
                for ox in range(-reach, reach + 1):
                    if keys_b.shape[0] == 0:
                        continue
                    v = c + np.array([ox, oy, oz], np.float64)
                    inside = (np.abs(v) <= ref.CELL_MAX).all(axis=1)                # (NaN and the infinities compare false)
                    key = ref.pack_key(np.where(inside[:, None], v, 0.0).astype(np.int64))
                    j = np.minimum(np.searchsorted(keys_b, key), keys_b.shape[0] - 1)
                    hit = inside & (keys_b[j] == key)
                    q = q_all[j]
                    dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
                    d2 = ((dx * dx) + dy * dy) + dz * dz
                    better = hit & ((d2 < best) | ((d2 == best) & (key < best_key)))
                    best = np.where(better, d2, best)
                    best_key = np.where(better, key, best_key)
                    best_q = np.where(better[:, None], q, best_q)
        d = np.sqrt(best)
        matched = (best_key != 0) & (d <= radius)
        U, V = quantise(p[matched], quantum), quantise(best_q[matched], quantum)
    out = moments_of(U, V, M, quantum, reach)
    out.update(keys=np.asarray(cells_a["keys"], np.uint64), keys_other=np.where(matched, best_key, np.uint64(0)),
               dist=np.where(matched, d, np.inf).astype(np.float32), U=U, V=V, matched=matched)
    return out


MOMENT_KEYS = ("n_cells", "n_matched", "n_unmatched", "su", "sv", "suv_hi", "suv_lo", "e2", "quantum", "reach")


def assert_steps_equal(got, want, correspondences=True):
    """equality of every moment and (by key) of the correspondences, the distances by their float BITS"""
    for k in MOMENT_KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    if correspondences:
        for k in ("keys", "keys_other"):
            assert got[k].dtype == np.uint64 and np.array_equal(got[k], want[k]), k
        assert got["dist"].dtype == np.float32 and np.array_equal(got["dist"].view(np.uint32), want["dist"].view(np.uint32)), "dist bits"


# ---- the solver ----

def solve(m):
    """(T_delta, info) of dsx_map_align_solve, in Python ints and floats; raises Refused as the engine refuses"""
    n = int(m["n_matched"])
    if n < 3:
        raise Refused("n_matched")
    quantum = float(m["quantum"])
    nd = float(n)
    scale = (quantum * quantum) / (nd * nd)
    S = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            sum_p = int(m["suv_hi"][3 * r + c]) * (1 << 32) + int(m["suv_lo"][3 * r + c])
            S[r][c] = float(n * sum_p - int(m["su"][r]) * int(m["sv"][c])) * scale   # (int -> float rounds to nearest even)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    A = [[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]]
    Vm = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
                if A[p][q] == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                for k in range(4):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
                for k in range(4):
                    vkp, vkq = Vm[k][p], Vm[k][q]
                    Vm[k][p], Vm[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    lam = [A[k][k] for k in range(4)]
    i0 = max(range(4), key=lambda k: (lam[k], -k))                                # the first maximum
    i1 = max((k for k in range(4) if k != i0), key=lambda k: (lam[k], -k))
    size = ((abs(lam[0]) + abs(lam[1])) + abs(lam[2])) + abs(lam[3])
    rms = math.sqrt((float(m["e2"]) * (quantum * quantum)) / nd)
    if not lam[i0] - lam[i1] > SEPARATION * size:
        raise Refused("degenerate")
    w, x, y, z = (Vm[k][i0] for k in range(4))
    norm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / norm, x / norm, y / norm, z / norm
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    mu = [(float(int(m["su"][r])) / nd) * quantum for r in range(3)]
    mv = [(float(int(m["sv"][r])) / nd) * quantum for r in range(3)]
    t = [mv[r] - ((R[r][0] * mu[0] + R[r][1] * mu[1]) + R[r][2] * mu[2]) for r in range(3)]
    T = np.array([R[0] + [t[0]], R[1] + [t[1]], R[2] + [t[2]]], np.float64).reshape(12)
    info = {"n_matched": n, "rms": rms, "angle": 2.0 * math.atan2(math.sqrt((x * x + y * y) + z * z), w),
            "trans": math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]), "lambda": [lam[i0], lam[i1]]}
    return T, info


def kabsch(P, Q):
    """(R, t) minimising sum |R P + t - Q|^2 by numpy's SVD: the yardstick of the solver, not a restatement of it"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    mp, mq = P.mean(axis=0), Q.mean(axis=0)
    H = (P - mp).T @ (Q - mq)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, mq - R @ mp


# ---- the loop ----

def align(cells_a, cells_b, leaf_b, radius, T_init=IDENTITY, max_iterations=20, min_matched=3, eps_rot=1e-6, eps_trans=0.0,
          solver=solve, composer=compose):
    """dsx_map_align with this file's step: returns (T, info, history); history holds every round's (moments, T_delta or
    None, T after the round).  Raises Refused with .T and .info as WorldMap.align's DsiError has them."""
    T = np.asarray(T_init, np.float64).reshape(12).copy()
    info = {"iterations": 0, "converged": 0, "stopped": 0, "reach": 0, "n_cells": 0, "n_matched_first": 0, "n_matched_last": 0,
            "rms_first": 0.0, "rms_last": 0.0, "angle_last": 0.0, "trans_last": 0.0}
    history = []
    for it in range(int(max_iterations)):
        m = step(cells_a, cells_b, leaf_b, radius, T)
        info.update(iterations=it + 1, reach=m["reach"], n_cells=m["n_cells"], n_matched_last=m["n_matched"])
        if it == 0:
            info["n_matched_first"] = m["n_matched"]
        err = None
        if m["n_matched"] < min_matched:
            info["stopped"], err = 1, Refused("min_matched")
        else:
            try:
                T_delta, si = solver(m)
            except Exception as e:                                                 # (Refused here, DsiError from the engine's)
                info["stopped"], err = 2, e
        if err is not None:
            history.append((m, None, T.copy()))
            err.T, err.info, err.history = T, info, history
            raise err
        if it == 0:
            info["rms_first"] = si["rms"]
        info.update(rms_last=si["rms"], angle_last=si["angle"], trans_last=si["trans"])
        T = composer(T_delta, T)
        history.append((m, T_delta, T.copy()))
        if si["angle"] <= eps_rot and si["trans"] <= eps_trans:
            info["converged"] = 1
            break
    return T, info, history


# ---- one map into another's frame ----

def integrate_map(dst, src, T=IDENTITY, min_points=1, min_windows=1):
    """dsx_map_integrate_map on two reference maps: one integrate call of src's extracted centroids; returns
    (cells integrated, of those rejected)"""
    pts = src.extract(min_points, min_windows)["xyz"]
    return len(pts), dst.integrate(pts, T)


# ---- the scenes the CPU and GPU tests share ----

LEAF_A, LEAF_B = 0.05, 0.04


def surface_points(n, half, seed):
    """n float64 points on three mutually transverse wavy sheets through the cube [-half, half]^3: the rotation and the
    translation of a rigid motion are both observable from them"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
    sheet = rng.integers(0, 3, n)
    a, b = u / half, v / half                                                   # (products and sums only: the same bits everywhere)
    w = 0.12 * (a * (1.0 - a * a) * 2.0 + 0.3) * (1.0 - 1.4 * b * b) + 0.05 * u * v
    pts = np.where((sheet == 0)[:, None], np.stack([u, v, w - 0.3 * half], 1),
                   np.where((sheet == 1)[:, None], np.stack([w + 0.2 * half, u, v], 1), np.stack([u, w - 0.1 * half, v], 1)))
    return pts


def moved(pts, T):
    """float32 points T^-1 applied to float64 points: what a map whose frame lies at T in the other's sees"""
    Ti = ref.invert_pose(T).reshape(3, 4)
    x, y, z = (np.asarray(pts, np.float64)[:, k] for k in range(3))
    return np.stack([((Ti[r, 0] * x + Ti[r, 1] * y) + Ti[r, 2] * z) + Ti[r, 3] for r in range(3)], axis=1).astype(np.float32)


def reference_map(calls, leaf):
    rm = merge_ref.MergeReferenceMap(leaf)
    for pts in calls:
        assert rm.integrate(pts, IDENTITY) == 0
    return rm


T_TRUE_1 = axis_angle_pose((0.3, -0.5, 0.8), math.radians(2.0), (0.6 * LEAF_B * 0.6, -0.6 * LEAF_B * 0.64, 0.6 * LEAF_B * 0.48))
T_FAR = axis_angle_pose((0.0, 0.0, 1.0), 0.0, (7.0, -3.0, 5.0))


def scene1_calls():
    """(calls of a, calls of b): b sees the sheets where x < 0.2, in two calls and with a little noise; a sees its own
    sample of them from a frame that lies at T_TRUE_1 in b's, in three calls"""
    pa = moved(surface_points(9000, 0.8, 21), T_TRUE_1)
    pb = surface_points(9000, 0.8, 22)
    pb = pb[pb[:, 0] < 0.2]
    pb = (pb + np.random.default_rng(23).normal(0.0, 0.004, pb.shape)).astype(np.float32)
    return [pa[:4000], pa[4000:4001], pa[4001:]], [pb[:2500], pb[2500:]]


SCENE1_CELLS = (3169, 2923)
SCENE1_RADII = (0.04, 0.08, 0.12)                                               # reach 1, 2 and 3 at LEAF_B
SCENE1_LOOP = dict(radius=0.08, max_iterations=12, min_matched=100, eps_rot=2e-5, eps_trans=2e-5)
# what test_map_align_cpu.py recorded of align(scene 1, **SCENE1_LOOP) with the library's solver; the GPU loop must give it
SCENE1_LOOP_RESULT = dict(iterations=12, converged=0, n_matched_first=2241, n_matched_last=2239, rms_first=0.031602394622860526,
                          rms_last=0.025003228221491258, pose_error=(0.004081259648922497, 0.0070244743881649864))

T_TRUE_2 = axis_angle_pose((-0.6, 0.2, 0.4), math.radians(0.7), (0.011, 0.007, -0.013))


def scene2_calls():
    """the larger scene: about 20,000 cells of a on both sides of the origin"""
    pa = moved(surface_points(70000, 2.0, 31), T_TRUE_2)
    pb = surface_points(60000, 2.0, 32).astype(np.float32)
    return [pa[:30000], pa[30000:]], [pb]
