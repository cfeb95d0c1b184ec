"""evaluateDSI / process_1 / process_2 assembled from the CPU oracle's pieces, for tests
and for bench.py's cpu_baseline leg.  TEST INFRASTRUCTURE (imports oracle/)."""
import numpy as np

from oracle import oracle as orc

PACKET = 1024


class OracleMapper:
    """MapperEMVS restated with oracle calls (mapper_emvs_stereo.cpp:29-64, 208-241)."""

    def __init__(self, cam, dimX=0, dimY=0, dimZ=100, min_depth=0.3, max_depth=5.0, fov=0.0,
                 lut=None, inverse_depth=False, exact=False):
        """exact=True: the DSI is the engine's exact contract instead of the reference's fp32 event-order sums -- every
        weight added as trunc(w * 2^31) into a uint64 per voxel (self.acc), rounded to fp32 once (self.dsi);
        self.count holds the votes per voxel."""
        w, h, fx, fy, cx, cy = cam
        self.W, self.H = int(w), int(h)
        self.K = np.array([fx, fy, cx, cy], np.float32)
        self.nx = dimX if dimX > 0 else self.W
        self.ny = dimY if dimY > 0 else self.H
        self.nz = dimZ
        self.planes = orc.depth_planes(min_depth, max_depth, dimZ, inverse_depth)
        f = orc.virtual_focal(np.float32(fx), fov, self.nx)
        self.Kv = np.array([f, f, np.float32(cx), np.float32(cy)], np.float32)
        self.lut = None if lut is None else np.ascontiguousarray(lut, np.float32)
        self.dsi = np.zeros((self.nz, self.ny, self.nx), np.float32)
        self.exact = bool(exact)
        self.acc = self.count = None

    def packetize(self, ts, trajectory, T_rv_w):
        """mapper_emvs_stereo.cpp:67-105 -> (first[np], Rt[np][12]) or None."""
        times, poses = trajectory
        n = ts.shape[0]
        if n < PACKET:
            return None
        first, Rt = [], []
        cur = 0
        while cur + PACKET < n:
            T = orc.pose_at(times, poses, ts[cur + PACKET // 2])
            if T is None:
                cur += 1
                continue
            first.append(cur)
            Rt.append(orc.event_pose_Rt(T_rv_w, T))
            cur += PACKET
        return (np.array(first, np.int64), np.array(Rt, np.float32).reshape(-1, 12))

    def stage_a(self, x, y, first, Rt):
        centers, H = orc.packet_geometry(Rt, self.K, self.Kv, self.planes[0])
        idx = (first[:, None] + np.arange(PACKET)[None, :]).reshape(-1)
        xy = orc.warp_z0(x[idx], y[idx], H, self.lut, self.W)
        return xy, centers

    def evaluate_packets(self, x, y, first, Rt):
        xy, centers = self.stage_a(x, y, first, Rt)
        if self.exact:
            self.acc, self.count = orc.fill_voxel_grid_q31(xy, centers, self.planes, self.Kv, self.nx, self.ny)
            self.dsi = orc.q31_to_float(self.acc)
            return xy, centers
        self.dsi[:] = 0  # resetGrid, :145
        orc.fill_voxel_grid(xy, centers, self.planes, self.Kv, self.nx, self.ny, self.dsi)
        return xy, centers

    def evaluate_packets_rows(self, x, y, first, Rt, row_begin, row_count):
        """Rows [row_begin, row_begin + row_count) of every plane of the DSI evaluate_packets builds, bit-equal to
        them (oracle.fill_voxel_grid_rows): for grids whose full DSI the CPU cannot afford."""
        xy, centers = self.stage_a(x, y, first, Rt)
        return orc.fill_voxel_grid_rows(xy, centers, self.planes, self.Kv, self.nx, self.ny, row_begin, row_count)

    def evaluateDSI(self, events, trajectory, T_rv_w):
        x, y, ts = events
        pk = self.packetize(ts, trajectory, T_rv_w)
        if pk is None:
            return False
        self.evaluate_packets(x, y, *pk)
        self.n_voted = pk[0].shape[0] * PACKET
        return True

    def depth_map(self, dsi=None):
        conf, idx = orc.collapse_max_z(self.dsi if dsi is None else dsi)
        return orc.indices_to_depth(idx, self.planes), conf, idx


# ---- process_1 / process_2 of the reference, assembled from oracle pieces ----------------
def _pose_mul(a, b):
    from dvs_mcemvs_amd import synthetic as syn
    qa, qb = a[3:], b[3:]
    w = qa[0] * qb[0] - qa[1] * qb[1] - qa[2] * qb[2] - qa[3] * qb[3]
    x = qa[0] * qb[1] + qa[1] * qb[0] + qa[2] * qb[3] - qa[3] * qb[2]
    y = qa[0] * qb[2] + qa[2] * qb[0] + qa[3] * qb[1] - qa[1] * qb[3]
    z = qa[0] * qb[3] + qa[3] * qb[0] + qa[1] * qb[2] - qa[2] * qb[1]
    return np.concatenate([a[:3] + syn.quat_rotate(qa, b[:3]), [w, x, y, z]])


def oracle_process_1(make_mapper, events, trajectories, ts, fusion_method, rv_pos=0.0):
    """process1.cpp:54-191 -> (per-camera DSIs, fused DSI)."""
    from dvs_mcemvs_amd import synthetic as syn
    T_w_l = orc.pose_at(trajectories[0][0], trajectories[0][1], ts)
    T_rv_w = syn.pose_inverse(_pose_mul(T_w_l, np.array([rv_pos, 0, 0, 1, 0, 0, 0.0])))
    dsis = []
    for ev, tr in zip(events, trajectories):
        m = make_mapper()
        m.evaluateDSI(ev, tr, T_rv_w)
        dsis.append(m.dsi.copy())
    fused = orc.accumulate(np.zeros_like(dsis[0]), dsis[0], 0)
    fused = orc.fuse2(fused, dsis[1], fusion_method)
    if len(dsis) > 2:
        if fusion_method == 1:
            fused = orc.fuse2(fused, dsis[2], 1)
        elif fusion_method == 2:
            fused = orc.fuse_hm_n(fused, dsis[2], 3)
        elif fusion_method == 6:
            fused = orc.fuse2(fused, dsis[2], 6)
    return dsis, fused


def oracle_process_2(make_mapper, events, trajectories, n_sub, ts, stereo_fusion, temporal_fusion,
                     shuffle_right=False):
    """process2.cpp:46-289 (process5.cpp when shuffle_right) -> dict(left, right, fused, camera_time)."""
    from dvs_mcemvs_amd import synthetic as syn
    T_rv_w = syn.pose_inverse(orc.pose_at(trajectories[0][0], trajectories[0][1], ts))
    per = [events[c][0].shape[0] // n_sub for c in range(2)]
    zero = np.zeros_like(make_mapper().dsi)
    left, right, fused = zero.copy(), zero.copy(), zero.copy()
    right_sel = None
    if shuffle_right:  # process5.cpp:89-93, :136-150
        n1, idx, right_sel = events[1][0].shape[0], (n_sub // 2) * per[1], []
        for _ in range(n_sub):
            if idx + per[1] >= n1:
                right_sel.append(np.concatenate([np.arange(idx, n1), np.arange(0, idx + per[1] - n1)]))
                idx = idx + per[1] - n1
            else:
                right_sel.append(np.arange(idx, idx + per[1]))
                idx += per[1]
    for k in range(n_sub):
        d = []
        for c in range(2):
            sl = slice(k * per[c], (k + 1) * per[c])
            if c == 1 and right_sel is not None:
                sl = right_sel[k]
            m = make_mapper()
            m.evaluateDSI(tuple(a[sl] for a in events[c]), trajectories[c], T_rv_w)
            d.append(m.dsi.copy())
        sub = orc.fuse2(orc.accumulate(zero, d[0], 0), d[1], stereo_fusion)
        if temporal_fusion in (2, 4):
            mode = 1 if temporal_fusion == 2 else 0
            left, right, fused = (orc.accumulate(left, d[0], mode), orc.accumulate(right, d[1], mode),
                                  orc.accumulate(fused, sub, mode))
            if k == n_sub - 1:
                left, right, fused = (orc.finalize(g, mode, n_sub) for g in (left, right, fused))
    converse = {1: 1, 2: 2, 3: 4, 4: 3, 5: 5, 6: 6}[stereo_fusion]  # process2.cpp:274-279 swap
    cam_time = orc.fuse2(orc.accumulate(zero, left, 0), right, converse)
    return {"left": left, "right": right, "fused": fused, "camera_time": cam_time}


# ---- the depth-map statement ---------------------------------------------------------------
def argmax_report(idx_gpu, ref_volume, vol_tol):
    """Closes "depth map equal to the CPU reference" for EVERY pixel (cartesian3dgrid.cpp:132-134).

    ref_volume: the CPU oracle's volume [nz][ny][nx] the arg-max runs over; idx_gpu: the GPU's plane
    index per pixel, taken from ITS volume g, which agrees with ref_volume to
    |g - ref| <= vol_tol * max(1, |ref|) for every voxel (asserted separately by the caller).
    Then for every pixel either the indices are equal, or the GPU's plane is a provable near-tie of
    the oracle's column:  ref[idx_gpu] >= ref_max - 2 * vol_tol * max(1, ref_max), because
    ref[idx_gpu] >= g[idx_gpu] - t >= g[idx_cpu] - t >= ref_max - 2 t.  Anything else is a wrong
    depth.  Returns the fractions and the violation count (0 = the statement holds)."""
    ref_max = ref_volume.max(axis=0)
    idx_cpu = ref_volume.argmax(axis=0)                     # first maximum, like std::max_element
    picked = np.take_along_axis(ref_volume, idx_gpu[None].astype(np.int64), axis=0)[0]
    same = idx_gpu == idx_cpu
    slack = 2.0 * vol_tol * np.maximum(1.0, np.abs(ref_max.astype(np.float64)))
    near = (~same) & (picked.astype(np.float64) >= ref_max.astype(np.float64) - slack)
    bad = ~(same | near)
    return {"argmax_agree_frac": float(same.mean()), "near_tie_frac": float(near.mean()),
            "violations": int(bad.sum()), "pixels": int(same.size),
            "worst_deficit_over_slack": float(np.max((ref_max.astype(np.float64) - picked) / slack))}
