"""Orchestration of the reference's process_1 / process_2 (Alg. 1 / Alg. 2) over the GPU
engine: which mapper gets which events, where the reference view sits, the fusion order and
op codes, and the temporal accumulators.  Pure call sequencing -- every voxel operation is an
engine kernel.

    process_1   mapper_emvs_stereo/src/process1.cpp:28-224
    process_2   mapper_emvs_stereo/src/process2.cpp:28-302
    process_5   mapper_emvs_stereo/src/process5.cpp:28-260  (process_2 with the right camera's
                sub-intervals circularly shifted by num_subintervals/2)
    full_sequence / WindowStream   mapper_emvs_stereo/src/main.cpp:174-302  (--full_seq: a window of
                `duration` seconds every `out_skip` seconds, process_1 per window)
"""
import collections

import numpy as np

from . import engine as E
from . import synthetic as _q  # quaternion helpers only (numpy)


def pose_mul(a, b):
    """T_a * T_b for 7-vector poses (tx,ty,tz,qw,qx,qy,qz)."""
    qa, qb = np.asarray(a[3:], np.float64), np.asarray(b[3:], np.float64)
    w = qa[0] * qb[0] - qa[1] * qb[1] - qa[2] * qb[2] - qa[3] * qb[3]
    x = qa[0] * qb[1] + qa[1] * qb[0] + qa[2] * qb[3] - qa[3] * qb[2]
    y = qa[0] * qb[2] + qa[2] * qb[0] + qa[3] * qb[1] - qa[1] * qb[3]
    z = qa[0] * qb[3] + qa[3] * qb[0] + qa[1] * qb[2] - qa[2] * qb[1]
    t = np.asarray(a[:3], np.float64) + _q.quat_rotate(qa, np.asarray(b[:3], np.float64))
    return np.concatenate([t, [w, x, y, z]])


def apply_transformation_right(trajectory, T):
    """TrajectoryBase::applyTransformationRight (trajectory.hpp:57-63): every control pose becomes pose * T -- how
    main.cpp:199-216 turns the recorded poses into a camera's (hand-eye calibration, then the inverse extrinsics of the
    other cameras).  trajectory = (times, poses[n][7]); returns a new one."""
    times, poses = trajectory
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    return np.asarray(times, np.float64), np.stack([pose_mul(p, T) for p in poses])


def apply_transformation_left(trajectory, T):
    """TrajectoryBase::applyTransformationLeft (trajectory.hpp:65-71): every control pose becomes T * pose."""
    times, poses = trajectory
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    return np.asarray(times, np.float64), np.stack([pose_mul(T, p) for p in poses])


def reference_view_process1(trajectory_left, ts, rv_pos=0.0):
    """process1.cpp:56-68: T_w_rv = T_w_l(ts) * baseline(rv_pos along x); returns T_rv_w."""
    T_w_l = E.pose_at(trajectory_left, ts)
    if T_w_l is None:
        raise E.DsiError(E.ERR_INVALID, "no pose at the reference timestamp %r" % ts)
    baseline = np.array([rv_pos, 0, 0, 1, 0, 0, 0], np.float64)
    return _q.pose_inverse(pose_mul(T_w_l, baseline))


def reference_view_process2(trajectory_left, ts):
    """process2.cpp:79-81: T_rv_w = T_w_l(ts)^-1."""
    T = E.pose_at(trajectory_left, ts)
    if T is None:
        raise E.DsiError(E.ERR_INVALID, "no pose at the reference timestamp %r" % ts)
    return _q.pose_inverse(T)


def _fuse_cameras(fused, other, method):
    if method not in (1, 2, 3, 4, 5, 6):
        raise E.DsiError(E.ERR_BAD_OP, "Improper fusion method selected")
    fused.fuseTwoGrids(other, method)


def process_1(mappers, events, trajectories, mapper_fused, ts, fusion_method, rv_pos=0.0):
    """Alg. 1: one DSI per camera, fused across cameras (process1.cpp:54-191).
    mappers/events/trajectories: lists of 2 or 3 (a third camera is the EVIMO2 case).
    Returns T_rv_w; the fused DSI is mapper_fused.dsi_."""
    T_rv_w = reference_view_process1(trajectories[0], ts, rv_pos)
    for m, ev, tr in zip(mappers, events, trajectories):
        m.evaluateDSI(ev, tr, T_rv_w)                      # :76, :94, :110
    mapper_fused.dsi_.resetGrid()                          # :126
    mapper_fused.dsi_.addTwoGrids(mappers[0].dsi_)         # :127
    _fuse_cameras(mapper_fused.dsi_, mappers[1].dsi_, fusion_method)   # :136-158
    if len(mappers) > 2 and events[2][0].shape[0] > 0:     # :169-191
        g = mappers[2].dsi_
        if fusion_method == 1:
            mapper_fused.dsi_.minTwoGrids(g)
        elif fusion_method == 2:
            mapper_fused.dsi_.harmonicMeanTwoGrids(g, 3)
        elif fusion_method == 6:
            mapper_fused.dsi_.maxTwoGrids(g)
        # 3, 4, 5: the reference silently ignores the third camera
    return T_rv_w


def shuffled_subintervals(n_events, num_subintervals):
    """Index arrays of the right camera's sub-intervals in process_5 (process5.cpp:89-93,
    :136-150): start at shift*per with shift = n/2, wrap around the END OF THE EVENT VECTOR
    (not per*n), so a wrapped sub-interval is the tail followed by the head."""
    per = int(n_events) // int(num_subintervals)
    idx = (int(num_subintervals) // 2) * per
    out = []
    for _ in range(int(num_subintervals)):
        if idx + per >= n_events:
            sel = np.concatenate([np.arange(idx, n_events), np.arange(0, idx + per - n_events)])
            idx = idx + per - n_events
        else:
            sel = np.arange(idx, idx + per)
            idx += per
        out.append(sel)
    return out


def subinterval_ranges(n_events, num_subintervals, process_method=2, camera=0):
    """Python restatement of engine.alg2_subintervals (dsi_alg2_subintervals): per sub-interval (begin0, end0, begin1,
    end1) -- per = n_events // N, the tail dropped (process2.cpp:46-47, :105-107, :132-134); camera 1 of process_method 5
    starts at (N // 2) * per and wraps around the end of its events when idx + per >= n_events (process5.cpp:89-93,
    :135-150), as shuffled_subintervals does with index arrays."""
    n_events, n = int(n_events), int(num_subintervals)
    per = n_events // n
    shuffled = int(process_method) == 5 and int(camera) == 1
    idx = (n // 2) * per if shuffled else 0
    out = []
    for _ in range(n):
        if shuffled and idx + per >= n_events:
            out.append((idx, n_events, 0, idx + per - n_events))
            idx = idx + per - n_events
        else:
            out.append((idx, idx + per, 0, 0))
            idx += per
    return out


def subinterval_events(events, r):
    """The events (x, y, ts) of one sub-interval range (begin0, end0, begin1, end1) of subinterval_ranges."""
    b0, e0, b1, e1 = r
    if e1 > b1:
        return tuple(np.concatenate([a[b0:e0], a[b1:e1]]) for a in events)
    return tuple(a[b0:e0] for a in events)


def alg2_plan(num_subintervals, n_events, nx, camera_time=True):
    """'fused' (the DSI-less kernel) or 'materialize' (process_2 and the arg-max of its DSIs) for one window: the engine's
    planner (engine.alg2_plan, dsi_alg2_plan), the one dsi::full_sequence_depth_maps_alg2 uses too."""
    return E.alg2_plan(num_subintervals, n_events, nx, camera_time)


def process_2(ctx, cams, dsi_shape, events, trajectories, num_subintervals, mapper_fused,
              mapper_fused_camera_time, ts, stereo_fusion, temporal_fusion, luts=(None, None),
              inverse_depth=False, shuffle_right=False, lenses=(None, None)):
    """Alg. 2: per sub-interval camera fusion, then temporal fusion; and the converse order
    (process2.cpp:46-289).  shuffle_right=True is process_5.  Returns dict with the left / right
    temporal DSIs (Grid3D).  lenses: one engine.Lens (or None) per camera instead of its table in luts."""
    mapper0 = E.MapperEMVS(ctx, cams[0], dsi_shape, lut=luts[0], inverse_depth=inverse_depth, lens=lenses[0])
    mapper1 = E.MapperEMVS(ctx, cams[1], dsi_shape, lut=luts[1], inverse_depth=inverse_depth, lens=lenses[1])
    dims = mapper0.dsi_.getDimensions()
    sub = E.Grid3D(ctx, *dims)     # mapper_fused_subinterval.dsi_
    left = E.Grid3D(ctx, *dims)    # mapper_fused_left.dsi_
    right = E.Grid3D(ctx, *dims)   # mapper_fused_right.dsi_
    T_rv_w = reference_view_process2(trajectories[0], ts)
    per = [int(events[c][0].shape[0]) // int(num_subintervals) for c in range(2)]   # :46-47
    mapper_fused.dsi_.resetGrid()                                                    # :90
    right_sel = shuffled_subintervals(events[1][0].shape[0], num_subintervals) if shuffle_right else None
    for k in range(num_subintervals):
        for c, m in ((0, mapper0), (1, mapper1)):
            sl = slice(k * per[c], (k + 1) * per[c])                                 # :105-107, :132-134
            if c == 1 and right_sel is not None:
                sl = right_sel[k]                                                    # process5.cpp:136-150
            m.dsi_.resetGrid()
            m.evaluateDSI(tuple(a[sl] for a in events[c]), trajectories[c], T_rv_w)  # :119, :146
        sub.resetGrid()                                                              # :159
        sub.addTwoGrids(mapper0.dsi_)                                                # :160
        _fuse_cameras(sub, mapper1.dsi_, stereo_fusion)                              # :168-189
        if temporal_fusion == 2:                                                     # :216-226
            left.addInverseOfTwoGrids(mapper0.dsi_)
            right.addInverseOfTwoGrids(mapper1.dsi_)
            mapper_fused.dsi_.addInverseOfTwoGrids(sub)
            if k == num_subintervals - 1:
                for g in (left, right, mapper_fused.dsi_):
                    g.computeHMfromSumOfInv(num_subintervals)
        elif temporal_fusion == 4:                                                   # :229-239
            left.addTwoGrids(mapper0.dsi_)
            right.addTwoGrids(mapper1.dsi_)
            mapper_fused.dsi_.addTwoGrids(sub)
            if k == num_subintervals - 1:
                for g in (left, right, mapper_fused.dsi_):
                    g.computeAMfromSum(num_subintervals)
        # temporal_fusion 1, 3, 5, 6: nothing happens (:213, :227, :240-243)
    # converse order: time first, cameras second (:266-289).  NOTE the reference swaps cases 3
    # and 4 here (3 -> arithmetic, 4 -> geometric, process2.cpp:274-279); kept as is.
    mapper_fused_camera_time.dsi_.addTwoGrids(left)                                  # :266
    converse = {1: 1, 2: 2, 3: 4, 4: 3, 5: 5, 6: 6}
    if stereo_fusion not in converse:
        raise E.DsiError(E.ERR_BAD_OP, "Improper stereo fusion method selected")
    mapper_fused_camera_time.dsi_.fuseTwoGrids(right, converse[stereo_fusion])
    mapper0.close()
    mapper1.close()
    sub.close()
    return {"left": left, "right": right, "T_rv_w": T_rv_w}


def exact_depth_map_process_2(ctx, cams, dsi_shape, events, trajectories, num_subintervals, mapper_fused, ts,
                              stereo_fusion, temporal_fusion, luts=(None, None), inverse_depth=False, rel_gap=0.0, prove=False,
                              lenses=(None, None)):
    """Alg. 2's fused DSI (camera fusion per sub-interval, then temporal fusion; process2.cpp:98-249) and its arg-max
    with the plane index map EQUAL TO THE CPU REFERENCE'S ON EVERY PIXEL (BASELINE configs[3]).  The engine's exact
    vote sums and the reference's fp32, event-ordered sums agree to ~1e-5, so the first-maximum plane can differ in
    near-tie columns; dsi_mapper_resolve_near_ties covers Alg. 1's topology (one camera fusion), this is the same idea
    built from its public pieces for the camera-then-time topology:
      1. Alg. 2 on the device as process_2 does it, every sub-interval's event batches kept;
      2. near-tie columns of the FINAL fused DSI (Grid3D near-tie voxels);
      3. those voxels of every (sub-interval, camera) DSI re-summed in the reference's order (MapperEMVS.exactVoxels);
      4. the reference's scalar ops on the host (engine.reference_fuse2 / _accumulate / _finalize) in process_2's
         order, the first maximum per column (cartesian3dgrid.cpp:132-134), and the few pixels patched.
    mapper_fused.dsi_ holds the fused DSI afterwards, mapper_fused's depth map (fetchDepthMap) the resolved arg-max.
    temporal_fusion 2 (harmonic) or 4 (arithmetic), like the reference (anything else leaves the fused DSI zero).
    Returns the statistics of the resolution.
    prove=True (ABI 10): the premise of that resolution as a per-column PROOF, for this topology built from INTERVAL GRIDS --
    every (sub-interval, camera) DSI's votes counted and its reference value bounded (MapperEMVS.referenceInterval), the bounds
    carried through the same camera fusion / temporal accumulate / finalize as the values (each widened by its roundings;
    the harmonic accumulation's inverse sums with the directions swapped), MapperEMVS.proveColumns at the end; columns the
    bounds do not settle are re-summed on all their planes (at most 4,096).  info["proof"] holds the statistics:
    columns_unproven == columns_resolved_fully means the index map is the reference's on every pixel by proof.
    lenses: one engine.Lens (or None) per camera instead of its table in luts, as in process_2."""
    mappers = [E.MapperEMVS(ctx, cams[c], dsi_shape, lut=luts[c], inverse_depth=inverse_depth, lens=lenses[c]) for c in range(2)]
    dims = mappers[0].dsi_.getDimensions()
    sub = E.Grid3D(ctx, *dims)
    iv = None
    if prove and {2: E.ACC_INV_SUM, 4: E.ACC_SUM}.get(int(temporal_fusion)) is not None:
        iv = {k: E.Grid3D(ctx, *dims) for k in ("lo0", "hi0", "lo1", "hi1", "acc_lo", "acc_hi")}
        iv["acc_lo"].resetGrid()
        iv["acc_hi"].resetGrid()
    T_rv_w = reference_view_process2(trajectories[0], ts)
    per = [int(events[c][0].shape[0]) // int(num_subintervals) for c in range(2)]
    mode = {2: E.ACC_INV_SUM, 4: E.ACC_SUM}.get(int(temporal_fusion))
    mapper_fused.dsi_.resetGrid()
    batches = []
    for k in range(num_subintervals):
        pair = []
        for c in range(2):
            ev = tuple(a[k * per[c]:(k + 1) * per[c]] for a in events[c])
            pk = E.packetize(ev[2], trajectories[c], T_rv_w)
            first, Rt = pk if pk is not None else (np.zeros(0, np.uint32), np.zeros((0, 12), np.float32))
            b = E.EventBatch(ctx, ev[0], ev[1], Rt, first)
            if pk is None:
                mappers[c].dsi_.resetGrid()          # evaluateDSI returns false: the DSI keeps its reset state
            else:
                mappers[c].evaluateDSI_batch(b)
            pair.append(b)
        batches.append(pair)
        sub.resetGrid()
        sub.addTwoGrids(mappers[0].dsi_)
        _fuse_cameras(sub, mappers[1].dsi_, stereo_fusion)
        if mode is not None:
            mapper_fused.dsi_.accumulate(sub, mode)
            if k == num_subintervals - 1:
                mapper_fused.dsi_.finalize(mode, num_subintervals)
        if iv is not None:
            # the sub-interval's bounds: per camera from the counted votes, through the camera fusion (<= 5 roundings), into
            # the temporal accumulators (3 roundings per step).  The harmonic accumulator holds a SUM OF INVERSES, which falls
            # where the values rise: the lower values' accumulator bounds that sum from ABOVE, so it is widened upwards
            for c in range(2):
                if pair[c].n_packets:
                    mapper_fused.referenceInterval(mappers[c], pair[c], iv["lo%d" % c], iv["hi%d" % c])
                else:
                    iv["lo%d" % c].resetGrid()
                    iv["hi%d" % c].resetGrid()
            _fuse_cameras(iv["lo0"], iv["lo1"], stereo_fusion)       # (in place: lo0 <- op(lo0, lo1), like sub above)
            _fuse_cameras(iv["hi0"], iv["hi1"], stereo_fusion)
            E.widen_interval(iv["lo0"], iv["hi0"], 8)
            iv["acc_lo"].accumulate(iv["lo0"], mode)
            iv["acc_hi"].accumulate(iv["hi0"], mode)
            if mode == E.ACC_INV_SUM:
                E.widen_interval(iv["acc_hi"], iv["acc_lo"], 4)      # (swapped: see above)
            else:
                E.widen_interval(iv["acc_lo"], iv["acc_hi"], 4)
            if k == num_subintervals - 1:
                iv["acc_lo"].finalize(mode, num_subintervals)
                iv["acc_hi"].finalize(mode, num_subintervals)
                E.widen_interval(iv["acc_lo"], iv["acc_hi"], 4)
    mapper_fused.computeDepthMap()
    info = {"near_tie_pixels": 0, "candidate_voxels": 0, "votes": 0, "changed_pixels": 0, "max_order_diff": 0.0}
    if mode is not None:
        vox, cols = mapper_fused.nearTieVoxels(rel_gap=rel_gap)
        info["near_tie_pixels"], info["candidate_voxels"] = int(cols), int(vox.size)
        if vox.size:
            acc = np.zeros(vox.shape, np.float32)
            for k in range(num_subintervals):
                vals = []
                for c in range(2):
                    v, n = mappers[c].exactVoxels(batches[k][c], vox)
                    info["votes"] += int(n.sum())
                    vals.append(v)
                acc = E.reference_accumulate(mode, acc, E.reference_fuse2(stereo_fusion, vals[0], vals[1]))
            final = E.reference_finalize(mode, acc, num_subintervals)
            nx, ny, nz = dims
            pix, new_idx, new_conf = _first_maxima(vox, final, nx * ny)
            _, conf0, idx0 = mapper_fused.fetchDepthMap()
            info["changed_pixels"] = int((idx0.reshape(-1)[pix] != new_idx).sum())
            fused_now = mapper_fused.dsi_.download().reshape(-1)[vox]
            info["max_order_diff"] = float(np.max(np.abs(fused_now.astype(np.float64) - final) /
                                                  np.maximum(1.0, np.abs(final))))
            mapper_fused.patchDepthMap(pix, new_idx, new_conf)
    if iv is not None:
        proof = mapper_fused.proveColumns(mapper_fused.dsi_, iv["acc_lo"], iv["acc_hi"], rel_gap=rel_gap)
        if 0 < proof["columns_unproven"] <= 4096:
            # the columns the bounds do not settle: ALL their planes re-summed, in process_2's order, on the host
            pixels = np.unique(mapper_fused.proofUnproven()[0])
            nx, ny, nz = dims
            vox = (pixels[:, None].astype(np.uint64) + np.arange(nz, dtype=np.uint64)[None, :] * (nx * ny)).reshape(-1).astype(np.uint32)
            acc = np.zeros(vox.shape, np.float32)
            for k in range(num_subintervals):
                vals = [mappers[c].exactVoxels(batches[k][c], vox)[0] for c in range(2)]
                acc = E.reference_accumulate(mode, acc, E.reference_fuse2(stereo_fusion, vals[0], vals[1]))
            final = E.reference_finalize(mode, acc, num_subintervals)
            pix, new_idx, new_conf = _first_maxima(vox, final, nx * ny)
            mapper_fused.patchDepthMap(pix, new_idx, new_conf)
            proof["columns_resolved_fully"] = int(pixels.size)
        info["proof"] = proof
        for g in iv.values():
            g.close()
    for pair in batches:
        for b in pair:
            b.close()
    for o in mappers + [sub]:
        o.close()
    return info


def fuseDSIs_HarmonicMeanOfLocalFocus(mapper0, mapper1, cam0, cam1, dsi_shape, focus_method, mapper_focus_fused):
    """utils.cpp:155-181: the harmonic mean of the two DSIs' local focus volumes (computeLocalFocusInPlace;
    focus_method 0 the local standard deviation, 1 the local mean square) into mapper_focus_fused.dsi_.  The
    reference builds two scratch mappers from cam0 / cam1 / dsi_shape; here two scratch grids of the fused
    mapper's context hold the focus volumes, and mapper0 / mapper1 are left unchanged."""
    shape = mapper0.dsi_.getDimensions()
    ctx = mapper_focus_fused.ctx
    focus = [E.Grid3D(ctx, *shape), E.Grid3D(ctx, *shape)]
    try:
        focus[0].setToLocalFocusOf(mapper0.dsi_, focus_method)   # resetGrid; addTwoGrids; computeLocalFocusInPlace
        focus[1].setToLocalFocusOf(mapper1.dsi_, focus_method)
        mapper_focus_fused.dsi_.setToFusionOf(focus[0], focus[1], E.FUSE_HM)
    finally:
        for g in focus:
            g.close()   # (waits for the context's stream)


def process_5(*args, **kw):
    """process5.cpp:28-260: process_2 with the right camera's sub-intervals circularly shifted."""
    kw["shuffle_right"] = True
    return process_2(*args, **kw)


def process_1_nary(mappers, events, trajectories, mapper_fused, ts, mode, rv_pos=0.0):
    """Alg. 1 for n >= 2 cameras with an n-ary mean across ALL cameras (BASELINE configs[4]: 4-camera
    rig, geometric mean).  The reference's process_1 fuses two cameras and, for GM / AM / RMS,
    silently drops a third one (process1.cpp:169-191); this is the n-ary form of the same ops
    (engine.ACC_SUM arithmetic, ACC_LOG_SUM geometric, ACC_SQ_SUM rms, ACC_MIN, ACC_MAX;
    include/dsi_engine.h dsi_acc_mode_t).  Returns T_rv_w; the fused DSI is mapper_fused.dsi_."""
    T_rv_w = reference_view_process1(trajectories[0], ts, rv_pos)
    for m, ev, tr in zip(mappers, events, trajectories):
        m.evaluateDSI(ev, tr, T_rv_w)
    mapper_fused.dsi_.setToFusionOfN([m.dsi_ for m in mappers], mode)
    return T_rv_w


def _first_maxima(vox, values, npix):
    """Per column of the (pixel-major, planes ascending) voxel list: pixel, first-maximum plane, its value."""
    pix_of = vox % npix
    z_of = (vox // npix).astype(np.int64)
    starts = np.flatnonzero(np.r_[True, pix_of[1:] != pix_of[:-1]])
    ends = np.r_[starts[1:], vox.size]
    j = np.array([a + int(np.argmax(values[a:b])) for a, b in zip(starts, ends)], np.int64)   # argmax: the first maximum
    return pix_of[starts].astype(np.uint32), z_of[j].astype(np.uint8), values[j].astype(np.float32)


def resolve_columns_fully(mapper_fused, mappers, batches, fusion_method, pixels):
    """ALL planes of the listed columns (pixels y * dimX + x) re-summed per camera in the reference's order
    (MapperEMVS.exactVoxels), fused with the reference's scalar op (engine.reference_fuse2; one camera: as they are), the first
    maximum taken (cartesian3dgrid.cpp:132-134) and the depth map of mapper_fused patched: these columns are then the
    reference's by construction, whatever their values.  For the FEW columns a proof cannot settle -- it costs
    planes x columns voxels.  Returns the number of pixels whose plane changed."""
    pixels = np.unique(np.asarray(pixels, np.uint32))
    if not pixels.size:
        return 0
    nx, ny, nz = mapper_fused.dsi_.getDimensions()
    npix = nx * ny
    vox = (pixels[:, None].astype(np.uint64) + np.arange(nz, dtype=np.uint64)[None, :] * npix).reshape(-1).astype(np.uint32)
    vals = [m.exactVoxels(b, vox)[0] for m, b in zip(mappers, batches)]   # (pixel-major, planes ascending)
    final = vals[0] if len(mappers) == 1 else E.reference_fuse2(fusion_method, vals[0], vals[1])
    pix, new_idx, new_conf = _first_maxima(vox, final, npix)
    idx0 = mapper_fused.fetchDepthMap()[2].reshape(-1)[pix]
    mapper_fused.patchDepthMap(pix, new_idx, new_conf)
    return int((idx0 != new_idx).sum())


def resolve_near_ties_proven(mapper_fused, mappers, batches, fusion_method=E.FUSE_HM, rel_gap=0.0, max_gap=4e-3,
                             max_full_columns=4096):
    """MapperEMVS.resolveNearTies in PROVEN mode (ABI 10): resolve, then MapperEMVS.proveNearTies -- every voxel's votes counted,
    the reference's fp32 event-order sums bounded from the counts.  Columns whose bounds reach beyond the gap: if a gap of at
    most `max_gap` covers some of them the resolver runs again with it (and the proof again); the columns that remain -- maxima
    made of a handful of tiny weights, where the engine's 2^-31 weight grid is as coarse as the values -- are re-summed on ALL
    their planes (resolve_columns_fully; at most `max_full_columns`, else they stay unproven).  Returns (resolver info, proof
    info); proof["columns_unproven"] - proof["columns_resolved_fully"] == 0 means the index map is the reference's on every
    pixel by proof.  The proof passes are verification passes (global-atomic vote counts): not for a timed loop."""
    info = mapper_fused.resolveNearTies(mappers, batches, fusion_method, rel_gap=rel_gap)
    proof = mapper_fused.proveNearTies(mappers, batches, fusion_method, rel_gap=info["rel_gap"])
    if proof["columns_unproven"]:
        pix, gaps = mapper_fused.proofUnproven()
        moderate = gaps[gaps.astype(np.float64) * 1.05 <= max_gap]
        if moderate.size:
            info = mapper_fused.resolveNearTies(mappers, batches, fusion_method, rel_gap=float(moderate.max()) * 1.05)
            proof = mapper_fused.proveNearTies(mappers, batches, fusion_method, rel_gap=info["rel_gap"])
            pix = mapper_fused.proofUnproven()[0] if proof["columns_unproven"] else pix[:0]
        if pix.size and pix.size <= max_full_columns:
            resolve_columns_fully(mapper_fused, mappers, batches, fusion_method, pix)
            proof["columns_resolved_fully"] = int(pix.size)
    return info, proof


def _fuse_nary_host(vals, mode):
    """The n-ary camera fusion of reference-order values on the host, with the reference's scalar ops (bit for bit what
    setToFusionOfN computes on the device)."""
    n = len(vals)
    if mode == E.ACC_GM_TREE:
        if n not in (2, 4, 8):
            raise E.DsiError(E.ERR_BAD_OP, "ACC_GM_TREE needs 2, 4 or 8 cameras")
        level = vals
        while len(level) > 1:       # geometricMeanTwoGrids on pairs, then on the results (cartesian3dgrid.h:150-156)
            level = [E.reference_fuse2(E.FUSE_GM, level[i], level[i + 1]) for i in range(0, len(level), 2)]
        return level[0]
    if mode in (E.ACC_MIN, E.ACC_MAX):
        final = vals[0]
        for v in vals[1:]:
            final = E.reference_fuse2(E.FUSE_MIN if mode == E.ACC_MIN else E.FUSE_MAX, final, v)
        return final
    if mode == E.ACC_SUM:
        acc = np.zeros(vals[0].shape, np.float32)
        for v in vals:
            acc = E.reference_accumulate(E.ACC_SUM, acc, v)
        return E.reference_finalize(E.ACC_SUM, acc, n)
    raise E.DsiError(E.ERR_BAD_OP, "mode %r has no host restatement" % (mode,))


def exact_depth_map_nary_proven(mapper_fused, mappers, batches, mode, rel_gap=0.0, fused_grid=None, max_gap=4e-3,
                                max_full_columns=4096):
    """exact_depth_map_nary in PROVEN mode (ABI 10, dsi_mapper_prove_near_ties_n): resolve, prove from counted votes, once
    more with a moderately wider gap where the bounds ask for it, and the columns no such gap settles re-summed on all their
    planes.  At BASELINE configs[4]'s size the oracle covers a strip of the image; this covers every column.  Returns
    (resolver info, proof info): proof["columns_unproven"] == proof["columns_resolved_fully"] means every column is settled."""
    gap = rel_gap if rel_gap > 0 else 2.5e-4
    info = exact_depth_map_nary(mapper_fused, mappers, batches, mode, rel_gap=gap, fused_grid=fused_grid)
    proof = mapper_fused.proveNearTiesN(mappers, batches, mode, fused_grid=fused_grid, rel_gap=gap)
    if proof["columns_unproven"]:
        pix, gaps = mapper_fused.proofUnproven()
        moderate = gaps[gaps.astype(np.float64) * 1.05 <= max_gap]
        if moderate.size:
            gap = float(moderate.max()) * 1.05
            info = exact_depth_map_nary(mapper_fused, mappers, batches, mode, rel_gap=gap, fused_grid=fused_grid)
            proof = mapper_fused.proveNearTiesN(mappers, batches, mode, fused_grid=fused_grid, rel_gap=gap)
            pix = mapper_fused.proofUnproven()[0] if proof["columns_unproven"] else pix[:0]
        if pix.size and pix.size <= max_full_columns:
            pixels = np.unique(pix)
            nx, ny, nz = mapper_fused.dsi_.getDimensions()
            npix = nx * ny
            vox = (pixels[:, None].astype(np.uint64) + np.arange(nz, dtype=np.uint64)[None, :] * npix).reshape(-1).astype(np.uint32)
            final = _fuse_nary_host([m.exactVoxels(b, vox)[0] for m, b in zip(mappers, batches)], mode)
            p2, new_idx, new_conf = _first_maxima(vox, final, npix)
            mapper_fused.patchDepthMap(p2, new_idx, new_conf)
            proof["columns_resolved_fully"] = int(pixels.size)
    info["rel_gap"] = gap
    return info, proof


def exact_depth_map_nary(mapper_fused, mappers, batches, mode, rel_gap=0.0, fused_grid=None):
    """The n-camera counterpart of MapperEMVS.resolveNearTies (BASELINE configs[4]): mapper_fused.dsi_ holds
    setToFusionOfN([m.dsi_ for m in mappers], mode) of the DSIs the mappers built from `batches`, and mapper_fused
    the depth map of it; the near-tie columns' voxels are re-summed per camera in the reference's order, fused on the
    host with the reference's scalar ops and the first maximum re-picked.  mode: ACC_GM_TREE (the balanced tree of the
    reference's 2-ary sqrt(a*b); n = 2, 4, 8), ACC_MIN, ACC_MAX, ACC_SUM (arithmetic mean).  fused_grid: the grid that
    holds the fusion when it is not mapper_fused.dsi_.  Returns statistics."""
    n = len(mappers)
    nx, ny, nz = mapper_fused.dsi_.getDimensions()
    vox, cols = mapper_fused.nearTieVoxels(grid=fused_grid, rel_gap=rel_gap)
    info = {"near_tie_pixels": int(cols), "candidate_voxels": int(vox.size), "votes": 0, "changed_pixels": 0}
    if not vox.size:
        return info
    vals = []
    for m, b in zip(mappers, batches):
        v, cnt = m.exactVoxels(b, vox)
        info["votes"] += int(cnt.sum())
        vals.append(v)
    final = _fuse_nary_host(vals, mode)
    pix, new_idx, new_conf = _first_maxima(vox, final, nx * ny)
    _, _, idx0 = mapper_fused.fetchDepthMap()
    info["changed_pixels"] = int((idx0.reshape(-1)[pix] != new_idx).sum())
    mapper_fused.patchDepthMap(pix, new_idx, new_conf)
    return info


def window_bounds(start_time_s, stop_time_s, duration, out_skip):
    """The intervals of main.cpp:177: for (t = start; t + duration <= stop; t += out_skip)."""
    out = []
    t = float(start_time_s)
    while t + duration <= stop_time_s:
        out.append((t, t + duration))
        t += out_skip
    return out


def window_events(events, t_start, t_stop):
    """Events of one camera with t_start <= ts <= t_stop, on an already time-sorted array.
    NOT identical to parse_rosbag (data_loading.cpp:272-285) on a real bag: the reference tests its stop flag only
    at the NEXT EventArray message, so it also keeps the first event past t_stop and the rest of that message
    (a few hundred events; the 1024-event packetisation can shift by one packet).  Message boundaries do not
    exist in an event array; io.read_event_bag reproduces the message-granular cut when reading a bag."""
    x, y, ts = events
    a = int(np.searchsorted(ts, t_start, side="left"))
    b = int(np.searchsorted(ts, t_stop, side="right"))
    return x[a:b], y[a:b], ts[a:b]


class WindowStream:
    """The --full_seq loop of main.cpp:174-302 with process_method 1 as a STREAM: per window
    packetise on the host, upload both cameras' events (pooled device blocks on the copy stream, so
    window w+1's upload overlaps window w's voting), evaluateDSI x2 (reset + vote), camera fusion,
    arg-max + depth; the depth map of window w is fetched while window w+1 is already queued
    (`depth` fused grids / extraction mappers alternate).  The reference constructs fresh mappers per
    window (main.cpp:262-275); here they are reused -- evaluateDSI resets the DSI anyway (:145)."""

    def __init__(self, ctx, cams, dsi_shape, fusion_method=E.FUSE_HM, luts=(None, None),
                 inverse_depth=False, depth=2, materialize_fused=True, fused_vote=False, concurrent=False,
                 exact_ties=False, process_method=1, num_subintervals=4, temporal_fusion=4, camera_time=None,
                 lenses=(None, None)):
        """materialize_fused=False: the fused DSI (the reference's mapper_fused.dsi_) is not written;
        the camera fusion happens inside the arg-max kernel (same bits, one pass less over the
        volume) -- for streams that only keep the depth maps.
        process_method 2 / 5 (main.cpp:275-299): Alg. 2 per window -- fusion_method is the stereo fusion, num_subintervals /
        temporal_fusion as the reference's flags; camera_time (default: on for 2, off for 5, which saves time_camera only)
        also computes mapper_fused_camera_time's map.  Windows go through the DSI-less kernel
        (MapperEMVS.computeDepthMapOfEventsAlg2) or, where alg2_plan says so, through process_2; fetch() then returns
        (time_camera outputs, camera_time outputs or None), each shaped like a process_method 1 result.
        fused_vote=True (implies materialize_fused=False): not even the camera DSIs are written -- one
        kernel votes, fuses and keeps the running arg-max on the CU (MapperEMVS.computeDepthMapOfEvents;
        the same depth maps bit for bit).
        exact_ties=True: every window's arg-max goes through the exact tie resolver (MapperEMVS.resolveNearTies), so
        that its plane index map equals the CPU reference's on every pixel; it needs the camera DSIs, so it excludes
        fused_vote; the call's statistics (and cost) are in `last_resolve`.
        lenses: one engine.Lens (or None) per camera -- the camera mappers' rectification tables are then made on the
        device from the calibration numbers (MapperEMVS(lens=)) instead of being passed in luts; a camera takes one or
        the other."""
        self.ctx = ctx
        self.process_method = int(process_method)
        if self.process_method not in (1, 2, 5):
            raise ValueError("process_method 1, 2 or 5 (got %r)" % (process_method,))
        self.num_subintervals = int(num_subintervals)
        self.temporal_fusion = int(temporal_fusion)
        self.camera_time = (self.process_method == 2) if camera_time is None else bool(camera_time)
        self.cams, self.dsi_shape, self.luts, self.inverse_depth = cams, dsi_shape, luts, inverse_depth
        self.lenses = lenses
        self.last_plan = None
        if self.process_method != 1:
            if self.num_subintervals < 1:
                raise ValueError("num_subintervals must be >= 1")
            # (the options of the process_method 1 paths have no meaning here: refused rather than ignored)
            if fused_vote or exact_ties or materialize_fused is not True:
                raise ValueError("fused_vote, materialize_fused and exact_ties apply to process_method 1 only")
            materialize_fused = False
        self.exact_ties = bool(exact_ties)
        self.last_resolve = None
        fused_vote = bool(fused_vote) and not self.exact_ties
        self.fused_vote = bool(fused_vote)
        self.materialize_fused = bool(materialize_fused) and not self.fused_vote
        self.fusion_method = int(fusion_method)
        # concurrent=True: every slot owns a context (HIP stream) and its own pair of camera mappers, so that
        # consecutive windows are INDEPENDENT streams of work: the next window's preparation kernels and the
        # first workgroups of its voting kernel run on the CUs the current window's tail has already left
        # (the fused kernel is one persistent workgroup per CU; they finish between 0.5x and 1x its duration).
        # Windows are independent in the reference too (main.cpp:177: fresh mappers per window).
        self.concurrent = bool(concurrent) and depth > 1
        self.contexts = [ctx] + ([E.Context(ctx.device) for _ in range(depth - 1)] if self.concurrent else [])
        self._own_contexts = self.contexts[1:]
        sets = len(self.contexts)
        self.mapper_sets = [[E.MapperEMVS(self.contexts[k], cams[c], dsi_shape, lut=luts[c], inverse_depth=inverse_depth,
                                          lens=lenses[c]) for c in range(2)] for k in range(sets)]
        self.mappers = self.mapper_sets[0]
        dims = self.mappers[0].dsi_.getDimensions()
        self.fused = [E.Grid3D(self.contexts[k % sets], *dims) if self.materialize_fused else None for k in range(depth)]
        self.extract = [E.MapperEMVS(self.contexts[k % sets], cams[0], dsi_shape, inverse_depth=inverse_depth)
                        for k in range(depth)]
        self.extract_ct = [E.MapperEMVS(self.contexts[k % sets], cams[0], dsi_shape, inverse_depth=inverse_depth)
                           for k in range(depth)] if self.process_method != 1 and self.camera_time else []
        self.k = 0
        self.voted = 0
        self.T_rv_w = [None] * depth   # per slot: the reference view of the window submitted into it (7-vector)
        self._pins = {}     # (slot, camera) -> page-locked (Rt, packet_first) staging of asynchronous uploads

    def _staging(self, slot, c, n_packets):
        cur = self._pins.get((slot, c))
        if cur is None or cur[0].a.shape[0] < n_packets:
            if cur is not None:
                for a in cur:
                    a.close()
            cap = max(1024, 2 * n_packets)
            cur = (E.PinnedArray((cap, 12), np.float32), E.PinnedArray((cap,), np.uint32))
            self._pins[(slot, c)] = cur
        return cur

    def submit(self, events, trajectories, ts, rv_pos=0.0, batches=None, asynchronous=False):
        """Queue one window (process1.cpp:54-166 + :222).  events: per camera (x, y, ts) of the
        window; batches: optional pre-uploaded EventBatch per camera (device-resident inputs).
        asynchronous: the x / y arrays live in page-locked memory (engine.PinnedArray) and stay
        unchanged until this window's result has been fetched; the uploads then run as plain DMAs
        and the host does not wait for them.  Returns the slot to pass to fetch()."""
        slot = self.k % len(self.fused)
        ctx = self.contexts[slot % len(self.contexts)]
        mappers = self.mapper_sets[slot % len(self.mapper_sets)]
        if self.process_method != 1:
            if batches is not None or asynchronous or rv_pos != 0.0:
                raise ValueError("batches, asynchronous and rv_pos apply to process_method 1 only (Alg. 2 cuts and packetises "
                                 "its sub-intervals itself; its reference view is the left camera, process2.cpp:79-81)")
            self.T_rv_w[slot] = reference_view_process2(trajectories[0], ts)
            self._submit_alg2(slot, ctx, mappers, events, trajectories, ts)
            self.k += 1
            return slot
        T_rv_w = reference_view_process1(trajectories[0], ts, rv_pos)
        self.T_rv_w[slot] = T_rv_w
        own, fused_batches, all_batches = [], [], []
        for c in range(2):
            if batches is not None:
                b = batches[c]
            else:
                pk = E.packetize(events[c][2], trajectories[c], T_rv_w)
                if pk is None:                      # evaluateDSI returns false: < 1024 events (:71-75)
                    if not self.fused_vote and not self.exact_ties:
                        mappers[c].dsi_.resetGrid()
                        continue
                    pk = (np.zeros(0, np.uint32), np.zeros((0, 12), np.float32))   # a batch without packets
                first, Rt = pk
                if asynchronous:
                    pr, pf = self._staging(slot, c, first.shape[0])
                    pr.a[:Rt.shape[0]] = Rt
                    pf.a[:first.shape[0]] = first
                    Rt, first = pr.a[:Rt.shape[0]], pf.a[:first.shape[0]]
                b = E.EventBatch(ctx, events[c][0], events[c][1], Rt, first, asynchronous=asynchronous)
                own.append(b)
            all_batches.append(b)
            if self.fused_vote:
                fused_batches.append(b)
            elif b.n_packets:
                mappers[c].evaluateDSI_batch(b)
            else:                                   # a batch without packets: evaluateDSI resets the DSI and returns false;
                mappers[c].dsi_.resetGrid()         # the resolver takes the batch as it is -- no votes from this camera
            self.voted += b.n_packets * E.PACKET_SIZE
        if self.fused_vote:
            self.extract[slot].computeDepthMapOfEvents(mappers, fused_batches, self.fusion_method)
        elif self.materialize_fused:
            self.fused[slot].setToFusionOf(mappers[0].dsi_, mappers[1].dsi_, self.fusion_method)
            self.extract[slot].computeDepthMap(self.fused[slot])
        else:
            self.extract[slot].computeDepthMapOfFusion(mappers[0].dsi_, mappers[1].dsi_,
                                                       self.fusion_method)
        if self.exact_ties:
            self.last_resolve = self.extract[slot].resolveNearTies(mappers, all_batches, self.fusion_method)
        for b in own:
            b.close()                               # the block returns to the pool once its readers are done
        self.k += 1
        return slot

    def _submit_alg2(self, slot, ctx, mappers, events, trajectories, ts):
        """process_2 / process_5 of one window (process2.cpp:28-302) into extract[slot] (time_camera) and
        extract_ct[slot] (camera_time)."""
        n = self.num_subintervals
        out_ct = self.extract_ct[slot] if self.camera_time else None
        self.last_plan = alg2_plan(n, sum(int(events[c][0].shape[0]) for c in range(2)), self.extract[slot].dimX,
                                   self.camera_time)
        if self.last_plan == "materialize":
            # the materialising path: the reference's sequence on the engine's grids, then the arg-max of each DSI
            scratch_ct = out_ct or E.MapperEMVS(ctx, self.cams[0], self.dsi_shape, inverse_depth=self.inverse_depth)
            scratch_ct.dsi_.resetGrid()                 # (a fresh mapper_fused_camera_time per window, main.cpp:262-275)
            res = process_2(ctx, self.cams, self.dsi_shape, events, trajectories, n, self.extract[slot], scratch_ct, ts,
                            self.fusion_method, self.temporal_fusion, luts=self.luts, inverse_depth=self.inverse_depth,
                            shuffle_right=self.process_method == 5, lenses=self.lenses)
            res["left"].close()
            res["right"].close()
            self.extract[slot].computeDepthMap()
            if out_ct is not None:
                out_ct.computeDepthMap()
            else:
                scratch_ct.close()
            self.voted += sum(int(events[c][0].shape[0]) // n * n for c in range(2))
            return
        # (temporal_fusion 1, 3, 5, 6: the engine votes nothing -- every grid stays zero, process2.cpp:240-243)
        batches = alg2_window_batches(ctx, events, trajectories, ts, n, self.process_method)
        try:
            self.extract[slot].computeDepthMapOfEventsAlg2(out_ct, mappers, batches, n, self.fusion_method,
                                                           self.temporal_fusion)
            self.voted += sum(b.n_packets for b in batches) * E.PACKET_SIZE
        finally:
            for b in batches:
                b.close()

    def fetch(self, slot, options_depth_map=None, options_point_cloud=None):
        """(depth, confidence, indices) of the window submitted into `slot` (synchronises).  With
        options_depth_map (OptionsDepthMap): the reference's per-window outputs instead --
        (depth_map, confidence_map, mask) after the adaptive threshold, masked median and border removal
        of getDepthMapFromDSI (main.cpp:281 -> mapper_emvs_stereo.cpp:390-437), whichever way the
        window's arg-max was produced.  With options_point_cloud (OptionsPointCloud; needs options_depth_map) as
        well: (depth_map, confidence_map, mask, points), points the (N, 4) cloud of getPointcloud (main.cpp:396)
        made of the filtered maps still on the device."""
        if options_point_cloud is not None and options_depth_map is None:
            raise ValueError("options_point_cloud needs options_depth_map: the point cloud is made of the filtered maps")
        if self.process_method != 1:
            ct = self.extract_ct[slot] if self.camera_time else None
            return (self._fetch_from(self.extract[slot], options_depth_map, options_point_cloud),
                    None if ct is None else self._fetch_from(ct, options_depth_map, options_point_cloud))
        return self._fetch_from(self.extract[slot], options_depth_map, options_point_cloud)

    def _fetch_from(self, m, options_depth_map, options_point_cloud):
        if options_depth_map is not None:
            out = m.filterDepthMap(options_depth_map)
            if options_point_cloud is not None:
                out = out + (m.getPointcloud(options_pc=options_point_cloud),)
            return out
        # (every slot has its own context when the stream is concurrent: the copies follow the window's kernels on its
        #  compute stream -- one stream per window in flight, plus the device's shared upload stream)
        return m.fetchDepthMap(in_order=self.concurrent)

    def fused_grid(self, slot):
        return self.fused[slot]

    def context_of_slot(self, slot):
        """The context window `slot` runs in (pre-uploaded batches must live there).  Lifetime: with concurrent=True
        the stream OWNS the contexts of slots >= 1 and close() destroys them -- after closing every object still alive
        in them (Context.close() does that: a caller's EventBatch created here is closed with the stream; closing it
        again later is a no-op).  At the C level dsi_context_destroy refuses while children are alive."""
        return self.contexts[slot % len(self.contexts)]

    def close(self):
        for o in ([m for ms in self.mapper_sets for m in ms] + [f for f in self.fused if f is not None] + self.extract +
                  self.extract_ct):
            o.close()
        for c in self._own_contexts:
            c.close()
        self._own_contexts = []
        for pair in self._pins.values():
            for a in pair:
                a.close()
        self._pins = {}


def _prune_world_map(opts, local_box, T_rv_w):
    """The options of one prune of a streamed map: opts as WorldMap.prune takes them; with local_box the box around the
    window's reference position, the translation of engine.invert_pose(T_rv_w) -- the T_w_rv the window's cloud was
    integrated with."""
    if local_box is None:
        return opts
    t = E.invert_pose(T_rv_w)[[3, 7, 11]]
    return dict(opts, box=(t - local_box, t + local_box))


def _pop_local_box(opts):
    """world_map_prune's local_box, taken out of opts before its keys are checked: the half extents as three doubles"""
    local_box = opts.pop("local_box", None)
    if local_box is not None:
        if opts.get("box") is not None:
            raise ValueError("world_map_prune takes box or local_box, not both")
        local_box = np.asarray(local_box, np.float64).reshape(3)
    return local_box


def _check_keep(opts):
    if E.shape_mask(opts.get("keep", ("linear", "planar"))) not in range(1, 8):
        raise ValueError("world_map_shapes['keep'] must name at least one of linear, planar and scattered")


def _pop_views(opts):
    """world_map_carve's `views`, taken out of opts before its keys are checked: the ring of the last windows' views"""
    if "views" not in opts:
        raise ValueError("world_map_carve needs views")
    views = opts.pop("views")
    if isinstance(views, bool) or int(views) != views or views < 1:
        raise ValueError("world_map_carve['views'] must be an integer >= 1")
    return {"ring": collections.deque(maxlen=int(views)), "camera": None}


def _check_carve(opts):
    """the bounds of dsi_map_visibility.h, before the stream starts"""
    window, min_through, agree_weight = opts.get("window", 1), opts.get("min_through", 2), opts.get("agree_weight", 1)
    if isinstance(window, bool) or int(window) != window or not 0 <= window <= 3:
        raise ValueError("world_map_carve['window'] must be an integer in 0..3")
    for k in ("abs_tol", "rel_tol"):
        if not (np.isfinite(opts.get(k, 0.0)) and opts.get(k, 0.0) >= 0.0):
            raise ValueError("world_map_carve[%r] must be finite and >= 0" % k)
    if int(min_through) != min_through or not 1 <= min_through <= 0xffffffff:
        raise ValueError("world_map_carve['min_through'] must be an integer >= 1")
    if int(agree_weight) != agree_weight or not 0 <= agree_weight <= 0xffffffff:
        raise ValueError("world_map_carve['agree_weight'] must be an integer >= 0")


def _collect_view(state, maps, T_rv_w, mapper):
    """world_map_carve's hook on every window: the window's filtered depth map and mask -- the host arrays the stream yields
    -- and its T_rv_w join the ring; the camera is the mapper's virtual one, the depth range that of its planes"""
    state["ring"].append((maps[0], maps[2], np.array(E.pose_matrix(T_rv_w))))
    state["camera"] = (mapper.virtual_cam_, float(mapper.raw_depths_vec_.min()), float(mapper.raw_depths_vec_.max()))


def _observe_ring(world_map, state, **observe_opts):
    """world_map_carve's pass: the tally cleared, then every view of the ring; the last one's counts"""
    K, min_depth, max_depth = state["camera"]
    return _observe_views(world_map, state["ring"], K, min_depth, max_depth, **observe_opts)


def _observe_views(world_map, views, K, min_depth, max_depth, **observe_opts):
    world_map.clearVisibility()
    counts = None
    for depth, mask, T_v_w in views:
        counts = world_map.observe(depth, mask, K, min_depth, max_depth, T_v_w, **observe_opts)
    if counts is None:
        raise ValueError("no view to carve the map with")
    return counts


def carve_world_map(world_map, views, K, min_depth, max_depth, window=1, abs_tol=0.0, rel_tol=0.0, min_through=2, agree_weight=1,
                    shrink=False):
    """Carves a map by the free space that depth maps saw (engine.WorldMap.observe / pruneCarved; the rule is stated in
    dsi_map_visibility.h and DESIGN.md 7j "Visibility"): the tally is cleared, every view of `views` -- (depth, mask, T_v_w)
    with depth a host depth map (height, width), mask its mask or None and T_v_w the pose world -> view (a window's T_rv_w)
    -- is observed through K = (fx, fy, cx, cy) with the depth range and window, abs_tol, rel_tol, and the cells with
    through >= min_through and through > agree_weight * agree are removed.  Returns the last view's counts and, under
    "prune", those of pruneCarved."""
    counts = _observe_views(world_map, views, K, min_depth, max_depth, window=window, abs_tol=abs_tol, rel_tol=rel_tol)
    counts["prune"] = world_map.pruneCarved(min_through, agree_weight, shrink)
    return counts


# full_sequence's map stages, in the order they run on a window.  name: the keyword, and the key of the element a window's
# result gains; run, run_keys: the WorldMap method of the pass (None: the stage only prunes; a function: called as
# run(world_map, what prepare returned, **keywords)) and the keywords it takes;
# required: those that have no default; prune, prune_keys: the method that removes cells, and its keywords; prepare(opts):
# called before the keys are checked, takes what belongs to neither method out of opts and returns it; check(opts): a last
# look at the values; per_window(prune_opts, what prepare returned, the window's T_rv_w): the prune's keywords for one window;
# collect(what prepare returned, the window's filtered maps, its T_rv_w, its mapper): called on EVERY window, also those
# between two every-th ones.
# A new stage is one more row (and its keyword in full_sequence's signature and docstring).
_MapStage = collections.namedtuple("_MapStage", "name run run_keys required prune prune_keys prepare check per_window collect",
                                   defaults=(None, None, None, None))
_MAP_STAGES = (
    _MapStage("world_map_prune", None, (), (), "prune",
              ("min_points", "min_windows", "max_age", "box", "reach", "min_neighbors", "shrink"), _pop_local_box, None, _prune_world_map),
    _MapStage("world_map_components", "components", ("min_points", "min_windows", "connectivity"), (), "pruneComponents",
              ("min_cells", "min_component_points", "keep_largest", "shrink")),
    _MapStage("world_map_outliers", "knn", ("k", "radius", "min_found", "min_points", "min_windows"), ("k", "radius"), "pruneOutliers",
              ("std_mult", "shrink")),
    _MapStage("world_map_shapes", "pca", ("k", "radius", "min_found", "orient", "viewpoint", "min_points", "min_windows"), ("k", "radius"),
              "pruneShapes", ("keep", "remove_sparse", "shrink"), None, _check_keep),
    _MapStage("world_map_carve", _observe_ring, ("window", "abs_tol", "rel_tol"), (), "pruneCarved", ("min_through", "agree_weight", "shrink"),
              _pop_views, _check_carve, None, _collect_view),
)


def _map_stage_options(stage, opts, world_map):
    """One stage's keyword of full_sequence, checked: (the pass's keywords, the prune's, every, what stage.prepare returned)"""
    if world_map is None:
        raise ValueError("%s needs world_map" % stage.name)
    opts = dict(opts)
    every = opts.pop("every", 1)
    if int(every) != every or every < 1:
        raise ValueError("%s['every'] must be an integer >= 1" % stage.name)
    state = stage.prepare(opts) if stage.prepare else None
    unknown = set(opts) - set(stage.run_keys) - set(stage.prune_keys)
    if unknown:
        raise ValueError("%s: unknown keys %s" % (stage.name, sorted(unknown)))
    if any(k not in opts for k in stage.required):
        raise ValueError("%s needs %s" % (stage.name, " and ".join(stage.required)))
    if stage.check:
        stage.check(opts)
    return ({k: v for k, v in opts.items() if k in stage.run_keys}, {k: v for k, v in opts.items() if k in stage.prune_keys}, int(every),
            state)


def full_sequence(ctx, cams, dsi_shape, events, trajectories, start_time_s, stop_time_s, duration,
                  out_skip, fusion_method=E.FUSE_HM, forward_looking=True, rv_pos=0.0, options_depth_map=None,
                  options_point_cloud=None, polarities=None, save_images=False, out_path=None, lut=None, score=None,
                  ground_truth=None, ground_truth_disparity=None, thicken_edges=False, world_map=None, world_map_prune=None,
                  world_map_components=None, world_map_outliers=None, world_map_shapes=None, world_map_carve=None,
                  **kw):
    """Generator over the windows of main.cpp:177-302: yields (ts, depth, confidence, indices) per
    window, pipelined one window deep; with options_depth_map, (ts, depth_map, confidence_map, mask)
    -- the filtered outputs the reference saves per window; with options_point_cloud as well, the window's
    point cloud (main.cpp:396, an (N, 4) array: WindowStream.fetch) as a fifth element.
    lenses= (a keyword of WindowStream, like luts=): one engine.Lens per camera, the rectification tables made on the device.
    process_method=2 / 5 (keywords of WindowStream: num_subintervals, temporal_fusion, camera_time; fusion_method is the
    stereo fusion): yields (ts, time_camera outputs, camera_time outputs or None), each output element shaped like what
    process_method 1 yields after ts (main.cpp:275-299).
    save_images=True (process_method 1, needs options_depth_map and polarities = one array per camera, aligned with its
    events): each window's result gains a last element, a dict of the pictures the reference writes per window --
    "event_images" (one per camera, accumulateEvents with polarity, main.cpp:245-252; the sensor's size),
    "confidence_negated" and "inv_depth_colored_dilated" (saveDepthMaps, process1.cpp:209-223; B G R, colour table `lut`)
    -- all computed on the device.  The event images go through the host-array form (accumulate_events), before the
    window is submitted as in main.cpp: x and y travel a second time and the slot's stream is synchronised per window, so
    this opt-in path gives up the overlap of consecutive windows; a caller who keeps EventBatch objects uses
    EventBatch.event_image instead, which uploads the polarity bytes only.  out_path and lut are keywords of this path
    alone.  With out_path (a prefix, like --out_path) they are written as well:
    out_path + "%f" % ts + "events_<c>.png" (main.cpp:251) and saveDepthMaps' three files as process1.cpp:121-122, 223 names
    them: prefix out_path + "%013.9f" % ts, suffix "fused_<fusion_method>".
    score= (an engine.DepthScore) with ground_truth= (a callable ts -> ground-truth depth map of the DSI's (dimY, dimX), or
    None for a window without one: nearest_ground_truth picks the frame as the reference's script does): every window's
    filtered depth map and mask -- the host arrays this generator yields anyway, for process_method 2 / 5 those of the
    time_camera output -- are added to the score against that window's ground truth before the window is yielded.  Needs
    options_depth_map.  Nothing more is downloaded for it; the caller reads score.metrics() / score.curves() at the end.
    score= with ground_truth_disparity=(frames_u16, gt_times, projector) instead: the ground truth is made on the device
    from DSEC's disparity images (scripts/evaluate_mcemvs_dsec.py:98-122).  frames_u16: the uint16 samples of the PNGs
    (io.read_png_gray16), a sequence or a callable index -> image; gt_times: their times in the unit and origin of ts;
    projector: an engine.GroundTruthProjector of the score's context and the DSI's (dimY, dimX).  Per window
    nearest_ground_truth picks the frame -- a window whose nearest frame is 0.1 or more away is not scored, as the script
    skips it --, the projector makes its depth map and the score reads it where it lies: 2 bytes per pixel travel.
    thicken_edges=True (this path only): the window's depth map and mask go through engine.thicken_edges first, the
    script's switch of that name (:75-79).
    world_map= (an engine.WorldMap of `ctx`; needs options_depth_map and options_point_cloud): every window's cloud -- the
    one this generator yields, for process_method 2 / 5 the time_camera output's -- is also merged into the map where it
    lies on the device (WorldMap.integrate_mapper) with T_w_rv = engine.invert_pose(the window's T_rv_w), before the
    window is yielded: the reference views differ per window, the map is in the world frame.  What is yielded does not
    change.  The map lives on one context, so concurrent=True (a context per window in flight) is refused.
    world_map_prune= (with world_map=; None leaves the stream as it is): a dict of WorldMap.prune's keywords plus `every`
    (default 1: the map is pruned after every every-th window, right after that window's cloud went in) and optionally
    `local_box` = (hx, hy, hz) instead of `box`: the box is then the window's reference position +- the half extents,
    lo = t - h and hi = t + h in double with t the translation of the T_w_rv the window was integrated with -- a local map
    that forgets what lies behind the vehicle (max_age does the same by calls).  A pruned window's result gains a last
    element, {"world_map_prune": the counts WorldMap.prune returns}.
    world_map_components= (with world_map=; None leaves the stream as it is): a dict of the keywords of WorldMap.components
    (min_points, min_windows, connectivity) and of WorldMap.pruneComponents (min_cells, min_component_points, keep_largest,
    shrink) plus `every` (default 1): after every every-th window, right after that window's cloud went in -- and after
    world_map_prune's prune, when both fall on the window --, the map is labelled and pruned by component.  Such a window's
    result gains a last element, {"world_map_components": the counts of WorldMap.components, and under "prune" those of
    WorldMap.pruneComponents}.
    world_map_outliers= (with world_map=; None leaves the stream as it is): a dict of the keywords of WorldMap.knn (k, radius,
    min_found, min_points, min_windows) and of WorldMap.pruneOutliers (std_mult, shrink) plus `every` (default 1): after
    every every-th window, after world_map_prune's and world_map_components' work on that window, the map queries itself
    and loses its isolated cells and statistical outliers.  Such a window's result gains a last element,
    {"world_map_outliers": the counts of WorldMap.knn, and under "prune" those of WorldMap.pruneOutliers}.
    world_map_shapes= (with world_map=; None leaves the stream as it is): a dict of the keywords of WorldMap.pca (k, radius,
    min_found, orient, viewpoint, min_points, min_windows) and of WorldMap.pruneShapes (keep, remove_sparse, shrink) plus
    `every` (default 1): after every every-th window, after world_map_outliers' work on that window, the map analyses its
    cells' local shape and keeps the labels in keep.  Such a window's result gains a last element, {"world_map_shapes": the
    counts of WorldMap.pca, and under "prune" those of WorldMap.pruneShapes}.
    world_map_carve= (with world_map=; None leaves the stream as it is): a dict of `views` (required: how many of the last
    windows' views are kept), the keywords of WorldMap.observe (window, abs_tol, rel_tol) and of WorldMap.pruneCarved
    (min_through, agree_weight, shrink) plus `every` (default 1).  Every window's filtered depth map, mask and T_rv_w --
    the host arrays this generator yields anyway, for process_method 2 / 5 those of the time_camera output: nothing more
    is downloaded -- join a ring of the last `views` windows.  After every every-th window, after world_map_shapes' work on
    that window, the ring is replayed against the map (carve_world_map: the tally cleared, one observe per view through
    the mapper's virtual camera and the depth range of its planes) and the cells that the views look through are
    removed: a floater of one window is refuted by the windows around it.  Such a window's result gains a last element,
    {"world_map_carve": the counts of the last observe, and under "prune" those of WorldMap.pruneCarved}."""
    given = {"world_map_prune": world_map_prune, "world_map_components": world_map_components,
             "world_map_outliers": world_map_outliers, "world_map_shapes": world_map_shapes, "world_map_carve": world_map_carve}
    checked = {}
    for stage in reversed(_MAP_STAGES):              # the last stage's keyword is checked first: its refusal wins
        if given[stage.name] is not None:
            checked[stage.name] = _map_stage_options(stage, given[stage.name], world_map)
    stages = [(stage, checked[stage.name]) for stage in _MAP_STAGES if stage.name in checked]    # in the order they run
    windows_seen = 0
    if world_map is not None:
        if options_point_cloud is None:
            raise ValueError("world_map needs options_depth_map and options_point_cloud: the map is made of the windows' clouds")
        if kw.get("concurrent"):
            raise ValueError("world_map lives on one context: concurrent=True gives every window in flight its own")
    if ground_truth is not None and ground_truth_disparity is not None:
        raise ValueError("ground_truth and ground_truth_disparity exclude each other")
    if thicken_edges and ground_truth_disparity is None:
        raise ValueError("thicken_edges belongs to ground_truth_disparity")
    if (score is None) != (ground_truth is None and ground_truth_disparity is None):
        raise ValueError("score and ground_truth (or ground_truth_disparity) go together")
    if ground_truth_disparity is not None and len(ground_truth_disparity) != 3:
        raise ValueError("ground_truth_disparity is (frames_u16, gt_times, projector)")
    if score is not None and options_depth_map is None:
        raise ValueError("score needs options_depth_map: the filtered depth maps are what is scored")
    if options_point_cloud is not None and options_depth_map is None:
        raise ValueError("options_point_cloud needs options_depth_map: the point cloud is made of the filtered maps")
    if save_images:
        if options_depth_map is None:
            raise ValueError("save_images needs options_depth_map: saveDepthMaps' images are made of the filtered maps")
        if polarities is None or len(polarities) != 2 or any(p is None for p in polarities):
            raise ValueError("save_images needs polarities: one array per camera")
        if kw.get("process_method", 1) != 1:
            raise ValueError("save_images applies to process_method 1 only")
        for c in range(2):
            if np.shape(polarities[c]) != np.shape(events[c][0]):
                raise ValueError("polarities[%d] must hold one polarity per event of camera %d" % (c, c))
    elif out_path is not None or polarities is not None or lut is not None:
        raise ValueError("polarities, out_path and lut are used by save_images=True only")
    ws = WindowStream(ctx, cams, dsi_shape, fusion_method, **kw)
    pending = None
    images = None
    scoring = None if score is None else (score, ground_truth, ground_truth_disparity, bool(thicken_edges))
    if save_images:
        images = {"fusion_method": int(fusion_method), "min_depth": dsi_shape.min_depth_, "max_depth": dsi_shape.max_depth_, "out_path": out_path,
                  "lut": lut}

    def result(pending):
        nonlocal windows_seen
        out = _window_result(ws, pending, options_depth_map, options_point_cloud, images, scoring, world_map)
        windows_seen += 1
        for stage, (pass_opts, prune_opts, every, state) in stages:
            if stage.collect is not None:
                stage.collect(state, out[1:] if ws.process_method == 1 else out[1], pending[3], ws.extract[pending[1]])
            if windows_seen % every:
                continue
            if stage.per_window is not None:
                prune_opts = stage.per_window(prune_opts, state, pending[3])
            if callable(stage.run):
                counts = stage.run(world_map, state, **pass_opts)
            else:
                counts = getattr(world_map, stage.run)(**pass_opts) if stage.run else None
            pruned = getattr(world_map, stage.prune)(**prune_opts)
            if counts is None:
                counts = pruned
            else:
                counts["prune"] = pruned
            out = out + ({stage.name: counts},)
        return out

    try:
        for t0, t1 in window_bounds(start_time_s, stop_time_s, duration, out_skip):
            ts = t1 if forward_looking else 0.5 * (t0 + t1)          # main.cpp:185-189
            ev = [window_events(events[c], t0, t1) for c in range(2)]
            event_images = None
            if save_images:                                          # main.cpp:245-252, before the window is processed
                event_images = [_window_event_image(ws.context_of_slot(ws.k % len(ws.fused)), events[c], polarities[c], t0, t1,
                                                    cams[0]) for c in range(2)]       # cam0.fullResolution(), :246
            slot = ws.submit(ev, trajectories, ts, rv_pos)
            if pending is not None:
                yield result(pending)
            pending = (ts, slot, event_images, ws.T_rv_w[slot])
        if pending is not None:
            yield result(pending)
    finally:
        ws.close()


def _window_event_image(ctx, events, polarity, t_start, t_stop, cam):
    """accumulateEvents(interval_events, true, event_image) of one camera's window (the slice window_events takes)."""
    x, y, ts = events
    a = int(np.searchsorted(ts, t_start, side="left"))               # window_events' cut
    b = int(np.searchsorted(ts, t_stop, side="right"))
    x, y = x[a:b], y[a:b]
    return E.accumulate_events(ctx, x, y, np.asarray(polarity)[a:b], int(cam[0]), int(cam[1]), True)


def nearest_ground_truth(gt_times, t, max_dt=0.1):
    """evaluate_mcemvs_dsec.py:98-105: the index of the ground-truth frame nearest in time to t (gt_times and t in one
    unit and origin; the first of equally near frames, as argmin), or None when even that one is max_dt or more away --
    the script skips such a window."""
    gt_times = np.asarray(gt_times, np.float64)
    if gt_times.ndim != 1 or gt_times.size == 0:
        return None
    i = int(np.abs(gt_times - float(t)).argmin())
    return None if abs(float(gt_times[i]) - float(t)) >= max_dt else i


def score_world_map(world_map, score, frames, camera, min_depth, max_depth, splat=0, min_points=1, min_windows=1):
    """Map-level metrics of a finished full_sequence(..., world_map=) run: per frame of `frames` -- (T_w_v, gt) with T_w_v
    the camera's pose in the world (as engine.pose_matrix takes it) and gt a host depth map (height, width) or a
    GroundTruthProjector already holding that frame -- the map is rendered into camera = (width, height, fx, fy, cx, cy) at
    engine.invert_pose(T_w_v), without fetching the images, and added to `score` (a DepthScore of the map's context)
    against gt.  Cells farther than max_depth or nearer than min_depth are clipped; splat, min_points, min_windows as
    WorldMap.render takes them.  Returns the list of the frames' count dicts."""
    width, height, fx, fy, cx, cy = camera
    counts = []
    for T_w_v, gt in frames:
        counts.append(world_map.render(E.invert_pose(T_w_v), width, height, fx, fy, cx, cy, min_depth, max_depth, splat=splat,
                                       min_points=min_points, min_windows=min_windows, fetch=False))
        score.addMapRender(world_map, gt)
    return counts


def ground_truth_map(ctx, frames, camera, leaf, min_depth, max_depth, capacity_log2=16):
    """A ground-truth map for score_world_map_3d: an engine.WorldMap of `ctx` with cells of edge `leaf`, holding every frame
    of `frames` -- (gt, T_w_c) with gt a host depth map (height, width) or a GroundTruthProjector already holding that frame
    and T_w_c the camera's pose in the world (as engine.pose_matrix takes it) -- back-projected through
    camera = (width, height, fx, fy, cx, cy), one integrate call per frame.  Pixels without a finite depth in
    [min_depth, max_depth] are left out.  What goes into the map is the caller's choice: nothing is culled."""
    width, height, fx, fy, cx, cy = camera
    gt_map = E.WorldMap(ctx, leaf, capacity_log2)
    for gt, T_w_c in frames:
        if isinstance(gt, E.GroundTruthProjector):
            gt_map.integrateGroundTruth(gt, (fx, fy, cx, cy), min_depth, max_depth, T_w_c)
        else:
            gt = np.asarray(gt, np.float32)
            if gt.shape != (int(height), int(width)):
                raise ValueError("a ground-truth depth map must be (height, width) of the camera")
            gt_map.integrateDepth(gt, None, (fx, fy, cx, cy), min_depth, max_depth, T_w_c)
    return gt_map


def align_world_maps(src, dst, radius, T_init=None, max_iterations=20, min_matched=3, eps_rot=1e-6, eps_trans=None, min_points=1,
                     min_windows=1, min_points_dst=1, min_windows_dst=1):
    """The rigid motion that carries the map `src` onto the map `dst` (engine.WorldMap.align: ICP whose correspondence
    passes run on the device and hand back exact integer moments; the arithmetic is stated in dsi_map_align.h and
    DESIGN.md 7j "Aligning").  radius: how far a cell of src looks for its partner in dst, at most 3 of dst's leaves; T_init:
    a first guess of src's frame in dst's, within that radius of the truth (None: the identity).  Returns (T, info): T the
    12 doubles of src's frame in dst's -- dst.integrateMap(src, T) puts src into dst's frame -- and info the loop's dict."""
    return src.align(dst, radius, T_init, max_iterations, min_matched, eps_rot, eps_trans, min_points, min_windows, min_points_dst,
                     min_windows_dst)


def score_world_map_3d(world_map, gt_map, radius, n_bins=16, min_points=1, min_windows=1, min_points_gt=1, min_windows_gt=1,
                       align=None):
    """3-D accuracy, completeness and F-score of a finished full_sequence(..., world_map=) run against a ground-truth map
    (ground_truth_map): engine.map_f_score of the two maps -- thresholds, precision, recall and f1 per threshold, and the
    two directions' counts (`est`: the map's cells against the ground truth, `gt`: the reverse) with their mean distances.
    align: None scores the maps as they stand; a dict of align_world_maps' options (`radius` defaults to this call's)
    first registers the estimate to the ground truth, as multi-view-stereo benchmarks do -- the estimate's filtered cells
    are re-integrated at the pose found into a scratch map of the estimate's leaf (WorldMap.integrateMap) and that map is
    scored with the filter (1, 1); the result gains "T" (the estimate's frame in the ground truth's) and "align" (the
    loop's info).  world_map itself is not changed."""
    if align is None:
        return E.map_f_score(world_map, gt_map, radius, n_bins, min_points, min_windows, min_points_gt, min_windows_gt)
    opts = dict(align)
    opts.setdefault("radius", radius)
    opts.setdefault("min_points", min_points)
    opts.setdefault("min_windows", min_windows)
    opts.setdefault("min_points_dst", min_points_gt)
    opts.setdefault("min_windows_dst", min_windows_gt)
    T, info = align_world_maps(world_map, gt_map, **opts)
    scratch = E.WorldMap(world_map.ctx, world_map.info()["leaf"])
    try:
        scratch.integrateMap(world_map, T, min_points, min_windows)
        out = E.map_f_score(scratch, gt_map, radius, n_bins, 1, 1, min_points_gt, min_windows_gt)
    finally:
        scratch.close()
    out["T"], out["align"] = T, info
    return out


def merge_world_maps(dst, maps):
    """Appends every map of `maps` to `dst` in the given order (engine.WorldMap.merge; the rule is stated in
    dsi_map_merge.h and DESIGN.md 7j "Merging"): afterwards dst is, bit for bit, the map that had made its own integrate
    calls, then those of maps[0], then those of maps[1] and so on -- for maps that hold consecutive runs of windows, the
    map of the whole run, stamps included.  A map on dst's context is merged on the device; a map of another context
    (another GPU, another process's state read with io.load_world_map and imported there) goes through exportState and
    importState, with the same result.  The sources stay as they are.  Returns the list of the merges' info dicts."""
    infos = []
    for m in maps:
        if m.ctx is dst.ctx:
            infos.append(dst.merge(m))
        else:
            infos.append(dst.importState(m.exportState(sort=False)))
    return infos


def _window_result(ws, pending, options_depth_map, options_point_cloud, images=None, scoring=None, world_map=None):
    out = ws.fetch(pending[1], options_depth_map, options_point_cloud)
    if world_map is not None:       # (the filtered maps of the window are still on the device: fetch left them there)
        world_map.integrate_mapper(ws.extract[pending[1]], E.invert_pose(pending[3]), options_point_cloud)
    if scoring is not None and scoring[1] is not None:
        gt = scoring[1](pending[0])
        if gt is not None:
            maps = out if ws.process_method == 1 else out[0]
            scoring[0].add(maps[0], maps[2], gt)
    elif scoring is not None:
        frames, gt_times, projector = scoring[2]
        i = nearest_ground_truth(gt_times, pending[0])               # evaluate_mcemvs_dsec.py:98-105
        if i is not None:
            maps = out if ws.process_method == 1 else out[0]
            depth, mask = maps[0], maps[2]
            if scoring[3]:
                depth, mask = E.thicken_edges(projector.ctx, depth, mask)
            projector.project_png16(frames(i) if callable(frames) else frames[i])
            scoring[0].addGroundTruth(depth, mask, projector)
    if images is not None:
        from . import io as _io
        ts = pending[0]
        neg, bgr = ws.extract[pending[1]].depthImages(images["min_depth"], images["max_depth"], images["lut"])
        pics = {"event_images": pending[2], "confidence_negated": neg, "inv_depth_colored_dilated": bgr}
        if images["out_path"] is not None:
            for c, img in enumerate(pending[2]):
                _io.write_png_gray8(images["out_path"] + "%f" % ts + "events_%d.png" % c, img)
            _io.save_depth_maps(images["out_path"] + "%013.9f" % ts, "fused_%d" % images["fusion_method"], out[0], out[1], out[2], images["min_depth"],
                                images["max_depth"], images=(neg, bgr))
        out = out + (pics,)
    return (pending[0],) + (out if ws.process_method == 1 else tuple(out))


def alg2_window_batches(ctx, events, trajectories, ts, num_subintervals, process_method=2):
    """The 2 N EventBatch of one Alg. 2 window, k-major (camera 0, camera 1 of sub-interval k): each sub-interval
    packetised on its own against T_rv_w = T_w_l(ts)^-1 (process2.cpp:79-81, :119, :146); one with fewer than 1024
    events becomes a batch without packets (evaluateDSI returns false: its DSI stays zero)."""
    T_rv_w = reference_view_process2(trajectories[0], ts)
    ranges = [subinterval_ranges(events[c][0].shape[0], num_subintervals, process_method, c) for c in range(2)]
    batches = []
    try:
        for k in range(int(num_subintervals)):
            for c in range(2):
                ev = subinterval_events(events[c], ranges[c][k])
                pk = E.packetize(ev[2], trajectories[c], T_rv_w)
                first, Rt = pk if pk is not None else (np.zeros(0, np.uint32), np.zeros((0, 12), np.float32))
                batches.append(E.EventBatch(ctx, ev[0], ev[1], Rt, first))
    except Exception:
        for b in batches:
            b.close()
        raise
    return batches
