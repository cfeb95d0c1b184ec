"""Regenerates tests/golden/dsec_ground_truth.npz.

    python tests/golden/make_dsec_ground_truth.py

For every case the expected depth map is built the way scripts/evaluate_mcemvs_dsec.py:108-122 builds it -- np.where on the
reprojected image, np.r_ for the homogeneous row, np.linalg.inv(T) @ P_homo, K_0 @ P_new, the two in-place divides and the
fancy assignment out_d[px[1].astype(int), px[0].astype(int)] = P_new[2] inside try / except -- with one substitution:
cv2.reprojectImageTo3D (no OpenCV here) is restated as DESIGN.md 7g spells it.  The drop-outside mode, which the script
does not have, is the same code with the points selected by their indices before the assignment.  Then the case is run
through tests/ground_truth_reference.py and must give the same bits; a seed where it does not is rejected (BLAS may round
the matrix products differently from the fixed left-to-right order), and at most one seed in ten may be.

Per case <c> the file holds <c>_raw (uint16 [H][W], the PNG's samples), <c>_d (float32: the script's
disp.astype(np.float32) * 256), <c>_Q, <c>_T (the matrix that is APPLIED, the script's inv(T_rect0_0)), <c>_K, and per mode
m in (script, drop): <c>_<m>_depth, <c>_<m>_counts = (n_points, n_outside).  No test imports the reference: they read this
file."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ground_truth_reference as gr  # noqa: E402

BASELINE = 0.6


def reproject_image_to_3d(d, Q):
    """cv2.reprojectImageTo3D(d, Q) for a float32 image, handleMissingValues off, restated: [x y d 1] times Q in double,
    divided by the fourth component, stored as float32"""
    H, W = d.shape
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dd = d.astype(np.float64)
    with np.errstate(all="ignore"):
        h = [((Q[i, 0] * x + Q[i, 1] * y) + Q[i, 2] * dd) + Q[i, 3] for i in range(4)]
        return np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], axis=2).astype(np.float32)


def as_the_script_does(d, Q, T_rect0_0, K_0, drop_outside=False):
    """lines 108-122; returns (out_d, n_points, n_outside)"""
    h, w = d.shape
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        _3dImage = reproject_image_to_3d(d, Q)
        points = (_3dImage[np.where(_3dImage[:, :, 2] < np.inf)]).T
        P_homo = np.r_[points, np.ones((1, points.shape[1]))]
        P_new = np.linalg.inv(T_rect0_0) @ P_homo
        px = K_0 @ P_new
        px[0, :] /= px[2, :]
        px[1, :] /= px[2, :]
        out_d = np.zeros_like(d)
        finite = np.isfinite(px[0]) & np.isfinite(px[1])
        col, row = np.where(finite, px[0], -4.0 * w).astype(int), np.where(finite, px[1], -4.0 * h).astype(int)
        outside = ~((col >= -w) & (col < w) & (row >= -h) & (row < h))
        if drop_outside:
            ok = (col >= 0) & (col < w) & (row >= 0) & (row < h)
            out_d[row[ok], col[ok]] = P_new[2, ok]
        else:
            try:
                out_d[px[1, :].astype(int), px[0, :].astype(int)] = P_new[2, :]
            except Exception:                                        # 'Depth out of bounds'
                assert outside.any()
            else:
                assert not outside.any()
    return out_d, int(points.shape[1]), int(outside.sum())


def calibration(rng, H, W, focal_scale, centre_shift=(0.0, 0.0), F=None, baseline=BASELINE, tx=0.002, rot=0.01):
    cx, cy = W / 2.0 + rng.uniform(-0.4, 0.4), H / 2.0 + rng.uniform(-0.4, 0.4)
    F = (30.0 + rng.uniform(-1, 1)) if F is None else F
    Q = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, F], [0, 0, 1.0 / baseline, 0]], np.float64)
    a, b, c = rng.uniform(-rot, rot, 3)                          # a small rotation, like R_rect0
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T_rect = np.eye(4)
    T_rect[:3, :3] = Rz @ Ry @ Rx
    T_rect[0, 3] = -tx
    K_0 = np.zeros((3, 4))
    K_0[0, 0] = K_0[1, 1] = focal_scale * F
    K_0[0, 2], K_0[1, 2], K_0[2, 2] = cx + centre_shift[0], cy + centre_shift[1], 1.0
    return Q, T_rect, K_0


def raw_image(rng, H, W, lo=256, hi=20000, p_zero=0.3):
    raw = rng.integers(lo, hi, (H, W)).astype(np.uint16)
    raw[rng.random((H, W)) < p_zero] = 0
    return raw


def make_case(name, seed):
    rng = np.random.default_rng(seed)
    H, W = (29, 37) if name == "odd_size" else (24, 32)
    raw = raw_image(rng, H, W)
    if name in ("near_identity", "odd_size"):
        Q, T_rect, K_0 = calibration(rng, H, W, 0.97)
    elif name == "collisions":
        Q, T_rect, K_0 = calibration(rng, H, W, 0.55)
    elif name == "one_pixel":
        Q, T_rect, K_0 = calibration(rng, H, W, 1e-3)
    elif name == "negative_indices":
        Q, T_rect, K_0 = calibration(rng, H, W, 0.9, centre_shift=(-9.0, -7.0))
    elif name == "one_outside":
        raw = raw_image(rng, H, W, 256, 2000)
        raw[11, 13] = 65535                                          # so near that the translation carries it out of the image
        Q, T_rect, K_0 = calibration(rng, H, W, 0.9, tx=0.1)
    elif name == "overflow_and_negative_z":
        # a negative baseline entry: h_3 = -d / b + q33 < 0 and Z < 0 (kept) for every ordinary disparity; q33 sits just
        # above the smallest disparity's d / b, so that pixel's h_3 is a tiny positive number and Z = F / h_3 = 1.5e43
        # overflows float32 to +inf (dropped, like the zero disparities: F / q33 = 1.5e39)
        Q, T_rect, K_0 = calibration(rng, H, W, 0.97, F=1e37, baseline=-BASELINE, rot=0.0)
        raw[raw > 0] = np.maximum(raw[raw > 0], 4096)
        raw[3, 5] = raw[20, 30] = 1
        Q[3, 3] = 1.0001 * (256.0 / 65535.0) / BASELINE
    elif name == "all_zero":
        raw[:] = 0
        Q, T_rect, K_0 = calibration(rng, H, W, 0.97)
    else:
        raise KeyError(name)
    d = gr.disparity_from_png16(raw)
    T = np.linalg.inv(T_rect)
    out = {"raw": raw, "d": d, "Q": Q, "T": T, "K": K_0}
    agree = True
    for tag, mode in (("script", gr.AS_SCRIPT), ("drop", gr.DROP_OUTSIDE)):
        depth, n_points, n_outside = as_the_script_does(d, Q, T_rect, K_0, drop_outside=(mode == gr.DROP_OUTSIDE))
        rdepth, rn, ro = gr.project(d, Q, T, K_0, mode)
        agree = agree and np.array_equal(depth, rdepth) and (n_points, n_outside) == (rn, ro)
        out[tag + "_depth"], out[tag + "_counts"] = depth, np.array([n_points, n_outside], np.int64)
    return out, agree


def check_case(name, c):
    """each case shows what it is there for"""
    pt = gr.points(c["d"], c["Q"], c["T"], c["K"])
    H, W = c["d"].shape
    keep = pt["kept"] & ~pt["outside"]
    targets = (pt["iv"] % H) * W + (pt["iu"] % W)
    per_target = np.bincount(targets[keep], minlength=H * W)
    n_points, n_outside = (int(v) for v in c["script_counts"])
    negative = keep & ((pt["iu"] < 0) | (pt["iv"] < 0))
    zero_share = float((c["raw"] == 0).mean())
    if name != "all_zero":
        assert 0.2 < zero_share < 0.4 and n_points == int((c["raw"] > (1 if name == "overflow_and_negative_z" else 0)).sum())
    if name in ("near_identity", "odd_size"):
        assert n_outside == 0 and not negative.any() and per_target.max() <= 3 and (per_target == 1).sum() > n_points // 2
    elif name == "collisions":
        assert n_outside == 0 and not negative.any() and per_target.max() > 2 and (per_target > 2).sum() >= 20
    elif name == "one_pixel":
        assert n_outside == 0 and (per_target > 0).sum() == 1 and per_target.max() == n_points
        last = int(np.flatnonzero(pt["kept"])[-1])
        assert c["script_depth"].ravel()[targets[last]] == pt["value"][last]
    elif name == "negative_indices":
        assert n_outside == 0 and negative.sum() >= 20 and (keep & (pt["iu"] < 0)).any() and (keep & (pt["iv"] < 0)).any()
        assert not np.array_equal(c["script_depth"], c["drop_depth"])
    elif name == "one_outside":
        assert n_outside == 1 and not negative.any() and not c["script_depth"].any() and (c["drop_depth"] != 0).sum() > 100
    elif name == "overflow_and_negative_z":
        assert n_outside == 0 and (c["script_depth"] < 0).sum() > 50 and not (c["script_depth"] > 0).any()
        assert not pt["kept"].reshape(H, W)[3, 5] and not pt["kept"].reshape(H, W)[20, 30]
    elif name == "all_zero":
        assert n_points == 0 and n_outside == 0 and not c["script_depth"].any() and not c["drop_depth"].any()
    if name not in ("negative_indices", "one_outside"):
        assert np.array_equal(c["script_depth"], c["drop_depth"])


CASES = ("near_identity", "collisions", "one_pixel", "negative_indices", "one_outside", "overflow_and_negative_z", "all_zero",
         "odd_size")


def main():
    out, tried, rejected = {"cases": np.array(CASES)}, 0, 0
    for k, name in enumerate(CASES):
        seed = 1000 * (k + 1)
        while True:
            c, agree = make_case(name, seed)
            tried += 1
            if agree:
                break
            rejected += 1
            seed += 1
            assert 10 * rejected <= tried + 9, "more than one seed in ten rejected: the restatement is not the script's arithmetic"
        check_case(name, c)
        print("%-26s seed %d: n_points %d, n_outside %d" % ((name, seed) + tuple(int(v) for v in c["script_counts"])))
        for key, val in c.items():
            out["%s_%s" % (name, key)] = val
    assert 10 * rejected <= tried, "%d of %d seeds rejected" % (rejected, tried)
    path = os.path.join(HERE, "dsec_ground_truth.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; %d of %d seeds rejected" % (path, os.path.getsize(path), rejected, tried))


if __name__ == "__main__":
    main()
