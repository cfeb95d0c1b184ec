"""numpy float64 restatement of the lens rectification table (precomputeRectifiedPoints,
mapper_emvs_stereo.cpp:256-299), written from the contract and not from the kernel: vectorised over the pixels, every
product and sum a separate numpy operation evaluated left to right (numpy fuses nothing), the data-dependent exits as
masks.  Also the FORWARD models (undistorted -> raw pixel), which only the tests use to close the loop without the
restatement.  A lens is anything with model (0 plumb_bob, 1 fisheye), K 3 x 3, D, R 3 x 3, P 3 x 4 (engine.Lens)."""
import numpy as np

PLUMB_BOB, FISHEYE = 0, 1
SENTINEL = -1000000.0


def rr_of(R, P):
    """RR = P[:, 0:3] R, entry (i, j) = ((0 + p_i0 r_0j) + p_i1 r_1j) + p_i2 r_2j."""
    R, P = np.asarray(R, np.float64).reshape(3, 3), np.asarray(P, np.float64).reshape(3, 4)
    RR = np.zeros((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            s = np.float64(0.0)
            for k in range(3):
                s = s + P[i, k] * R[k, j]
            RR[i, j] = s
    return RR


def pixel_grid(width, height):
    """(x, y) of entry y * width + x, as float64."""
    idx = np.arange(width * height)
    return (idx % width).astype(np.float64), (idx // width).astype(np.float64)


def plumb_bob_coefficients(D):
    D = np.asarray(D, np.float64).reshape(-1)
    if D.size not in (0, 4, 5, 8):
        raise ValueError("plumb_bob takes 0, 4, 5 or 8 coefficients")
    return np.concatenate([D, np.zeros(8 - D.size)])      # k1 k2 p1 p2 k3 k4 k5 k6


def plumb_bob_undistort(K, D, x, y):
    """The 5 fixed rounds: normalised undistorted (X, Y) of the raw pixels (x, y), and the mask of the pixels that
    left through icdist < 0 (they get (x0, y0))."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3, k4, k5, k6 = plumb_bob_coefficients(D)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ifx, ify = 1.0 / fx, 1.0 / fy
    x0, y0 = (x - cx) * ifx, (y - cy) * ify
    X, Y = x0.copy(), y0.copy()
    active = np.ones(x0.shape, bool)
    negative = np.zeros(x0.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(5):
            r2 = X * X + Y * Y
            icdist = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            neg = active & (icdist < 0.0)
            negative |= neg
            active &= ~neg
            dX = 2.0 * p1 * X * Y + p2 * (r2 + 2.0 * X * X)
            dY = p1 * (r2 + 2.0 * Y * Y) + 2.0 * p2 * X * Y
            Xn = (x0 - dX) * icdist
            Yn = (y0 - dY) * icdist
            X = np.where(active, Xn, np.where(negative, x0, X))
            Y = np.where(active, Yn, np.where(negative, y0, Y))
    return X, Y, negative


def fisheye_undistort(K, D, x, y):
    """Newton on theta_d = theta (1 + k1 theta^2 + ...): (X, Y, ok, info); ok False where the result is the sentinel."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    D = np.asarray(D, np.float64).reshape(-1)
    if D.size != 4:
        raise ValueError("fisheye takes 4 coefficients")
    k1, k2, k3, k4 = D
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    px, py = (x - cx) / fx, (y - cy) / fy
    theta_d_raw = np.sqrt(px * px + py * py)
    theta_d = np.minimum(np.maximum(-np.pi / 2.0, theta_d_raw), np.pi / 2.0)
    theta = theta_d.copy()
    small = ~(np.abs(theta_d) > 1e-8)
    converged = small.copy()
    running = ~small
    with np.errstate(all="ignore"):
        for _ in range(10):
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            a, b, c, d = k1 * t2, k2 * t4, k3 * t6, k4 * t8
            fix = (theta * (1.0 + a + b + c + d) - theta_d) / (1.0 + 3.0 * a + 5.0 * b + 7.0 * c + 9.0 * d)
            theta = np.where(running, theta - fix, theta)
            done = running & (np.abs(fix) < 1e-8)
            converged |= done
            running &= ~done
        scale = np.where(small, 0.0, np.tan(theta) / theta_d)
    flipped = ((theta_d < 0.0) & (theta > 0.0)) | ((theta_d > 0.0) & (theta < 0.0))
    ok = converged & ~flipped
    info = {"small": small, "clamped": theta_d_raw > np.pi / 2.0, "not_converged": ~converged, "flipped": flipped}
    return px * scale, py * scale, ok, info


def rectify_lut(lens, width, height, return_info=False):
    """float32 [height * width, 2]: the table."""
    x, y = pixel_grid(width, height)
    RR = rr_of(lens.R, lens.P)
    with np.errstate(all="ignore"):
        if lens.model == PLUMB_BOB:
            X, Y, negative = plumb_bob_undistort(lens.K, lens.D, x, y)
            xx = RR[0, 0] * X + RR[0, 1] * Y + RR[0, 2]
            yy = RR[1, 0] * X + RR[1, 1] * Y + RR[1, 2]
            ww = 1.0 / (RR[2, 0] * X + RR[2, 1] * Y + RR[2, 2])
            u, v = xx * ww, yy * ww
            info = {"icdist_negative": negative}
        elif lens.model == FISHEYE:
            X, Y, ok, info = fisheye_undistort(lens.K, lens.D, x, y)
            w = RR[2, 0] * X + RR[2, 1] * Y + RR[2, 2]
            u = np.where(ok, (RR[0, 0] * X + RR[0, 1] * Y + RR[0, 2]) / w, SENTINEL)
            v = np.where(ok, (RR[1, 0] * X + RR[1, 1] * Y + RR[1, 2]) / w, SENTINEL)
            info["sentinel"] = ~ok
        else:
            raise ValueError("unknown model")
        lut = np.stack([u, v], axis=1).astype(np.float32)
    return (lut, info) if return_info else lut


# ---- forward models (tests only): normalised undistorted point -> raw pixel ----

def plumb_bob_distort(K, D, X, Y):
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3, k4, k5, k6 = plumb_bob_coefficients(D)
    r2 = X * X + Y * Y
    cdist = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = X * cdist + (2.0 * p1 * X * Y + p2 * (r2 + 2.0 * X * X))
    yd = Y * cdist + (p1 * (r2 + 2.0 * Y * Y) + 2.0 * p2 * X * Y)
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def fisheye_distort(K, D, X, Y):
    """Kannala-Brandt: theta = atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, k3, k4 = np.asarray(D, np.float64).reshape(-1)
    r = np.sqrt(X * X + Y * Y)
    theta = np.arctan(r)
    t2 = theta * theta
    theta_d = theta * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    with np.errstate(all="ignore"):
        s = np.where(r > 1e-300, theta_d / r, 1.0)
    return K[0, 0] * (X * s) + K[0, 2], K[1, 1] * (Y * s) + K[1, 2]


def forward_pixels(lens, lut):
    """Raw pixels of a table made with R = I, P = [K | 0] (entries are then K applied to the undistorted point)."""
    K = np.asarray(lens.K, np.float64).reshape(3, 3)
    lut = np.asarray(lut, np.float64)
    X = (lut[:, 0] - K[0, 2]) / K[0, 0]
    Y = (lut[:, 1] - K[1, 2]) / K[1, 1]
    return (plumb_bob_distort if lens.model == PLUMB_BOB else fisheye_distort)(K, lens.D, X, Y)


def round_trip_residual(lens, lut, width, height, keep=None):
    """Largest |forward(table) - raw pixel| over the kept entries (default: all but the fisheye sentinels)."""
    x, y = pixel_grid(width, height)
    xr, yr = forward_pixels(lens, lut)
    lut = np.asarray(lut)
    if keep is None:
        keep = lut[:, 0] != np.float32(SENTINEL)
    return float(max(np.abs(xr - x)[keep].max(), np.abs(yr - y)[keep].max()))
