"""The focus-based collapses of Grid3D (cartesian3dgrid.cpp:139-483) restated in numpy, with the arithmetic the
engine defines (DESIGN.md "Focus-based collapses"): fp32 per operation, no FMA, OpenCV's borderInterpolate per axis,
rows filtered first into an fp32 intermediate, then columns.  The GPU kernels (k_focus_tile, k_focus_finish,
k_collapse_min_z) must equal these functions bit for bit.

Volumes are numpy float32 arrays [dimZ][dimY][dimX]; maps are [dimY][dimX].  `rows` = (y0, y1) restricts the output
to rows y0..y1-1 of every slice (the filters still read the reflected rows around them), for checks on strips of large
volumes."""
import numpy as np

F32 = np.float32


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# getGaussianKernel(ksize, sigma, CV_32F) for sigma 0.5 (5 taps) and 0.8 (7 taps): the correctly rounded normalised
# Gaussian, centre tap first
G5 = tuple(_f(b) for b in (0x3f495cb3, 0x3dda02dd, 0x398a575f))
G7 = tuple(_f(b) for b in (0x3eff5285, 0x3e69ca49, 0x3cb37d42, 0x39e71393))

REFLECT, REFLECT_101 = 0, 1
LOCAL_VAR, LOCAL_MS, GRAD_MAG, LAPLACIAN, DOG = 0, 1, 2, 3, 4


def border_interpolate(p, n, delta):
    """cv::borderInterpolate for BORDER_REFLECT (delta 0) and BORDER_REFLECT_101 (delta 1)."""
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p - 1 + delta if p < 0 else n - 1 - (p - n) - delta
    return p


def _reflected(lo, hi, n, delta):
    return np.array([border_interpolate(p, n, delta) for p in range(lo, hi)], np.int64)


# A tap set: (kind, taps) with kind "sym" (taps c0, c1, ..., cr) or "anti" (taps c1, ..., cr; centre 0).
SOBEL_D = ("anti", (F32(1),))                     # [-1, 0, 1]
SOBEL_S = ("sym", (F32(2), F32(1)))               # [1, 2, 1]
LAP_D2 = ("sym", (F32(-2), F32(0), F32(1)))       # [1, 0, -2, 0, 1]
LAP_S = ("sym", (F32(6), F32(4), F32(1)))         # [1, 4, 6, 4, 1]
GAUSS5 = ("sym", G5)
GAUSS7 = ("sym", G7)


def _radius(taps):
    kind, c = taps
    return len(c) - 1 if kind == "sym" else len(c)


def _apply(taps, tap):
    """tap(j) = the samples at offset j (arrays); the project's rule: symmetric s = S0*c0, then s = s + (S[-j] + S[j])*cj;
    antisymmetric s = (S[1] - S[-1])*c1 + ...; zero taps skipped."""
    kind, c = taps
    s = None
    if kind == "sym":
        if c[0] != 0:
            s = (tap(0) * c[0]).astype(F32)
        for j in range(1, len(c)):
            if c[j] == 0:
                continue
            t = ((tap(-j) + tap(j)) * c[j]).astype(F32)
            s = t if s is None else (s + t).astype(F32)
    else:
        for j in range(1, len(c) + 1):
            if c[j - 1] == 0:
                continue
            t = ((tap(j) - tap(-j)) * c[j - 1]).astype(F32)
            s = t if s is None else (s + t).astype(F32)
    return s


def sep_filter(vol, row_taps, col_taps, delta, ylo, yhi, xlo, xhi):
    """The separable filter of every slice of vol [nz][ny][nx], evaluated at rows ylo..yhi-1 and columns xlo..xhi-1
    (outside the image they are reflected positions like any other).  Rows first into fp32, then columns."""
    vol = np.asarray(vol, F32)
    nz, ny, nx = vol.shape
    rr, rc = _radius(row_taps), _radius(col_taps)
    ys = _reflected(ylo - rc, yhi + rc, ny, delta)
    xs = _reflected(xlo - rr, xhi + rr, nx, delta)
    src = vol[:, ys][:, :, xs]                       # [nz][rows + 2 rc][cols + 2 rr]
    w = xhi - xlo
    inter = _apply(row_taps, lambda j: src[:, :, rr + j: rr + j + w])
    h = yhi - ylo
    return _apply(col_taps, lambda j: inter[:, rc + j: rc + j + h, :])


def _gauss(vol, taps, ylo, yhi, nx):
    return sep_filter(vol, taps, taps, REFLECT, ylo, yhi, 0, nx)


def focus_volume(vol, method, half_patchsize=1, rows=None):
    """The per-slice focus [nz][rows][nx] of a collapse (0..4), before the selection.  GradMag: 0 outside
    [h, nx - h) x [h, ny - h), and those pixels are never candidates (see collapse_focus)."""
    vol = np.asarray(vol, F32)
    nz, ny, nx = vol.shape
    y0, y1 = rows if rows is not None else (0, ny)
    if method == LOCAL_VAR:
        m = _gauss(vol, GAUSS5, y0, y1, nx)
        q = _gauss((vol * vol).astype(F32), GAUSS5, y0, y1, nx)
        v = (q - (m * m).astype(F32)).astype(F32)
        v = np.where(v > 0, v, F32(0)).astype(F32)      # THRESH_TOZERO: NaN -> 0
        return np.abs(v)
    if method == LOCAL_MS:
        return _gauss((vol * vol).astype(F32), GAUSS5, y0, y1, nx)
    if method == GRAD_MAG:
        h = int(half_patchsize)
        lo, hi = max(y0, h), min(y1, ny - h)
        out = np.zeros((nz, y1 - y0, nx), F32)
        if hi <= lo or nx - 2 * h <= 0:
            return out
        gx = sep_filter(vol, SOBEL_D, SOBEL_S, REFLECT_101, lo - h, hi + h, 0, nx)
        gy = sep_filter(vol, SOBEL_S, SOBEL_D, REFLECT_101, lo - h, hi + h, 0, nx)
        g = ((gx * gx).astype(F32) + (gy * gy).astype(F32)).astype(F32).astype(np.float64)
        s = np.zeros((nz, hi - lo, nx - 2 * h), np.float64)
        for dy in range(2 * h + 1):                      # row-major double sum over the patch
            for dx in range(2 * h + 1):
                s = s + g[:, dy: dy + hi - lo, dx: dx + nx - 2 * h]
        out[:, lo - y0: hi - y0, h: nx - h] = (s * (1.0 / ((2 * h + 1) ** 2))).astype(F32)
        return out
    if method == LAPLACIAN:
        dxx = sep_filter(vol, LAP_D2, LAP_S, REFLECT_101, y0, y1, 0, nx)
        dyy = sep_filter(vol, LAP_S, LAP_D2, REFLECT_101, y0, y1, 0, nx)
        lap = (dxx + dyy).astype(F32)
        return (lap * lap).astype(F32)
    if method == DOG:
        a = _gauss(vol, GAUSS5, y0, y1, nx)
        b = _gauss(vol, GAUSS7, y0, y1, nx)
        return np.abs((a - b).astype(F32))
    raise ValueError("focus method %r" % method)


def select_first_max(focus, valid=None):
    """conf = +0, idx = 0; for k ascending: focus > conf -> (focus, k).  Strict: ties keep the first plane, NaN and
    values <= 0 are never taken."""
    conf = np.zeros(focus.shape[1:], F32)
    idx = np.zeros(focus.shape[1:], np.uint8)
    for k in range(focus.shape[0]):
        take = focus[k] > conf
        if valid is not None:
            take &= valid
        conf[take] = focus[k][take]
        idx[take] = k
    return conf, idx


def collapse_focus(vol, method, half_patchsize=1, rows=None):
    """Grid3D::collapseZSliceBy* -> (confidence [rows][nx] f32, depth_cell_indices u8)."""
    vol = np.asarray(vol, F32)
    nz, ny, nx = vol.shape
    f = focus_volume(vol, method, half_patchsize, rows)
    y0, y1 = rows if rows is not None else (0, ny)
    valid = None
    if method == GRAD_MAG:
        h = int(half_patchsize)
        yy, xx = np.meshgrid(np.arange(y0, y1), np.arange(nx), indexing="ij")
        valid = (xx >= h) & (xx < nx - h) & (yy >= h) & (yy < ny - h)
    conf, idx = select_first_max(f, valid)
    if method in (GRAD_MAG, LAPLACIAN):
        conf = np.sqrt(conf).astype(F32)                 # correctly rounded
    return conf, idx


def collapse_min_z(vol):
    """Grid3D::collapseMinZSlice: std::min_element along z, i.e. `if (v < best)` from plane 0."""
    vol = np.asarray(vol, F32)
    best = vol[0].copy()
    idx = np.zeros(best.shape, np.uint8)
    for k in range(1, vol.shape[0]):
        take = vol[k] < best
        best[take] = vol[k][take]
        idx[take] = k
    return best, idx


def local_focus(vol, focus_method, rows=None):
    """Grid3D::computeLocalFocusInPlace: 1 -> G.5(s*s); any other value -> sqrtf of the thresholded local variance."""
    vol = np.asarray(vol, F32)
    if focus_method == 1:
        return focus_volume(vol, LOCAL_MS, rows=rows)
    return np.sqrt(focus_volume(vol, LOCAL_VAR, rows=rows)).astype(F32)
