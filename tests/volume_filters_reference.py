"""numpy restatement of the reference's volume filters: laplacianInPlace and smoothInPlace (the free functions
laplacian3D and diffuse, cartesian3dgrid_filter.cpp:72-104 and :19-62), smoothInPlaceIIR3D (the 3-sigma gaussianiir3d,
gaussianiir3d.cpp:143-251), computeMoranIndexGaussianWeights (cartesian3dgrid_filter.cpp:113-199) and the project's
definition of computeMeanStd, which the reference calls and never defines.  TEST INFRASTRUCTURE, written from the cited
lines; volumes are numpy [dimZ][dimY][dimX] as everywhere in the tests.

numpy float32 arithmetic is IEEE single with one rounding per operation and whole-array passes cannot fuse, so every
product below is a separately rounded fp32 multiply followed by an fp32 add, subnormals included.  The recurrences are
vectorised ACROSS lines and sequential ALONG the line, as the definition demands.
"""
import math

import numpy as np

F = np.float32


def same_bits(a, b):
    """Element-wise: identical bit patterns, or both NaN."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _shifted(v, axis, step):
    """v at index +-1 along axis, the index clamped into the volume (homogeneous Neumann, :40-45)."""
    n = v.shape[axis]
    idx = np.clip(np.arange(n) + step, 0, n - 1)
    return np.take(v, idx, axis=axis)


def _second_differences(v):
    two_v = F(2) * v                      # exact
    d = []
    for axis in (2, 1, 0):                # Dxx, Dyy, Dzz: (v[+] - 2 v) + v[-]
        d.append((_shifted(v, axis, 1) - two_v) + _shifted(v, axis, -1))
    return (d[0] + d[1]) + d[2]


def laplacian(vol):
    """cartesian3dgrid_filter.cpp:72-104."""
    return _second_differences(np.ascontiguousarray(vol, F))


def diffusion_schedule(sigma):
    """(dt, steps) of :24-27, all fp32."""
    sigma = F(sigma)
    dt_cfl = F(1) / F(12)
    t_final = F(0.5) * sigma * sigma
    dt = min(F(0.5) * dt_cfl, F(0.5) * t_final)
    steps = int(np.ceil(F(t_final / dt)))
    return F(dt), steps


def diffuse(vol, sigma):
    """cartesian3dgrid_filter.cpp:19-62: explicit Euler steps of the heat equation.  Returns (volume, steps)."""
    v = np.ascontiguousarray(vol, F)
    dt, steps = diffusion_schedule(sigma)
    for _ in range(steps):
        v = v + dt * _second_differences(v)
    return v, steps


def iir_coefficients(sigma, numsteps):
    """(nu, boundaryscale, postscale of the axis) of gaussianiir3d.cpp:158-163."""
    sigma = F(sigma)
    lam = float(F(sigma * sigma)) / (2.0 * numsteps)
    dnu = (1.0 + 2.0 * lam - math.sqrt(1.0 + 4.0 * lam)) / (2.0 * lam)
    return F(dnu), F(1.0 / (1.0 - dnu)), F(math.pow(dnu / lam, numsteps))


def _sweep(v, axis, nu, bs, numsteps):
    """The line recurrence along one axis for every line at once (v is modified in place)."""
    p = np.moveaxis(v, axis, 0)
    n = p.shape[0]
    for _ in range(numsteps):
        p[0] *= bs
        for i in range(1, n):
            p[i] += nu * p[i - 1]
        p[n - 1] *= bs
        for i in range(n - 1, 0, -1):
            p[i - 1] += nu * p[i]


def iir3(vol, sigma_x, sigma_y, sigma_z, numsteps=3):
    """gaussianiir3d.cpp:143-251: x lines, y lines, z lines, then the post-scale."""
    v = np.array(vol, F, copy=True, order="C")
    if sigma_x <= 0 or sigma_y <= 0 or sigma_z <= 0 or numsteps <= 0:
        return v
    postscale = F(1)
    for axis, sigma in ((2, sigma_x), (1, sigma_y), (0, sigma_z)):
        nu, bs, post = iir_coefficients(sigma, numsteps)
        postscale = F(postscale * post)
        _sweep(v, axis, nu, bs, numsteps)
    v *= postscale
    return v


def mean_std(vol):
    """The project's computeMeanStd: mean and two-pass population deviation, in double."""
    v = np.asarray(vol, np.float64).ravel()
    mean = v.sum() / v.size
    return float(mean), float(math.sqrt(((v - mean) ** 2).sum() / v.size))


def moran_kernel(sigma):
    """(sigma used, kernel size, centre weight) of :115-146."""
    sigma = F(sigma)
    if float(sigma) < 0.2:
        sigma = F(0.2)
    half = int(2 * np.ceil(F(3) * sigma))
    k = 2 * half + 1
    w = np.zeros((k, k, k), F)
    w[half, half, half] = 1
    return sigma, k, F(iir3(w, sigma, sigma, sigma, 3)[half, half, half])


def moran(vol, sigma, details=False):
    """cartesian3dgrid_filter.cpp:113-199.  details=True: (I, per-voxel terms as float64, denominator)."""
    v = np.ascontiguousarray(vol, F)
    sigma, _, c = moran_kernel(sigma)
    mean, std = mean_std(v)
    inv = F(1.0 / std)
    z = ((v.astype(np.float64) - mean) * float(inv)).astype(F)
    s = iir3(z, sigma, sigma, sigma, 3)
    t = (z * (s - c * z)).astype(np.float64)
    denom = float(F(1) - c) * (float(v.size) - 1.0)
    result = float(t.sum()) / (denom + 1e-6)
    return (result, t, denom) if details else result
