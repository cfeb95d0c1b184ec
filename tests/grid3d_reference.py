"""numpy restatement of the Grid3D members added with the slice / min-max / slice-image work: subtractTwoGrids,
ratioTwoGrids, quadraticMeanTwoGrids, cubicMeanTwoGrids (cartesian3dgrid.h:95-109,166-184), getMinMax
(cartesian3dgrid.cpp:177-188), getSlice (:72-113), accumulateZSliceAt (.h:195-204) and what imwriteSlices
(cartesian3dgrid_IO.cpp:39-76) computes before it writes files.  TEST INFRASTRUCTURE, written from the cited lines and
from DESIGN.md 7d; volumes are numpy [dimZ][dimY][dimX] as everywhere in the tests.

numpy float32 arithmetic is IEEE single with one rounding per operation; whole-array passes cannot fuse.
"""
import sys
from fractions import Fraction

import numpy as np

from filters_reference import round_half_even_u8, scale_shift

F = np.float32
OP_SUBTRACT, OP_RATIO, OP_QUADRATIC_MEAN, OP_CUBIC_MEAN = 1, 2, 3, 4
RATIO_EPS = F(0.1)          # const float eps = 1e-1


def _next_float(f, up):
    return np.nextafter(F(f), F(np.inf) if up else F(-np.inf))


def cbrt_exact_f32(x):
    """The float nearest to the REAL cube root of the double x (scalar), decided in exact rational arithmetic: the
    midpoint m of the two floats around the estimate has 25 significant bits, m^3 has 75 and cannot equal a double, so
    there is no tie.  +-0, +-inf and NaN as cbrt."""
    x = float(x)
    if x != x or x == 0.0 or x in (float("inf"), float("-inf")):
        return F(x)
    s, ax = (-1.0, -x) if x < 0 else (1.0, x)
    y = float(np.cbrt(ax))
    f = F(y)
    lo, hi = (f, _next_float(f, True)) if float(f) <= y else (_next_float(f, False), f)
    # the estimate is good to an ulp of a double: the root lies between the floats around it, or we step once
    while Fraction(float(lo)) ** 3 > Fraction(ax):
        lo, hi = _next_float(lo, False), lo
    while Fraction(float(hi)) ** 3 < Fraction(ax):
        lo, hi = hi, _next_float(hi, True)
    mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
    r = hi if mid ** 3 < Fraction(ax) else lo
    return F(s * float(r))


def cbrt_rn_f32(x):
    """cbrt_exact_f32 over an array of doubles: np.cbrt rounded to float wherever that double is farther than 2^-40
    (relative; np.cbrt is good to ~2^-52) from a float rounding boundary, the exact decision elsewhere."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.cbrt(x)
        f = y.astype(F)
        fd = f.astype(np.float64)
        other = np.where(fd <= y, np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))).astype(np.float64)
        mid = 0.5 * (fd + other)
        close = np.isfinite(y) & (y != 0) & (np.abs(y - mid) <= np.abs(y) * 2.0 ** -40)
    out = f.copy()
    for i in np.flatnonzero(close.ravel()):
        out.ravel()[i] = cbrt_exact_f32(x.ravel()[i])
    return out


def binary_op(a, g, op, ratio_in_double=True):
    """op(a, g) element-wise, the bits the reference's member leaves in its grid."""
    a = np.asarray(a, F)
    g = np.asarray(g, F)
    with np.errstate(all="ignore"):
        if op == OP_SUBTRACT:
            return (a - g).astype(F)
        if op == OP_RATIO:
            if ratio_in_double:   # fabs -> double fabs(double): sum and quotient in double, one rounding to float
                den = np.abs(g.astype(np.float64)) + np.float64(RATIO_EPS)
                return (a.astype(np.float64) / den).astype(F)
            den = (np.abs(g) + RATIO_EPS).astype(F)
            return (a / den).astype(F)
        if op == OP_QUADRATIC_MEAN:
            s = ((a * a).astype(F) + (g * g).astype(F)).astype(F)
            return np.sqrt(0.5 * s.astype(np.float64)).astype(F)     # IEEE double sqrt, then one rounding to float
        if op == OP_CUBIC_MEAN:
            s = (((a * a).astype(F) * a).astype(F) + ((g * g).astype(F) * g).astype(F)).astype(F)
            return cbrt_rn_f32(0.5 * s.astype(np.float64))
    raise ValueError("op %r" % (op,))


def min_max(vol):
    """std::minmax_element over the flat array: (min, max, min_pos, max_pos); the FIRST smallest and the LAST largest
    element; -0 == +0, so position decides and the value keeps that element's bits.  No NaN."""
    v = np.asarray(vol, F).ravel()
    lo = int(np.argmin(v))                              # first occurrence
    hi = v.size - 1 - int(np.argmax(v[::-1]))           # last occurrence
    return v[lo], v[hi], lo, hi


def slice_shape(dims, dim_idx):
    nx, ny, nz = dims
    return ((ny, nz), (nx, nz), (ny, nx))[dim_idx]


def get_slice(vol, slice_idx, dim_idx):
    """getSlice: dim 0 -> [y][z] at x, dim 1 -> [x][z] at y, dim 2 -> [y][x] at z."""
    vol = np.asarray(vol)
    if dim_idx == 0:
        return np.ascontiguousarray(vol[:, :, slice_idx].T)
    if dim_idx == 1:
        return np.ascontiguousarray(vol[:, slice_idx, :].T)
    if dim_idx == 2:
        return np.ascontiguousarray(vol[slice_idx])
    raise ValueError("dim_idx %r" % (dim_idx,))


def all_slices(vol, dim_idx):
    """Every slice of one orientation, (size[dim], rows, cols)."""
    vol = np.asarray(vol)
    if dim_idx == 0:
        return np.ascontiguousarray(vol.transpose(2, 1, 0))      # [x][y][z]
    if dim_idx == 1:
        return np.ascontiguousarray(vol.transpose(1, 2, 0))      # [y][x][z]
    return np.ascontiguousarray(vol)


def slices_u8(vol, dim_idx, normalize_by_minmax=True):
    """The 8-bit images of imwriteSlices, (size[dim], rows, cols) uint8 (the project's definition)."""
    s = all_slices(np.asarray(vol, F), dim_idx)
    if normalize_by_minmax:
        lo, hi, _, _ = min_max(vol)
        with np.errstate(all="ignore"):
            rng = F(hi - lo)
            t = (s - lo).astype(F)
            t = (t / rng).astype(F)
            w = (t * F(255)).astype(F)
        return round_half_even_u8(w)
    out = np.empty(s.shape, np.uint8)
    for i in range(s.shape[0]):
        smin, smax = float(np.min(s[i])), float(np.max(s[i]))
        with np.errstate(all="ignore"):
            rng = smax - smin
            scale = 255.0 * ((1.0 / rng) if rng > sys.float_info.epsilon else 0.0)
            shift = 0.0 - smin * scale
            out[i] = round_half_even_u8(scale_shift(s[i], F(scale), F(shift)))
    return out


def accumulate_z_slice(vol, iz, img):
    """vol(ix, iy, iz) += img(iy, ix) on the image's extent; returns a new volume."""
    out = np.array(vol, F, copy=True)
    img = np.asarray(img, F)
    r, c = img.shape
    out[iz, :r, :c] = (out[iz, :r, :c] + img).astype(F)
    return out


def decode_png_gray8(data):
    """(rows, cols) uint8 of an 8-bit grayscale, non-interlaced PNG whose scanlines all use filter type 0."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(kind + body) & 0xffffffff), "chunk CRC"
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        if kind == b"IDAT":
            idat += body
        pos += 12 + n
        if kind == b"IEND":
            break
    assert pos == len(data) and hdr is not None
    w, h, depth, colour, comp, filt, interlace = hdr
    assert (depth, colour, comp, filt, interlace) == (8, 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)
    assert not raw[:, 0].any(), "filter type 0 on every scanline"
    return np.ascontiguousarray(raw[:, 1:])


def same_bits(a, b):
    """Element-wise: identical bit patterns, or both NaN (sign and payload of a NaN are not part of any contract here:
    x86 produces the negative default NaN, gfx950 the positive one)."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
