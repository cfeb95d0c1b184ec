"""CPU side of the focus-based collapses (Grid3D::collapseZSliceBy*, collapseMinZSlice, computeLocalFocusInPlace,
cartesian3dgrid.cpp:139-483): the restatement of tests/focus_reference.py against an independent float64 computation
(scipy.ndimage.correlate1d; mode 'mirror' is BORDER_REFLECT_101, 'reflect' is BORDER_REFLECT), the Gaussian taps pinned
against mpmath, the k_focus_* / k_collapse_min_z ISA (no scratch, no spills) and the C++ call sites (they compile and
refuse to run without a GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

import focus_reference as fr
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f64_sep(vol, row, col, mode):
    from scipy.ndimage import correlate1d
    t = correlate1d(np.asarray(vol, np.float64), np.asarray(row, np.float64), axis=2, mode=mode)
    return correlate1d(t, np.asarray(col, np.float64), axis=1, mode=mode)


G5_64 = [float(fr.G5[2]), float(fr.G5[1]), float(fr.G5[0]), float(fr.G5[1]), float(fr.G5[2])]
G7_64 = [float(fr.G7[i]) for i in (3, 2, 1, 0, 1, 2, 3)]


def _independent(vol, method, h=1):
    """float64 focus per slice, computed with scipy's border modes (no restated index arithmetic)."""
    v = np.asarray(vol, np.float64)
    if method in (fr.LOCAL_VAR, fr.LOCAL_MS):
        q = _f64_sep(v * v, G5_64, G5_64, "reflect")
        if method == fr.LOCAL_MS:
            return q
        m = _f64_sep(v, G5_64, G5_64, "reflect")
        return np.maximum(q - m * m, 0.0)
    if method == fr.GRAD_MAG:
        gx = _f64_sep(v, [-1, 0, 1], [1, 2, 1], "mirror")
        gy = _f64_sep(v, [1, 2, 1], [-1, 0, 1], "mirror")
        g = gx * gx + gy * gy
        nz, ny, nx = v.shape
        out = np.zeros_like(g)
        for y in range(h, ny - h):
            for x in range(h, nx - h):
                out[:, y, x] = g[:, y - h: y + h + 1, x - h: x + h + 1].mean(axis=(1, 2))
        return out
    if method == fr.LAPLACIAN:
        lap = _f64_sep(v, [1, 0, -2, 0, 1], [1, 4, 6, 4, 1], "mirror") + _f64_sep(v, [1, 4, 6, 4, 1], [1, 0, -2, 0, 1], "mirror")
        return lap * lap
    return np.abs(_f64_sep(v, G5_64, G5_64, "reflect") - _f64_sep(v, G7_64, G7_64, "reflect"))


SHAPES = [(3, 1, 1), (2, 1, 7), (2, 7, 1), (3, 2, 2), (2, 3, 5), (2, 5, 3), (2, 9, 13), (2, 20, 17)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4])
def test_restatement_matches_float64_filters(shape, method):
    rng = np.random.default_rng(hash((shape, method)) & 0xffff)
    vol = rng.uniform(0.0, 4.0, shape).astype(np.float32)
    hs = (0, 1, 2) if method == fr.GRAD_MAG else (1,)
    for h in hs:
        got = fr.focus_volume(vol, method, h).astype(np.float64)
        want = _independent(vol, method, h)
        scale = max(1.0, float(np.abs(want).max()))
        assert np.allclose(got, want, rtol=2e-5, atol=2e-5 * scale), (shape, method, h, np.abs(got - want).max())


def test_restatement_strip_equals_whole():
    rng = np.random.default_rng(3)
    vol = rng.uniform(0.0, 1.0, (3, 40, 23)).astype(np.float32)
    for method, h in ((0, 1), (1, 1), (2, 0), (2, 2), (3, 1), (4, 1)):
        whole = fr.collapse_focus(vol, method, h)
        for rows in ((0, 5), (7, 21), (35, 40)):
            strip = fr.collapse_focus(vol, method, h, rows=rows)
            assert np.array_equal(strip[0].view(np.uint32), whole[0][rows[0]: rows[1]].view(np.uint32)), (method, h, rows)
            assert np.array_equal(strip[1], whole[1][rows[0]: rows[1]])
    lf = fr.local_focus(vol, 0)
    assert np.array_equal(fr.local_focus(vol, 0, rows=(10, 30)).view(np.uint32), lf[:, 10:30].view(np.uint32))


def test_border_interpolate():
    # gfedcb|abcdefgh|gfedcba and fedcba|abcdefgh|hgfedcb
    assert [fr.border_interpolate(p, 8, 1) for p in range(-6, 0)] == [6, 5, 4, 3, 2, 1]
    assert [fr.border_interpolate(p, 8, 1) for p in range(8, 15)] == [6, 5, 4, 3, 2, 1, 0]
    assert [fr.border_interpolate(p, 8, 0) for p in range(-6, 0)] == [5, 4, 3, 2, 1, 0]
    assert [fr.border_interpolate(p, 8, 0) for p in range(8, 15)] == [7, 6, 5, 4, 3, 2, 1]
    assert all(fr.border_interpolate(p, 1, d) == 0 for p in range(-9, 10) for d in (0, 1))
    # narrower than the radius: reflected repeatedly
    assert [fr.border_interpolate(p, 2, 1) for p in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert [fr.border_interpolate(p, 2, 0) for p in range(-3, 5)] == [1, 1, 0, 0, 1, 1, 0, 0]


def test_selection_rule():
    f = np.array([[[0.0, 1.0, np.nan, -1.0]], [[0.0, 1.0, 2.0, -0.5]], [[3.0, 1.0, 1.0, 0.0]]], np.float32)
    conf, idx = fr.select_first_max(f)
    assert conf.tolist() == [[3.0, 1.0, 2.0, 0.0]] and idx.tolist() == [[2, 0, 1, 0]]
    v, i = fr.collapse_min_z(np.array([[[np.nan, 2.0, -0.0]], [[1.0, 2.0, 0.0]], [[0.5, 1.0, -1.0]]], np.float32))
    assert np.isnan(v[0, 0]) and i[0, 0] == 0 and v[0, 1] == 1.0 and i[0, 1] == 2 and i[0, 2] == 2


def test_gaussian_taps_are_the_correctly_rounded_normalised_gaussian():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    for sigma, ksize, taps in ((0.5, 5, fr.G5), (0.8, 7, fr.G7)):
        assert ksize == (int(round(sigma * 8 + 1)) | 1)    # cvRound(sigma * 4 * 2 + 1) | 1 for float images
        r = ksize // 2
        w = [mpmath.exp(-mpmath.mpf(i * i) / (2 * mpmath.mpf(sigma) ** 2)) for i in range(-r, r + 1)]
        s = mpmath.fsum(w)
        exact = [wi / s for wi in w]
        for i in range(ksize):
            want = np.float32(float(exact[i]))          # double then float: exact is far from a float tie here
            lo, hi = np.nextafter(want, np.float32(0)), np.nextafter(want, np.float32(1))
            assert abs(exact[i] - mpmath.mpf(float(want))) <= abs(exact[i] - mpmath.mpf(float(lo)))
            assert abs(exact[i] - mpmath.mpf(float(want))) <= abs(exact[i] - mpmath.mpf(float(hi)))
            assert want == taps[abs(i - r)], (sigma, i)
    bits = [int(np.float32(t).view(np.uint32)) for t in fr.G5 + fr.G7]
    assert bits == [0x3f495cb3, 0x3dda02dd, 0x398a575f, 0x3eff5285, 0x3e69ca49, 0x3cb37d42, 0x39e71393]


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_focus_kernels_isa():
    text = kernel_asm_text()
    seen = set()
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if not ("k_focus_" in name or "k_local_focus" in name or "k_collapse_min_z" in name):
            continue
        seen.add(name)
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0, name
        assert val("sgpr_spill_count") == 0, name
    # 5 collapses (GradMag for half_patchsize 0..8), 2 local-focus modes, the finish and the arg-min
    assert len(seen) == 4 + 9 + 2 + 1 + 1, sorted(seen)
    # no fused multiply-add in the collapses' filters (fp32 per operation; the local-std transform's correctly rounded
    # sqrtf is a refinement sequence with FMAs of its own, so it is not scanned)
    scanned = 0
    for m in re.finditer(r"^(_ZN\w*k_focus_tile\w*Lb1E\w*):.*?$(.*?)s_endpgm", text, re.S | re.M):
        assert not re.search(r"v_(fma|fmac|mac|mad|pk_fma)_f32", m.group(2)), m.group(1)
        scanned += 1
    assert scanned == 4 + 9


def test_focus_cpp_compiles_and_refuses_without_gpu(built, tmp_path):
    exe = str(tmp_path / "test_focus")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_focus.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    import dvs_mcemvs_amd as d
    if d.device_count() == 0:   # (with a GPU, tests/test_gpu_focus.py runs the program)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no HIP device" in (r.stdout + r.stderr)
