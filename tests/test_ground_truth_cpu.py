"""CPU tests of the ground truth from disparity images: the restatement in tests/ground_truth_reference.py
against the fixture built the way the reference's script builds it (tests/golden/dsec_ground_truth.npz, written by
tests/golden/make_dsec_ground_truth.py), the 16-bit PNG reader, the PNG-to-disparity rule on every 16-bit value, known
answers of the erosion, the exported symbols and their argument checks, the C++ adapter's call sites, and the resource
usage of the new kernels."""
import ctypes
import math
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import ground_truth_reference as gr
from dvs_mcemvs_amd import engine, io as dio, process
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("dsi_gt_create", "dsi_gt_destroy", "dsi_gt_project", "dsi_gt_project_u16", "dsi_gt_fetch", "dsi_score_add_gt",
               "dsi_score_add_mapper_gt", "dsi_depth_erode")
NEW_KERNELS = ("k_gt_project", "k_gt_write", "k_depth_erode_cross")
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "dsec_ground_truth.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
MODES = (("script", gr.AS_SCRIPT), ("drop", gr.DROP_OUTSIDE))


def golden_case(name):
    return {k[len(name) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "_")}


# ------------------------------------------------------------------------ the restatement against the script's code
def test_fixture_holds_the_eight_cases():
    assert CASES == ["near_identity", "collisions", "one_pixel", "negative_indices", "one_outside", "overflow_and_negative_z",
                     "all_zero", "odd_size"]
    for name in CASES:
        g = golden_case(name)
        assert g["d"].shape == ((29, 37) if name == "odd_size" else (24, 32)) and g["d"].dtype == F and g["raw"].dtype == np.uint16
        assert g["Q"].shape == (4, 4) and g["T"].shape == (4, 4) and g["K"].shape == (3, 4)
        assert np.array_equal(g["d"], gr.disparity_from_png16(g["raw"]))
    assert int(golden_case("one_outside")["script_counts"][1]) == 1 and not golden_case("one_outside")["script_depth"].any()
    assert golden_case("one_outside")["drop_depth"].any()
    g = golden_case("negative_indices")
    assert not np.array_equal(g["script_depth"], g["drop_depth"]) and int(g["script_counts"][1]) == 0
    assert np.count_nonzero(golden_case("one_pixel")["script_depth"]) == 1
    assert (golden_case("overflow_and_negative_z")["script_depth"] < 0).any()
    assert [int(v) for v in golden_case("all_zero")["script_counts"]] == [0, 0]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tag,mode", MODES)
def test_restatement_equals_the_script(name, tag, mode):
    g = golden_case(name)
    depth, n_points, n_outside = gr.project(g["d"], g["Q"], g["T"], g["K"], mode)
    assert depth.dtype == F and np.array_equal(depth, g[tag + "_depth"])
    assert n_points == int(g[tag + "_counts"][0]) and n_outside == int(g[tag + "_counts"][1])


def test_restatement_known_answers():
    # Q: (X, Y, Z) = (x, y, d);  K with T = identity: u = X, v = Y, value = Z -- the map is the disparity image itself
    Q = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    K = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
    img = np.arange(1, 13, dtype=F).reshape(3, 4)
    img[1, 2], img[0, 0], img[2, 3] = np.inf, np.nan, -7.0             # +inf and NaN are dropped, a negative Z is kept
    depth, n, o = gr.project(img, Q, np.eye(4), K)
    want = img.copy()
    want[1, 2] = want[0, 0] = 0
    assert np.array_equal(depth, want) and (n, o) == (10, 0)
    # Z = -1 / d: a zero disparity gives -inf, which is kept -- and lies outside, its X and Y being infinite
    Qn = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -1], [0, 0, 1, 0]], np.float64)
    one = np.ones((3, 4), F)
    one[1, 1] = 0
    pt = gr.points(one, Qn, np.eye(4), K)
    assert pt["kept"].all() and pt["outside"].reshape(3, 4)[1, 1] and int(pt["outside"].sum()) == 1
    assert gr.project(one, Qn, np.eye(4), K)[1:] == (12, 1)
    # every point on pixel (row 1, column 2): the last kept source pixel's value stays
    K1 = np.array([[0, 0, 0, 2], [0, 0, 0, 1], [0, 0, 0, 1]], np.float64)
    depth, n, o = gr.project(img, Q, np.eye(4), K1)
    assert n == 10 and np.count_nonzero(depth) == 1 and depth[1, 2] == -7.0
    img[2, 3] = np.inf
    assert gr.project(img, Q, np.eye(4), K1)[0][1, 2] == 11.0
    # u = X - 2: columns 0, 1 get indices -2, -1 -> wrapped by the script, dropped by the other mode; trunc(-0.5) = 0
    Ks = np.array([[1, 0, 0, -2], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
    img = np.arange(1, 13, dtype=F).reshape(3, 4)
    depth, n, o = gr.project(img, Q, np.eye(4), Ks)
    assert np.array_equal(depth, np.roll(img, -2, axis=1)) and (n, o) == (12, 0)
    depth, n, o = gr.project(img, Q, np.eye(4), Ks, gr.DROP_OUTSIDE)
    assert np.array_equal(depth[:, :2], img[:, 2:]) and not depth[:, 2:].any() and (n, o) == (12, 0)
    Kh = np.array([[1, 0, 0, -0.5], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
    assert gr.project(img, Q, np.eye(4), Kh, gr.DROP_OUTSIDE)[0][0, 0] == 2.0       # x = 0 and x = 1 both land on column 0
    # u = X + 1: column 3 -> index 4 = W: outside.  The script's frame is zeros; the other mode writes the rest
    Ko = np.array([[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
    depth, n, o = gr.project(img, Q, np.eye(4), Ko)
    assert not depth.any() and (n, o) == (12, 3)
    depth, n, o = gr.project(img, Q, np.eye(4), Ko, gr.DROP_OUTSIDE)
    assert np.array_equal(depth[:, 1:], img[:, :3]) and not depth[:, 0].any() and (n, o) == (12, 3)
    # p_2 = 0: u is not finite -> outside
    Kz = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]], np.float64)
    assert gr.project(img, Q, np.eye(4), Kz)[1:] == (12, 12)


# ----------------------------------------------------------------------------------------------- 16-bit PNGs
def _png(rows, cols, depth, colour, interlace, payload):
    return (b"\x89PNG\r\n\x1a\n" + dio._png_chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, depth, colour, 0, 0, interlace)) +
            dio._png_chunk(b"IDAT", zlib.compress(payload)) + dio._png_chunk(b"IEND", b""))


def test_png16_round_trip_with_every_filter(tmp_path):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 65536, (13, 17)).astype(np.uint16)
    img[0, 0], img[12, 16], img[5, :] = 0, 65535, 256
    p = str(tmp_path / "000010.png")
    for filters in (0, 1, 2, 3, 4, np.arange(13) % 5):
        assert dio.write_png_gray16(p, img, filters) == (13, 17)
        got = dio.read_png_gray16(p)
        assert got.dtype == np.uint16 and np.array_equal(got, img), filters
    one = np.array([[513]], np.uint16)
    dio.write_png_gray16(p, one, 4)
    assert np.array_equal(dio.read_png_gray16(p), one)
    with pytest.raises(ValueError):
        dio.write_png_gray16(p, img.astype(np.uint8))
    assert dio.dsec_disparity_name(5) == "000010.png" and dio.dsec_disparity_name(0) == "000000.png"
    assert dio.dsec_disparity_name(np.int64(123456)) == "246912.png"


def test_png16_hand_built_files_with_each_filter(tmp_path):
    """2 x 3 samples written out byte by byte, independently of write_png_gray16: the filtered bytes of each scanline are
    worked out by hand from the PNG specification's definitions"""
    want = np.array([[0x0102, 0x0304, 0x0a0b], [0x0203, 0x0101, 0xff00]], np.uint16)
    r0 = [1, 2, 3, 4, 10, 11]
    r1 = [2, 3, 1, 1, 255, 0]
    none = bytes([0] + r0) + bytes([0] + r1)
    sub = bytes([1, 1, 2, 2, 2, 7, 7]) + bytes([1, 2, 3, 255, 254, 254, 255])
    up = bytes([2] + r0) + bytes([2, 1, 1, 254, 253, 245, 245])
    # average: floor((left + up) / 2);  row 0: up = 0 -> left >> 1;  row 1 predictions: 0, 1, 2, 3, 5, 6
    avg = bytes([3, 1, 2, 3, 3, 9, 9]) + bytes([3, 2 - 0, 3 - 1, (1 - 2) & 255, (1 - 3) & 255, (255 - 5) & 255, (0 - 6) & 255])
    # Paeth, row 0: c = b = 0 -> predictor a (left);  row 1: (a, b, c) = (0,1,0) (0,2,0) (2,3,1) (3,4,2) (1,10,3) (1,11,4)
    #   -> p = 1, 2, 4, 5, 8, 8 -> nearest: b=1, b=2, b=3, b=4, b=10, b=11
    paeth = bytes([4, 1, 2, 2, 2, 7, 7]) + bytes([4, 1, 1, (1 - 3) & 255, (1 - 4) & 255, 245, 245])
    for tag, payload in (("none", none), ("sub", sub), ("up", up), ("avg", avg), ("paeth", paeth)):
        p = str(tmp_path / (tag + ".png"))
        with open(p, "wb") as f:
            f.write(_png(2, 3, 16, 0, 0, payload))
        assert np.array_equal(dio.read_png_gray16(p), want), tag
    # two IDAT chunks and an ancillary chunk in between
    z = zlib.compress(none)
    p = str(tmp_path / "split.png")
    with open(p, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + dio._png_chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 2, 16, 0, 0, 0, 0)) +
                dio._png_chunk(b"IDAT", z[:5]) + dio._png_chunk(b"tEXt", b"k\x00v") + dio._png_chunk(b"IDAT", z[5:]) +
                dio._png_chunk(b"IEND", b""))
    assert np.array_equal(dio.read_png_gray16(p), want)


def test_png16_refuses_everything_else(tmp_path):
    img8 = np.arange(6, dtype=np.uint8).reshape(2, 3)
    p = str(tmp_path / "x.png")
    dio.write_png_gray8(p, img8)
    with pytest.raises(ValueError, match="bit depth 8"):
        dio.read_png_gray16(p)
    dio.write_png_rgb8(p, np.zeros((2, 3, 3), np.uint8))
    with pytest.raises(ValueError, match="colour type 2"):
        dio.read_png_gray16(p)
    for depth, colour, interlace, nbytes in ((16, 2, 0, 18), (16, 4, 0, 12), (16, 0, 1, 6)):   # RGB16, gray + alpha, Adam7
        with open(p, "wb") as f:
            f.write(_png(2, 3, depth, colour, interlace, (b"\x00" + bytes(nbytes)) * 2))
        with pytest.raises(ValueError):
            dio.read_png_gray16(p)
    good = _png(2, 3, 16, 0, 0, (b"\x00" + bytes(6)) * 2)
    for bad in (good[:-20], good[:40] + bytes([good[40] ^ 1]) + good[41:], b"not a png at all", _png(2, 3, 16, 0, 0, bytes(13)),
                _png(2, 3, 16, 0, 0, (b"\x05" + bytes(6)) * 2)):                             # cut, corrupt, short, filter 5
        with open(p, "wb") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            dio.read_png_gray16(p)
    with open(p, "wb") as f:
        f.write(good)
    assert not dio.read_png_gray16(p).any()


def test_disparity_from_png16_on_every_value():
    raw = np.arange(65536, dtype=np.uint16)
    want = np.divide(raw, 65535, dtype=np.float32) * 256
    got = engine.disparity_from_png16(raw)
    assert got.dtype == F and want.dtype == F and np.array_equal(got, want)
    assert np.array_equal(got, gr.disparity_from_png16(raw))
    # the correctly rounded quotient, from exact rational arithmetic, on a spread of values
    from fractions import Fraction
    for r in (1, 2, 3, 255, 256, 257, 4097, 21845, 32767, 32768, 43690, 65533, 65534, 65535):
        q = F(r) / F(65535)
        lo, hi = np.nextafter(q, F(0)), np.nextafter(q, F(2))
        exact = Fraction(r, 65535)
        assert abs(Fraction(float(q)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
        assert got[r] == q * F(256)
    assert got[0] == 0 and got[65535] == 256
    with pytest.raises(ValueError):
        engine.disparity_from_png16(raw.astype(np.int32))


def test_png16_and_the_disparity_rule_against_matplotlib_and_pil(tmp_path):
    """The script reads the disparity images with plt.imread: where matplotlib (and PIL, which it reads PNGs with) can be
    imported, every 16-bit value goes through both and must give the reader's samples and the script's d, bit for bit."""
    Image = pytest.importorskip("PIL.Image")
    raw = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    p = str(tmp_path / dio.dsec_disparity_name(21))
    dio.write_png_gray16(p, raw, np.arange(256) % 5)
    with Image.open(p) as im:
        assert np.array_equal(np.array(im), raw)
    assert np.array_equal(dio.read_png_gray16(p), raw)
    image = pytest.importorskip("matplotlib.image")
    disp = image.imread(p)                                            # what plt.imread calls
    assert disp.dtype == F and np.array_equal(disp.astype(np.float32) * 256, engine.disparity_from_png16(raw))


# ------------------------------------------------------------------------------------------------ the erosion
def test_erosion_known_answers():
    depth = np.zeros((5, 7), F)
    mask = np.zeros((5, 7), np.uint8)
    depth[2, 3], mask[2, 3] = 4.0, 1                                   # an isolated estimate grows to a cross
    e, m = gr.erode_cross(depth, mask)
    cross = np.zeros((5, 7), np.uint8)
    cross[2, 2:5] = cross[1:4, 3] = 1
    assert np.array_equal(m, cross) and np.array_equal(e, np.where(cross, F(4.0), F(255.0)))
    depth[:], mask[:] = 0, 0                                           # the four corners: two neighbours each, no wrap
    for (r, c), v in zip(((0, 0), (0, 6), (4, 0), (4, 6)), (1.0, 2.0, 3.0, 5.0)):
        depth[r, c], mask[r, c] = v, 1
    e, m = gr.erode_cross(depth, mask)
    want = np.full((5, 7), 255.0, F)
    want[0, 0] = want[0, 1] = want[1, 0] = 1.0
    want[0, 6] = want[0, 5] = want[1, 6] = 2.0
    want[4, 0] = want[4, 1] = want[3, 0] = 3.0
    want[4, 6] = want[4, 5] = want[3, 6] = 5.0
    assert np.array_equal(e, want) and np.array_equal(m, (want != 255).astype(np.uint8)) and int(m.sum()) == 12
    e, m = gr.erode_cross(np.full((4, 3), 7.0, F), np.zeros((4, 3), np.uint8))            # everything masked
    assert not m.any() and (e == 255).all()
    rng = np.random.default_rng(2)
    depth = rng.uniform(1, 50, (6, 5)).astype(F)                                           # nothing masked: a plain erosion
    e, m = gr.erode_cross(depth, np.ones((6, 5), np.uint8))
    assert m.all()
    for r in range(6):
        for c in range(5):
            nb = [depth[r, c]] + [depth[rr, cc] for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1))
                                  if 0 <= rr < 6 and 0 <= cc < 5]
            assert e[r, c] == min(nb)
    # the smaller of two neighbours wins; an estimate of exactly no_estimate is no estimate; another marker
    depth, mask = np.array([[9.0, 0.0, 3.0, 255.0]], F), np.array([[1, 0, 1, 1]], np.uint8)
    e, m = gr.erode_cross(depth, mask)
    assert e.tolist() == [[9.0, 3.0, 3.0, 3.0]] and m.tolist() == [[1, 1, 1, 1]]
    e, m = gr.erode_cross(np.array([[255.0]], F), np.array([[1]], np.uint8))
    assert e[0, 0] == 255 and m[0, 0] == 0
    e, m = gr.erode_cross(np.array([[300.0, 0.0]], F), np.array([[1, 0]], np.uint8), no_estimate=1000.0)
    assert e.tolist() == [[300.0, 300.0]] and m.tolist() == [[1, 1]]


# ------------------------------------------------------------------------------------------- the built library
def test_new_symbols_are_exported_declared_and_bound(built):
    L = d.load_library()
    header = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"DSI_API int %s\(" % name, header), name
    assert L.dsi_gt_device_ptr.argtypes is not None and re.search(r"DSI_API float \*dsi_gt_device_ptr\(", header)
    assert L.dsi_abi_version() == 10
    assert (engine.GT_AS_SCRIPT, engine.GT_DROP_OUTSIDE) == (0, 1)
    assert re.search(r"#define DSI_GT_AS_SCRIPT 0\b", header) and re.search(r"#define DSI_GT_DROP_OUTSIDE 1\b", header)
    for name in ("GroundTruthProjector", "thicken_edges", "disparity_from_png16", "GT_AS_SCRIPT", "GT_DROP_OUTSIDE"):
        assert hasattr(d, name) and name in d.__all__, name
    for name in ("project", "project_png16", "fetch", "device_ptr", "close"):
        assert hasattr(d.GroundTruthProjector, name)
    assert hasattr(d.DepthScore, "addGroundTruth") and hasattr(d.DepthScore, "addMapperGroundTruth")
    for name in ("read_png_gray16", "write_png_gray16", "dsec_disparity_name"):
        assert hasattr(dio, name)
    readme = open(os.path.join(ROOT, "README.md")).read()
    n_declared = len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", header)))
    assert "%d entry points" % n_declared in readme


def test_new_entry_points_validate_arguments_without_gpu(built):
    L = d.load_library()
    h = ctypes.c_void_p()
    fake = ctypes.c_void_p(0x1000)                                            # never dereferenced: the checks come first
    f64 = lambda n, v=1.0: (ctypes.c_double * n)(*([v] * n))
    Q, T, K = f64(16), f64(16), f64(12)
    f32 = (ctypes.c_float * 4)()
    u8 = (ctypes.c_uint8 * 4)()
    u16 = (ctypes.c_uint16 * 4)()
    assert L.dsi_gt_create(None, 2, 2, Q, T, K, 0, ctypes.byref(h)) == engine.ERR_INVALID
    assert b"null" in L.dsi_last_error()
    assert L.dsi_gt_create(fake, 2, 2, None, T, K, 0, ctypes.byref(h)) == engine.ERR_INVALID
    assert L.dsi_gt_create(fake, 2, 2, Q, None, K, 0, ctypes.byref(h)) == engine.ERR_INVALID
    assert L.dsi_gt_create(fake, 2, 2, Q, T, None, 0, ctypes.byref(h)) == engine.ERR_INVALID
    assert L.dsi_gt_create(fake, 2, 2, Q, T, K, 0, None) == engine.ERR_INVALID
    for w, hgt, mode in ((0, 2, 0), (2, 0, 0), (-1, 2, 0), (2, 2, 2), (2, 2, -1), (65536, 65536, 0), (65535, 65537, 0)):
        assert L.dsi_gt_create(fake, w, hgt, Q, T, K, mode, ctypes.byref(h)) == engine.ERR_INVALID, (w, hgt, mode)
        assert not h.value
    assert b"2^32" in L.dsi_last_error()                                      # 65535 * 65537 = 2^32 - 1: one too many
    for which in range(3):
        for bad in (math.nan, math.inf, -math.inf):
            m = [f64(16), f64(16), f64(12)]
            m[which][5] = bad
            assert L.dsi_gt_create(fake, 2, 2, m[0], m[1], m[2], 0, ctypes.byref(h)) == engine.ERR_INVALID
            assert b"finite" in L.dsi_last_error() and not h.value
    assert L.dsi_gt_project(None, f32) == engine.ERR_INVALID and L.dsi_gt_project(fake, None) == engine.ERR_INVALID
    assert L.dsi_gt_project_u16(None, u16) == engine.ERR_INVALID and L.dsi_gt_project_u16(fake, None) == engine.ERR_INVALID
    assert L.dsi_gt_fetch(None, f32, None, None) == engine.ERR_INVALID
    assert L.dsi_gt_device_ptr(None) is None
    assert L.dsi_gt_destroy(None) == engine.OK                                # like the other destroy calls
    assert L.dsi_score_add_gt(None, f32, u8, 4, fake) == engine.ERR_INVALID
    assert L.dsi_score_add_gt(fake, None, u8, 4, fake) == engine.ERR_INVALID
    assert L.dsi_score_add_gt(fake, f32, None, 4, fake) == engine.ERR_INVALID
    assert L.dsi_score_add_gt(fake, f32, u8, 4, None) == engine.ERR_INVALID
    assert L.dsi_score_add_gt(fake, f32, u8, 0, fake) == engine.ERR_INVALID
    assert L.dsi_score_add_mapper_gt(None, fake, fake) == engine.ERR_INVALID
    assert L.dsi_score_add_mapper_gt(fake, None, fake) == engine.ERR_INVALID
    assert L.dsi_score_add_mapper_gt(fake, fake, None) == engine.ERR_INVALID
    for args in ((None, f32, u8, 2, 2, 255.0, f32, u8), (fake, None, u8, 2, 2, 255.0, f32, u8), (fake, f32, None, 2, 2, 255.0, f32, u8),
                 (fake, f32, u8, 2, 2, 255.0, None, u8), (fake, f32, u8, 2, 2, 255.0, f32, None), (fake, f32, u8, 0, 2, 255.0, f32, u8),
                 (fake, f32, u8, 2, 0, 255.0, f32, u8), (fake, f32, u8, 1 << 15, 1 << 15, 255.0, f32, u8)):
        assert L.dsi_depth_erode(*args) == engine.ERR_INVALID
    # the Python layer's own checks
    with pytest.raises(ValueError):
        d.GroundTruthProjector(None, 4, 3, np.eye(3), np.eye(4), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        d.thicken_edges(None, np.zeros((2, 2), F), np.zeros((2, 3), np.uint8))
    gen = lambda **kw: process.full_sequence(None, None, None, None, None, 0, 1, 0.1, 0.1, **kw).__next__()
    with pytest.raises(ValueError):
        gen(score=object(), ground_truth=lambda t: None, ground_truth_disparity=([], [], None))
    with pytest.raises(ValueError):
        gen(ground_truth_disparity=([], [], None))                            # no score
    with pytest.raises(ValueError):
        gen(score=object(), ground_truth_disparity=([], []), options_depth_map=object())
    with pytest.raises(ValueError):
        gen(score=object(), ground_truth=lambda t: None, thicken_edges=True, options_depth_map=object())
    with pytest.raises(ValueError):
        gen(score=object(), ground_truth_disparity=([], [], None))           # no filtered maps


def _compile_cpp(exe):
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_ground_truth.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


def test_cpp_call_sites_compile_and_refuse_without_gpu(built, tmp_path):
    exe = str(tmp_path / "test_ground_truth")
    _compile_cpp(exe)
    if d.device_count() == 0:   # (with a GPU, tests/test_gpu_ground_truth.py runs the program)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no HIP device" in (r.stdout + r.stderr)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_ground_truth_kernels_use_no_scratch():
    text = kernel_asm_text()
    seen = set()
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if not any(k in name for k in NEW_KERNELS):
            continue
        seen.add(name)
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, name
        assert val("wavefront_size") == 64 and val("max_flat_workgroup_size") == 256 and val("vgpr_count") <= 32, name
    # project and write, each for float32 and for uint16 input, and the erosion
    assert len(seen) == 5, seen
    # the winner table takes an integer maximum, the counters integer adds; nothing floating-point is atomic
    for m in re.finditer(r"^(_ZN\w*k_gt_project\w*):.*?$(.*?)s_endpgm", text, re.S | re.M):
        body = m.group(2)
        assert "global_atomic_umax" in body and "global_atomic_add" in body and not re.search(r"atomic_\w*(f64|f32)", body)
