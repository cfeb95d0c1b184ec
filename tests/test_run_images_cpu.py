"""CPU tests of the run's pictures: the known answers of the numpy restatement in
tests/run_images_reference.py, the colour PNG writer, saveDepthMaps' file names, the exported symbols and their argument
checks, the reference-spelled C++ call sites, and the resource usage of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import run_images_reference as rr
from dvs_mcemvs_amd import engine, io as dio
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("dsi_event_image", "dsi_event_image_dev", "dsi_batch_event_image", "dsi_batch_event_image_dev",
               "dsi_depth_images", "dsi_mapper_depth_images", "dsi_default_jet_lut")
NEW_KERNELS = ("k_event_image_count", "k_event_image_minmax", "k_event_image_u8", "k_image_conf_minmax", "k_conf_negated_u8",
               "k_inv_depth_colored_dilated")


# ------------------------------------------------------------------------------ the restatement's known answers
def test_cross_dilation():
    img = np.zeros((5, 6, 3), np.uint8)
    img[2, 3] = (10, 20, 30)
    out = rr.dilate_cross(img)
    want = np.zeros_like(img)
    for r, c in ((2, 3), (1, 3), (3, 3), (2, 2), (2, 4)):
        want[r, c] = (10, 20, 30)
    assert np.array_equal(out, want)                                   # the cross, not the 3 x 3 square
    # corners: nothing outside contributes, nothing wraps around
    img = np.zeros((3, 4, 3), np.uint8)
    img[0, 0], img[2, 3] = (1, 2, 3), (9, 8, 7)
    out = rr.dilate_cross(img)
    assert {tuple(p) for p in np.argwhere(out.any(axis=2))} == {(0, 0), (0, 1), (1, 0), (2, 3), (1, 3), (2, 2)}
    # two neighbours with different colours: the maximum per channel
    img = np.zeros((1, 3, 3), np.uint8)
    img[0, 0], img[0, 2] = (200, 10, 0), (5, 90, 7)
    assert tuple(rr.dilate_cross(img)[0, 1]) == (200, 90, 7)
    assert tuple(rr.dilate_cross(img)[0, 0]) == (200, 10, 0)


def test_default_lut_end_points_and_segments():
    lut = rr.default_jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    b, g, r = lut[:, 0].astype(int), lut[:, 1].astype(int), lut[:, 2].astype(int)
    assert tuple(lut[0]) == (128, 0, 0) and tuple(lut[255]) == (0, 0, 128)       # B G R: dark blue to dark red
    assert b.max() == g.max() == r.max() == 255
    # blue rises, holds, falls, stays 0; red is its mirror image; green is a symmetric trapezoid
    for ch, up in ((b, False), (r, True)):
        ch = ch if not up else ch[::-1]
        k = int(np.argmax(ch == 255))
        assert (np.diff(ch[:k + 1]) >= 0).all() and (np.diff(ch[k:]) <= 0).all() and ch[-1] == 0
    # (mirror images up to the rounding of the exact halves 127.5 + 4 i, which the doubles miss by an ulp either way)
    assert np.abs(b - r[::-1]).max() <= 1 and np.abs(g - g[::-1]).max() <= 1
    k = int(np.argmax(g == 255))
    assert (np.diff(g[:k + 1]) >= 0).all() and g[0] == 0 and g[127] == 255 and g[128] == 255
    # t = 0.5 exactly does not exist (255 is odd); i = 51: t = 0.2, b = clamp(1.5 - |0.8 - 1|) = 1, g = 1.5 - 1.2 = 0.3
    assert tuple(lut[51]) == (255, int(np.rint((1.5 - abs(4.0 * (51 / 255.0) - 2.0)) * 255.0)), 0)


def test_event_image_known_answers():
    # half == 0: no events, and equal numbers of both polarities on every touched pixel
    img, dropped = rr.event_image([], [], [], 7, 5, True)
    assert dropped == 0 and (img == 128).all() and img.shape == (5, 7)
    img, _ = rr.event_image([1, 1, 3, 3], [2, 2, 0, 0], [1, 0, 0, 1], 7, 5, True)
    assert (img == 128).all()
    # the rounding ties: 256 positive events -> a = 0.5; one event 128.5 -> 128, three events 129.5 -> 130
    x = [0] * 256 + [1] + [2] * 3
    img, _ = rr.event_image(x, [0] * 260, [1] * 260, 4, 1, True)
    assert list(img[0]) == [255, 128, 130, 128]
    # all negative: -half is 0, an untouched pixel stays 128
    img, _ = rr.event_image([0, 0, 1], [0, 0, 0], [0, 0, 0], 3, 1, True)
    assert list(img[0]) == [0, 64, 128]
    # outside the sensor: dropped and counted
    img, dropped = rr.event_image([0, 7, 3, 65535], [0, 0, 5, 65535], [1, 1, 1, 1], 7, 5, True)
    assert dropped == 3 and img[0, 0] == 255 and (np.delete(img.ravel(), 0) == 128).all()


def test_event_image_without_polarity_wraps_at_256():
    x = [0] * 255 + [1] * 256 + [2] * 257
    c, _ = rr.event_counts(x, [0] * len(x), None, 4, 1, False)
    assert list(c[0]) == [255, 256, 257, 0]
    img, _ = rr.event_image(x, [0] * len(x), None, 4, 1, False)
    assert list(img[0]) == [255, 0, 1, 0]                              # 255, 0, 1, 0 after the wrap: min 0, max 255, scale 1
    img, _ = rr.event_image([0, 0, 1], [0, 0, 0], None, 3, 1, False)
    assert list(img[0]) == [255, 128, 0]                               # 2, 1, 0 -> 255, 127.5 -> 128 (even), 0
    img, _ = rr.event_image([], [], None, 3, 2, False)
    assert not img.any()                                               # range 0 -> scale 0


def test_conf_negated_known_answers():
    assert (rr.conf_negated(np.full((3, 4), 7.5, F)) == 255).all()     # constant: scale 0 -> 255 - 0
    c = np.array([[0.0, 2.0, 1.0, 0.5]], F)                            # 0, 255, 127.5, 63.75 -> 255 - n, ties to even
    assert list(rr.conf_negated(c)[0]) == [255, 0, 128, 191]


def test_inv_depth_index_known_answers():
    i = rr.inv_depth_index(np.array([4.0, 200.0, 3.0, 300.0, 0.0, np.nan, -5.0, np.inf], F), 4.0, 200.0)
    assert list(i) == [255, 0, 255, 0, 255, 0, 0, 0]
    mid = 1.0 / (0.5 * (1 / 4.0 + 1 / 200.0))                          # half-way in inverse depth
    assert rr.inv_depth_index(np.array([mid], F), 4.0, 200.0)[0] in (127, 128)


# ------------------------------------------------------------------------------------------------- files
def test_png_rgb8_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (5, 7), (260, 346)):
        bgr = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
        p = str(tmp_path / ("c%dx%d.png" % shape))
        assert dio.write_png_rgb8(p, bgr) == shape
        px, ctype = rr.decode_png(open(p, "rb").read())
        assert ctype == 2 and np.array_equal(px, bgr[:, :, ::-1])      # R G B in the file
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2, 3), F)):
        with pytest.raises(ValueError):
            dio.write_png_rgb8(str(tmp_path / "bad.png"), bad)


def test_save_depth_maps_file_names(tmp_path):
    rng = np.random.default_rng(5)
    depth = rng.uniform(4, 50, (6, 8)).astype(F)
    conf = rng.uniform(0, 9, (6, 8)).astype(F)
    mask = (rng.random((6, 8)) < 0.4).astype(np.uint8)
    neg = rr.conf_negated(conf)
    bgr = rr.inv_depth_colored_dilated(depth, mask, 4.0, 200.0)
    prefix = str(tmp_path / "run_")
    names = dio.save_depth_maps(prefix, "fused_2", depth, conf, mask, 4.0, 200.0, images=(neg, bgr))
    assert names == [prefix + "depth_points_fused_2.txt", prefix + "confidence_map_negated_fused_2.png",
                     prefix + "inv_depth_colored_dilated_fused_2.png"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(n) for n in names)
    lines = open(names[0]).read().splitlines()
    assert len(lines) == int(mask.sum()) and lines[0].split()[:2] == [str(v) for v in np.argwhere(mask > 0)[0][::-1]]
    px, ctype = rr.decode_png(open(names[1], "rb").read())
    assert ctype == 0 and np.array_equal(px, neg)
    px, ctype = rr.decode_png(open(names[2], "rb").read())
    assert ctype == 2 and np.array_equal(px, bgr[:, :, ::-1])
    with pytest.raises(ValueError):
        dio.save_depth_maps(prefix, "x", depth, conf, mask, 4.0, 200.0)          # no images and no context


# ------------------------------------------------------------------------------------------- the built library
def test_new_symbols_are_exported_and_declared(built):
    L = d.load_library()
    header = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
        assert re.search(r"DSI_API int %s\(" % name, header), name
    assert L.dsi_abi_version() == 10
    for name in ("accumulate_events", "depth_images", "default_jet_lut"):
        assert hasattr(d, name)
    assert hasattr(d.EventBatch, "event_image") and hasattr(d.MapperEMVS, "depthImages")


def test_new_entry_points_validate_arguments_without_gpu(built):
    L = d.load_library()
    u8 = (ctypes.c_uint8 * 16)()
    assert L.dsi_event_image(None, None, None, None, 0, 4, 4, 0, u8, None) == engine.ERR_INVALID
    assert b"null" in L.dsi_last_error()
    assert L.dsi_event_image_dev(None, None, None, None, 0, 4, 4, 0, None, None) == engine.ERR_INVALID
    assert L.dsi_batch_event_image(None, None, 4, 4, 0, u8, None) == engine.ERR_INVALID
    assert L.dsi_batch_event_image_dev(None, None, 4, 4, 0, None, None) == engine.ERR_INVALID
    assert L.dsi_depth_images(None, None, None, None, 4, 4, 4.0, 200.0, None, u8, None) == engine.ERR_INVALID
    assert L.dsi_mapper_depth_images(None, 4.0, 200.0, None, u8, None) == engine.ERR_INVALID
    assert L.dsi_default_jet_lut(None) == engine.ERR_INVALID


def test_default_lut_of_the_library_is_the_restatement(built):
    assert np.array_equal(d.default_jet_lut(), rr.default_jet_lut())


def test_cpp_call_sites_compile_and_refuse_without_gpu(built, tmp_path):
    exe = str(tmp_path / "test_run_images")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_run_images.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    if d.device_count() == 0:   # (with a GPU, tests/test_gpu_run_images.py runs the program)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no HIP device" in (r.stdout + r.stderr)


def test_cpp_png_rgb8_writer_decodes_to_the_bytes_written(built, tmp_path):
    src = tmp_path / "png.cpp"
    src.write_text('#include "dsi_engine.hpp"\n#include <cstdlib>\n'
                   "int main(int argc, char** argv) {\n"
                   "  if (argc < 4) return 2;\n"
                   "  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);\n"
                   "  std::vector<uint8_t> bgr((size_t)rows * cols * 3);\n"
                   "  for (size_t i = 0; i < bgr.size(); ++i) bgr[i] = (uint8_t)((i * 7 + i / 13) & 255);\n"
                   "  return dsi::write_png_rgb8(argv[1], bgr.data(), rows, cols) ? 0 : 1;\n}\n")
    exe = str(tmp_path / "png")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    for rows, cols in ((1, 1), (5, 7), (200, 150)):                    # 200 x 150 x 3 needs two stored deflate blocks
        p = str(tmp_path / "c.png")
        subprocess.check_call([exe, p, str(rows), str(cols)])
        i = np.arange(rows * cols * 3)
        want = ((i * 7 + i // 13) & 255).astype(np.uint8).reshape(rows, cols, 3)
        px, ctype = rr.decode_png(open(p, "rb").read())
        assert ctype == 2 and np.array_equal(px, want[:, :, ::-1])


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_run_image_kernels_use_no_scratch():
    text = kernel_asm_text()
    seen = set()
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernel = next((k for k in NEW_KERNELS if k in name), None)
        if kernel is None:
            continue
        seen.add(name)
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, name
        assert val("vgpr_count") <= 64, name
    # both instances of the three event-image templates, and the three depth-image kernels
    assert len(seen) == 9, seen
    # the counting kernel's atomics return nothing, its event reads are 16-byte loads
    m = re.search(r"^(_ZN\w*k_event_image_countILb1E\w*):.*?$(.*?)s_endpgm", text, re.S | re.M)
    assert m, "k_event_image_count<true> not found"
    body = m.group(2)
    adds = re.findall(r"global_atomic_add\S*\s+([^\n]*)", body)
    assert len(adds) >= 9 and "global_load_dwordx4" in body
    assert not re.search(r"global_atomic_add\S*[^\n]*\b(sc0|glc)\b", body)
