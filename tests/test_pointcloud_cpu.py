"""CPU side of the point cloud (MapperEMVS::getPointcloud, mapper_emvs_stereo.cpp:440-480): the restatement's two
keep-set paths agree (tests/pointcloud_reference.py), io.save_pcd_ascii writes the PCD v0.7 ascii layout, the k_pc_*
kernels use no scratch and do not spill and the back-projection's double divide / square root are the IEEE
sequences, and the C++ call sites compile (and refuse to run without a GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

import pointcloud_reference as ref
from dvs_mcemvs_amd import io as dio
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bruteforce_and_kdtree_agree_on_random_clouds(seed):
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0, 1.0, (3000, 3)).astype(np.float32)
    xyz[:200] = xyz[200:400]                              # duplicates
    xyz[400:420] = np.float32(1e30)                       # far away, and together
    for r in (0.05, 0.2, 0.5):
        for k in (0, 1, 3, 10):
            a = ref.keep_bruteforce(xyz, r, k)
            b = ref.keep_kdtree(xyz, r, k)
            assert np.array_equal(a, b), (r, k)
    assert ref.keep_bruteforce(xyz, 0.2, 3).any() and not ref.keep_bruteforce(xyz, 0.2, 3).all()


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (3.0, -7.5, 100.0)])
def test_bruteforce_and_kdtree_agree_on_lattices(offset):
    base = ref.lattice(7, 0.25, offset)
    r32 = np.float32(0.25)
    for xyz in (base, ref.perturb_ulps(base, 0.3, 5), ref.perturb_ulps(base, 0.05, 6)):
        for r in (r32, np.nextafter(r32, np.float32(0)), np.nextafter(r32, np.float32(1))):
            for k in (3, 6):
                a = ref.keep_bruteforce(xyz, r, k)
                assert np.array_equal(a, ref.keep_kdtree(xyz, r, k)), (r, k)
    # the exact lattice at r = spacing: an interior point has its 6 neighbours at d2 == r^2 exactly -- kept with k = 6;
    # one ulp less radius and only the point itself is left
    assert ref.keep_bruteforce(base, r32, 6).sum() == 5 ** 3
    assert not ref.keep_bruteforce(base, np.nextafter(r32, np.float32(0)), 1).any()


def test_restatement_on_colliding_cells():
    xyz, n_cells = ref.colliding_cloud(1.0, 600, seed=3)
    assert n_cells >= 20 and len(xyz) > 400
    for k in (0, 2, 5):
        assert np.array_equal(ref.keep_bruteforce(xyz, 1.0, k), ref.keep_kdtree(xyz, 1.0, k))


def test_backprojection_restatement_basics():
    depth = np.full((3, 4), 2.0, np.float32)
    mask = np.zeros((3, 4), np.uint8)
    mask[1, 2] = 1
    mask[0, 0] = 3
    pts = ref.backproject(depth, mask, 2.0, 2.0, 2.0, 1.0)
    assert pts.shape == (2, 4)
    assert np.array_equal(pts[1], np.float32([0.0, 0.0, 2.0, 0.5]))    # the principal point, row 1 after row 0
    assert np.allclose(pts[0], [-2.0, -1.0, 2.0, 0.5])


def test_save_pcd_ascii(tmp_path):
    pts = np.array([[1.0, 2.5, -3e-7, 1.0 / 3.0], [123456789.0, -0.0, 0.1, np.inf], [np.nan, 5e-39, 1e30, -2.0]],
                   np.float32)
    p = tmp_path / "pointcloud.pcd"
    assert dio.save_pcd_ascii(str(p), pts) == 3
    lines = p.read_text().split("\n")
    assert lines == ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS x y z intensity",
                     "SIZE 4 4 4 4", "TYPE F F F F", "COUNT 1 1 1 1", "WIDTH 3", "HEIGHT 1",
                     "VIEWPOINT 0 0 0 1 0 0 0", "POINTS 3", "DATA ascii",
                     "1 2.5 -3.0000001e-07 0.33333334",
                     "1.2345679e+08 -0 0.1 inf",
                     "nan 4.9999997e-39 1e+30 -2", ""]
    e = tmp_path / "empty.pcd"
    assert dio.save_pcd_ascii(str(e), np.zeros((0, 4), np.float32)) == 0
    el = e.read_text().split("\n")
    assert el[6] == "WIDTH 0" and el[9] == "POINTS 0" and el[10] == "DATA ascii" and el[11:] == [""]


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_pointcloud_kernels_isa():
    text = kernel_asm_text()
    seen = set()
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_pc_" not in name:
            continue
        seen.add(name)
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0, name
    assert len(seen) >= 9, seen
    # the back-projection: IEEE double divide (div_scale / div_fmas / div_fixup) and the correctly rounded double
    # square root (scaled v_rsq_f64 seed, FMA refinement, class check) -- never the bare v_sqrt_f64 / v_rcp_f64 answer
    m = re.search(r"^(_ZN\w*k_pc_backproject\w*):.*?$(.*?)s_endpgm", text, re.S | re.M)
    assert m, "k_pc_backproject not found"
    body = m.group(2)
    assert "v_sqrt_f64" not in body
    assert body.count("v_div_fixup_f64") >= 6 and "v_div_fmas_f64" in body and "v_div_scale_f64" in body
    assert "v_rsq_f64" in body and "v_cmp_class_f64" in body and "v_ldexp_f64" in body and "v_fma_f64" in body


def test_pointcloud_cpp_compiles_and_refuses_without_gpu(built, tmp_path):
    exe = str(tmp_path / "test_pointcloud")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_pointcloud.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    import dvs_mcemvs_amd as d
    if d.device_count() == 0:   # (with a GPU, tests/test_gpu_pointcloud.py runs the program)
        r = subprocess.run([exe, "--cloud", str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no HIP device" in (r.stdout + r.stderr)
