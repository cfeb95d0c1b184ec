"""dsi::WorldMap::integrateDepth / integrateGroundTruth / compare / fetchDistances and dsi::map_f_score
(tests/cpp/test_map_eval.cpp) on the scene of test_gpu_map_eval.py: the files the program dumps equal the numpy restatement
(tests/map_eval_reference.py), array_equal on the histogram, the counts, the distance bits by key, the curves and the cells
of an integrated depth image."""
import os
import subprocess

import numpy as np
import pytest

import map_eval_reference as mref
import world_map_reference as ref
import world_map_render_reference as rref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_map_eval_on_the_scene(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_eval")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_eval.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    calls_a, calls_b = rref.scene_calls(), mref.scene_b_calls()
    for name, calls in (("a", calls_a), ("b", calls_b)):
        for k, pts in enumerate(calls):
            pts.tofile(str(tmp_path / ("%s_%d.f32" % (name, k))))
    ra, rb = mref.scene_maps()
    w, h = 67, 5
    depth, mask, lo, hi = mref.depth_image(w, h, 3)
    K = (40.0, 41.0, 33.0, 2.0)
    T = mref.camera_pose(1)
    depth.tofile(str(tmp_path / "depth.f32"))
    mask.tofile(str(tmp_path / "mask.u8"))
    T.tofile(str(tmp_path / "T_w_c.f64"))
    args = [str(tmp_path), mref.LEAF_A, len(calls_a), mref.LEAF_B, len(calls_b), mref.N_BINS, w, h, K[0], K[1], K[2], K[3], lo, hi]
    args += list(mref.RADII)
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    ca, cb = ra.extract(), rb.extract()
    for k, radius in enumerate(mref.RADII):
        wants = {"ab": mref.compare(ca, cb, mref.LEAF_B, radius, mref.N_BINS), "ba": mref.compare(cb, ca, mref.LEAF_A, radius, mref.N_BINS)}
        for way, want in wants.items():
            base = str(tmp_path / ("cmp_%s_%d" % (way, k)))
            got = dict(zip(mref.COUNTS, np.fromfile(base + ".info.u64", np.uint64).tolist()))
            got.update(hist=np.fromfile(base + ".hist.u64", np.uint64), keys=np.fromfile(base + ".keys.u64", np.uint64),
                       dist=np.fromfile(base + ".dist.f32", np.float32))
            assert want["n_matched"] >= 5000 and want["n_unmatched"] >= 300
            mref.assert_compares_equal(got, want)
        f = mref.f_score(wants["ab"], wants["ba"], radius, mref.N_BINS)
        got = np.fromfile(str(tmp_path / ("f_%d.f64" % k)), np.float64).reshape(4, mref.N_BINS)
        for row, name in zip(got, ("thresholds", "precision", "recall", "f1")):
            assert np.array_equal(row, f[name]), name
    # the depth image: the cells equal the restatement's map of the back-projected points
    pts = mref.backproject(depth, mask, *K, lo, hi)
    rm = ref.ReferenceMap(mref.LEAF_A)
    rejected = rm.integrate(pts, T)
    base = str(tmp_path / "depth_cells")
    got = {"keys": np.fromfile(base + ".keys.u64", np.uint64), "n": np.fromfile(base + ".n.u32", np.uint32),
           "windows": np.fromfile(base + ".windows.u32", np.uint32), "xyz": np.fromfile(base + ".xyz.f32", np.float32).reshape(-1, 3)}
    ref.assert_maps_equal(got, rm.extract())
    assert np.fromfile(str(tmp_path / "depth_info.u64"), np.uint64).tolist() == [len(pts), rejected] and len(pts) > 100
