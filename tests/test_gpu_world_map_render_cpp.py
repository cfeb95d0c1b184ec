"""dsi::WorldMap::render / fetch_render (tests/cpp/test_world_map_render.cpp) on the random scene of
test_gpu_world_map_render.py: the images the program dumps equal the numpy restatement
(tests/world_map_render_reference.py), array_equal on the depth bits, windows, hits, mask and the counts."""
import os
import subprocess

import numpy as np
import pytest

import world_map_reference as ref
import world_map_render_reference as rref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_render_of_the_random_scene(built, ctx, tmp_path):
    exe = str(tmp_path / "test_world_map_render")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_world_map_render.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    calls = rref.scene_calls()
    rm = ref.ReferenceMap(rref.SCENE_LEAF)
    for k, pts in enumerate(calls):
        pts.tofile(str(tmp_path / ("call_%d.f32" % k)))
        rm.integrate(pts, rref.IDENTITY)
    rref.scene_pose().tofile(str(tmp_path / "T_v_w.f64"))
    v = rref.SCENE_VIEW
    args = [str(tmp_path), rref.SCENE_LEAF, len(calls), v["width"], v["height"], v["fx"], v["fy"], v["cx"], v["cy"], v["min_depth"],
            v["max_depth"]]
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    shape = (v["height"], v["width"])
    for splat in (0, 1, 2):
        for mw in (1, 2):
            base = str(tmp_path / ("render_s%d_w%d" % (splat, mw)))
            info = np.fromfile(base + ".info.u64", np.uint64).tolist()
            got = dict(zip(rref.COUNTS + ("width", "height"), info))
            got.update(depth=np.fromfile(base + ".depth.f32", np.float32).reshape(shape),
                       windows=np.fromfile(base + ".windows.u32", np.uint32).reshape(shape),
                       hits=np.fromfile(base + ".hits.u32", np.uint32).reshape(shape),
                       mask=np.fromfile(base + ".mask.u8", np.uint8).reshape(shape))
            want = rref.render(rm.extract(min_windows=mw), rref.scene_pose(), splat=splat, **v)
            assert want["n_drawn"] > 50
            rref.assert_renders_equal(got, want)
