"""dsi::WorldMap through dsi::full_sequence_depth_maps (tests/cpp/test_world_map.cpp) on the rig of
test_gpu_world_map.py's device-path test: the map the program extracts equals the numpy restatement
(tests/world_map_reference.py) of the clouds and poses the program's windows had."""
import os
import subprocess

import numpy as np
import pytest

import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_world_map_through_the_window_stream(built, ctx, tmp_path):
    exe = str(tmp_path / "test_world_map")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_world_map.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    n_win, dur, t0, leaf = 4, 0.05, 10.0, 0.5
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    for c in range(2):
        x, y, ts = rig["events"][c]
        times, poses = rig["trajectories"][c]
        for name, a, dt in (("ev%d_x.u16", x, np.uint16), ("ev%d_y.u16", y, np.uint16), ("ev%d_t.f64", ts, np.float64),
                            ("traj%d_t.f64", times, np.float64), ("traj%d_p.f64", poses, np.float64)):
            np.ascontiguousarray(a, dt).tofile(str(tmp_path / (name % c)))
    w, h, fx, fy, cx, cy = rig["cam"]
    args = [str(tmp_path), w, h, fx, fy, cx, cy, 16, 4.0, 50.0, t0, t0 + n_win * dur + 1e-9, dur, leaf, 2.0, 1]
    r = subprocess.run([exe] + [repr(v) if isinstance(v, float) else str(v) for v in args], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    rm = ref.ReferenceMap(leaf)
    for k in range(n_win):
        cloud = np.fromfile(str(tmp_path / ("window_%d.cloud.f32" % k)), np.float32).reshape(-1, 4)
        T_rv_w = np.fromfile(str(tmp_path / ("window_%d.T_rv_w.f64" % k)), np.float64)
        T_w_rv = np.fromfile(str(tmp_path / ("window_%d.T_w_rv.f64" % k)), np.float64)
        assert np.abs(T_w_rv - E.invert_pose(T_rv_w)).max() < 1e-12        # the inverse of the window's reference view
        rm.integrate(cloud, T_w_rv)
    got = {"xyz": np.fromfile(str(tmp_path / "map.xyz.f32"), np.float32).reshape(-1, 3),
           "n": np.fromfile(str(tmp_path / "map.n.u32"), np.uint32),
           "windows": np.fromfile(str(tmp_path / "map.windows.u32"), np.uint32),
           "keys": np.fromfile(str(tmp_path / "map.keys.u64"), np.uint64)}
    want = rm.extract()
    assert len(want["keys"]) > 20
    ref.assert_maps_equal(got, want)
    info = np.fromfile(str(tmp_path / "map.info.u64"), np.uint64)
    assert info.tolist() == [len(want["keys"]), n_win, rm.accepted, rm.rejected]
