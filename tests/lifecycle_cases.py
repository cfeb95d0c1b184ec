"""The smallest calls that make each kind of engine object allocate its device scratch, shared by
tests/test_gpu_lifecycle.py and its child process tests/lifecycle_child.py: a 32 x 24 sensor, 8 depth planes and 2,048
events per camera (two packets).  Every function returns the open objects it made and a dict of named output arrays."""
import numpy as np

import dvs_mcemvs_amd as d
from dvs_mcemvs_amd import synthetic as syn

WIDTH, HEIGHT, PLANES, EVENTS = 32, 24, 8, 2048
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])  # x y z qw qx qy qz
# the projector that copies its input: (X, Y, Z) = (x, y, d), u = X, v = Y, value = Z
Q_IMAGE = np.eye(4)
K_IMAGE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)

_RIG = []


def rig():
    if not _RIG:
        _RIG.append(syn.stereo_rig(EVENTS, width=WIDTH, height=HEIGHT, duration=0.2, seed=7, n_points=400))
    return _RIG[0]


def shape():
    return d.ShapeDSI(0, 0, PLANES, 4.0, 200.0, 0.0)


def mapper_case(ctx):
    """two camera mappers, their batches and the output mapper: one fused depth map, one filter, one point cloud"""
    r = rig()
    cams, batches = [], []
    for c in range(2):
        cams.append(d.MapperEMVS(ctx, r["cam"], shape()))
        # (the reference's packet loop closes a packet only when an event follows it: 2,048 time stamps alone give one
        #  packet, so the last one is repeated for the pose look-up; the batch holds the 2,048 events, both packets full)
        ts = r["events"][c][2]
        first, Rt = d.packetize(np.append(ts, ts[-1]), r["trajectories"][c], r["T_rv_w"])
        assert first.tolist() == [0, 1024] and Rt.shape == (2, 12)
        batches.append(d.EventBatch(ctx, r["events"][c][0], r["events"][c][1], Rt, first))
    out = d.MapperEMVS(ctx, r["cam"], shape())
    out.computeDepthMapOfEvents(cams, batches, d.FUSE_HM)
    depth, conf, idx = out.fetchDepthMap()
    fdepth, fconf, mask = out.filterDepthMap(d.OptionsDepthMap(3, 0.0, 3, 0.0))
    cloud = out.getPointcloud(options_pc=d.OptionsPointCloud(1000.0, 1))
    return cams + batches + [out], {"depth": depth, "conf": conf, "idx": idx, "fdepth": fdepth, "fconf": fconf, "mask": mask,
                                    "cloud": cloud}


def _maps():
    rng = np.random.default_rng(3)
    depth = rng.uniform(1.0, 9.0, (HEIGHT, WIDTH)).astype(np.float32)
    mask = (rng.uniform(size=(HEIGHT, WIDTH)) < 0.7).astype(np.uint8)
    gt = (depth * rng.uniform(0.8, 1.25, (HEIGHT, WIDTH))).astype(np.float32)
    return depth, mask, gt


def score_case(ctx):
    depth, mask, gt = _maps()
    s = d.DepthScore(ctx, WIDTH * HEIGHT, 0.6, 50.0)
    s.add(depth, mask, gt)
    m = s.metrics()
    reals = np.array([m[k] for k in sorted(m) if isinstance(m[k], float)] + m["delta"], np.float64)
    ints = np.array([int(m[k]) for k in sorted(m) if isinstance(m[k], (int, bool))] + m["n_delta"], np.int64)
    return [s], {"reals": reals, "ints": ints}


def projector_case(ctx):
    p = d.GroundTruthProjector(ctx, WIDTH, HEIGHT, Q_IMAGE, np.eye(4), K_IMAGE)
    p.project(_maps()[0])
    depth, n_points, n_outside = p.fetch()
    return [p], {"depth": depth, "counts": np.array([n_points, n_outside], np.int64)}


def map_case(ctx):
    rng = np.random.default_rng(4)
    pts = np.column_stack([rng.uniform(-1.0, 1.0, 1500), rng.uniform(-0.8, 0.8, 1500), rng.uniform(1.0, 4.0, 1500)]).astype(np.float32)
    wm = d.WorldMap(ctx, 0.05, 8)  # (2^8 slots: the 1,500 points make the table grow)
    assert wm.integrate(pts, IDENTITY) == 0
    r = wm.render(IDENTITY, WIDTH, HEIGHT, 20.0, 20.0, (WIDTH - 1) / 2.0, (HEIGHT - 1) / 2.0, 0.5, 5.0, splat=1)
    counts = np.array([r[k] for k in ("n_cells", "n_clipped", "n_outside", "n_drawn", "n_pixels")], np.int64)
    assert wm.info()["growths"] >= 1 and r["n_drawn"] > 0
    return [wm], {"depth": r["depth"], "windows": r["windows"], "hits": r["hits"], "mask": r["mask"], "counts": counts}


def grid_case(ctx):
    rng = np.random.default_rng(5)
    g = d.Grid3D(ctx, WIDTH, HEIGHT, PLANES)
    g.upload(rng.uniform(0.0, 50.0, (PLANES, HEIGHT, WIDTH)).astype(np.float32))
    images = g.slicesU8(0)
    g.laplacian()
    return [g], {"images": images, "volume": g.download()}


CASES = {"mapper": mapper_case, "score": score_case, "projector": projector_case, "map": map_case, "grid": grid_case}
