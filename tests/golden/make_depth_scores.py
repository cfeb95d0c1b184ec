"""Regenerates tests/golden/depth_scores.npz from the reference's own evaluation programs.

    python tests/golden/make_depth_scores.py <the reference's mapper_emvs_stereo/scripts directory>

The reference's depth_metrics.error_metrics and precision_completeness.precision_completeness are imported from that
directory and run on masked float64 arrays built from float32 inputs, the way evaluate_mcemvs_dsec.py builds its
consolidated stacks: an estimate is masked where there is none (its 255 marker, :71-78), the ground truth where it is below
0.05 (:122).  matplotlib is not needed: a stand-in for matplotlib.pyplot records every plot() call, which is where the four
curves come from.  The printed metrics are parsed from the programs' output.  np.ma.mean / np.ma.median of the absolute
error, the largest ground-truth depth and the number of error points are taken as :131-139 take them.

Per case <c> the file holds <c>_est, <c>_mask, <c>_gt (float32 / uint8 / float32, windows x H x W), <c>_bf = (b, f),
<c>_printed = (delta1, delta2, delta3, SILog, Abs. Rel Error, log RMSE, bad-p), <c>_counts = (ground-truth points,
estimated points, error points), <c>_mean, <c>_median, <c>_max_gt and the recorded curves <c>_{p,c,f,o}_{x,y}
(precision, completeness = recall, F1, outliers).  No test imports the reference: they read this file.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B, F = 0.6, 557.25


def install_pyplot_recorder():
    calls = []
    plt = types.ModuleType("matplotlib.pyplot")
    plt.rcParams = {}
    state = {"figure": None}

    def figure(name=None, *a, **k):
        state["figure"] = name
        return name

    def plot(x, y, *a, **k):
        calls.append((state["figure"], np.array(x, np.float64), np.array(np.ma.filled(y, np.nan), np.float64)))

    def nothing(*a, **k):
        return None

    plt.figure, plt.plot = figure, plot
    for name in ("legend", "title", "xlabel", "ylabel", "xlim", "ylim", "show", "gca"):
        setattr(plt, name, nothing)
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = plt
    sys.modules["matplotlib"] = mpl
    sys.modules["matplotlib.pyplot"] = plt
    return calls


def random_case(seed, shape, p_est, p_gt):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(1.0, 4.0, shape).astype(np.float32)
    est = (gt.astype(np.float64) * np.exp(rng.normal(0.0, 0.15, shape))).astype(np.float32)
    mask = (rng.random(shape) < p_est).astype(np.uint8)
    no_gt = rng.random(shape) >= p_gt
    gt[no_gt] = np.where(rng.random(shape) < 0.5, 0.0, 0.03).astype(np.float32)[no_gt]   # nothing, and something below 0.05
    # a depth is left behind most unestimated pixels: the mask alone says that there is no estimate
    est[(mask == 0) & (rng.random(shape) < 0.2)] = 0.0
    return est, mask, gt


def tie_case(seed, shape, drop):
    """g = d + k / 128 with d a multiple of 1 / 128 and k in 32 .. 160, most k many times: errors 0.25 .. 1.25 that repeat and
    sit on bin edges, the smallest and the largest among them; `drop` joint pixels fewer, to reach the other parity."""
    rng = np.random.default_rng(seed)
    d = (rng.integers(4 * 128, 9 * 128, shape) / 128.0).astype(np.float32)
    k = rng.choice(np.array([32, 40, 48, 64, 64, 64, 80, 96, 96, 112, 128, 128, 144, 160]), shape)
    k.flat[0], k.flat[1] = 32, 160
    sign = np.where(rng.random(shape) < 0.3, -1.0, 1.0)
    sign.flat[0] = sign.flat[1] = 1.0
    g = (d.astype(np.float64) + sign * k / 128.0).astype(np.float32)
    mask = (rng.random(shape) < 0.6).astype(np.uint8)
    mask.flat[0] = mask.flat[1] = 1
    joint = np.flatnonzero(mask.ravel())
    for i in joint[2:2 + drop]:
        mask.flat[i] = 0
    return d, mask, g


def ratio_case():
    """ratios of exactly 1.25, 1.25^2 and 1.25^3 between estimate and ground truth, either way round, next to their
    float32 neighbours on both sides"""
    j = np.arange(40, 40 + 8 * 12, dtype=np.float64).reshape(1, 8, 12)
    g = (j / 64.0).astype(np.float32)
    ratio = np.array([1.25, 1.5625, 1.953125])[(np.arange(96) % 3)].reshape(1, 8, 12)
    est = (g.astype(np.float64) * ratio).astype(np.float32)
    assert np.array_equal(est.astype(np.float64), g.astype(np.float64) * ratio)       # exact in float32
    swap = (np.arange(96) // 3 % 2 == 1).reshape(1, 8, 12)
    est, g = np.where(swap, g, est), np.where(swap, est, g)
    nudge = (np.arange(96) // 6 % 3).reshape(1, 8, 12)
    est = np.where(nudge == 1, np.nextafter(est, np.float32(0)), np.where(nudge == 2, np.nextafter(est, np.float32(100)), est))
    mask = np.ones(g.shape, np.uint8)
    mask[0, 7, 11] = 0
    return est.astype(np.float32), mask, g.astype(np.float32)


def run_reference(error_metrics, precision_completeness, calls, est, mask, gt):
    depthmap = np.where(mask != 0, est.astype(np.float64), 255.0)            # evaluate_mcemvs_dsec.py:71-78
    assert not (est[mask != 0] == 255).any()
    est_ma = np.ma.array(depthmap, mask=(depthmap == 255))
    gt64 = gt.astype(np.float64)
    gt_ma = np.ma.array(gt64, mask=(gt64 < 0.05))                            # :122
    error = np.absolute(gt_ma - est_ma)                                      # :134
    mean, median = float(np.ma.mean(error)), float(np.ma.median(error))      # :136-137
    max_gt = float(np.max(gt_ma[~np.isnan(gt_ma)]))                          # :131
    n_err = int(np.ma.count(error))                                          # :139
    del calls[:]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        error_metrics(est_ma, gt_ma, name="case", b=B, f=F)                  # :140
        precision_completeness(est_ma, gt_ma, "case")                        # :141
    printed, counts = {}, {}
    for line in out.getvalue().splitlines():
        if ":" in line and not line.startswith("---"):
            key, val = line.rsplit(":", 1)
            (counts if key.startswith("Number") else printed)[key.strip()] = val.strip()
    printed = [float(printed[k]) for k in ("delta1", "delta2", "delta3", "SILog", "Abs. Rel Error", "log RMSE", "bad-p")]
    counts = [int(counts["Number of gt points"]), int(counts["Number of estimated points"]), n_err]
    curves = {}
    for (fig, x, y), tag in zip(calls, "pcfo"):
        assert fig == tag, (fig, tag)
        curves[tag + "_x"], curves[tag + "_y"] = x, y
    assert len(curves) == 8
    return dict(printed=np.array(printed), counts=np.array(counts, np.int64), mean=mean, median=median, max_gt=max_gt, **curves)


def main():
    scripts = sys.argv[1]
    calls = install_pyplot_recorder()
    sys.path.insert(0, scripts)
    from depth_metrics import error_metrics
    from precision_completeness import precision_completeness

    cases = {
        "random3": random_case(11, (3, 18, 24), 0.24, 0.69),
        "random1": random_case(12, (1, 29, 37), 0.35, 0.6),
        "ties_a": tie_case(13, (2, 15, 20), 0),
        "ties_b": tie_case(13, (2, 15, 20), 1),
        "ratios": ratio_case(),
    }
    out = {}
    for name, (est, mask, gt) in cases.items():
        r = run_reference(error_metrics, precision_completeness, calls, est, mask, gt)
        n_joint = int(r["counts"][2])
        if name.startswith("random"):
            joint = (mask != 0) & (gt >= np.float32(0.05))
            di = np.log(gt[joint].astype(np.float64)) - np.log(est[joint].astype(np.float64))
            assert 2 * int((np.abs(di) >= 0.01).sum()) >= n_joint, "too many joint pixels with a tiny log difference"
        print("%-8s gt %d est %d joint %d bins %d median %.17g" % (name, r["counts"][0], r["counts"][1], n_joint, r["p_x"].size,
                                                                 r["median"]))
        out[name + "_est"], out[name + "_mask"], out[name + "_gt"] = est, mask, gt
        out[name + "_bf"] = np.array([B, F])
        for k, v in r.items():
            out[name + "_" + k] = np.asarray(v)
    assert out["ties_a_counts"][2] % 2 != out["ties_b_counts"][2] % 2, "the tie cases must have both parities of n_joint"
    out["cases"] = np.array(sorted(cases))
    path = os.path.join(HERE, "depth_scores.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 64 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
