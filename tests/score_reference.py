"""Plain-array numpy restatement of the depth-map scores: the reference's scripts/depth_metrics.py:4-37,
precision_completeness.py:43-92 and evaluate_mcemvs_dsec.py:127-139 without masked arrays, and np.histogram's uniform-bin
arithmetic written out (numpy/lib/_histograms_impl.py) instead of called.  tests/test_score_cpu.py holds it against the
recorded output of the reference's own programs (tests/golden/depth_scores.npz); the GPU tests hold the engine against
both."""
import math

import numpy as np

THRESHOLDS = (1.25, 1.5625, 1.953125)


def validity(est, mask, gt, gt_min=0.05):
    est, gt = np.asarray(est, np.float32).ravel(), np.asarray(gt, np.float32).ravel()
    mask = np.asarray(mask).ravel()
    with np.errstate(invalid="ignore"):
        est_valid = (mask != 0) & np.isfinite(est) & (est > 0)
        gt_valid = np.isfinite(gt) & (gt.astype(np.float64) >= gt_min)
    return est_valid, gt_valid


def terms(est, mask, gt, b, f, gt_min=0.05):
    """Per joint pixel, in float64 on the exact float32 values: the summands and the predicates that are counted."""
    est_valid, gt_valid = validity(est, mask, gt, gt_min)
    joint = est_valid & gt_valid
    d = np.asarray(est, np.float32).ravel()[joint].astype(np.float64)
    g = np.asarray(gt, np.float32).ravel()[joint].astype(np.float64)
    ratio = np.maximum(d / g, g / d)
    di = np.log(g) - np.log(d)
    e = np.abs(1.0 / d - 1.0 / g) * b * f
    r = e * g / b / f
    return dict(est_valid=est_valid, gt_valid=gt_valid, ratio=ratio, di=di, di2=di * di, are=np.abs(d - g) / d, err=np.abs(g - d),
                bad=(e > 5) & (r > 0.05))


def median(err):
    """np.ma.median of a 1-D array: the middle element, or the sum of the two middle ones divided by two."""
    n = err.size
    if n == 0:
        return math.nan
    s = np.sort(err)
    return float(s[n // 2]) if n % 2 else float((s[n // 2 - 1] + s[n // 2]) / 2.0)


def metrics(est, mask, gt, b, f, gt_min=0.05):
    t = terms(est, mask, gt, b, f, gt_min)
    n = int(t["err"].size)
    gt64 = np.asarray(gt, np.float32).ravel().astype(np.float64)
    out = dict(n_est=int(t["est_valid"].sum()), n_gt=int(t["gt_valid"].sum()), n_joint=n,
               n_delta=[int((t["ratio"] < th).sum()) for th in THRESHOLDS], n_bad=int(t["bad"].sum()),
               sum_di=float(np.sum(t["di"])), sum_di2=float(np.sum(t["di2"])), sum_are=float(np.sum(t["are"])),
               sum_abs=float(np.sum(t["err"])), max_gt=float(gt64[t["gt_valid"]].max()) if t["gt_valid"].any() else math.nan)
    if n:
        out["delta"] = [c / n for c in out["n_delta"]]
        out["silog"] = 1 / n * out["sum_di2"] - 1 / (n * n) * out["sum_di"] ** 2
        out["are"] = 1 / n * out["sum_are"]
        out["lrmse"] = (1 / n * out["sum_di2"]) ** 0.5
        out["badp"] = out["n_bad"] / n
        out["mean_abs"] = out["sum_abs"] / n
    else:
        out["delta"] = [math.nan] * 3
        for k in ("silog", "are", "lrmse", "badp", "mean_abs"):
            out[k] = math.nan
    out["median_abs"] = median(t["err"])
    return out


def edges(first, last, nb):
    """np.linspace(first, last, nb + 1)"""
    delta = last - first
    step = delta / nb
    y = np.arange(0, nb + 1, dtype=np.float64)
    y = y * step if step != 0 else (y / nb) * delta
    y = y + first
    y[-1] = last
    return y


def histogram(err, binwidth=0.01):
    """np.histogram(err, bins=int(max(err) / binwidth)) -> (counts int64, first_edge, last_edge); zero bins (where numpy
    raises) and no errors give an empty histogram."""
    err = np.asarray(err, np.float64)
    if err.size == 0:
        return np.zeros(0, np.int64), math.nan, math.nan
    nb = int(err.max() / binwidth)
    if nb < 1:
        return np.zeros(0, np.int64), math.nan, math.nan
    first, last = float(err.min()), float(err.max())
    if first == last:
        first, last = first - 0.5, last + 0.5
    e = edges(first, last, nb)
    idx = (((err - first) / (last - first)) * nb).astype(np.int64)
    idx[idx == nb] -= 1
    idx[err < e[idx]] -= 1
    idx[(err >= e[idx + 1]) & (idx != nb - 1)] += 1
    return np.bincount(idx, minlength=nb).astype(np.int64), first, last


def curves(est, mask, gt, b=1.0, f=1.0, binwidth=0.01, gt_min=0.05):
    """precision_completeness.py:43-92 -> dict of base, precision, recall, f1, outliers"""
    t = terms(est, mask, gt, b, f, gt_min)
    counts, first, last = histogram(t["err"], binwidth)
    if counts.size == 0:
        z = np.zeros(0)
        return dict(base=z, precision=z, recall=z, f1=z, outliers=z)
    n_est, n_gt, n = int(t["est_valid"].sum()), int(t["gt_valid"].sum()), int(t["err"].size)
    cum = np.cumsum(counts)
    with np.errstate(divide="ignore", invalid="ignore"):       # (empty leading bins: 0 / 0 in F1, as in the script)
        precision = cum / n_est * 100
        recall = cum / n_gt * 100
        f1 = 2 * precision * recall / (precision + recall)
    return dict(base=edges(first, last, counts.size)[:-1], precision=precision, recall=recall, f1=f1,
                outliers=(n - cum) / n * 100)
