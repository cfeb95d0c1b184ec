"""Inputs of the rank-partition tests (test_rank_partitions_cpu.py, test_gpu_rank_partitions.py): the partition
restated in numpy, tie-rich "already reduced" accumulators with forced columns at every range boundary, the poison
of the planes a rank does not own, and the arg-max key word in numpy.  No engine call in here."""
import numpy as np

# accumulate modes (dsi_acc_mode_t): SUM, INV_SUM, LOG_SUM, SQ_SUM, MIN, MAX
ACC_SUM, ACC_INV_SUM, ACC_LOG_SUM, ACC_SQ_SUM, ACC_MIN, ACC_MAX = range(6)
MODES = (ACC_SUM, ACC_INV_SUM, ACC_LOG_SUM, ACC_SQ_SUM, ACC_MIN, ACC_MAX)
N_MAPS = (1, 3, 8)
RANKS = tuple(range(1, 10))
# nx * ny mod 4 = 1, 2, 3, 0; the last one for the full range of the 8-bit plane index
SHAPES = ((37, 21, 21), (35, 6, 13), (13, 7, 7), (32, 8, 24), (9, 5, 256))

PEAK = 9.0          # the forced maxima; the background is 0..6, the forced columns' own background 0..5

# what a plane that a rank does not own holds: its finalized value (n_maps <= 8) is above every finalized value of
# legitimate data -- SUM 1e30 / n, INV_SUM n / 1e-30, LOG_SUM exp(80 / n) >= exp(10) > exp(PEAK / n), SQ_SUM
# sqrt(1e30 / n), MIN / MAX 1e30 -- with ONE exception: an accumulator of 0 in INV_SUM finalizes to +inf (the all-zero column)
POISON = {ACC_SUM: 1e30, ACC_INV_SUM: 1e-30, ACC_LOG_SUM: 80.0, ACC_SQ_SUM: 1e30, ACC_MIN: 1e30, ACC_MAX: 1e30}


def restated_plan(nz, n, r):
    """Reduce-scatter by planes: rank r of n owns [r q, (r + 1) q), q = nz // n, and every rank the tail [q n, nz)."""
    q = nz // n
    return {"q": q, "own_begin": r * q, "own_count": q, "tail_begin": q * n, "tail_count": nz - q * n}


def owned_planes(nz, n, r):
    sp = restated_plan(nz, n, r)
    own = np.zeros(nz, bool)
    own[sp["own_begin"]:sp["own_begin"] + sp["own_count"]] = True
    own[sp["tail_begin"]:sp["tail_begin"] + sp["tail_count"]] = True
    return own


def scatter_boundaries(nz, n):
    """Planes b in 1..nz-1 at which a rank's own range or the tail begins."""
    q = nz // n
    return sorted(b for b in ({r * q for r in range(n)} | {q * n}) if 0 < b < nz)


def shard_boundaries(ranges):
    nz = sum(c for _, c in ranges)
    return sorted({b for b, c in ranges if c > 0 and 0 < b < nz})


def score_volume(shape, bounds, seed):
    """Integer-valued [nz][ny][nx] volume whose columns tie often, plus forced columns.  Returns (volume,
    {name: (flat pixel, plane the first maximum is on)}).  Forced: "zero" all 0; "equal" all 4; "last" the only
    maximum on the last plane (pixel npix - 1: the plane's last element); "ends" equal maxima on plane 0 and the last
    plane (pixel 0); "b<k>" equal maxima on planes k - 1 and k for every k in bounds."""
    nx, ny, nz = shape
    npix = nx * ny
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, 7, (nz, npix)).astype(np.float32)
    names = ["zero", "equal"] + ["b%d" % b for b in bounds]
    assert npix >= len(names) + 2
    free = 1 + rng.permutation(npix - 2)[:len(names)]           # pixels 1 .. npix - 2, distinct
    cols = {"ends": (0, 0), "last": (npix - 1, nz - 1)}
    for name, p in zip(names, free):
        cols[name] = (int(p), 0 if name in ("zero", "equal") else int(name[1:]) - 1)
    for name, (p, _) in cols.items():
        vol[:, p] = rng.integers(0, 6, nz)
        if name == "zero":
            vol[:, p] = 0.0
        elif name == "equal":
            vol[:, p] = 4.0
        elif name == "last":
            vol[nz - 1, p] = PEAK
        elif name == "ends":
            vol[0, p] = vol[nz - 1, p] = PEAK
        else:
            b = int(name[1:])
            vol[b - 1, p] = vol[b, p] = PEAK
    return vol.reshape(nz, ny, nx), cols


def accumulator(score, cols, mode):
    """The accumulator whose FINALIZED columns order like `score`: finalize is increasing in the accumulator for every
    mode but INV_SUM (n / acc), which gets PEAK + 1 - score (1..10).  The "zero" column is literally 0 in every mode."""
    acc = (PEAK + 1.0 - score) if mode == ACC_INV_SUM else score.copy()
    acc = np.ascontiguousarray(acc, np.float32)
    nz = acc.shape[0]
    acc.reshape(nz, -1)[:, cols["zero"][0]] = 0.0
    return acc


def poisoned(acc, own, mode):
    out = np.full_like(acc, POISON[mode])
    out[own] = acc[own]
    return out


def numpy_keys(conf, global_idx):
    """(confidence bits << 8) | (255 - global plane): dsi_host.hpp argmax_key, restated."""
    bits = np.ascontiguousarray(conf, np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(8)) | (np.uint64(255) - np.asarray(global_idx).astype(np.uint64))


def numpy_unkeys(keys):
    conf = (keys >> np.uint64(8)).astype(np.uint32).view(np.float32)
    return conf, (255 - (keys & np.uint64(255)).astype(np.int64)).astype(np.uint8)


def rank_keys(finalized, nz, n, r, collapse):
    """What rank r's local step must leave: the keys' maximum over its own range and the tail (zeros if it owns
    nothing), from the finalized volume with `collapse` = a collapseMaxZSlice of a slab -> (conf, local idx)."""
    sp = restated_plan(nz, n, r)
    keys = np.zeros(finalized.shape[1:], np.uint64)
    for b, c in ((sp["own_begin"], sp["own_count"]), (sp["tail_begin"], sp["tail_count"])):
        if c > 0:
            conf, idx = collapse(finalized[b:b + c])
            keys = np.maximum(keys, numpy_keys(conf, idx.astype(np.int64) + b))
    return keys
