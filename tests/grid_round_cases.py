"""The inputs of test_gpu_grid_rounds.py, and what test_grid_rounds_cpu.py proves of them without a GPU: the
capped launchers of dsi_kernels.hip outside the world map walk their input in grid-stride rounds, and these inputs are the
smallest that walk a second round and leave a ragged end, with a member of every special class on both sides of the
boundary.  Nothing here restates arithmetic: every expected value comes from oracle.py, grid3d_reference.py,
volume_filters_reference.py, filters_reference.py, score_reference.py and run_images_reference.py.

    ROWS        per capped launcher: the block size, the cap and the items per thread, hence the items of one round; the
                CPU test derives every row again from the launcher's source
    two faults  first_round_only: the items past one round are left out (left as they were, or not seen); without_tail: the
                n % items-per-thread items that block 0 does alone are left out.  The CPU test computes both with the
                restatements and asserts that each differs from the truth in a field the GPU test compares.
"""
import functools

import numpy as np

import filters_reference as fr
import grid3d_reference as gr
import run_images_reference as rr
import volume_filters_reference as vf
from oracle import oracle as orc

F = np.float32

# ---- the round table ----
# kernel, launcher: where the launch stands in dsi_kernels.hip; block, cap: threads per workgroup and the most workgroups;
# per_thread: consecutive items a thread takes per step (the n % per_thread last items are block 0's scalar tail); cap_name:
# the named constant of dsi_kernels.h behind the cap; shape: the test shape; pinned_by: the test that walks a second round
ROWS = {
    "voxelwise": dict(kernel="k_voxelwise", launcher="launch_voxelwise", block=256, cap=2048, per_thread=4, cap_name=None,
                      shape="127x131x127", pinned_by="test_gpu_grid_rounds.py::test_voxelwise"),
    "fill": dict(kernel="k_fill", launcher="launch_fill", block=256, cap=2048, per_thread=1, cap_name=None,
                 shape="127x131x127", pinned_by="test_gpu_grid_rounds.py::test_voxelwise[sequence-4], [sequence-5]"),
    "mean_square": dict(kernel="k_mean_square", launcher="launch_mean_square", block=256, cap=1024, per_thread=1, cap_name=None,
                        shape="127x131x127", pinned_by="test_gpu_grid_rounds.py::test_mean_square"),
    "grid_min_max": dict(kernel="k_grid_min_max", launcher="launch_grid_min_max", block=256, cap=1024, per_thread=4,
                         cap_name="kGridMinMaxBlocks", shape="127x131x127", pinned_by="test_gpu_grid_rounds.py::test_min_max"),
    "slices_u8_z": dict(kernel="k_grid_slices_u8_z", launcher="launch_grid_slices_u8", block=256, cap=2048, per_thread=4,
                        cap_name=None, shape="127x131x127", pinned_by="test_gpu_grid_rounds.py::test_slice_images"),
    "vf_partials": dict(kernel="k_vf_partials", launcher="launch_vf_sum", block=256, cap=1024, per_thread=1,
                        cap_name="kVolumeSumBlocks", shape="67x89x89",
                        pinned_by="test_gpu_grid_rounds.py::test_mean_std, test_moran"),
    "standardize": dict(kernel="k_standardize", launcher="launch_volume_standardize", block=256, cap=2048, per_thread=1,
                        cap_name=None, shape="67x89x89", pinned_by="test_gpu_grid_rounds.py::test_moran"),
    "scale": dict(kernel="k_scale", launcher="launch_iir_axis", block=256, cap=2048, per_thread=1, cap_name=None, shape=None,
                  pinned_by=None),     # only an x axis with a post-scale launches it: no call of the production ABI does
    "conf_minmax": dict(kernel="k_conf_minmax", launcher="launch_depth_map_filters", block=256, cap=512, per_thread=1,
                        cap_name=None, shape="362x363", pinned_by="test_gpu_grid_rounds.py::test_depth_map_filters"),
    "score_accumulate": dict(kernel="k_score_accumulate", launcher="launch_score_accumulate", block=256, cap=512, per_thread=1,
                             cap_name="kScoreMaxBlocks", shape="362x363, 480x640",
                             pinned_by="test_gpu_grid_rounds.py::test_score_planted, test_score_dsec_frame"),
    "score_minmax": dict(kernel="k_score_minmax", launcher="launch_score_minmax", block=256, cap=512, per_thread=1,
                         cap_name="kScoreMaxBlocks", shape="131,406 errors", pinned_by="test_gpu_grid_rounds.py::test_score_stored_errors"),
    "score_histogram": dict(kernel="k_score_histogram", launcher="launch_score_histogram", block=256, cap=512, per_thread=1,
                            cap_name="kScoreMaxBlocks", shape="131,406 errors",
                            pinned_by="test_gpu_grid_rounds.py::test_score_stored_errors"),
    "score_select": dict(kernel="k_score_select", launcher="launch_score_select", block=256, cap=512, per_thread=1,
                         cap_name="kScoreMaxBlocks", shape="131,406 errors", pinned_by="test_gpu_grid_rounds.py::test_score_stored_errors"),
    "event_image_count": dict(kernel="k_event_image_count", launcher="launch_event_image", block=256, cap=4096, per_thread=8,
                              cap_name=None, shape="8,389,639 events on 346x260",
                              pinned_by="test_gpu_grid_rounds.py::test_event_image"),
    # a capped launcher the first count missed: HOT_PIXEL and TAIL_PIXEL, the image's extremes, lie past its round too
    "event_image_minmax": dict(kernel="k_event_image_minmax", launcher="launch_event_image", block=256, cap=256, per_thread=1,
                               cap_name=None, shape="346x260",
                               pinned_by="test_gpu_run_images.py::test_event_image_rounding_ties, test_gpu_grid_rounds.py::test_event_image"),
    # covered before this file
    "reduce_partials": dict(kernel="k_reduce_partials", launcher="launch_reduce_partials", block=256, cap=2048, per_thread=2,
                            cap_name=None, shape="346x260x20", pinned_by="test_gpu_exact_voxels.py"),
    "image_conf_minmax": dict(kernel="k_image_conf_minmax", launcher="launch_depth_images", block=256, cap=256, per_thread=1,
                              cap_name=None, shape="260x346", pinned_by="test_gpu_run_images.py"),
    "store_depth_map": dict(kernel="k_store_depth_map", launcher="launch_store_depth_map", block=256, cap=64, per_thread=1,
                            cap_name=None, shape="every depth map", pinned_by="every fetchDepthMap"),
}
for _r in ROWS.values():
    _r["items"] = _r["block"] * _r["cap"] * _r["per_thread"]


def round_of(row):
    return ROWS[row]["items"]


def rounds(row, n):
    """how many rounds the vector body of a row's kernel walks over n items"""
    r = ROWS[row]
    body = n // r["per_thread"] * r["per_thread"]
    return -(-body // r["items"])


def tail_start(row, n):
    return n // ROWS[row]["per_thread"] * ROWS[row]["per_thread"]


# ---- the two faults ----
def first_round_only(new, old, row):
    """a kernel that stops after one round: the items past it stay as they were"""
    out = np.array(new, copy=True).reshape(-1)
    out[round_of(row):] = np.asarray(old).reshape(-1)[round_of(row):]
    return out.reshape(np.shape(new))


def without_tail(new, old, row):
    """a kernel whose scalar tail is never done"""
    out = np.array(new, copy=True).reshape(-1)
    t = tail_start(row, out.size)
    out[t:] = np.asarray(old).reshape(-1)[t:]
    return out.reshape(np.shape(new))


def same_bits(a, b):
    return gr.same_bits(a, b)


# ---- volumes: 127 x 131 x 127 ----
VOL_SHAPE = (127, 131, 127)                                                    # (dimZ, dimY, dimX)
VOL_N = 127 * 131 * 127                                                        # 2,112,899: 15,747 past one k_voxelwise round, n & 3 == 3
STALE = F(-7.0)                                                                # what a destination holds before an out-of-place op
STALE_MAX = F(3.0e38)                                                          # ... before a running maximum: above every finite source
ACC_SUM, ACC_INV_SUM, ACC_LOG_SUM, ACC_SQ_SUM, ACC_MIN, ACC_MAX = range(6)
SEQUENCE_SOURCES = 3

# (a, g) pairs for the three tail voxels of an in-place 2-ary op: the first three that the op changes are taken, so that a
# tail left undone shows in every tail voxel whatever the op (min keeps a where a < g, max where a > g, a product 0 where a is 0)
TAIL_PAIRS = ((0, 4), (6, 0), (9, 2), (2, 9), (7, 3), (3, 7), (8, 1), (1, 8))

VOXEL_CASES = ([("fuse2", op) for op in range(1, 7)] + [("fuse2_into", op) for op in range(1, 7)] + [("hm_n", 3), ("hm_n", 4)]
               + [("binary", op) for op in range(1, 5)]                        # GridOp: subtract, ratio, quadratic and cubic mean
               + [("sequence", mode) for mode in range(6)] + [("fuse_n", n, mode) for n in (2, 3, 8) for mode in range(6)]
               + [("gm_tree", n) for n in (2, 4, 8)])


def case_id(case):
    return "-".join(str(c) for c in case)


@functools.lru_cache(maxsize=None)
def pair_volumes():
    """(a, g) as test_fusion_ops_bit_exact makes them: vote-like magnitudes, zeros at periods 7 and 5"""
    rng = np.random.default_rng(VOL_N)
    a = rng.gamma(2.0, 8.0, VOL_SHAPE).astype(F)
    g = rng.gamma(2.0, 8.0, VOL_SHAPE).astype(F)
    a.flat[::7] = 0.0
    g.flat[::5] = 0.0
    a.flags.writeable = g.flags.writeable = False
    return a, g


def _apply2(kind, a, g, k):
    if kind == "fuse2":
        return orc.fuse2(a, g, k)
    if kind == "hm_n":
        return orc.fuse_hm_n(a, g, k)
    if kind == "binary":
        return gr.binary_op(a, g, k)
    return orc.fuse2(orc.accumulate(np.zeros_like(a), a, ACC_SUM), g, k)      # setToFusionOf: resetGrid, addTwoGrids(a), <op>TwoGrids(g)


def pair_inputs(kind, k):
    """(a, g) of one 2-ary case: pair_volumes() with the three tail voxels set from TAIL_PAIRS"""
    a, g = (v.copy() for v in pair_volumes())
    ta = np.array([p[0] for p in TAIL_PAIRS], F)
    tg = np.array([p[1] for p in TAIL_PAIRS], F)
    if kind == "fuse2_into":
        take = np.arange(3)                                                    # the destination held STALE: every result differs
    else:
        take = np.flatnonzero(~same_bits(_apply2(kind, ta, tg, k), ta))[:3]
    assert take.size == 3
    a.flat[VOL_N - 3:] = ta[take]
    g.flat[VOL_N - 3:] = tg[take]
    a.flags.writeable = g.flags.writeable = False
    return a, g


NARY_TAILS = ((0.0, 1e-41, np.inf), (3e37, 2.0 ** -20, 12.5))                 # the tail voxels of sources 0 and 1


@functools.lru_cache(maxsize=None)
def nary_volumes():
    """eight sources as test_nary_fusion_modes_bit_exact makes them: zeros, denormals, 3e37 and 2^-20 at periods 11, 97, 101
    and 103, shifted per source; +inf in source 0 once in the first round, once in the second and once in the tail"""
    rng = np.random.default_rng(40 + VOL_N)
    maps = []
    for k in range(8):
        v = rng.gamma(2.0, 8.0, VOL_SHAPE).astype(F)
        v.flat[k::11] = 0.0
        v.flat[3 + k::97] = F(1e-41)
        v.flat[5 + k::101] = F(3e37)
        v.flat[7 + k::103] = F(2.0 ** -20)
        v.flat[VOL_N - 3:] = F(3.0 + k)
        maps.append(v)
    maps[0].flat[50] = np.inf
    maps[0].flat[round_of("voxelwise") + 50] = np.inf
    for k, tail in enumerate(NARY_TAILS):
        maps[k].flat[VOL_N - 3:] = np.array(tail, F)
    for v in maps:
        v.flags.writeable = False
    return tuple(maps)


def voxel_steps(case):
    """(what the destination holds first, [(row or None, state -> state, compared after it)]): the kernels of one case in
    launch order, each as the restatement's call.  A row of None is no kernel of the table (a memset, or nothing at all)."""
    kind = case[0]
    stale = np.full(VOL_SHAPE, STALE_MAX if case == ("sequence", ACC_MAX) else STALE, F)
    if kind in ("fuse2", "hm_n", "binary"):
        a, g = pair_inputs(kind, case[1])
        return a, [("voxelwise", lambda s: _apply2(kind, s, g, case[1]), True)]
    if kind == "fuse2_into":
        a, g = pair_inputs(kind, case[1])
        return stale, [("voxelwise", lambda s: _apply2(kind, a, g, case[1]), True)]
    maps = nary_volumes()
    if kind == "sequence":
        mode = case[1]
        steps = [("fill" if mode in (ACC_MIN, ACC_MAX) else None, lambda s: orc.accumulate_begin(VOL_SHAPE, mode), False)]
        for k in range(SEQUENCE_SOURCES):
            steps.append(("voxelwise", lambda s, k=k: orc.accumulate(s, maps[k], mode), k == SEQUENCE_SOURCES - 1))
        steps.append((None if mode in (ACC_MIN, ACC_MAX) else "voxelwise", lambda s: orc.finalize(s, mode, SEQUENCE_SOURCES), True))
        return stale, steps
    if kind == "fuse_n":
        return stale, [("voxelwise", lambda s: orc.fuse_nary(maps[:case[1]], case[2]), True)]
    if kind == "gm_tree":
        return stale, [("voxelwise", lambda s: orc.fuse_gm_tree(maps[:case[1]]), True)]
    raise ValueError(case)


def voxel_fields(case, fault=None, row=None):
    """the volumes the GPU test compares, in order; with `fault` applied to every kernel of `row`"""
    state, steps = voxel_steps(case)
    out = []
    for step_row, fn, compared in steps:
        new = fn(state)
        if fault is not None and step_row == row:
            new = fault(new, state, row)
        state = new
        if compared:
            out.append(state)
    return out


def voxel_expected(case):
    return tuple(voxel_fields(case))


# ---- min / max, slice images, mean square ----
MINMAX_LO, MINMAX_HI = F(-5.0), F(9.0)
_R = round_of("grid_min_max")
MINMAX_TIED_LO = (1000, _R - 1, _R + 70_001, 2 * _R + 3, 2 * _R + 15_700, VOL_N - 3, VOL_N - 1)   # first, middle and last round, tail
MINMAX_TIED_HI = (7, 40_002, _R, 2 * _R - 1, 2 * _R + 64, 2 * _R + 15_743, VOL_N - 2)
MINMAX_LATER = (_R + 280_001, 2 * _R + 15_743)                                 # the minimum in the second round (workgroup 273), the maximum the body's last voxel


@functools.lru_cache(maxsize=None)
def minmax_volume(name):
    """"tied": both extremes in every round and in the tail; "tail": both extremes in the tail alone; "later": the minimum in
    the second round alone and the maximum in the third alone -- what a kernel that walks one round and then does its tail
    never sees (with "tied" it finds the first minimum in its round and the last maximum in its tail)"""
    rng = np.random.default_rng(2)
    v = rng.uniform(1.0, 2.0, VOL_N).astype(F)
    if name == "tied":
        v[list(MINMAX_TIED_LO)] = MINMAX_LO
        v[list(MINMAX_TIED_HI)] = MINMAX_HI
    elif name == "tail":
        v[VOL_N - 3], v[VOL_N - 1] = MINMAX_LO, MINMAX_HI
    else:
        v[MINMAX_LATER[0]], v[MINMAX_LATER[1]] = MINMAX_LO, MINMAX_HI
    v = v.reshape(VOL_SHAPE)
    v.flags.writeable = False
    return v


def min_max_seen(vol, lo, hi, and_from=None):
    """the restatement's (min, max, min_pos, max_pos) of the items [lo, hi) of a volume -- and of [and_from, n) with them --,
    positions in the whole volume"""
    flat = np.asarray(vol).reshape(-1)
    at = np.arange(lo, hi) if and_from is None else np.concatenate([np.arange(lo, hi), np.arange(and_from, flat.size)])
    mn, mx, mn_pos, mx_pos = gr.min_max(flat[at])
    return mn, mx, int(at[mn_pos]), int(at[mx_pos])


@functools.lru_cache(maxsize=None)
def slices_volume():
    """as test_slices_u8_shapes: vote-like values, a fifth of them zero; its largest value in the tail, its smallest
    non-zero slice minimum in the last plane"""
    rng = np.random.default_rng(sum(VOL_SHAPE))
    v = rng.uniform(0.0, 50.0, VOL_SHAPE).astype(F)
    v[rng.random(VOL_SHAPE) < 0.2] = 0.0
    v[-1][v[-1] < 10.0] = F(10.0)                                              # the last plane's own minimum is 10, not 0
    v.flat[VOL_N - 1] = F(80.0)
    v.flags.writeable = False
    return v


@functools.lru_cache(maxsize=None)
def mean_square_volume(name):
    """"integers": 0..5 as test_collapse_max_z_exact, so every square and every partial sum is an integer below 2^53 and
    the sum is exact in any order; "votes": vote-like floats for the existing relative bound"""
    rng = np.random.default_rng(127)
    if name == "integers":
        v = rng.integers(0, 6, VOL_SHAPE).astype(F)
    else:
        v = rng.gamma(2.0, 8.0, VOL_SHAPE).astype(F)
    v.flags.writeable = False
    return v


# ---- mean / deviation, Moran: 67 x 89 x 89 ----
STAT_SHAPE = (89, 89, 67)                                                      # (dimZ, dimY, dimX)
STAT_N = 67 * 89 * 89                                                          # 530,707: 6,419 past a round of 524,288, n & 3 == 3
MORAN_SIGMA = 1.0


@functools.lru_cache(maxsize=None)
def stat_volume(name):
    """"balanced": 3 + e with e in -2..2 and sum(e) = 0, so the mean is 3 exactly and every deviation, square and partial sum
    an integer: mean and deviation are exact in any order.  No single round is balanced: the surplus of the whole is
    paid back in the first round alone.
    "votes": vote-like magnitudes, a third zero, as the existing tests.  "smooth": noise after the IIR Gaussian, for a Moran
    index near 1."""
    rng = np.random.default_rng(1000 + STAT_N)
    if name == "balanced":
        e = rng.integers(-2, 3, STAT_N)
        e[0] = 2                                                               # (so that the deviation is not constant zero anywhere)
        surplus = int(e.sum())                                                 # paid back inside the first vf round alone
        first = e[:round_of("vf_partials")]
        pay = np.flatnonzero(first > -2 if surplus > 0 else first < 2)[1:abs(surplus) + 1]
        first[pay] -= np.sign(surplus)
        assert e.sum() == 0 and e.min() >= -2 and e.max() <= 2 and surplus != 0
        v = (3 + e).astype(F).reshape(STAT_SHAPE)
    elif name == "votes":
        v = (rng.random(STAT_SHAPE) * 50).astype(F)
        v[rng.random(STAT_SHAPE) < 0.33] = 0
    else:
        v = vf.iir3(rng.random(STAT_SHAPE).astype(F), 3, 3, 3)
    v.flags.writeable = False
    return v


@functools.lru_cache(maxsize=None)
def moran_reference(name):
    """(index, terms, denominator) of volume_filters_reference.moran"""
    return vf.moran(stat_volume(name), MORAN_SIGMA, details=True)


def moran_bound(name):
    """test_moran_index's bound, unchanged"""
    _, t, denom = moran_reference(name)
    return 1e-9 * float(np.abs(t).sum()) / (denom + 1e-6)


# ---- depth-map filters: 362 rows x 363 columns ----
IMG_SHAPE = (362, 363)
IMG_N = 362 * 363                                                              # 131,406: 334 past a round of 131,072, n & 3 == 2
FILTER_PLANES = 16
FILTER_OPTIONS = ((5, 5.0, 5, 10.0), (9, 4.5, 3, 10.0), (15, 0.0, 9, 12.0), (3, -2.0, 15, 10.0))   # ksize, C, median, max_confidence
FILTER_MIN, FILTER_MAX = F(0.25), F(60.0)


@functools.lru_cache(maxsize=None)
def filter_image(name):
    """(confidence, index): gamma confidences held inside [1, 20]; "high": the minimum and the maximum lie only at pixels past
    the round (the first item of the second round, the last of its full workgroup, the last pixel); "low": only below it.
    The max_confidence of FILTER_OPTIONS, which overwrites pixel 0, lies inside [1, 20]."""
    rng = np.random.default_rng(IMG_N)
    conf = np.clip(rng.gamma(1.0, 3.0, IMG_N), 1.0, 20.0).astype(F)
    idx = rng.integers(0, FILTER_PLANES, IMG_N).astype(np.uint8)
    R = round_of("conf_minmax")
    lo, hi = ((R, IMG_N - 1), (R + 255, R + 300)) if name == "high" else ((777, R - 1), (5000, R - 2))
    conf[list(lo)] = FILTER_MIN
    conf[list(hi)] = FILTER_MAX
    conf, idx = conf.reshape(IMG_SHAPE), idx.reshape(IMG_SHAPE)
    conf.flags.writeable = idx.flags.writeable = False
    return conf, idx


def filter_planes():
    return orc.depth_planes(1.0, 5.0, FILTER_PLANES)


@functools.lru_cache(maxsize=None)
def filter_reference(name, option):
    conf, idx = filter_image(name)
    return fr.depth_map_filters(conf, idx, filter_planes(), *option, walk=False)


def filter_seen(name, option, lo, hi):
    """the filters when k_conf_minmax sees only the pixels [lo, hi): the normalisation runs on their range, and a value
    outside it saturates to 0 or 255 exactly as that range's own ends do -- the restatement on the image clipped to it"""
    conf, idx = filter_image(name)
    c = conf.copy()
    c[0, 0] = F(option[3])
    seen = c.reshape(-1)[lo:hi]
    return fr.depth_map_filters(np.clip(conf, seen.min(), seen.max()), idx, filter_planes(), *option, walk=False)


# ---- the scorer: 362 x 363 planted, 480 x 640 random ----
SCORE_B, SCORE_FOCAL = 0.6, 557.25
DSEC_SHAPE = (480, 640)                                                        # 307,200 pixels: three rounds
Q = 2.0 ** -16                                                                 # every depth and every error is a multiple of it
SCORE_MID = (2.25 / 64, 2.3125 / 64)                                           # the two middle errors: the median is their mean
# offsets of the special pixels inside the round that holds them (334 pixels: a full workgroup, a full wave and 14 lanes)
SCORE_SPECIAL = dict(smallest=0, mid0=63, mid1=64, d2=5, d3=255, none=256, bad=319, max_gt=320, d2_last=333)
SCORE_HIST_BINS = (8192, 8193, 163840)                                         # LDS counters, global counters


@functools.lru_cache(maxsize=None)
def score_planted(where):
    """(est, mask, gt): every pixel joint.  Plain pixels: gt on the 1/64 grid in [2, 3], |error| on the 2^-16 grid in
    [1/64, 3/64], so delta1 and not bad; half of them below SCORE_MID and half above.  The special pixels -- the two middle
    errors, the smallest and the largest error, the largest ground truth, delta2-only, delta3-only, no delta, bad -- lie at
    SCORE_SPECIAL in the second round ("second") or at the same offsets from pixel 0 ("first")."""
    rng = np.random.default_rng(IMG_N + 1)
    base = round_of("score_accumulate") if where == "second" else 0
    gt = (2.0 + rng.integers(0, 65, IMG_N) / 64.0)
    err = np.empty(IMG_N)
    sign = np.where(rng.random(IMG_N) < 0.5, -1.0, 1.0)
    special = {k: base + o for k, o in SCORE_SPECIAL.items()}
    # (gt, est) of the special pixels
    planted = dict(smallest=(2.0, 2.0 + Q), mid0=(2.5, 2.5 + SCORE_MID[0]), mid1=(2.5, 2.5 - SCORE_MID[1]), d2=(2.0, 2.75),
                   d3=(2.0, 3.5), none=(2.0, 4.5), bad=(2.0, 2.25), max_gt=(3.5, 3.5 + 1.0 / 64), d2_last=(2.0, 2.75))
    is_special = np.zeros(IMG_N, bool)
    is_special[list(special.values())] = True
    plain = np.flatnonzero(~is_special)
    above = sum(abs(g - e) > SCORE_MID[1] for g, e in planted.values())       # specials above the middle pair
    below = sum(abs(g - e) < SCORE_MID[0] for g, e in planted.values())
    n_low = IMG_N // 2 - 1 - below
    assert n_low + (IMG_N // 2 - 1 - above) == plain.size
    rng.shuffle(plain)
    err[plain[:n_low]] = (1024 + rng.integers(0, 1024, n_low)) * Q             # [1/64, 2/64)
    err[plain[n_low:]] = (2560 + rng.integers(0, 513, plain.size - n_low)) * Q  # [2.5/64, 3/64]
    est = gt + sign * err
    for k, (g, e) in planted.items():
        gt[special[k]], est[special[k]] = g, e
    est32, gt32 = est.astype(F).reshape(IMG_SHAPE), gt.astype(F).reshape(IMG_SHAPE)
    assert np.array_equal(est32.astype(np.float64).ravel(), est) and np.array_equal(gt32.astype(np.float64).ravel(), gt)
    mask = np.ones(IMG_SHAPE, np.uint8)
    for a in (est32, gt32, mask):
        a.flags.writeable = False
    return est32, mask, gt32


def score_adds(where):
    """score_planted(where) as two stream-ordered adds of flat maps, for the kernels that walk the STORED errors (min / max,
    histogram, select).  k_score_accumulate appends a wave's errors wherever the cursor stands when the wave reaches it, so
    within one add the order of the buffer is the scheduler's; across two adds it is not: every error of the second add
    lies behind every error of the first.  "second": 131,072 plain pixels, then the 334 with every special one -- all of
    them at positions >= 131,072.  "first": the 334 first, then 131,072 plain pixels -- whichever 334 of those end up past
    the round, no special error is among them."""
    cut = round_of("score_minmax") if where == "second" else IMG_N - round_of("score_minmax")
    maps = score_planted(where)
    return [score_maps_seen(maps, 0, cut), score_maps_seen(maps, cut, IMG_N)]


def score_maps_seen(maps, lo, hi):
    """the pixels [lo, hi) of (est, mask, gt), flat"""
    return tuple(np.asarray(m).reshape(-1)[lo:hi] for m in maps)


@functools.lru_cache(maxsize=None)
def score_dsec():
    """as test_gpu_score.random_maps, on DSEC's own frame"""
    rng = np.random.default_rng(480 * 640)
    gt = rng.uniform(1.0, 4.0, DSEC_SHAPE).astype(F)
    est = (gt.astype(np.float64) * np.exp(rng.normal(0.0, 0.15, DSEC_SHAPE))).astype(F)
    mask = (rng.random(DSEC_SHAPE) < 0.3).astype(np.uint8)
    gt[rng.random(DSEC_SHAPE) >= 0.7] = 0.0
    return est, mask, gt


def histogram_binwidth(err, nb):
    """test_histogram_in_lds_and_in_global_memory's bin width for nb bins"""
    bw = float(err.max()) / (nb + 0.5)
    assert int(err.max() / bw) == nb
    return bw


# ---- the event image: one round of events and 1,031 more, on a 346 x 260 sensor ----
SENSOR = (346, 260)                                                            # width, height
EVENTS_N = round_of("event_image_count") + 1031                                # 8,389,639: n & 7 == 7
HOT_PIXEL = (173, 200)                                                         # x, y
HOT_FIRST_ROUND = 256                                                          # its events in the first round: 256 + 1,023 = 1,279 = 4 * 256 + 255
TAIL_PIXEL = (180, 201)                                                        # the tail's events, and no others, land here


@functools.lru_cache(maxsize=None)
def events():
    """(x, y, polarity): random events, a few outside the sensor in both rounds and in the tail; nothing random lands on
    HOT_PIXEL or TAIL_PIXEL.  HOT_PIXEL gets 256 positive events in the first round and every event of the second round but
    a dropped one: its count is the largest with polarity (1,279) and without (1,279 mod 256 = 255; after one round it would
    be 256 mod 256 = 0), and its last increments are the second round's.  TAIL_PIXEL gets the tail's events alone (six
    positive ones and a dropped one): 6, the smallest count of the image, or 0 without the tail."""
    rng = np.random.default_rng(EVENTS_N)
    w, h = SENSOR
    R = round_of("event_image_count")
    x = rng.integers(0, w, EVENTS_N).astype(np.uint16)
    y = rng.integers(0, h, EVENTS_N).astype(np.uint16)
    pol = rng.random(EVENTS_N) < 0.55
    for px, py in (HOT_PIXEL, TAIL_PIXEL):
        x[(x == px) & (y == py)] += 1
    outside = np.concatenate([rng.integers(0, R, 40), [R - 1]])
    x[outside] = w + (outside % 3).astype(np.uint16)
    first = rng.choice(R - 1, HOT_FIRST_ROUND, replace=False)
    for sel, (px, py) in ((first, HOT_PIXEL), (np.arange(R, EVENTS_N - 7), HOT_PIXEL), (np.arange(EVENTS_N - 7, EVENTS_N), TAIL_PIXEL)):
        x[sel], y[sel], pol[sel] = px, py, True
    x[R + 500] = w                                                             # one dropped event in the second round
    x[EVENTS_N - 1], y[EVENTS_N - 1] = 0, h                                    # and one in the tail
    for a in (x, y, pol):
        a.flags.writeable = False
    return x, y, pol


@functools.lru_cache(maxsize=None)
def event_image_seen(use_polarity, lo=0, hi=EVENTS_N):
    """the restatement's (image, dropped) of the events [lo, hi)"""
    x, y, pol = events()
    return rr.event_image(x[lo:hi], y[lo:hi], pol[lo:hi], SENSOR[0], SENSOR[1], use_polarity)
