"""The capped launchers outside the world map, past one launch round: k_voxelwise in every op and mode,
k_fill, k_mean_square, k_grid_min_max and its finish, the z slice images, the volume sums (mean, deviation, Moran),
k_standardize, k_conf_minmax under the whole filter chain, the scorer's five strided kernels and k_event_image_count, each on
the smallest input that walks a second round and leaves a ragged end (tests/grid_round_cases.py).  Every expected value is a
restatement's; every comparison is the one the existing test of the same operation makes: uint32 views with NaN matched
against NaN, or that test's derived bound unchanged.  Where the sum can be made exact in float64 whatever its order (small
integers, a 2^-16 grid) the comparison is ==.  test_grid_rounds_cpu.py proves without a GPU that a kernel which stops after
one round, or never does its scalar tail, fails each of these tests."""
import math

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import grid_round_cases as gc
import score_reference as sr
import volume_filters_reference as vf
from oracle import oracle as orc
from test_depthmap_filters import _assert_same, _filtered, _mapper, _plant
from test_gpu_grid3d import check_min_max, check_slices_u8
from test_gpu_run_images import check_event_image
from test_gpu_score import check_against_restatement, check_curves

pytestmark = pytest.mark.gpu

F = np.float32


def grid_of(ctx, vol):
    nz, ny, nx = vol.shape
    g = d.Grid3D(ctx, nx, ny, nz)
    g.upload(vol)
    return g


def assert_same_bits(got, want, what):
    same = gc.same_bits(got, want)
    assert same.all(), "%s: %d voxels differ, first at flat index %d: gpu %r cpu %r" % (
        what, (~same).sum(), np.flatnonzero(~same.ravel())[0], got[~same][0], want[~same][0])


# ------------------------------------------------------------------------------------------------------ k_voxelwise
@pytest.mark.parametrize("case", gc.VOXEL_CASES, ids=gc.case_id)
def test_voxelwise(ctx, case):
    """fuseTwoGrids in place and setToFusionOf for ops 1-6, harmonicMeanTwoGrids(., 3 | 4), the four members that are no
    camera fusion (subtract, ratio, quadratic and cubic mean), begin / accumulate / finalize for modes 0-5 (k_fill behind MIN
    and MAX), setToFusionOfN of 2, 3 and 8 sources in every mode, the GM tree of 2, 4 and 8, on 2,112,899 voxels: one round,
    15,744 voxels of a second and a tail of three."""
    kind = case[0]
    first, _ = gc.voxel_steps(case)
    want = gc.voxel_expected(case)
    A = grid_of(ctx, first)
    got, sources = [], []
    if kind in ("fuse2", "fuse2_into", "hm_n", "binary"):
        a, g = gc.pair_inputs(kind, case[1])
        sources = [grid_of(ctx, g)]
        if kind == "fuse2":
            A.fuseTwoGrids(sources[0], case[1])
        elif kind == "binary":
            A._binary(sources[0], case[1])
        elif kind == "hm_n":
            A.harmonicMeanTwoGrids(sources[0], case[1])
        else:
            sources.append(grid_of(ctx, a))
            A.setToFusionOf(sources[1], sources[0], case[1])
        got.append(A.download())
    elif kind == "sequence":
        mode = case[1]
        sources = [grid_of(ctx, v) for v in gc.nary_volumes()[:gc.SEQUENCE_SOURCES]]
        A.accumulateBegin(mode)
        for g in sources:
            A.accumulate(g, mode)
        got.append(A.download())
        A.finalize(mode, gc.SEQUENCE_SOURCES)
        got.append(A.download())
    else:
        sources = [grid_of(ctx, v) for v in gc.nary_volumes()[:case[1]]]
        A.setToFusionOfN(sources, d.ACC_GM_TREE if kind == "gm_tree" else case[2])
        got.append(A.download())
    assert len(got) == len(want)
    for k, (g_, w_) in enumerate(zip(got, want)):
        assert_same_bits(g_, w_, "%s, field %d" % (gc.case_id(case), k))
    for o in sources + [A]:
        o.close()


def test_acc_modes_are_the_cases_modes():
    assert (d.ACC_SUM, d.ACC_INV_SUM, d.ACC_LOG_SUM, d.ACC_SQ_SUM, d.ACC_MIN, d.ACC_MAX) == tuple(range(6))
    assert d.ACC_GM_TREE not in range(6)


# ------------------------------------------------------------------------ min / max, slice images, mean square
@pytest.mark.parametrize("name", ["tied", "tail", "later"])
def test_min_max(ctx, name):
    """three rounds of k_grid_min_max and a tail of three: the extremes tied in every round and in the tail (first minimum,
    last maximum), then in the tail alone, then in the second and the third round alone"""
    vol = gc.minmax_volume(name)
    lo, hi, lp, hp = check_min_max(ctx, vol)
    assert (lo, hi) == (gc.MINMAX_LO, gc.MINMAX_HI)
    assert (lp, hp) == {"tied": (min(gc.MINMAX_TIED_LO), max(gc.MINMAX_TIED_HI)), "tail": (gc.VOL_N - 3, gc.VOL_N - 1),
                        "later": gc.MINMAX_LATER}[name]


def test_slice_images(ctx):
    """the three orientations, scaled by the volume's extremes (its maximum is the last voxel) and per slice"""
    check_slices_u8(ctx, gc.slices_volume())


def test_mean_square(ctx):
    """nine rounds of k_mean_square.  Small integers: the sum of squares is exact in any order, so ==; vote-like floats within
    the existing relative bound."""
    g = grid_of(ctx, gc.mean_square_volume("integers"))
    got, want = g.computeMeanSquare(), orc.mean_square(gc.mean_square_volume("integers"))
    print("mean square of integers: gpu %r cpu %r" % (got, want))
    assert got == want
    g.upload(gc.mean_square_volume("votes"))
    got, want = g.computeMeanSquare(), orc.mean_square(gc.mean_square_volume("votes"))
    print("mean square of votes: gpu %r cpu %r rel %.3g" % (got, want, abs(got - want) / want))
    assert got == pytest.approx(want, rel=1e-12)
    g.close()


# -------------------------------------------------------------------------------------------- mean, deviation, Moran
def test_mean_std(ctx):
    """three rounds of k_vf_partials and their finishing block on 530,707 voxels.  "balanced": mean 3 and integer deviations,
    exact in any order, so ==; vote-like floats within the existing bound."""
    v = gc.stat_volume("balanced")
    g = grid_of(ctx, v)
    got, want = g.mean_std(), vf.mean_std(v)
    print("balanced: gpu %r cpu %r" % (got, want))
    assert got == want and got[0] == 3.0
    v = gc.stat_volume("votes")
    g.upload(v)
    (mean, std), (want_mean, want_std) = g.mean_std(), vf.mean_std(v)
    print("votes: gpu %r %r cpu %r %r" % (mean, std, want_mean, want_std))
    assert abs(mean - want_mean) <= 1e-10 * abs(want_mean) and abs(std - want_std) <= 1e-10 * abs(want_std)
    assert np.array([mean, std]).tobytes() == np.array(g.mean_std()).tobytes()
    g.close()


@pytest.mark.parametrize("name", ["smooth", "votes"])
def test_moran(ctx, name):
    """k_standardize past its round of 524,288 and the Moran numerator's partials, within test_moran_index's bound"""
    v = gc.stat_volume(name)
    want, _, _ = gc.moran_reference(name)
    bound = gc.moran_bound(name)
    g = grid_of(ctx, v)
    got = g.moran_index(gc.MORAN_SIGMA)
    print("moran %s: gpu %r reference %r difference %.3g bound %.3g" % (name, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound
    assert gc.same_bits(g.download(), v).all()
    g.close()


# ------------------------------------------------------------------------------------------------ depth-map filters
@pytest.mark.parametrize("name", ["high", "low"])
def test_depth_map_filters(ctx, name):
    """362 x 363: the confidence's minimum and maximum only past k_conf_minmax's round, then only below it; the whole chain
    against the restatement and the oracle, bit for bit"""
    conf, idx = gc.filter_image(name)
    m = _mapper(ctx, gc.IMG_SHAPE, nz=gc.FILTER_PLANES)
    assert np.array_equal(m.raw_depths_vec_, gc.filter_planes())
    _plant(m, conf, idx)
    for option in gc.FILTER_OPTIONS:
        where = "%s ksize=%d C=%g median=%d max_confidence=%g" % ((name,) + option)
        got = _filtered(m, d.OptionsDepthMap(*option))
        _assert_same(got, gc.filter_reference(name, option), where, "restatement")
        _assert_same(got, orc.depth_map_filters(conf, idx, m.raw_depths_vec_, *option), where, "oracle")
    m.close()


# ------------------------------------------------------------------------------------------------------- the scorer
@pytest.mark.parametrize("where", ["second", "first"])
def test_score_planted(ctx, where):
    """362 x 363, every pixel joint, in one add: k_score_accumulate and its finish walk a second round of 334 pixels.  The
    two middle errors, the smallest and the largest error, the largest ground truth and every pixel that is not plain delta1
    lie in the second round, then in the first.  (131,406 errors are stored, so the kernels that walk them take a second
    round as well, but in an order the scheduler decides: test_score_stored_errors is their test.)"""
    est, mask, gt = gc.score_planted(where)
    s = d.DepthScore(ctx, est.size, gc.SCORE_B, gc.SCORE_FOCAL)
    s.add(est, mask, gt)
    m = s.metrics()
    check_against_restatement(m, est, mask, gt, gc.SCORE_B, gc.SCORE_FOCAL)
    err = sr.terms(est, mask, gt, gc.SCORE_B, gc.SCORE_FOCAL)["err"]
    assert m["n_stored"] == gc.IMG_N and m["sum_abs"] == math.fsum(err)       # multiples of 2^-16: exact in any order
    assert m["median_abs"] == s.median() == (gc.SCORE_MID[0] + gc.SCORE_MID[1]) / 2
    for nb in gc.SCORE_HIST_BINS:
        bw = gc.histogram_binwidth(err, nb)
        counts, lo, hi = s.histogram(bw)
        want, wlo, whi = sr.histogram(err, bw)
        assert counts.size == nb and (lo, hi) == (wlo, whi) == (gc.Q, 2.5) and np.array_equal(counts, want), nb
    check_curves(s.curves(), sr.curves(est, mask, gt))
    s.close()


@pytest.mark.parametrize("where", ["second", "first"])
def test_score_stored_errors(ctx, where):
    """k_score_minmax, _histogram and _select past one round of the STORED errors.  Inside one add the buffer's order is the
    order in which waves reach an atomic; two adds fix it.  "second": 131,072 plain pixels, then the 334 with the smallest,
    the largest and the two middle errors, all of them stored at positions >= 131,072.  "first": the 334, then the plain ones."""
    adds = gc.score_adds(where)
    est, mask, gt = (np.concatenate([a[k] for a in adds]) for k in range(3))
    s = d.DepthScore(ctx, est.size, gc.SCORE_B, gc.SCORE_FOCAL)
    for a in adds:
        s.add(*a)
    m = s.metrics()
    check_against_restatement(m, est, mask, gt, gc.SCORE_B, gc.SCORE_FOCAL)
    err = sr.terms(est, mask, gt, gc.SCORE_B, gc.SCORE_FOCAL)["err"]
    assert m["n_stored"] == gc.IMG_N and m["sum_abs"] == math.fsum(err)
    assert m["median_abs"] == s.median() == (gc.SCORE_MID[0] + gc.SCORE_MID[1]) / 2
    for nb in gc.SCORE_HIST_BINS:
        bw = gc.histogram_binwidth(err, nb)
        counts, lo, hi = s.histogram(bw)
        want, wlo, whi = sr.histogram(err, bw)
        assert counts.size == nb and (lo, hi) == (wlo, whi) == (gc.Q, 2.5) and np.array_equal(counts, want), nb
    check_curves(s.curves(), sr.curves(est, mask, gt))
    s.close()


def test_score_dsec_frame(ctx):
    """480 x 640, DSEC's own frame: three rounds"""
    est, mask, gt = gc.score_dsec()
    s = d.DepthScore(ctx, est.size, gc.SCORE_B, gc.SCORE_FOCAL)
    s.add(est, mask, gt)
    check_against_restatement(s.metrics(), est, mask, gt, gc.SCORE_B, gc.SCORE_FOCAL)
    check_curves(s.curves(), sr.curves(est, mask, gt))
    s.close()


# -------------------------------------------------------------------------------------------------- the event image
def test_event_image(ctx):
    """one round of k_event_image_count, 1,024 events of a second and a tail of seven, with and without polarity, through the
    host-array and the batch form: the brightest pixel's last increments are the second round's, the darkest pixel's the
    tail's"""
    x, y, pol = gc.events()
    img = check_event_image(ctx, x, y, pol, *gc.SENSOR)
    assert img[gc.HOT_PIXEL[1], gc.HOT_PIXEL[0]] == 255
