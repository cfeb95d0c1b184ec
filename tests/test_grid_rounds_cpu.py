"""What test_gpu_grid_rounds.py relies on, proved without a GPU:

  * the round table of grid_round_cases.ROWS, derived again from the launchers of dsi_kernels.hip and the named constants of
    dsi_kernels.h, and every grid_for( / score_blocks( call site accounted for;
  * the shape arithmetic: every input is larger than its round, leaves the stated ragged end and walks the stated rounds;
  * the plantings: a member of each special class on both sides of the boundary;
  * for every GPU case, with the restatements alone, the result of the two modelled faults -- the items past one round
    left out, the scalar tail left out -- which must differ from the truth in a field the GPU test compares, by more than
    that comparison's bound where it has one.
"""
import math
import os
import re

import numpy as np
import pytest

import grid3d_reference as gr
import grid_round_cases as gc
import run_images_reference as rr
import score_reference as sr
import volume_filters_reference as vf
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvs_mcemvs_amd", "csrc")
with open(os.path.join(CSRC, "dsi_kernels.hip")) as _f:
    SRC = _f.read()
with open(os.path.join(CSRC, "dsi_kernels.h")) as _f:
    HDR = _f.read()
F = np.float32
FUNCTION = re.compile(r"^(?:static\s+)?(?:hipError_t|int|size_t|void)\s+(\w+)\(", re.M)


# ------------------------------------------------------------------------------------------- reading the source
def constant(name):
    for text in (HDR, SRC):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*([\d\s*]+);" % re.escape(name), text)
        if m:
            return math.prod(int(t) for t in m.group(1).split("*"))
    raise AssertionError("no constexpr int %s in dsi_kernels.h / .hip" % name)


def body_after(pos):
    """the text of the function whose header starts at pos, up to the closing brace in column 0"""
    end = SRC.index("\n}\n", pos)
    return SRC[pos:end]


def function_body(name):
    for m in FUNCTION.finditer(SRC):
        if m.group(1) == name:
            return body_after(m.start())
    raise AssertionError("no function %s in dsi_kernels.hip" % name)


def kernel_body(name):
    m = re.search(r"__global__[^;{]*?\bvoid\s+%s\(" % re.escape(name), SRC)
    assert m, "no kernel %s" % name
    return body_after(m.start())


def call_args(text, open_paren):
    """(the top-level arguments of the call whose '(' is at open_paren, the index after its ')')"""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i].strip())
                return args, i + 1
        elif c == "," and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
    raise AssertionError("unbalanced call")


def launches_of(body, kernel):
    """[(grid argument, block argument)] of every hipLaunchKernelGGL of `kernel` in a function body"""
    out = []
    for m in re.finditer(r"hipLaunchKernelGGL\(", body):
        args, _ = call_args(body, m.end() - 1)
        if re.match(r"\(*\s*%s\b" % re.escape(kernel), args[0]):
            out.append((args[1], args[2]))
    return out


def grid_call(expr, body):
    """the grid_for(...) / score_blocks(...) call behind a launch's grid argument: (name, [arguments])"""
    m = re.search(r"\b(grid_for|score_blocks)\(", expr)
    text = expr
    if not m:
        ident = re.fullmatch(r"(?:dim3\()?\s*(\w+)\s*\)?", expr)
        assert ident, "grid argument %r" % expr
        m = re.search(r"\b%s\s*(?:=\s*|\()(grid_for|score_blocks)\(" % ident.group(1), body)
        assert m, "no definition of %r by grid_for / score_blocks" % ident.group(1)
        text = body
    args, _ = call_args(text, m.end() - 1)
    return m.group(1), args


def block_of(expr, body):
    m = re.fullmatch(r"dim3\((\w+)\)", expr)
    tok = m.group(1) if m else None
    if tok is None:
        m = re.search(r"\b%s\((\w+)\)" % re.escape(expr), body)
        assert m, "block argument %r" % expr
        tok = m.group(1)
    return int(tok) if tok.isdigit() else constant(tok)


def derive(row):
    """(block, cap, per_thread, the cap's constant or None, {call texts}) of one row, from the source"""
    body = function_body(row["launcher"])
    found = launches_of(body, row["kernel"])
    assert found, "%s does not launch %s" % (row["launcher"], row["kernel"])
    got, texts = set(), set()
    for grid, block in found:
        name, args = grid_call(grid, body)
        texts.add("%s(%s)" % (name, ", ".join(args)))
        if name == "score_blocks":
            sb = function_body("score_blocks")
            assert args == ["n"] and "(n + kScoreBlock - 1) / kScoreBlock" in sb and "kScoreMaxBlocks" in sb, sb
            assert block_of(block, body) == constant("kScoreBlock")
            got.add((constant("kScoreBlock"), constant("kScoreMaxBlocks"), 1, "kScoreMaxBlocks"))
            continue
        assert len(args) in (2, 3), args
        vec = re.fullmatch(r"\w+ / (\d+) \+ 1", args[0])
        assert vec or re.fullmatch(r"\w+", args[0]), "work items %r" % args[0]
        per_thread = int(vec.group(1)) if vec else 1
        assert int(args[1]) == block_of(block, body), "grid_for's block %s, the launch's %s" % (args[1], block)
        cap_name = None
        if len(args) == 2:
            m = re.search(r"^int grid_for\(size_t work_items, int block, int max_blocks = ([\d\s*]+)\)", SRC, re.M)
            assert m, "grid_for's default cap"
            cap = math.prod(int(t) for t in m.group(1).split("*"))
        elif args[2].isdigit():
            cap = int(args[2])
        else:
            cap_name = args[2]
            if not cap_name.startswith("k"):                                   # a parameter: clamped to a named constant
                m = re.search(r"\b%s = (k\w+);" % cap_name, body)
                assert m, "where %r comes from" % cap_name
                cap_name = m.group(1)
            cap = constant(cap_name)
        got.add((int(args[1]), cap, per_thread, cap_name))
    assert len(got) == 1, "the launches of %s disagree: %s" % (row["kernel"], got)
    return got.pop() + (texts,)


def call_sites():
    """{(enclosing function, call text)} of every grid_for( and score_blocks( call in dsi_kernels.hip"""
    sites = set()
    for m in re.finditer(r"\b(grid_for|score_blocks)\(", SRC):
        line_start = SRC.rfind("\n", 0, m.start()) + 1
        line = SRC[line_start:SRC.index("\n", m.start())]
        if "//" in line[:m.start() - line_start] or re.match(r"(static )?int (grid_for|score_blocks)\(", line):
            continue                                                           # a comment, or the definition itself
        owner = [f for f in FUNCTION.finditer(SRC, 0, m.start())][-1].group(1)
        args, _ = call_args(SRC, m.end() - 1)
        sites.add((owner, "%s(%s)" % (m.group(1), ", ".join(args))))
    return sites


# ------------------------------------------------------------------------------------------------- the round table
@pytest.mark.parametrize("name", sorted(gc.ROWS))
def test_row_is_what_the_launcher_says(name):
    row = gc.ROWS[name]
    block, cap, per_thread, cap_name, _ = derive(row)
    stated = (row["block"], row["cap"], row["per_thread"], row["cap_name"])
    assert (block, cap, per_thread, cap_name) == stated, "row %s: the source says %s, the table %s" % (
        name, (block, cap, per_thread, cap_name), stated)
    assert row["items"] == block * cap * per_thread
    if per_thread in (4, 8):                                                   # the scalar tail is block 0's
        assert "blockIdx.x == 0 && threadIdx.x < (n & %d)" % (per_thread - 1) in kernel_body(row["kernel"]), name
    if per_thread > 1:
        assert "n / %d" % per_thread in kernel_body(row["kernel"]), name


def test_every_capped_call_site_is_a_row():
    covered = set()
    for name, row in gc.ROWS.items():
        covered |= {(row["launcher"], t) for t in derive(row)[4]}
    sites = call_sites()
    assert sites - covered == set(), "capped launchers the table misses: %s" % sorted(sites - covered)
    assert covered - sites == set(), sorted(covered - sites)
    assert len([s for s in sites if s[1].startswith("score_blocks")]) == 4 and len(sites) == 18


def test_the_issue_s_items_per_round():
    items = {k: r["items"] for k, r in gc.ROWS.items()}
    assert items["voxelwise"] == items["slices_u8_z"] == 2_097_152 and items["fill"] == items["standardize"] == 524_288
    assert items["mean_square"] == items["vf_partials"] == 262_144 and items["grid_min_max"] == 1_048_576
    assert items["conf_minmax"] == 131_072 and all(items["score_" + k] == 131_072 for k in ("accumulate", "minmax", "histogram", "select"))
    assert items["event_image_count"] == 8_388_608
    # the rows other tests cover already: their largest exact input is past one round
    assert 346 * 260 * 20 > items["reduce_partials"] and 260 * 346 > items["image_conf_minmax"] > items["store_depth_map"]
    assert 346 * 260 > items["event_image_minmax"]
    assert gc.ROWS["scale"]["pinned_by"] is None                               # no production call reaches it
    body = function_body("launch_iir_axis")
    assert body.index("if (axis == 2) return") < body.index("k_scale") and "if (with_post)" in body


def test_shape_arithmetic():
    n = gc.VOL_N
    assert n == 127 * 131 * 127 == 2_112_899 == int(np.prod(gc.VOL_SHAPE)) and n & 3 == 3
    assert n - gc.round_of("voxelwise") == 15_747 and gc.rounds("voxelwise", n) == 2 and gc.rounds("slices_u8_z", n) == 2
    assert gc.rounds("grid_min_max", n) == 3 and -(-n // gc.round_of("mean_square")) == 9 and -(-n // gc.round_of("fill")) == 5
    assert gc.tail_start("voxelwise", n) == n - 3
    s = gc.STAT_N
    assert s == 67 * 89 * 89 == 530_707 == int(np.prod(gc.STAT_SHAPE)) and s & 3 == 3
    assert s - gc.round_of("standardize") == 6_419 and -(-s // gc.round_of("vf_partials")) == 3
    p = gc.IMG_N
    assert p == 362 * 363 == 131_406 and p & 3 == 2 and p - gc.round_of("conf_minmax") == 334 == 256 + 64 + 14
    assert p - gc.round_of("score_accumulate") == 334 and max(gc.SCORE_SPECIAL.values()) == 333
    assert 480 * 640 == 307_200 and -(-307_200 // gc.round_of("score_accumulate")) == 3
    e = gc.EVENTS_N
    assert e - gc.round_of("event_image_count") == 1031 and e & 7 == 7 and gc.tail_start("event_image_count", e) == e - 7


# ------------------------------------------------------------------------------------------------------ k_voxelwise
def regions(n, row):
    """(first round, second and later rounds of the vector body, scalar tail) as slices of the flat volume"""
    return slice(0, gc.round_of(row)), slice(gc.round_of(row), gc.tail_start(row, n)), slice(gc.tail_start(row, n), n)


def test_voxel_inputs_have_every_kind_in_every_region():
    a, g = gc.pair_volumes()
    first, second, tail = regions(gc.VOL_N, "voxelwise")
    for v in (a.ravel(), g.ravel()):
        for part in (first, second):
            assert (v[part] == 0).sum() > 1000 and (v[part] > 0).sum() > 1000
    assert (a.ravel()[::7] == 0).all() and (g.ravel()[::5] == 0).all()
    for kind, k in [(c[0], c[1]) for c in gc.VOXEL_CASES if c[0] in ("fuse2", "fuse2_into", "hm_n", "binary")]:
        ta, tg = (v.ravel()[tail] for v in gc.pair_inputs(kind, k))
        assert ((ta == 0) | (tg == 0)).any() and ((ta > 0) & (tg > 0)).any(), (kind, k)
    maps = gc.nary_volumes()
    kinds = (lambda v: v == 0, lambda v: v == F(1e-41), lambda v: v == F(3e37), lambda v: v == F(2.0 ** -20), np.isinf)
    for n_src in (2, 3, 4, 8):
        for kind in kinds:
            for part in (first, second, tail):
                assert any(kind(v.ravel()[part]).any() for v in maps[:n_src]), (n_src, part)
    assert np.isinf(maps[0]).sum() == 3 and not any(np.isinf(v).any() for v in maps[1:])


@pytest.mark.parametrize("case", gc.VOXEL_CASES, ids=gc.case_id)
def test_voxel_case_shows_both_faults(case):
    truth = gc.voxel_expected(case)
    _, steps = gc.voxel_steps(case)
    first, second, tail = regions(gc.VOL_N, "voxelwise")
    for row in sorted({s[0] for s in steps if s[0]}):
        faulty = gc.voxel_fields(case, gc.first_round_only, row)
        differs = np.zeros(gc.VOL_N, bool)
        for t, f in zip(truth, faulty):
            differs |= ~gc.same_bits(t, f).ravel()
        assert differs[gc.round_of(row):].sum() >= 1000 and not differs[:gc.round_of(row)].any(), (case, row)
    faulty = gc.voxel_fields(case, gc.without_tail, "voxelwise")
    differs = np.zeros(gc.VOL_N, bool)
    for t, f in zip(truth, faulty):
        differs |= ~gc.same_bits(t, f).ravel()
    assert differs[tail].all() and not differs[:gc.VOL_N - 3].any(), case


# ------------------------------------------------------------------------ min / max, slice images, mean square
def test_min_max_plantings_and_faults():
    n, R = gc.VOL_N, gc.round_of("grid_min_max")
    first, later, tail = regions(n, "grid_min_max")
    last_round = slice(2 * R, later.stop)
    v = gc.minmax_volume("tied").ravel()
    for value, spots in ((gc.MINMAX_LO, gc.MINMAX_TIED_LO), (gc.MINMAX_HI, gc.MINMAX_TIED_HI)):
        assert sorted(np.flatnonzero(v == value)) == sorted(spots)
        for part in (first, slice(R, 2 * R), last_round, tail):
            assert (v[part] == value).any()
    truth = gr.min_max(v)
    assert truth == (gc.MINMAX_LO, gc.MINMAX_HI, min(gc.MINMAX_TIED_LO), max(gc.MINMAX_TIED_HI)) and truth[3] == n - 2
    assert gc.min_max_seen(v, 0, R) != truth and gc.min_max_seen(v, 0, R)[3] == 40_002             # one round
    assert gc.min_max_seen(v, 0, n - 3) != truth and gc.min_max_seen(v, 0, n - 3)[3] == later.stop - 1   # no tail
    assert gc.min_max_seen(v, R, n)[2] != truth[2]                                                     # the first round's partials unread
    # a kernel that walks one round and still does its tail finds both: the first minimum is in its round, the last
    # maximum in its tail.  That is what the tie rule asks of the planting; "later" is the volume for that kernel
    assert gc.min_max_seen(v, 0, R, and_from=n - 3) == truth
    t = gc.minmax_volume("tail").ravel()
    truth = gr.min_max(t)
    assert truth == (gc.MINMAX_LO, gc.MINMAX_HI, n - 3, n - 1)
    for seen in (gc.min_max_seen(t, 0, R), gc.min_max_seen(t, 0, n - 3)):
        assert seen[0] != truth[0] and seen[1] != truth[1] and seen[2] != truth[2] and seen[3] != truth[3]
    u = gc.minmax_volume("later").ravel()
    truth = gr.min_max(u)
    assert truth == (gc.MINMAX_LO, gc.MINMAX_HI) + gc.MINMAX_LATER and R <= truth[2] < 2 * R <= truth[3] < later.stop
    assert truth[2] // 4 % (R // 4) // 256 >= 256                            # a partial the finishing block's first pass does not reach
    for seen in (gc.min_max_seen(u, 0, R), gc.min_max_seen(u, 0, R, and_from=n - 3)):
        assert seen[0] != truth[0] and seen[1] != truth[1] and seen[2] != truth[2] and seen[3] != truth[3]
    assert gc.min_max_seen(u, 0, n - 3) == truth                              # (its tail holds nothing: "tied" and "tail" are the volumes for that)


def test_slice_images_show_both_faults():
    """k_grid_slices_u8_z writes bytes; what an unwritten byte holds is whatever the output buffer held, which no restatement
    knows.  So this is an argument, not a proof: the expected bytes past the round are not one constant (0 and 255 are
    tried), and they differ from the other normalisation's bytes at the same places, which is what the buffer holds when
    check_slices_u8's two calls per orientation reuse it."""
    v = gc.slices_volume()
    first, second, tail = regions(gc.VOL_N, "slices_u8_z")
    lo, hi, lo_pos, hi_pos = gr.min_max(v)
    assert hi_pos == gc.VOL_N - 1 and lo == 0
    for by_minmax in (True, False):
        want = gr.slices_u8(v, 2, by_minmax).ravel()
        # bytes past the round, or of the tail, that are left as they were: whatever the buffer held, most differ
        for stale in (0, 255):
            assert (want[second] != stale).sum() >= 1000 and (want[tail] != stale).any()
        assert len(np.unique(want[tail])) > 1 or by_minmax
    both = [gr.slices_u8(v, 2, by_minmax).ravel() for by_minmax in (True, False)]
    assert (both[0][second] != both[1][second]).sum() >= 1000 and (both[0][tail] != both[1][tail]).any()
    # the extremes of k_grid_min_max that the by-min-max image is scaled with: one round, or no tail, changes every byte's scale
    assert gc.min_max_seen(v, 0, gc.round_of("grid_min_max"))[1] != hi and gc.min_max_seen(v, 0, gc.VOL_N - 3)[1] != hi
    # per slice: the last plane's own minimum is not the first plane's
    assert float(v[-1].min()) == 10.0 and float(v[0].min()) == 0.0


def test_mean_square_is_exact_and_shows_the_fault():
    v = gc.mean_square_volume("integers").ravel()
    sq = v.astype(np.float64) ** 2
    assert sq.sum() < 2 ** 53 and (sq == np.rint(sq)).all()                   # integers: every partial sum is exact
    truth = orc.mean_square(v)
    assert truth == float(sq.sum()) / v.size
    R = gc.round_of("mean_square")
    assert orc.mean_square(v[:R]) * R / v.size != truth
    w = gc.mean_square_volume("votes").ravel()
    truth = orc.mean_square(w)
    assert abs(orc.mean_square(w[:R]) * R / w.size - truth) > 1e-12 * truth    # the existing relative bound


# -------------------------------------------------------------------------------------------- mean, deviation, Moran
def test_mean_std_is_exact_and_shows_the_fault():
    v = gc.stat_volume("balanced").ravel()
    mean, std = vf.mean_std(v)
    d = v.astype(np.float64) - 3.0
    assert mean == 3.0 and (d == np.rint(d)).all() and std == math.sqrt(float((d * d).sum()) / v.size)
    R = gc.round_of("vf_partials")
    assert v[:R].astype(np.float64).sum() / v.size != mean                     # the sum of one round
    assert v[R:2 * R].astype(np.float64).sum() != v[2 * R:].astype(np.float64).sum()
    assert math.sqrt(float((d[:R] ** 2).sum()) / v.size) != std
    w = gc.stat_volume("votes").ravel()
    mean, std = vf.mean_std(w)
    part = w[:R].astype(np.float64)
    assert abs(part.sum() / w.size - mean) > 1e-10 * mean                      # the existing bounds
    assert abs(math.sqrt(((part - mean) ** 2).sum() / w.size) - std) > 1e-10 * std


def moran_with(v, keep_z=None, keep_t=None):
    """volume_filters_reference.moran's own steps, with the standardized values past keep_z left at zero (a scratch
    volume starts zeroed) and the terms past keep_t not summed; without either it must give moran()'s bits"""
    sigma, _, c = vf.moran_kernel(gc.MORAN_SIGMA)
    mean, std = vf.mean_std(v)
    z = ((v.astype(np.float64) - mean) * float(F(1.0 / std))).astype(F)
    if keep_z is not None:
        z.reshape(-1)[keep_z:] = 0
    s = vf.iir3(z, sigma, sigma, sigma, 3)
    t = (z * (s - c * z)).astype(np.float64).reshape(-1)
    denom = float(F(1) - c) * (float(v.size) - 1.0)
    return float(t[:keep_t].sum()) / (denom + 1e-6)


@pytest.mark.parametrize("name", ["smooth", "votes"])
def test_moran_shows_the_faults_beyond_its_bound(name):
    v = gc.stat_volume(name)
    truth, t, denom = gc.moran_reference(name)
    assert moran_with(v) == truth
    bound = gc.moran_bound(name)
    one_standardize_round = moran_with(v, keep_z=gc.round_of("standardize"))
    one_sum_round = moran_with(v, keep_t=gc.round_of("vf_partials"))
    assert abs(one_standardize_round - truth) > 1000 * bound and abs(one_sum_round - truth) > 1000 * bound
    if name == "smooth":
        assert truth > 0.8


# ------------------------------------------------------------------------------------------------ depth-map filters
COMPARED = ("confidence", "mask", "idx_filtered", "depth")                    # test_depthmap_filters.OUTPUTS


@pytest.mark.parametrize("name", ["high", "low"])
def test_filter_images_show_the_fault(name):
    conf, idx = gc.filter_image(name)
    R = gc.round_of("conf_minmax")
    flat = conf.ravel()
    assert ((conf > 0) | (idx == 0)).all() and int(idx.max()) < gc.FILTER_PLANES
    lo_at, hi_at = np.flatnonzero(flat == gc.FILTER_MIN), np.flatnonzero(flat == gc.FILTER_MAX)
    assert flat.min() == gc.FILTER_MIN and flat.max() == gc.FILTER_MAX and lo_at.size == hi_at.size == 2
    if name == "high":
        assert lo_at.min() == R and hi_at.min() > R and lo_at.max() == gc.IMG_N - 1
        seen = (0, R)                                                          # the second round is not seen
    else:
        assert lo_at.max() < R and hi_at.max() < R
        seen = (R, gc.IMG_N)                                                   # the mirrored fault: only the last round's values count
    for option in gc.FILTER_OPTIONS:
        assert 1.0 < option[3] < 20.0 and option[0] <= 15
        truth = gc.filter_reference(name, option)
        faulty = gc.filter_seen(name, option, *seen)
        assert (truth["mask"] != faulty["mask"]).sum() >= 100, (name, option)
        assert truth["mask"].sum() >= 100
        whole = gc.filter_seen(name, option, 0, gc.IMG_N)                      # the model itself: the whole range changes nothing
        assert all(np.array_equal(truth[k], whole[k]) for k in COMPARED)


# ------------------------------------------------------------------------------------------------------- the scorer
def score_fields(maps):
    m = sr.metrics(*maps, gc.SCORE_B, gc.SCORE_FOCAL)
    return {k: m[k] for k in ("n_est", "n_gt", "n_joint", "n_delta", "n_bad", "max_gt", "median_abs", "sum_abs")}


@pytest.mark.parametrize("where", ["second", "first"])
def test_score_plantings_and_faults(where):
    maps = gc.score_planted(where)
    R = gc.round_of("score_accumulate")
    t = sr.terms(*maps, gc.SCORE_B, gc.SCORE_FOCAL)
    err, ratio, bad = t["err"], t["ratio"], t["bad"]
    assert err.size == gc.IMG_N and t["est_valid"].all() and t["gt_valid"].all()          # every pixel joint: 131,406 stored errors
    home = slice(R, gc.IMG_N) if where == "second" else slice(0, R)
    away = slice(0, R) if where == "second" else slice(R, gc.IMG_N)
    inside = lambda i: home.start <= i < home.stop
    order = np.argsort(err, kind="stable")
    mid = order[gc.IMG_N // 2 - 1], order[gc.IMG_N // 2]
    assert inside(mid[0]) and inside(mid[1]) and (err[mid[0]], err[mid[1]]) == gc.SCORE_MID
    assert (err == err[mid[0]]).sum() == 1 and (err == err[mid[1]]).sum() == 1
    assert sr.median(err) == (gc.SCORE_MID[0] + gc.SCORE_MID[1]) / 2
    assert inside(int(err.argmin())) and (err == err.min()).sum() == 1 and err.min() == gc.Q
    assert inside(int(err.argmax())) and (err == err.max()).sum() == 1 and err.max() == 2.5
    gt = maps[2].ravel()
    assert inside(int(gt.argmax())) and (gt == gt.max()).sum() == 1
    th = sr.THRESHOLDS
    classes = {"delta1": ratio < th[0], "delta2 only": (ratio >= th[0]) & (ratio < th[1]), "delta3 only": (ratio >= th[1]) & (ratio < th[2]),
               "no delta": ratio >= th[2], "bad": bad}
    for name, member in classes.items():
        assert member[home].any(), name
        if name != "delta1":
            assert not member[away].any(), name                                # the other round holds plain pixels alone
    assert classes["delta1"][away].all() and (classes["bad"] & classes["delta1"]).any()
    # every term of sum_abs is a multiple of 2^-16 below 4: the float64 sum is exact in any order
    assert (err / gc.Q == np.rint(err / gc.Q)).all() and math.fsum(err) == float(np.sum(err)) < 2.0 ** 36 * gc.Q
    # the fault: k_score_accumulate sees the pixels of one round alone.  (The kernels that walk the stored errors have their
    # own layout, whose buffer order does not depend on the scheduler: test_score_stored_errors_show_the_fault.)
    truth = score_fields(maps)
    for seen in ((0, R), (R, gc.IMG_N)):
        faulty = score_fields(gc.score_maps_seen(maps, *seen))
        assert faulty["n_joint"] != truth["n_joint"] and faulty["sum_abs"] != truth["sum_abs"]
    faulty = score_fields(gc.score_maps_seen(maps, *((0, R) if where == "second" else (R, gc.IMG_N))))
    for k in ("n_delta", "n_bad", "max_gt", "median_abs"):
        assert faulty[k] != truth[k], k


@pytest.mark.parametrize("where", ["second", "first"])
def test_score_stored_errors_show_the_fault(where):
    """k_score_minmax, _histogram and _select walk the buffer of stored errors, whose order inside one add is the order in
    which waves reach an atomic.  Two adds fix it: the second add's errors lie behind the first's.  "second": the buffer's
    second round IS the second add, which holds the smallest, the largest and the two middle errors -- a kernel that stops
    after one round sees exactly the first add's errors.  "first" is the mirror: whatever lies past the round is a part of
    the second add, which holds plain errors alone -- a kernel that keeps only its last round sees none of the special ones."""
    R = gc.round_of("score_minmax")
    assert R == gc.round_of("score_histogram") == gc.round_of("score_select")
    adds = gc.score_adds(where)
    whole = gc.score_planted(where)
    for k in range(3):
        assert np.array_equal(np.concatenate([a[k] for a in adds]), whole[k].ravel())
    errs = [sr.terms(*a, gc.SCORE_B, gc.SCORE_FOCAL)["err"] for a in adds]
    err = np.concatenate(errs)
    assert [e.size for e in errs] == ([R, gc.IMG_N - R] if where == "second" else [gc.IMG_N - R, R]) and gc.IMG_N - R == 334
    assert np.array_equal(np.sort(err), np.sort(sr.terms(*whole, gc.SCORE_B, gc.SCORE_FOCAL)["err"]))
    special = np.array([gc.Q, 2.5, gc.SCORE_MID[0], gc.SCORE_MID[1]])
    assert all((err == v).sum() == 1 for v in special) and (err.min(), err.max()) == (gc.Q, 2.5)
    assert sr.median(err) == (gc.SCORE_MID[0] + gc.SCORE_MID[1]) / 2
    holder, plain = (errs[1], errs[0]) if where == "second" else (errs[0], errs[1])
    assert np.isin(special, holder).all() and not np.isin(special, plain).any()
    # "second": positions >= R hold the second add, so one round is `plain` exactly.  "first": positions >= R hold some 334
    # errors of `plain`; the bounds below hold for every subset of it
    assert plain.min() > gc.Q and plain.max() < 2.5                           # min / max: both extremes, hence both histogram edges
    if where == "second":
        assert sr.median(plain) != sr.median(err)                             # select: the ranks (n - 1) / 2, n / 2 of 131,072 errors
        for nb in gc.SCORE_HIST_BINS:
            bw = gc.histogram_binwidth(err, nb)
            counts, lo, hi = sr.histogram(err, bw)
            assert counts.size == nb and counts.sum() == gc.IMG_N and (lo, hi) == (gc.Q, 2.5) and (counts > 0).sum() > 50
            assert plain.size == R != counts.sum() and counts[0] >= 1 and counts[-1] >= 1   # histogram: the counts' sum, the end bins
    else:
        assert 334 < gc.IMG_N // 2 - 1                                         # select: 334 errors have no ranks (n - 1) / 2 and n / 2 of 131,406


def test_score_dsec_frame_shows_the_fault():
    maps = gc.score_dsec()
    R = gc.round_of("score_accumulate")
    truth = score_fields(maps)
    assert truth["n_joint"] > 50_000
    for rounds in (1, 2):
        faulty = score_fields(gc.score_maps_seen(maps, 0, rounds * R))
        assert all(faulty[k] != truth[k] for k in ("n_est", "n_gt", "n_joint", "n_bad", "median_abs", "sum_abs"))


# -------------------------------------------------------------------------------------------------- the event image
def test_event_image_plantings_and_faults():
    x, y, pol = gc.events()
    w, h = gc.SENSOR
    R, n = gc.round_of("event_image_count"), gc.EVENTS_N
    hot = (x == gc.HOT_PIXEL[0]) & (y == gc.HOT_PIXEL[1])
    last = (x == gc.TAIL_PIXEL[0]) & (y == gc.TAIL_PIXEL[1])
    assert hot[:R].sum() == gc.HOT_FIRST_ROUND == 256 and pol[hot].all() and hot[R:n - 7].sum() == 1024 - 1 and hot.sum() == 1279
    assert last[n - 7:].sum() == 6 == last.sum() and pol[last].all()
    outside = (x >= w) | (y >= h)
    assert outside[:R].any() and outside[R:n - 7].sum() == 1 and outside[n - 7:].sum() == 1 and outside[R - 1]
    counts, dropped = rr.event_counts(x, y, pol, w, h, True)
    plain, _ = rr.event_counts(x, y, pol, w, h, False)
    (hx, hy), (tx, ty) = gc.HOT_PIXEL, gc.TAIL_PIXEL
    assert counts[hy, hx] == 1279 == np.abs(counts).max() and (np.abs(counts) == 1279).sum() == 1 and counts[ty, tx] == 6
    wrapped = plain % 256
    assert wrapped[hy, hx] == 255 and (wrapped == 255).sum() == 1 and np.sort(wrapped.ravel())[-2] < 200 and dropped == outside.sum()
    assert wrapped[ty, tx] == 6 == wrapped.min() and np.sort(wrapped.ravel())[1] > 6
    # k_event_image_minmax walks the counters in rounds of 65,536 pixels: both extremes of both images lie past the first
    P = gc.round_of("event_image_minmax")
    assert hy * w + hx >= P and ty * w + tx >= P
    assert np.abs(counts.ravel()[:P]).max() < 1279 and wrapped.ravel()[:P].max() < 255 and wrapped.ravel()[:P].min() > 6
    for use_polarity in (True, False):
        truth, truth_dropped = gc.event_image_seen(use_polarity)
        for seen in ((0, R), (0, n - 7)):                                      # one round; no tail
            img, d = gc.event_image_seen(use_polarity, *seen)
            assert (img != truth).any() and d != truth_dropped, (use_polarity, seen)
