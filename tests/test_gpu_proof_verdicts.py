"""The per-column proof pass, every verdict against a restatement (proof_reference.py, pinned on the CPU by
test_proof_reference_cpu.py): k_tie_prove, k_tie_prove_n, k_prove_columns, k_interval_of_counts, k_interval_widen and
k_tie_votes_of behind proveNearTies, proveNearTiesN, proveColumns, referenceInterval and widen_interval.

The kernels are pure functions of (DSI values, counted votes, rel_gap, op) in IEEE double and float without contraction, so
every comparison here is exact: the unproven columns and their gaps as sorted (pixel, float bits) pairs -- their order on the
device is an atomic's --, the counters, gap_needed's bits and max_votes.  Natural DSIs use at most half of an interval's width
and cannot see a proof that proves a little too much; part C overwrites chosen columns so that a verdict hangs on one fp32
step (proof_cases.py), and asserts first that these inputs tell every listed fault from the rule."""
import numpy as np
import pytest

import dvs_mcemvs_amd as d
from dvs_mcemvs_amd import engine, synthetic as syn
from oracle import oracle as orc
from oracle_pipeline import OracleMapper

import proof_cases as pc
import proof_reference as pr

pytestmark = pytest.mark.gpu
F32 = np.float32
GAPS = (1e-7, 2.5e-4, 1e-2)


class Rig:
    """n cameras' mappers with their DSIs built, the DSIs on the host, and every voxel's counted votes (proofVotes)."""

    def __init__(self, ctx, nx, ny, nz, events, seed, n_cams, n_points):
        self.nx, self.ny, self.nz, self.npix, self.n = nx, ny, nz, nx * ny, n_cams
        self.rig = syn.stereo_rig(events, width=nx, height=ny, duration=0.3, seed=seed, n_cams=n_cams, n_points=n_points)
        self.shape = d.ShapeDSI(0, 0, nz, 4.0, 200.0, 0.0)
        self.batches = []
        for c in range(n_cams):
            first, Rt = d.packetize(self.rig["events"][c][2], self.rig["trajectories"][c], self.rig["T_rv_w"])
            self.batches.append(d.EventBatch(ctx, self.rig["events"][c][0], self.rig["events"][c][1], Rt, first))
        self.ms = [d.MapperEMVS(ctx, self.rig["cam"], self.shape) for _ in range(n_cams)]
        for m, b in zip(self.ms, self.batches):
            m.evaluateDSI_batch(b)
        self.out = d.MapperEMVS(ctx, self.rig["cam"], self.shape)
        self.dsis = [m.dsi_.download() for m in self.ms]
        self.voxels = np.arange(nx * ny * nz, dtype=np.uint32)
        if n_cams == 2:
            self.out.proveNearTies(self.ms, self.batches, d.FUSE_HM, rel_gap=1e-7)
        else:
            self.out.dsi_.setToFusionOfN([m.dsi_ for m in self.ms], d.ACC_MAX)
            self.out.proveNearTiesN(self.ms, self.batches, d.ACC_MAX, rel_gap=1e-7)
        self.counts = [self.votes(c) for c in range(n_cams)]
        for c in self.counts:
            c.setflags(write=False)
        for v in self.dsis:
            v.setflags(write=False)

    def votes(self, camera):
        return self.out.proofVotes(camera, self.voxels).reshape(self.nz, self.ny, self.nx)

    def restore(self):
        for m, v in zip(self.ms, self.dsis):
            m.dsi_.upload(v)

    def close(self):
        for o in self.ms + [self.out] + self.batches:
            o.close()


@pytest.fixture(scope="module")
def two(ctx):
    """The rig of test_gpu_exact_ties.py: 96 x 72 x 32, 150 k events per camera (27 workgroups of columns, border columns)."""
    r = Rig(ctx, 96, 72, 32, 150_000, 11, 2, 700)
    yield r
    r.close()


@pytest.fixture(scope="module")
def eight(ctx):
    r = Rig(ctx, 64, 48, 12, 20_000, 13, 8, 600)
    yield r
    r.close()


def assert_verdict(info, mapper, verdict, what, max_votes=None):
    """Everything the ABI reports of a proof against the restated verdict."""
    s = pr.summary(verdict)
    pixels, gap_bits = pr.sorted_pairs(*mapper.proofUnproven())
    assert info["columns"] == s["columns"], what
    assert np.array_equal(pixels, s["pixels"]), "%s: %d columns unproven on the device, %d restated; first difference at pixel %s" % (
        what, pixels.size, s["pixels"].size, np.setxor1d(pixels, s["pixels"])[:1])
    assert np.array_equal(gap_bits, s["gap_bits"]), "%s: %d gaps differ" % (what, int((gap_bits != s["gap_bits"]).sum()))
    assert (info["columns_proven"], info["columns_unproven"]) == (s["columns_proven"], s["columns_unproven"]), what
    assert int(pr.bits(F32(info["gap_needed"])).reshape(-1)[0]) == s["gap_needed_bits"], what
    assert info["max_votes"] == (s["max_votes"] if max_votes is None else max_votes), what
    return s


# ---- A. proveColumns on hand-made grids ----
@pytest.mark.parametrize("nx,ny,nz", [(37, 11, 5), (37, 11, 1), (3, 2, 256)])
def test_prove_columns_on_hand_made_grids(ctx, two, nx, ny, nz):
    """407 columns are one full and one partial workgroup; 3 x 2 x 256 is the deepest column the engine takes.  Every
    hand-made kind (equal maxima, hi == the winner's lo, v == thr and one fp32 below, an all-zero column, the floor, hi = +inf,
    hi = NaN, lo = 0) at pixel 0, on either side of the workgroup boundary and at the last pixel; random columns elsewhere."""
    scratch = d.MapperEMVS(ctx, two.rig["cam"], d.ShapeDSI(nx, ny, nz, 4.0, 200.0, 0.0))
    grids = [d.Grid3D(ctx, nx, ny, nz) for _ in range(3)]
    kinds = len(pc.hand_columns(nz, 2.5e-4))
    seen = set()
    for rotate in range(kinds):
        for rel_gap in (2.5e-4,) if rotate else GAPS:
            fused, lo, hi, expect = pc.hand_grid(nx, ny, nz, rel_gap, seed=rotate, rotate=rotate)
            for g, v in zip(grids, (fused, lo, hi)):
                g.upload(v)
            info = scratch.proveColumns(*grids, rel_gap=rel_gap)
            what = "%dx%dx%d rotate %d gap %g" % (nx, ny, nz, rotate, rel_gap)
            assert_verdict(info, scratch, pr.prove_columns(fused, lo, hi, rel_gap), what, max_votes=0)   # no referenceInterval ran
            pixels, gaps = scratch.proofUnproven()
            got = dict(zip(pixels.tolist(), pr.bits(gaps).tolist()))
            for p, (kind, proven, need) in expect.items():        # and against the verdicts written by hand
                assert (p not in got) == proven, (what, p, kind)
                assert proven or got[p] == int(pr.bits(need).reshape(-1)[0]), (what, p, kind)
                seen.add((p, kind))
    assert len(seen) == kinds * len({0, 255, 256, nx * ny - 1} & set(range(nx * ny)))
    for o in grids + [scratch]:
        o.close()


# ---- B. natural DSIs, whole image ----
@pytest.mark.parametrize("op", range(7))
def test_prove_near_ties_equals_the_restatement(two, op):
    k = 1 if op == 0 else 2
    for rel_gap in GAPS:
        info = two.out.proveNearTies(two.ms[:k], two.batches[:k], op, rel_gap=rel_gap)
        v = pr.prove_two(two.dsis[0], two.dsis[1], two.counts[0], two.counts[1], op, rel_gap)
        s = assert_verdict(info, two.out, v, "op %d gap %g" % (op, rel_gap))
        assert info["rel_gap"] == F32(rel_gap)
        if rel_gap == 1e-7:
            assert s["columns_unproven"] > 0 and s["columns_proven"] > 0     # both verdicts occur
    for c in range(k):                                                       # the counts this file restates from are this call's
        assert np.array_equal(two.votes(c), two.counts[c])


@pytest.mark.parametrize("mode,n", [(m, n) for m in (pr.SUM, pr.MIN, pr.MAX) for n in (1, 3, 4)] + [(pr.GM_TREE, n) for n in (2, 4, 8)])
def test_prove_near_ties_n_equals_the_restatement(ctx, eight, mode, n):
    assert (d.ACC_SUM, d.ACC_MIN, d.ACC_MAX, d.ACC_GM_TREE) == (pr.SUM, pr.MIN, pr.MAX, pr.GM_TREE)
    fused = d.Grid3D(ctx, eight.nx, eight.ny, eight.nz)
    fused.setToFusionOfN([m.dsi_ for m in eight.ms[:n]], mode)
    values = fused.download()
    for rel_gap in GAPS:
        info = eight.out.proveNearTiesN(eight.ms[:n], eight.batches[:n], mode, fused_grid=fused, rel_gap=rel_gap)
        v = pr.prove_n(values, eight.dsis[:n], eight.counts[:n], mode, rel_gap)
        s = assert_verdict(info, eight.out, v, "mode %d n %d gap %g" % (mode, n, rel_gap))
        assert s["columns_proven"] > 0                # (with few votes a mode may leave no column open: part C supplies them)
    for c in range(n):
        assert np.array_equal(eight.votes(c), eight.counts[c])
    fused.close()


# ---- C. steered columns ----
class Doubled:
    """Four cameras for the n-ary steering: the two cameras' batches, each voted into two mappers.  A column with planes that
    NO camera voted for (the `zero` and `floor` kinds) and voted corner columns do not occur together in four independent
    synthetic cameras; the proof is a function of the values and the counts alone, and the values are overwritten."""

    def __init__(self, ctx, two):
        self.two, self.nx, self.ny, self.nz = two, two.nx, two.ny, two.nz
        self.own = [d.MapperEMVS(ctx, two.rig["cam"], two.shape) for _ in range(3)]
        self.ms, self.out = two.ms + self.own[:2], self.own[2]
        self.batches = two.batches * 2
        for m, b in zip(self.own[:2], two.batches):
            m.evaluateDSI_batch(b)
        self.dsis, self.counts = two.dsis * 2, two.counts * 2
        for c in range(2):
            assert np.array_equal(self.own[c].dsi_.download(), two.dsis[c])

    def restore(self):
        for m, v in zip(self.ms, self.dsis):
            m.dsi_.upload(v)


@pytest.fixture(scope="module")
def four(ctx, two):
    r = Doubled(ctx, two)
    yield r
    for o in r.own:
        o.close()


def check_steered(rule, plan, vols, counts, verdict, pixels, gap_bits, fused=None):
    """The plan's preconditions on the REAL counts (asserted, never skipped), the listed faults' visibility on these very
    volumes, and the device's verdict on the flip / below columns spelled out (assert_verdict compares the whole image)."""
    kinds = pc.check_plan(rule, plan, vols, verdict)
    assert kinds["flip"] >= 32 and kinds["below"] >= 32, kinds
    for fault in rule.faults:
        assert pc.detects(rule, vols, counts, 1e-7, verdict, fault, fused=fused), "the steered columns cannot see %s (%r)" % (fault, kinds)
    got = dict(zip(pixels.tolist(), gap_bits.tolist()))
    nz = vols[0].shape[0]
    value = rule.engine([v.reshape(nz, -1) for v in vols]) if fused is None else fused.reshape(nz, -1)
    best = verdict["best"].reshape(-1)
    for p, kind, zc in zip(plan["pixels"].tolist(), plan["kinds"].tolist(), plan["zc"].tolist()):
        if kind == "flip":
            assert got.get(p) == int(pr.bits(F32((best[p] - value[zc, p]) / best[p])).reshape(-1)[0]), (p, kind)
        elif kind == "below":
            assert p not in got, (p, kind)


@pytest.mark.parametrize("op,steer", [(0, 0)] + [(op, s) for op in range(1, 7) for s in (0, 1)])
def test_steered_columns_flip_where_the_restatement_says(two, op, steer):
    rule = pc.TwoRule(op)
    k = rule.k
    try:
        vols, plan = pc.steer(rule, two.dsis[:k], two.counts[:k], 1e-7, steer=steer, seed=10 * op + steer)
        for c in range(k):
            two.ms[c].dsi_.upload(vols[c])
        info = two.out.proveNearTies(two.ms[:k], two.batches[:k], op, rel_gap=1e-7)
        for c in range(k):
            assert np.array_equal(two.votes(c), two.counts[c])
        verdict = rule.prove(vols, two.counts[:k], 1e-7)
        pixels, gap_bits = pr.sorted_pairs(*two.out.proofUnproven())
        check_steered(rule, plan, vols, two.counts[:k], verdict, pixels, gap_bits)
        assert_verdict(info, two.out, verdict, "steered op %d camera %d" % (op, steer))
    finally:
        two.restore()


@pytest.mark.parametrize("mode", [pr.SUM, pr.GM_TREE])
def test_steered_columns_flip_where_the_restatement_says_n(four, mode):
    rule = pc.NRule(mode, 4)
    voxels = np.arange(four.nx * four.ny * four.nz, dtype=np.uint32)
    try:
        for steer in (0, 3):
            vols, plan = pc.steer(rule, four.dsis, four.counts, 1e-7, steer=steer, seed=mode + steer)
            for c in range(4):
                four.ms[c].dsi_.upload(vols[c])
            four.out.dsi_.setToFusionOfN([m.dsi_ for m in four.ms], mode)
            fused = four.out.dsi_.download()
            info = four.out.proveNearTiesN(four.ms, four.batches, mode, rel_gap=1e-7)
            for c in range(4):
                assert np.array_equal(four.out.proofVotes(c, voxels).reshape(fused.shape), four.counts[c])
            verdict = rule.prove(vols, four.counts, 1e-7, fused=fused)
            pixels, gap_bits = pr.sorted_pairs(*four.out.proofUnproven())
            check_steered(rule, plan, vols, four.counts, verdict, pixels, gap_bits, fused=fused)
            assert_verdict(info, four.out, verdict, "steered mode %d camera %d" % (mode, steer))
    finally:
        four.restore()


# ---- D. interval grids ----
def test_reference_interval_grids_bit_for_bit(ctx, two):
    lo, hi = d.Grid3D(ctx, two.nx, two.ny, two.nz), d.Grid3D(ctx, two.nx, two.ny, two.nz)
    for c in range(2):
        two.out.referenceInterval(two.ms[c], two.batches[c], lo, hi)
        want_lo, want_hi = pr.interval_grids(two.dsis[c], two.counts[c])
        assert np.array_equal(pr.bits(lo.download()), pr.bits(want_lo)), "camera %d lo" % c
        assert np.array_equal(pr.bits(hi.download()), pr.bits(want_hi)), "camera %d hi" % c
    # max_votes of the proof that follows: the largest count the interval kernels saw (both cameras' here)
    info = two.out.proveColumns(two.ms[1].dsi_, lo, hi, rel_gap=1e-5)
    assert info["max_votes"] == max(int(two.counts[0].max()), int(two.counts[1].max())) > 1000
    assert_verdict(info, two.out, pr.prove_columns(two.dsis[1], want_lo, want_hi, 1e-5), "camera 1 against its own interval",
                   max_votes=info["max_votes"])
    again = two.out.proveColumns(two.ms[1].dsi_, lo, hi, rel_gap=1e-5)
    assert again["max_votes"] == 0                                  # no referenceInterval since the last proof
    for o in (lo, hi):
        o.close()


@pytest.mark.parametrize("k", [1, 8, 4096])
def test_widen_interval_bit_for_bit(ctx, k):
    nx, ny, nz = 37, 11, 5                                          # 2035 voxels: seven full workgroups and a partial one
    rng = np.random.default_rng(k)
    special = np.array([0.0, -0.0, 1e-45, 2e-45, np.finfo(F32).tiny, np.finfo(F32).max, np.inf, 1.0, 3.3, 1e-20, 7e37], F32)
    a = (2.0 ** rng.uniform(-140, 127, (nz, ny, nx))).astype(F32)
    b = (2.0 ** rng.uniform(-140, 127, (nz, ny, nx))).astype(F32)
    a.reshape(-1)[:44] = np.tile(special, 4)
    a.reshape(-1)[-11:] = special
    b.reshape(-1)[:44] = np.tile(special[::-1], 4)
    b.reshape(-1)[-11:] = special
    lo, hi = d.Grid3D(ctx, nx, ny, nz), d.Grid3D(ctx, nx, ny, nz)
    lo.upload(a)
    hi.upload(b)
    engine.widen_interval(lo, hi, k)
    want_lo, want_hi = pr.widen(a, b, k)
    assert np.array_equal(pr.bits(lo.download()), pr.bits(want_lo))
    assert np.array_equal(pr.bits(hi.download()), pr.bits(want_hi))
    for o in (lo, hi):
        o.close()


# ---- E. the proof and the resolver share one threshold ----
@pytest.mark.parametrize("rel_gap", [1e-7, 2.5e-4, 0.05])
def test_no_plane_is_neither_resummed_nor_bounded(ctx, two, rel_gap):
    """nearTieVoxels (what the resolver re-sums) is the restated {v >= thr} of the columns with two or more such planes; in every
    other non-empty column that set is the maximum alone; and the planes the proof bounds (its restatement, equal to the device's
    in part B) are exactly the others."""
    for name, grid, values in (("camera 0", two.ms[0].dsi_, two.dsis[0]), ("hm", None, None)):
        if grid is None:
            grid = d.Grid3D(ctx, two.nx, two.ny, two.nz)
            grid.setToFusionOf(two.ms[0].dsi_, two.ms[1].dsi_, d.FUSE_HM)
            values = grid.download()
            assert np.array_equal(values, pr.engine_value(d.FUSE_HM, two.dsis[0], two.dsis[1]))
        voxels, n_columns = two.out.nearTieVoxels(grid, rel_gap=rel_gap)
        v = values.reshape(two.nz, -1)
        best, zbest = pr._first_maximum(v, None)
        thr = best - F32(rel_gap) * best
        within = (v >= thr) & (best > 0)
        several = within.sum(0) >= 2
        want = np.flatnonzero((within & several).reshape(-1)).astype(np.uint32)
        assert n_columns == int(several.sum()), name
        assert n_columns > 0 or rel_gap < 1e-6, name
        assert np.array_equal(np.sort(voxels), want), name
        alone = (best > 0) & ~several
        assert np.all(within.sum(0)[alone] == 1) and np.all(np.argmax(within, 0)[alone] == zbest[alone])
        if name == "camera 0":
            bounded = pr.prove_two(values, None, two.counts[0], None, 0, rel_gap)["below"].reshape(two.nz, -1)
        else:
            bounded = pr.prove_two(two.dsis[0], two.dsis[1], two.counts[0], two.counts[1], d.FUSE_HM, rel_gap)["below"].reshape(two.nz, -1)
        assert np.array_equal(bounded, ~within & (best > 0)), name
        if grid is not two.ms[0].dsi_:
            grid.close()


# ---- F. the claim itself, against the oracle ----
@pytest.fixture(scope="module")
def oracle_dsis(two):
    out = []
    for c in range(2):
        r = OracleMapper(two.rig["cam"], dimX=two.nx, dimY=two.ny, dimZ=two.nz, min_depth=4.0, max_depth=200.0)
        assert r.evaluateDSI(two.rig["events"][c], two.rig["trajectories"][c], two.rig["T_rv_w"])
        out.append(r.dsi)
    return out


@pytest.mark.parametrize("op", [0, d.FUSE_HM, d.FUSE_MIN])
def test_a_proven_column_holds_in_the_reference_order(two, oracle_dsis, op):
    """What `proven` promises (README: value_proven): in the reference's own arithmetic -- fp32, event order, its fusion op --
    every plane below the resolver's threshold is STRICTLY below the plane the engine picked.  Checked on every proven column
    directly, not through the resolver's map."""
    k = 1 if op == 0 else 2
    info = two.out.proveNearTies(two.ms[:k], two.batches[:k], op)              # the default gap
    assert info["rel_gap"] == F32(2.5e-4)
    pixels, _ = two.out.proofUnproven()
    proven = np.ones(two.npix, bool)
    proven[pixels] = False
    v = pr.engine_value(op, two.dsis[0], two.dsis[1]).reshape(two.nz, -1)
    best, zbest = pr._first_maximum(v, None)
    below = (v < best - F32(2.5e-4) * best) & (best > 0)
    R = (oracle_dsis[0] if op == 0 else orc.fuse2(oracle_dsis[0].copy(), oracle_dsis[1], op)).reshape(two.nz, -1)
    at_winner = np.take_along_axis(R, zbest[None], 0)[0]
    wrong = below & proven[None] & ~(R < at_winner[None])
    assert proven.sum() > 0.9 * two.npix and below[:, proven].sum() > 10 * two.npix
    assert not wrong.any(), "%d planes of proven columns reach the winner in the reference's order" % int(wrong.sum())


# ---- G. borders of the counts ----
def test_counted_votes_on_every_border_voxel(two):
    """tie_votes_of's x > 0 and y > 0 branches: proofVotes against the resolver's own event pass (exactVoxels: an independent
    kernel) on EVERY voxel of the first and last row and column of three planes."""
    nx, ny, nz = two.nx, two.ny, two.nz
    y, x = np.mgrid[0:ny, 0:nx]
    border = np.flatnonzero(((y == 0) | (y == ny - 1) | (x == 0) | (x == nx - 1)).reshape(-1))
    vox = np.concatenate([z * nx * ny + border for z in (0, nz // 2, nz - 1)]).astype(np.uint32)
    two.out.proveNearTies(two.ms, two.batches, d.FUSE_HM, rel_gap=1e-7)
    for c in range(2):
        got = two.out.proofVotes(c, vox)
        _, want = two.ms[c].exactVoxels(two.batches[c], vox)
        assert np.array_equal(got, want), "camera %d: %d of %d border counts differ" % (c, int((got != want).sum()), vox.size)
        assert np.array_equal(got, two.counts[c].reshape(-1)[vox])
        assert got.max() > 0
