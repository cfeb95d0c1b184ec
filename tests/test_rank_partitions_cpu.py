"""What test_gpu_rank_partitions.py relies on, without a GPU: the reduce-scatter partition (dsi::host::scatter_plan)
against an independent numpy restatement, its coverage / disjointness, and -- with the oracle and the key arithmetic
alone -- that the maximum of the per-rank keys over emulated ranks IS the unsharded collapseMaxZSlice on the very
inputs the GPU tests use (so a failure there is the device code's).  test_abi.py::test_partition_arithmetic_is_the_engines
checks the same functions at four depths and 1..8 ranks; here every depth 1..256 and 1..9 ranks."""
import numpy as np
import pytest

from dvs_mcemvs_amd import engine
from oracle import oracle as orc

import rank_partition_cases as rpc


def test_scatter_plan_is_the_restated_partition_and_covers_every_plane_once(built):
    for nz in range(1, 257):
        for n in rpc.RANKS:
            own = np.zeros(nz, int)
            covered = np.zeros(nz, bool)
            for r in range(n):
                sp = engine.scatter_plan(nz, n, r)
                assert sp == rpc.restated_plan(nz, n, r), (nz, n, r)
                own[sp["own_begin"]:sp["own_begin"] + sp["own_count"]] += 1
                covered |= rpc.owned_planes(nz, n, r)
                assert sp["own_begin"] + sp["own_count"] <= sp["tail_begin"] <= nz
                assert sp["tail_begin"] + sp["tail_count"] == nz and 0 <= sp["tail_count"] < n
            assert covered.all(), (nz, n)                       # own ranges + tail: every plane
            assert own.max() <= 1, (nz, n)                      # own ranges are disjoint ...
            q = nz // n
            assert (own[:q * n] == 1).all() and (own[q * n:] == 0).all()   # ... and stop where the tail begins
            if n > nz:                                          # more ranks than planes: every rank owns only the tail
                assert q == 0 and all(rpc.owned_planes(nz, n, r).all() for r in range(n))


def test_plane_ranges_leave_empty_ranges_at_the_end(built):
    """Plane sharding with more ranks than planes: the empty ranges begin at nz (what makes a mapper for them refused)."""
    from dvs_mcemvs_amd import distributed as dd
    for nz in (1, 3, 7):
        for n in range(nz + 1, 10):
            ranges = dd.plane_ranges(nz, n)
            assert [c for _, c in ranges] == [1] * nz + [0] * (n - nz)
            assert all(b == nz for b, c in ranges if c == 0)


def test_forced_columns_are_where_the_case_builder_says():
    for shape in rpc.SHAPES:
        nz = shape[2]
        for n in rpc.RANKS:
            bounds = rpc.scatter_boundaries(nz, n)
            assert len(bounds) == (0 if nz // n == 0 else n - 1 + (1 if nz % n else 0))
            score, cols = rpc.score_volume(shape, bounds, seed=n)
            assert set(cols) == {"zero", "equal", "last", "ends"} | {"b%d" % b for b in bounds}
            assert len({p for p, _ in cols.values()}) == len(cols)
            flat = score.reshape(nz, -1)
            assert flat.min() >= 0 and np.array_equal(flat, np.round(flat))
            for name, (p, first) in cols.items():
                col = flat[:, p]
                assert int(np.argmax(col)) == first, (shape, n, name)
                if name.startswith("b"):
                    b = int(name[1:])
                    assert col[b - 1] == col[b] == rpc.PEAK and (np.delete(col, [b - 1, b]) < rpc.PEAK).all()
            assert not flat[:, cols["zero"][0]].any() and cols["last"][0] == flat.shape[1] - 1 and cols["ends"][0] == 0


@pytest.mark.parametrize("shape", rpc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maximum_of_the_ranks_keys_is_the_unsharded_argmax(built, shape):
    nz = shape[2]
    for n in rpc.RANKS:
        score, cols = rpc.score_volume(shape, rpc.scatter_boundaries(nz, n), seed=n)
        for mode in rpc.MODES:
            acc = rpc.accumulator(score, cols, mode)
            for n_maps in rpc.N_MAPS:
                fin = orc.finalize(acc, mode, n_maps)
                # the key's precondition (dsi_host.hpp: values >= 0, never -0.0) holds for these inputs
                assert not np.signbit(fin).any() and not np.isnan(fin).any()
                conf, idx = orc.collapse_max_z(fin)
                keys = [rpc.rank_keys(fin, nz, n, r, orc.collapse_max_z) for r in range(n)]
                mconf, midx = rpc.numpy_unkeys(np.maximum.reduce(keys))
                assert np.array_equal(midx, idx), (n, mode, n_maps)
                assert np.array_equal(mconf.view(np.uint32), conf.view(np.uint32)), (n, mode, n_maps)
                for name, (p, first) in cols.items():           # the forced ties resolve to the smaller plane
                    assert idx.reshape(-1)[p] == first, (n, mode, n_maps, name)
                # every finalized poison beats every finalized datum (but the INV_SUM accumulator of 0: +inf)
                pfin = orc.finalize(np.float32([rpc.POISON[mode]]), mode, n_maps)[0]
                legit = fin[np.isfinite(fin)] if mode == rpc.ACC_INV_SUM else fin
                assert np.isfinite(pfin) and pfin > legit.max(), (mode, n_maps)
                if nz // n == 0:
                    assert all(np.array_equal(k, keys[0]) for k in keys)
                # the numpy key word is the engine's host key word
                sp = rpc.restated_plan(nz, n, n - 1)
                b, c = (sp["own_begin"], sp["own_count"]) if sp["own_count"] else (sp["tail_begin"], sp["tail_count"])
                sconf, sidx = orc.collapse_max_z(fin[b:b + c])
                assert np.array_equal(engine.argmax_keys_pack(sconf, sidx, b), rpc.numpy_keys(sconf, sidx.astype(int) + b))
