"""The reduce-scattered and the plane-sharded depth map for 1 to 9 (8) ranks, emulated one rank after another in ONE
process on ONE device: everything those paths run but the nccl* calls -- dsi::host::scatter_plan / plane_range,
scattered_local (finalize of an interior slab of the accumulator, k_collapse_max_z<Identity, 8> on it, k_pack_argmax with
combine), sharded_prepare (k_pack_argmax with plane_begin != 0) and k_unpack_argmax over the full depth vector.
The all-reduce(MAX) between ranks is np.maximum.reduce over the downloaded keys.  Every comparison is bit-exact.

Inputs (rank_partition_cases.py, checked on the CPU by test_rank_partitions_cpu.py): integer-valued accumulators,
so ties are the rule, with forced columns -- all zero, all equal, the maximum on the last plane, equal maxima on
plane 0 and the last plane, and equal maxima on planes b - 1 and b for every boundary b of the partition.  Planes a
rank does not own hold a poison whose finalized value beats all data: a rank that read one would pick it, a rank
that wrote one would change its bits.  Image sizes cover nx * ny mod 4 = 1, 2, 3, 0: with a plane that is no
multiple of 4 floats, a rank's slab starts off a 16-byte boundary (launch_finalize peels its head)."""
import numpy as np
import pytest

import rank_partition_cases as rpc

pytestmark = pytest.mark.gpu


def _ids(s):
    return "x".join(map(str, s))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mapper(d, ctx, shape, plane_range=None):
    nx, ny, nz = shape
    cam = (nx, ny, 40.0, 40.0, 0.5 * nx, 0.5 * ny)
    return d.MapperEMVS(ctx, cam, d.ShapeDSI(0, 0, nz, 1.0, 9.0, 0.0), plane_range=plane_range)


@pytest.fixture(scope="module")
def comm(ctx):
    import dvs_mcemvs_amd as d
    c = d.Comm(ctx, d.Comm.unique_id(), 1, 0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. reduce-scattered form
@pytest.mark.parametrize("mode", rpc.MODES)
@pytest.mark.parametrize("shape", rpc.SHAPES, ids=_ids)
def test_emulated_ranks_reduce_scattered_depth_map(ctx, shape, mode):
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import engine
    from oracle import oracle as orc
    assert (d.ACC_SUM, d.ACC_INV_SUM, d.ACC_LOG_SUM, d.ACC_SQ_SUM, d.ACC_MIN, d.ACC_MAX) == rpc.MODES
    nx, ny, nz = shape
    m = _mapper(d, ctx, shape)
    g = d.Grid3D(ctx, nx, ny, nz)
    planes = m.raw_depths_vec_
    assert planes.shape == (nz,)
    reached = 0
    for n in rpc.RANKS:
        score, cols = rpc.score_volume(shape, rpc.scatter_boundaries(nz, n), seed=n)
        acc = rpc.accumulator(score, cols, mode)
        for n_maps in rpc.N_MAPS:
            where = "%d ranks, mode %d, %d maps" % (n, mode, n_maps)
            # the references: the whole-grid path of the engine and the oracle, on the unpoisoned accumulator
            fin = orc.finalize(acc, mode, n_maps)
            oconf, oidx = orc.collapse_max_z(fin)
            g.upload(acc)
            g.finalize(mode, n_maps)
            assert np.array_equal(_u32(g.download()), _u32(fin)), where
            m.computeDepthMap(g)
            wdepth, wconf, widx = m.fetchDepthMap()
            assert np.array_equal(widx, oidx) and np.array_equal(_u32(wconf), _u32(oconf)), where
            keys = []
            for r in range(n):
                sp = engine.scatter_plan(nz, n, r)
                assert sp == rpc.restated_plan(nz, n, r)
                own = rpc.owned_planes(nz, n, r)
                up = rpc.poisoned(acc, own, mode)
                g.upload(up)
                m.computeDepthMapScatteredLocal(g, n, r, mode, n_maps)
                k = m.argmaxKeys()
                after = g.download()
                # planes of other ranks: untouched down to their first and last element; own planes: finalized
                assert np.array_equal(_u32(after[~own]), _u32(up[~own])), "%s: rank %d wrote outside its planes" % (where, r)
                assert np.array_equal(_u32(after[own]), _u32(fin[own])), "%s: rank %d, its own planes" % (where, r)
                assert np.array_equal(k, rpc.rank_keys(fin, nz, n, r, orc.collapse_max_z)), "%s: rank %d, keys" % (where, r)
                keys.append(k)
            if nz // n == 0:                                    # q = 0: every rank owns the tail alone
                assert all(np.array_equal(k, keys[0]) for k in keys), where
            m.setArgmaxKeys(np.maximum.reduce(keys))            # the all-reduce(MAX)
            m.computeDepthMapFromKeys()
            depth, conf, idx = m.fetchDepthMap()
            assert np.array_equal(idx, widx) and np.array_equal(_u32(conf), _u32(wconf)), where
            assert np.array_equal(_u32(depth), _u32(wdepth)), where
            assert np.array_equal(idx, oidx) and np.array_equal(_u32(conf), _u32(oconf)), where
            assert np.array_equal(_u32(depth), _u32(planes[idx])), where
            for name, (p, first) in cols.items():               # forced ties: the smaller global plane
                assert idx.reshape(-1)[p] == first, "%s: column %s" % (where, name)
            # no poisoned plane was selected: the selected voxel holds legitimate finalized data
            picked = np.take_along_axis(fin, idx[None].astype(np.int64), axis=0)[0]
            assert np.array_equal(_u32(picked), _u32(conf)), where
            reached = max(reached, int(idx.max()))
    assert reached == nz - 1                                    # (255 for nz = 256: the whole 8-bit index)
    g.close()
    m.close()


# ------------------------------------------------------------------ 2. plane-sharded form
@pytest.mark.parametrize("shape", [(37, 21, 21), (9, 5, 256)], ids=_ids)
def test_emulated_ranks_plane_sharded_depth_map(ctx, comm, shape):
    """sharded_finish unpacks with launch_unpack_argmax's default clear = 0, so argmaxKeys() after
    computeDepthMapSharded still reads the keys k_pack_argmax built (one rank: the all-reduce is the identity)."""
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import distributed as dd, engine
    from oracle import oracle as orc
    nx, ny, nz = shape
    whole = _mapper(d, ctx, shape)
    gw = d.Grid3D(ctx, nx, ny, nz)
    for n in range(1, 9):
        ranges = dd.plane_ranges(nz, n)
        vol, cols = rpc.score_volume(shape, rpc.shard_boundaries(ranges), seed=100 + n)
        assert len(cols) == 4 + n - 1
        gw.upload(vol)
        whole.computeDepthMap(gw)
        wdepth, wconf, widx = whole.fetchDepthMap()
        oconf, oidx = orc.collapse_max_z(vol)
        assert np.array_equal(widx, oidx) and np.array_equal(_u32(wconf), _u32(oconf))
        keys = []
        for b, c in ranges:
            ms = _mapper(d, ctx, shape, plane_range=(b, c))
            assert ms.plane_begin == b and ms.dsi_.shape == (c, ny, nx)
            shard = d.Grid3D(ctx, nx, ny, c)
            shard.upload(vol[b:b + c])
            ms.computeDepthMapSharded(shard, comm)
            k = ms.argmaxKeys()
            sconf, sidx = shard.collapseMaxZSlice()
            assert np.array_equal(k, engine.argmax_keys_pack(sconf, sidx, b)), (n, b)
            rconf, ridx = orc.collapse_max_z(vol[b:b + c])
            assert np.array_equal(k, rpc.numpy_keys(rconf, ridx.astype(np.int64) + b)), (n, b)
            sdepth, sc, si = ms.fetchDepthMap()                 # one rank: its own shard's arg-max, global indices
            assert np.array_equal(si, ridx.astype(np.int64) + b) and np.array_equal(_u32(sc), _u32(rconf))
            assert np.array_equal(_u32(sdepth), _u32(whole.raw_depths_vec_[si]))
            keys.append(k)
            shard.close()
            ms.close()
        whole.setArgmaxKeys(np.maximum.reduce(keys))
        whole.computeDepthMapFromKeys()
        depth, conf, idx = whole.fetchDepthMap()
        assert np.array_equal(idx, widx) and np.array_equal(_u32(conf), _u32(wconf)) and np.array_equal(_u32(depth), _u32(wdepth))
        assert np.array_equal(idx, oidx) and np.array_equal(_u32(conf), _u32(oconf))
        for name, (p, first) in cols.items():
            assert idx.reshape(-1)[p] == first, (n, name)
    gw.close()
    whole.close()


def test_a_mapper_for_an_empty_plane_range_is_refused(ctx):
    """More ranks than planes: plane_ranges gives the surplus ranks (nz, 0).  A mapper's plane_count 0 means "all
    planes from plane_begin on", so such a rank must not get a mapper at all: dsi_mapper_create refuses plane_begin
    == dimZ with DSI_ERR_INVALID ("plane range must lie inside [0, dimZ)")."""
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import distributed as dd, engine
    shape = (13, 7, 3)
    ranges = dd.plane_ranges(3, 5)
    assert ranges == [(0, 1), (1, 1), (2, 1), (3, 0), (3, 0)]
    for b, c in ranges:
        if c:
            _mapper(d, ctx, shape, plane_range=(b, c)).close()
            continue
        with pytest.raises(d.DsiError) as e:
            _mapper(d, ctx, shape, plane_range=(b, c))
        assert e.value.code == engine.ERR_INVALID and "plane range must lie inside" in str(e.value)


# ------------------------------------------------------------------ 3. the key word at its edges
@pytest.mark.parametrize("plane_begin", [0, 1, 128, 255])
def test_device_keys_equal_host_keys_at_the_edges_of_the_word(ctx, comm, plane_begin):
    """Confidence 0, a denormal, 1, the largest finite float and +inf on the first and on the last local plane of a
    shard of a 256-plane depth vector (global planes 0 .. 255).  Negative values, -0.0 and NaN are left out: the key's
    precondition is "DSI values are >= 0 and never -0.0" (csrc/dsi_host.hpp:210)."""
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import engine
    nx, ny, nz = 9, 5, 256
    count = nz - plane_begin
    values = np.array([0.0, 1e-41, 1.0, np.finfo(np.float32).max, np.inf], np.float32)
    assert 0 < values[1] < np.finfo(np.float32).tiny
    vol = np.zeros((count, ny * nx), np.float32)
    want_conf = np.zeros(ny * nx, np.float32)
    want_idx = np.zeros(ny * nx, np.uint8)                      # (the untouched columns: all zero -> local plane 0)
    for j, v in enumerate(values):
        for k, local in enumerate((0, count - 1)):
            p = 3 + 4 * j + k
            vol[:, p] = 0.5 * v if np.isfinite(v) else 1.0      # below the maximum (0 for 0 and, rounded, the denormal's half)
            vol[local, p] = v
            want_conf[p] = v
            want_idx[p] = local if v > 0 else 0                 # an all-zero column: the first plane
    assert (vol.max(axis=0) == want_conf).all() and (vol.argmax(axis=0) == want_idx).all()
    m = _mapper(d, ctx, (nx, ny, nz), plane_range=(plane_begin, count))
    shard = d.Grid3D(ctx, nx, ny, count)
    shard.upload(vol.reshape(count, ny, nx))
    m.computeDepthMapSharded(shard, comm)
    keys = m.argmaxKeys().reshape(-1)
    host = engine.argmax_keys_pack(want_conf, want_idx, plane_begin)
    assert np.array_equal(keys, host)
    assert np.array_equal(keys, rpc.numpy_keys(want_conf, want_idx.astype(np.int64) + plane_begin))
    gidx = want_idx.astype(np.int64) + plane_begin
    assert gidx.min() == plane_begin and gidx.max() == 255
    depth, conf, idx = m.fetchDepthMap()
    assert np.array_equal(_u32(conf).reshape(-1), _u32(want_conf)) and np.array_equal(idx.reshape(-1), gidx)
    # and through an unsharded mapper's unpack
    whole = _mapper(d, ctx, (nx, ny, nz))
    whole.setArgmaxKeys(keys.reshape(ny, nx))
    whole.computeDepthMapFromKeys()
    depth2, conf2, idx2 = whole.fetchDepthMap()
    assert np.array_equal(_u32(conf2).reshape(-1), _u32(want_conf)) and np.array_equal(idx2.reshape(-1), gidx)
    assert np.array_equal(_u32(depth2), _u32(whole.raw_depths_vec_[idx2])) and np.array_equal(_u32(depth), _u32(depth2))
    assert np.array_equal(whole.argmaxKeys().reshape(-1), keys)     # the unpack leaves the keys as they were
    for o in (whole, shard, m):
        o.close()
