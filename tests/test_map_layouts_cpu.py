"""What test_gpu_map_layouts.py relies on, proven here without a GPU (tests/map_layout_cases.py): the scenes
of table A have the members of every class on both sides of slot 2^18 of a 2^19-slot table, so that no second round is empty;
the wide render covers pixels beyond 2^18 and in the last, partial workgroup; the chains fill one run of slots that crosses
the table's end; and keys that the chain lacks have their home inside that run."""
import numpy as np
import pytest

import map_eval_reference as eref
import map_layout_cases as lc
import map_merge_reference as mref
import world_map_reference as ref

CAP = 1 << lc.BIG_LOG2
ENOUGH = 50


def both_halves(keys, what):
    lo, hi = lc.halves(keys)
    assert lo.sum() >= ENOUGH and hi.sum() >= ENOUGH, (what, int(lo.sum()), int(hi.sum()))


def test_the_big_tables_never_grow():
    """the 3/4 rule at 2^19 slots, call by call (the points of a call count before they are merged into cells)"""
    for calls, rm in ((lc.dense_calls(), lc.dense_reference()), (lc.sparse_calls(), lc.sparse_reference())):
        occupied = mref.MergeReferenceMap(lc.LEAF)
        for pts, T in calls:
            assert mref.grown_capacity(CAP, len(occupied.keys), len(pts)) == (CAP, 0)
            assert occupied.integrate(pts, T) == 0
        assert np.array_equal(occupied.keys, rm.keys)


def test_the_dense_scene():
    rm = lc.dense_reference()
    assert len(rm.keys) == lc.DENSE_CELLS > lc.ROUND and lc.DENSE_CELLS % 256 != 0
    assert (rm.n == 1).all() and sorted(np.unique(rm.stamp).tolist()) == [1, 2] and rm.calls == 2
    both_halves(rm.keys, "cells")
    # every tile of 256 slots is some cell's home: the offsets of the export's compaction are all in use
    tiles = np.bincount(lc.home_slots(rm.keys, CAP) >> 8, minlength=CAP >> 8)
    assert len(tiles) == 2048 and tiles.min() >= 64
    # the cells the merges share with the sparse scene, on both sides
    shared = np.isin(lc.sparse_reference().keys, rm.keys)
    assert shared.sum() >= 2000 and (~shared).sum() >= 2000
    both_halves(lc.sparse_reference().keys[shared], "shared")
    both_halves(lc.sparse_reference().keys[~shared], "new")
    both_halves(rm.keys[np.isin(rm.keys, lc.sparse_reference().keys)], "shared, in the dense table")
    # the states that the import refuses name each counter's word, and only cells of the second round are bad
    whole = rm.export_state()
    for counter, word, state in lc.second_round_bad_states(whole):
        differs = np.zeros(lc.DENSE_CELLS, bool)
        for k in ("keys", "n", "windows", "stamp"):
            differs |= state[k] != whole[k]
        differs |= (state["S"] != whole["S"]).any(axis=1)
        assert np.array_equal(np.flatnonzero(differs), np.sort(lc.BAD_INDICES)) and differs[:lc.ROUND].sum() == 0
        with pytest.raises(mref.Refused) as e:
            mref.MergeReferenceMap(lc.LEAF).import_state(state)
        assert e.value.args[0] == word, counter


def test_the_sparse_scene_has_every_class_in_both_halves():
    rm = lc.sparse_reference()
    assert 3000 <= len(rm.keys) <= 20000 and rm.calls == 5
    assert sorted(np.unique(rm.windows).tolist()) == [1, 2, 3, 4, 5]
    for mp, mw in lc.EXTRACT_FILTERS:
        both_halves(rm.extract(mp, mw)["keys"], ("filter", mp, mw))
    # the render's classes: the restatement run on the cells of one half gives the members of each class in that half
    for splat, mw in lc.RENDER_CASES:
        cells = rm.extract(1, mw)
        for half in lc.halves(cells["keys"]):
            r = lc.rref.render(lc.subset(cells, half), *lc.SMALL_VIEW, splat=splat)
            assert min(r["n_drawn"], r["n_clipped"], r["n_outside"]) >= ENOUGH, (splat, mw, r["n_drawn"], r["n_clipped"], r["n_outside"])
    # the compare's classes, per radius and direction
    other = lc.other_reference()
    assert 3000 <= len(other.keys) <= 20000
    for radius in eref.RADII:
        fwd, bwd = lc.sparse_compare(True, radius), lc.sparse_compare(False, radius)
        assert fwd["reach"] == eref.reach_of(radius, lc.LEAF_B) and bwd["reach"] == eref.reach_of(radius, lc.LEAF)
        matched = np.isfinite(fwd["dist"])
        both_halves(fwd["keys"][matched], ("matched", radius))
        both_halves(fwd["keys"][~matched], ("unmatched", radius))
        assert len(np.flatnonzero(fwd["hist"])) >= 8
        # the other way round the LOOKUPS land in the big table: the matched cells' partners are found there
        assert bwd["n_matched"] >= 1000 and bwd["n_unmatched"] >= 100
    # the prune's verdicts
    out = rm.classify(**lc.SPARSE_PRUNE)
    for reason in range(6):
        both_halves(out["keys"][out["reason"] == reason], ("reason", reason))


def test_the_wide_render_covers_the_second_round_and_the_partial_workgroup():
    npix = lc.WIDE_W * lc.WIDE_H
    assert npix == 263_069 > lc.ROUND and npix % 256 == 157
    r = lc.sparse_render("wide", 2, 1)
    mask = r["mask"].reshape(-1)
    assert mask[lc.ROUND:].sum() >= 20 and mask[npix - 157:].sum() >= 5 and mask[:lc.WIDE_W].sum() >= 20
    assert (lc.ROUND // lc.WIDE_W, npix // lc.WIDE_W - 1) == (501, 502)          # the rows that hold those pixels, counted from 0
    assert r["mask"][501].any() and r["mask"][502].any() and 0 < r["n_pixels"] < npix
    assert min(r["n_drawn"], r["n_clipped"], r["n_outside"]) >= ENOUGH


@pytest.mark.parametrize("name", list(lc.CHAINS))
def test_a_chain_crosses_the_tables_end(name):
    ch = lc.chain(name)
    cap, p = ch["capacity"], lc.CHAINS[name]
    cells = ch["cells"]
    assert len(cells) == p["take"] >= 100 and len(ch["spare"]) >= 40
    homes = lc.home_slots(ref.pack_key(cells), cap)
    assert (homes >= cap - p["tail"]).all() and len(np.unique(ref.pack_key(cells))) == len(cells)
    occ, run = lc.chain_run(name)
    assert run is not None and occ.sum() == len(cells)
    first, length = run
    assert first >= cap - p["tail"] and first + length > cap                       # it holds slot cap - 1 and slot 0
    if name == "2^8":
        assert len(cells) * 4 <= 3 * cap and (first, length) == (240, 120)
        assert np.array_equal(np.flatnonzero(occ), np.r_[0:104, 240:256])
        assert len(lc.chain("2^8")["cells"]) + len(lc.chain("2^8")["spare"]) == 275
    else:
        assert length >= 90 and (first + length) % cap >= 30
    # the occupied set does not depend on the order of insertion
    rng = np.random.default_rng(3)
    for _ in range(3):
        assert np.array_equal(lc.linear_probing(homes[rng.permutation(len(homes))], cap), occ)
    # most cells lie further from their home than a few steps, whatever the order: at most 16 (64) slots are homes
    assert length - p["tail"] >= 36
    # the first call is one point per cell; the second adds no more than the 3/4 rule lets a 2^8-slot table take
    rm = lc.chain_reference(name, ("first",))
    assert np.array_equal(rm.keys, np.sort(ref.pack_key(cells))) and (rm.n == 1).all()
    both = lc.chain_reference(name)
    assert mref.grown_capacity(cap, len(rm.keys), len(ch["again"][0])) == (cap, 0)
    assert 40 <= (both.n >= 2).sum() <= 50 and 20 <= len(both.keys) - len(rm.keys) <= 30   # (a +x neighbour may be a chain cell)
    guest = mref.reference_of(ch["guest_calls"], lc.CHAIN_LEAF)
    assert mref.grown_capacity(cap, len(both.keys), len(guest.keys)) == (cap, 0)
    assert np.isin(guest.keys, both.keys).sum() >= 20 and (~np.isin(guest.keys, both.keys)).sum() == 10


@pytest.mark.parametrize("name", list(lc.CHAINS))
def test_absent_keys_are_looked_up_through_the_run(name):
    """compare(other, chain) looks up, for every cell of `other`, the keys within `reach` cells of it in the chain's table:
    some are present, and some absent ones have their home inside the run, so that the lookup walks to the run's end"""
    ch = lc.chain(name)
    cap = ch["capacity"]
    _, run = lc.chain_run(name)
    chain_map, other = lc.chain_reference(name), mref.reference_of(ch["other_calls"], lc.CHAIN_LEAF)
    want = eref.compare(other.extract(), chain_map.extract(), lc.CHAIN_LEAF, lc.CHAIN_RADIUS, eref.N_BINS, details=True)
    reach = want["reach"]
    assert reach == 2 and want["n_matched"] >= 30 and want["n_unmatched"] >= 30
    span = np.arange(-reach, reach + 1)
    offs = np.stack([a.ravel() for a in np.meshgrid(span, span, span, indexing="ij")], axis=1)
    looked = np.unique(ref.pack_key((want["cell"].astype(np.int64)[:, None, :] + offs[None]).reshape(-1, 3)))
    present = np.isin(looked, chain_map.keys)
    absent_inside = lc.in_run(lc.home_slots(looked[~present], cap), run, cap)
    assert present.sum() >= 50 and absent_inside.sum() >= 30
    assert np.isin(ref.pack_key(ch["spare"][:40]), looked[~present]).all()       # the spare cells: absent, home in the tail
    # the chain against itself, and the prune's neighbour support, find cells of the chain through the run
    out = chain_map.classify(**lc.CHAIN_PRUNE)
    chain_keys = ref.pack_key(ch["cells"])
    kept = out["keys"][out["reason"] == 0]
    assert np.isin(kept, chain_keys).sum() >= 30 and (out["reason"] == 5).sum() >= 20
