"""What the Python binding of the world map hands back, stage by stage: the keys of every fetched dict in their order, each
column's dtype, trailing shape and contiguity, the two orders (ascending key; the table's, which is extract(sort=False)'s
under the pass's filter), the optional columns' coming and going, the refusals, and the Python types of every counts dict.
The stages' own tests pin the VALUES against their restatements; this one pins the SHAPE of the binding, so that the code
between the C entry points and these dicts can be rewritten under it.  The names, dtypes and shapes below are literals
taken from the docstrings of engine.WorldMap.

The map: leaf 1/8, 300 seeded points of the unit cube in two integrate calls of 150 -- about 225 cells in a table of 2^8
slots, which doubles once --, about 60 of the cells with two points or more; the passes run under min_points = 2, so that
"the pass's filter" is not the open one.  Beside it an empty map of the same leaf.
"""
import numpy as np
import pytest

import dvs_mcemvs_amd as d

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(4)[:3]
LEAF = 0.125
POINTS = np.random.default_rng(20261021).uniform(0.0, 1.0, (300, 3)).astype(np.float32)
OTHER = (POINTS[40:260] + np.float32(0.01)).astype(np.float32)
MP = 2  # min_points of every pass that takes a filter

U64, U32, U16, U8, F32, I64 = (np.dtype(t) for t in ("uint64", "uint32", "uint16", "uint8", "float32", "int64"))

# fetch -> (the pass that it reads, its columns (name, dtype, trailing shape) in the dict's order, the filter of its rows)
FETCHES = {
    "fetchDistances": (lambda wm, o: wm.compare(o, 0.2, min_points=MP), [("keys", U64, ()), ("dist", F32, ())], (MP, 1)),
    "fetchPruneReasons": (lambda wm, o: wm.classifyPrune(min_points=MP), [("keys", U64, ()), ("reason", U8, ())], (1, 1)),
    "fetchComponents": (lambda wm, o: wm.components(min_points=MP), [("keys", U64, ()), ("labels", U64, ())], (MP, 1)),
    "fetchKnn": (lambda wm, o: wm.knn(4, 0.3, min_points=MP),
                 [("keys", U64, ()), ("found", U8, ()), ("mean", F32, ()), ("q", U32, ())], (MP, 1)),
    "fetchPca": (lambda wm, o: wm.pca(4, 0.3, min_points=MP),
                 [("keys", U64, ()), ("normal", F32, (3,)), ("tangent", F32, (3,)), ("eval", F32, (3,)), ("members", U16, ()),
                  ("label", U8, ()), ("flags", U8, ())], (MP, 1)),
    "fetchAlignment": (lambda wm, o: wm.alignStep(o, 0.2, min_points=MP),
                       [("keys", U64, ()), ("keys_other", U64, ()), ("dist", F32, ())], (MP, 1)),
}
LIST_COLUMNS = [("labels", U64, ()), ("cells", U64, ()), ("points", U64, ())]
STATE_SCALARS = [("leaf", float), ("calls", int), ("accepted", int), ("rejected", int)]
STATE_COLUMNS = [("keys", U64, ()), ("n", U32, ()), ("S", U64, (3,)), ("windows", U32, ()), ("stamp", U32, ())]
REASON, MOMENTS = ("reason", U8, ()), ("moments", I64, (9,))


@pytest.fixture
def maps(ctx):
    wm, other, empty = d.WorldMap(ctx, LEAF, 8), d.WorldMap(ctx, LEAF, 8), d.WorldMap(ctx, LEAF, 8)
    assert wm.integrate(POINTS[:150], IDENTITY) == 0 and wm.info()["growths"] == 0
    assert wm.integrate(POINTS[150:], IDENTITY) == 0 and other.integrate(OTHER, IDENTITY) == 0
    info = wm.info()
    assert info["growths"] == 1 and info["capacity"] == 512 and 192 < info["occupied"] < 300
    assert 20 < wm.count(MP, 1) < info["occupied"] and empty.info()["occupied"] == 0
    yield wm, other, empty
    for m in (wm, other, empty):
        m.close()


def check_columns(got, columns, rows, scalars=()):
    """the dict's keys in order; per column a fresh C-contiguous array of (rows,) + trailing shape"""
    assert list(got) == [name for name, _ in scalars] + [name for name, _, _ in columns]
    for name, kind in scalars:
        assert type(got[name]) is kind, name
    for name, dtype, trailing in columns:
        a = got[name]
        assert type(a) is np.ndarray and a.dtype == dtype and a.shape == (rows,) + trailing and a.flags.c_contiguous, name


def check_orders(wm, fetch, columns, filt, scalars=()):
    """sort=False: the table's order, which is extract(sort=False)'s under the filter; sort=True: the same rows through the
    stable ascending order of their keys.  Returns the sorted dict."""
    table = wm.extract(*filt, sort=False)["keys"]
    raw, by_key = fetch(sort=False), fetch(sort=True)
    for got in (raw, by_key):
        check_columns(got, columns, len(table), scalars)
    assert np.array_equal(raw["keys"], table) and len(table) > 1
    assert np.all(by_key["keys"][1:] > by_key["keys"][:-1]) and not np.array_equal(raw["keys"], by_key["keys"])
    order = np.argsort(raw["keys"], kind="stable")
    for name, _, _ in columns:
        assert np.array_equal(by_key[name], raw[name][order], equal_nan=by_key[name].dtype.kind == "f"), name
    for name, _ in scalars:
        assert raw[name] == by_key[name], name
    return by_key


@pytest.mark.parametrize("name", sorted(FETCHES))
def test_a_fetch_gives_its_columns_in_both_orders_and_refuses_without_its_pass(maps, name):
    wm, other, empty = maps
    run, columns, filt = FETCHES[name]
    with pytest.raises(d.DsiError):                                           # before the pass
        getattr(wm, name)()
    run(wm, other)
    check_orders(wm, getattr(wm, name), columns, filt)
    assert list(getattr(wm, name)()) == [c[0] for c in columns]                # (the default order has the same columns)
    run(empty, other)                                                          # an empty map: no rows, the trailing shapes stay
    for sort in (False, True):
        check_columns(getattr(empty, name)(sort=sort), columns, 0)
    for m in (wm, empty):
        m.integrate(np.zeros((0, 3), np.float32), IDENTITY)                    # after an integrate call, even of no points
        with pytest.raises(d.DsiError):
            getattr(m, name)()


def test_default_orders(maps):
    wm, other, _ = maps
    for name, (run, _, filt) in FETCHES.items():
        run(wm, other)
        keys, table = getattr(wm, name)()["keys"], wm.extract(*filt, sort=False)["keys"]
        assert np.array_equal(keys, table if name == "fetchPca" else np.sort(table)), name
    assert np.array_equal(wm.exportState()["keys"], np.sort(wm.extract(sort=False)["keys"]))


def test_list_components(maps):
    wm, other, empty = maps
    with pytest.raises(d.DsiError):
        wm.listComponents()
    info = wm.components(min_points=MP)
    got = wm.listComponents()
    check_columns(got, LIST_COLUMNS, info["n_components"])
    assert info["n_components"] > 1 and int(got["cells"].sum()) == info["n_cells"]
    rows = list(zip((-got["cells"].astype(np.int64)).tolist(), got["labels"].tolist()))
    assert rows == sorted(rows) and len(set(got["labels"].tolist())) == len(rows)  # cells descending, then label ascending
    assert got["labels"][0] == info["largest_label"] and got["cells"][0] == info["largest_cells"]
    empty.components()
    check_columns(empty.listComponents(), LIST_COLUMNS, 0)
    wm.integrate(POINTS[:1], IDENTITY)
    with pytest.raises(d.DsiError):
        wm.listComponents()


def test_export_state(maps):
    wm, _, empty = maps
    state = check_orders(wm, wm.exportState, STATE_COLUMNS, (1, 1), STATE_SCALARS)
    assert (state["leaf"], state["calls"], state["accepted"], state["rejected"]) == (LEAF, 2, 300, 0)
    assert int(state["n"].sum()) == 300
    for sort in (False, True):
        got = empty.exportState(sort=sort)
        check_columns(got, STATE_COLUMNS, 0, STATE_SCALARS)
        assert (got["leaf"], got["calls"], got["accepted"], got["rejected"]) == (LEAF, 0, 0, 0)
    wm.integrate(POINTS[:1], IDENTITY)                                          # (the state needs no pass: it never refuses)
    assert wm.exportState()["calls"] == 3


def test_optional_columns_come_with_their_select_and_go_with_the_pass(maps):
    wm, other, empty = maps
    selects = {"fetchComponents": lambda m: m.selectComponents(min_cells=2), "fetchKnn": lambda m: m.selectOutliers(std_mult=0.5),
               "fetchPca": lambda m: m.selectShapes(keep=("planar",))}
    for name, select in selects.items():
        run, columns, filt = FETCHES[name]
        for m in (wm, empty):
            rows = m.count(*filt)
            run(m, other)
            check_columns(getattr(m, name)(), columns, rows)
            select(m)
            for sort in (False, True):
                check_columns(getattr(m, name)(sort=sort), columns + [REASON], rows)
        counts = select(wm)
        got = check_orders(wm, getattr(wm, name), columns + [REASON], filt)
        assert np.count_nonzero(got["reason"] == 0) == counts["n_kept"] and got["reason"].max() <= len(counts["n_removed"])
        for m in (wm, empty):
            run(m, other)                                                      # the pass again: the selection is gone
            check_columns(getattr(m, name)(), columns, m.count(*filt))
    # the moments of the local-shape pass: with keep_moments=True only, before the reasons
    run, columns, filt = FETCHES["fetchPca"]
    for m in (wm, empty):
        rows = m.count(*filt)
        m.pca(4, 0.3, min_points=MP, keep_moments=True)
        check_columns(m.fetchPca(), columns + [MOMENTS], rows)
        m.selectShapes()
        for sort in (False, True):
            check_columns(m.fetchPca(sort=sort), columns + [MOMENTS, REASON], rows)
    check_orders(wm, wm.fetchPca, columns + [MOMENTS, REASON], filt)
    for m in (wm, empty):
        run(m, other)
        check_columns(m.fetchPca(), columns, m.count(*filt))
    # a refused select leaves no reasons behind it
    wm.selectShapes()
    with pytest.raises(d.DsiError):
        wm.selectShapes(keep=0)
    check_columns(wm.fetchPca(), columns, wm.count(*filt))


def kinds(value):
    """int, float, [kinds of the elements] or (dtype, shape): what a counts dict is compared by"""
    if isinstance(value, dict):
        return {k: kinds(v) for k, v in value.items()}
    if type(value) is list:
        return [kinds(v) for v in value]
    if type(value) is np.ndarray:
        return (value.dtype, value.shape)
    return type(value)


SELECT = {"n_cells": int, "n_kept": int, "capacity": int}
COUNTS = {
    "info": dict(dict.fromkeys(("capacity", "occupied", "calls", "accepted", "rejected", "growths"), int), leaf=float),
    "render": dict.fromkeys(("width", "height", "n_cells", "n_clipped", "n_outside", "n_drawn", "n_pixels"), int),
    "compare": dict(dict.fromkeys(("n_cells", "n_matched", "n_unmatched", "sum_q", "reach"), int), hist=(U64, (16,)), mean=float),
    "prune": dict(SELECT, n_removed=[int] * 5),
    "components": dict.fromkeys(("n_cells", "n_unlabelled", "n_components", "n_singletons", "largest_label", "largest_cells",
                                 "largest_points"), int),
    "selectComponents": dict(SELECT, n_removed=[int] * 4, n_components_kept=int),
    "knn": dict.fromkeys(("n_cells", "n_unqueried", "n_scored", "n_isolated", "sum_q", "sum_q2", "reach"), int),
    "selectOutliers": dict(SELECT, n_removed=[int] * 3, T_q=int, mu=float, sigma=float),
    "pca": dict(dict.fromkeys(("n_cells", "n_unqueried", "n_sparse", "n_normal_determined", "n_tangent_determined", "sum_members",
                               "reach"), int), n_label=[int] * 3),
    "selectShapes": dict(SELECT, n_removed=[int] * 3),
    "merge": dict.fromkeys(("n_src_cells", "n_new", "n_common", "capacity", "growths"), int),
    "align": dict(dict.fromkeys(("iterations", "converged", "stopped", "reach", "n_cells", "n_matched_first", "n_matched_last"), int),
                  **dict.fromkeys(("rms_first", "rms_last", "angle_last", "trans_last"), float)),
}


def test_counts_are_plain_python(maps):
    wm, other, empty = maps
    for m in (wm, empty):
        got = {"info": m.info(),
               "render": m.render(IDENTITY, 16, 12, 8.0, 8.0, 8.0, 6.0, 0.05, 10.0, fetch=False),
               "compare": m.compare(other, 0.2),
               "classifyPrune": m.classifyPrune(min_points=MP, reach=1, min_neighbors=1),
               "components": m.components(),
               "selectComponents": m.selectComponents(min_cells=2),
               "knn": m.knn(4, 0.3),
               "selectOutliers": m.selectOutliers(),
               "pca": m.pca(4, 0.3),
               "selectShapes": m.selectShapes()}
        want = dict(COUNTS, classifyPrune=COUNTS["prune"])
        for name, counts in got.items():
            assert kinds(counts) == want[name], name
    T, info = wm.align(other, 0.2, max_iterations=2)
    assert kinds(T) == (np.dtype("float64"), (12,)) and kinds(info) == COUNTS["align"]
    assert kinds(wm.prune(min_points=MP)) == COUNTS["prune"] and kinds(empty.prune()) == COUNTS["prune"]
    assert kinds(wm.merge(other)) == COUNTS["merge"] and kinds(empty.merge(other)) == COUNTS["merge"]
    assert kinds(empty.importState(other.exportState())) == COUNTS["merge"]
    assert wm.knn(4, 0.3)["sum_q2"] >= 0
