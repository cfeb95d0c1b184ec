"""The world map's connected components restated in numpy and scipy (include/dsi_map_components.h; DESIGN.md 7j
"Components"), written from the header's rule, on top of map_prune_reference.PruneReferenceMap.  Everything is by ascending
key and integer.

    nodes      the cells with n >= min_points and windows >= min_windows; the other cells are unlabelled
    edges      two nodes whose cell indices differ by an offset o != 0 of the connectivity
                 6: |o|_inf = 1, |o|_1 = 1     18: |o|_inf = 1, |o|_1 <= 2     26: |o|_inf = 1     124: |o|_inf <= 2
               (an index with |c + o| > 2^20 - 2 has no key)
    label      the smallest key of the component; cells, points = its number of cells, the sum of their n
    reason     (the FIRST that holds, 0 = kept)  1 unlabelled   2 cells < min_cells   3 points < min_component_points
               4 keep_largest > 0 and not among the keep_largest first of those that pass 2 and 3, by cells descending,
                 then label ascending
"""
import functools
import itertools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import map_prune_reference as pref
import world_map_reference as ref

IDENTITY = pref.IDENTITY
CONNECTIVITIES = (6, 18, 26, 124)
SELECT_DEFAULTS = dict(min_cells=1, min_component_points=1, keep_largest=0)


def offsets(connectivity):
    """every offset o != 0 of the connectivity, as tuples (ox, oy, oz)"""
    reach, most = {6: (1, 1), 18: (1, 2), 26: (1, 3), 124: (2, 6)}[connectivity]
    span = range(-reach, reach + 1)
    out = [o for o in itertools.product(span, span, span) if o != (0, 0, 0) and sum(abs(v) for v in o) <= most]
    assert len(out) == connectivity
    return out


def positive_half(connectivity):
    """one offset of every pair (o, -o): an undirected edge is found from one of its ends"""
    return [o for o in offsets(connectivity) if o[::-1] > (0, 0, 0)]


def label_keys(keys, connectivity):
    """the label of every key of `keys` (ascending, distinct): the smallest key of its component"""
    keys = np.asarray(keys, np.uint64)
    m = len(keys)
    if m == 0:
        return np.zeros(0, np.uint64)
    c = ref.unpack_key(keys)
    rows, cols = [], []
    for off in positive_half(connectivity):
        nb = c + np.asarray(off, np.int64)
        valid = (np.abs(nb) <= ref.CELL_MAX).all(axis=1)
        k = ref.pack_key(np.where(valid[:, None], nb, 0))
        j = np.minimum(np.searchsorted(keys, k), m - 1)
        hit = valid & (keys[j] == k)
        rows.append(np.flatnonzero(hit))
        cols.append(j[hit])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(m, m))
    count, comp = connected_components(graph, directed=False)
    labels = np.full(count, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(labels, comp, keys)
    return labels[comp]


def components(rm, min_points=1, min_windows=1, connectivity=26):
    """dict of keys, labels (per node), list (labels, cells, points per component, by cells descending then label
    ascending), info (what dsx_map_components reports) and the filter"""
    node = (rm.n >= np.uint64(min_points)) & (rm.windows >= np.uint64(min_windows))
    keys, n = rm.keys[node], rm.n[node].astype(np.uint64)
    labels = label_keys(keys, connectivity)
    uniq, inverse, cells = np.unique(labels, return_inverse=True, return_counts=True)
    points = np.zeros(len(uniq), np.uint64)
    np.add.at(points, inverse, n)
    cells = cells.astype(np.uint64)
    order = np.lexsort((uniq, -cells.astype(np.int64)))
    lst = {"labels": uniq[order], "cells": cells[order], "points": points[order]}
    some = len(uniq) > 0
    info = {"n_cells": int(node.sum()), "n_unlabelled": int((~node).sum()), "n_components": len(uniq),
            "n_singletons": int((cells == 1).sum()), "largest_label": int(lst["labels"][0]) if some else 0,
            "largest_cells": int(lst["cells"][0]) if some else 0, "largest_points": int(lst["points"][0]) if some else 0}
    return {"keys": keys, "labels": labels, "list": lst, "info": info, "filter": (min_points, min_windows), "node": node}


def rank(lst, min_cells=1, min_component_points=1, keep_largest=0):
    """(reason per component of the list -- 0, 2, 3 or 4 --; the list is in criterion 4's order already)"""
    r = np.zeros(len(lst["labels"]), np.uint8)
    eligible = (lst["cells"] >= np.uint64(min_cells)) & (lst["points"] >= np.uint64(min_component_points))
    if keep_largest > 0:
        r[np.flatnonzero(eligible)[keep_largest:]] = 4
    r[lst["points"] < np.uint64(min_component_points)] = 3                     # (written last = found first)
    r[lst["cells"] < np.uint64(min_cells)] = 2
    return r


def select(rm, comp, **sel):
    """dict of keys (every occupied cell), reason, node_reason (per node, as the fetch returns it), n_cells, n_kept,
    n_removed (4), n_components_kept"""
    o = dict(SELECT_DEFAULTS, **sel)
    o.pop("shrink", None)
    by_component = rank(comp["list"], **o)
    node_reason = np.zeros(0, np.uint8)
    if len(comp["labels"]):
        sorter = np.argsort(comp["list"]["labels"])
        node_reason = by_component[sorter[np.searchsorted(comp["list"]["labels"], comp["labels"], sorter=sorter)]]
    reason = np.ones(len(rm.keys), np.uint8)
    reason[comp["node"]] = node_reason
    return {"keys": rm.keys.copy(), "reason": reason, "node_reason": node_reason, "n_cells": len(reason),
            "n_kept": int((reason == 0).sum()), "n_removed": [int((reason == q).sum()) for q in range(1, 5)],
            "n_components_kept": int((by_component == 0).sum())}


def prune_components(rm, comp, **sel):
    out = select(rm, comp, **sel)
    keep = out["reason"] == 0
    rm.keys, rm.n, rm.S = rm.keys[keep], rm.n[keep], rm.S[keep]
    rm.windows, rm.stamp = rm.windows[keep], rm.stamp[keep]
    return out


def partition(comp):
    """the labelling as a hashable partition of the nodes"""
    return tuple(comp["labels"].tolist())


# ---- independent statements, for the CPU tests ----
def bfs_labels(keys, connectivity):
    """plain Python: a breadth-first search over a dict of cell index -> key"""
    cells = {tuple(int(v) for v in c): int(k) for c, k in zip(ref.unpack_key(keys), keys)}
    label = {}
    for start in cells:
        if start in label:
            continue
        seen, queue = {start}, [start]
        while queue:
            cur = queue.pop()
            for o in offsets(connectivity):
                nb = (cur[0] + o[0], cur[1] + o[1], cur[2] + o[2])
                if nb in cells and nb not in seen:
                    seen.add(nb)
                    queue.append(nb)
        low = min(cells[c] for c in seen)
        for c in seen:
            label[c] = low
    return np.asarray([label[tuple(int(v) for v in c)] for c in ref.unpack_key(keys)], np.uint64)


def chebyshev_labels(keys, reach):
    """O(n^2): the graph of all pairs within `reach` per axis, through scipy on a dense matrix"""
    c = ref.unpack_key(keys)
    near = np.abs(c[:, None, :] - c[None, :, :]).max(axis=2) <= reach
    count, comp = connected_components(coo_matrix(near), directed=False)
    labels = np.full(count, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(labels, comp, np.asarray(keys, np.uint64))
    return labels[comp]


# ---- inputs ----
def centres(cells, leaf):
    """one float32 point at the centre of every cell (exact for a power-of-two leaf)"""
    return ((np.asarray(cells, np.float64).reshape(-1, 3) + 0.5) * leaf).astype(np.float32)


def map_of(calls, leaf, cls=pref.PruneReferenceMap):
    rm = cls(leaf)
    for pts, T in calls:
        rm.integrate(pts, T)
    return rm


@functools.lru_cache(maxsize=None)
def scene_reference():
    """the restatement's map of pref.scene_calls() (read-only: copy.deepcopy before changing it)"""
    return map_of(pref.scene_calls(), pref.LEAF)


@functools.lru_cache(maxsize=None)
def scene_components(min_points, min_windows, connectivity):
    return components(scene_reference(), min_points, min_windows, connectivity)


PAIR_LEAF = 0.5
PAIR_OFFSETS = {(1, 0, 0): (6, 18, 26, 124), (1, 1, 0): (18, 26, 124), (1, 1, 1): (26, 124), (2, 0, 0): (124,), (2, 2, 2): (124,),
                (3, 0, 0): ()}                                                  # offset: the connectivities that join the pair
EDGE_LEAF = 1.0


def pair_cells(offset):
    base = np.array([3, -2, 5])
    return np.stack([base, base + np.asarray(offset)])


def edge_pairs():
    """pairs of adjacent cells at the index bound 2^20 - 2: their outward neighbours have no key.  One pair per axis and
    sign, far from each other"""
    m = ref.CELL_MAX
    out = []
    for a in range(3):
        for s in (1, -1):
            hi, lo = [0, 0, 0], [0, 0, 0]
            hi[a], lo[a] = s * m, s * (m - 1)
            out += [hi, lo]
    return np.asarray(out, np.int64)


# the snake: three 6-connected serpentines, one cell thick, on the layers z = 0, 2 and 5
SNAKE_LEAF = 0.5
SNAKE_ROW, SNAKE_ROWS = 199, 200                                                # cells per row; rows, two apart in y
SNAKE_LAYERS = (0, 2, 5)
SNAKE_LOG2 = 19


def snake_layer(z):
    """the cells of one serpentine in path order: rows along x at y = 0, 2, 4, ... joined alternately at their ends by the
    one cell of the row between"""
    path = []
    for r in range(SNAKE_ROWS):
        xs = range(SNAKE_ROW) if r % 2 == 0 else range(SNAKE_ROW - 1, -1, -1)
        path += [(x - 100, 2 * r - 200, z) for x in xs]
        if r + 1 < SNAKE_ROWS:
            path.append((path[-1][0], 2 * r + 1 - 200, z))
    return np.asarray(path, np.int64)


@functools.lru_cache(maxsize=None)
def snake_cells():
    return np.concatenate([snake_layer(z) for z in SNAKE_LAYERS])


@functools.lru_cache(maxsize=None)
def snake_calls():
    """two calls: the cells in a random order, one point each"""
    cells = snake_cells()
    pts = centres(cells, SNAKE_LEAF)[np.random.default_rng(61).permutation(len(cells))]
    half = len(pts) // 2
    return ((pts[:half], IDENTITY), (pts[half:], IDENTITY))


@functools.lru_cache(maxsize=None)
def snake_reference():
    return map_of(snake_calls(), SNAKE_LEAF)


def selection_hand_cases():
    """list of dicts: name, cells (one list of cell indices per component, one point per cell unless `twice` names cells
    that get two), connectivity, sel, want_kept (the indices of the components that stay)"""
    line = lambda x0, y, n: [(x0 + i, y, 0) for i in range(n)]
    out = []
    # two components of three cells: the one with the smaller label (smaller y -> smaller key) ranks first
    out.append(dict(name="a tie goes to the smaller label", comps=[line(0, 5, 3), line(0, -5, 3), line(0, 0, 2)], sel=dict(keep_largest=1),
                    want_kept=[1]))
    out.append(dict(name="a tie, two kept", comps=[line(0, 5, 3), line(0, -5, 3), line(0, 0, 2)], sel=dict(keep_largest=2), want_kept=[0, 1]))
    out.append(dict(name="keep_largest above the number of components keeps all", comps=[line(0, 5, 3), line(0, -5, 3), line(0, 0, 2)],
                    sel=dict(keep_largest=16), want_kept=[0, 1, 2]))
    # criteria 2 and 3 remove before criterion 4 ranks: the largest has too few points, the next too few cells
    out.append(dict(name="criteria 2 and 3 come before the ranking", comps=[line(0, 0, 5), line(0, 4, 2), line(0, 8, 3), line(0, 12, 4)],
                    twice=line(0, 8, 3) + line(0, 12, 4) + line(0, 4, 2), sel=dict(min_cells=3, min_component_points=6, keep_largest=1),
                    want_kept=[3], want_reasons=[3, 2, 4, 0]))
    out.append(dict(name="criterion 3 alone", comps=[line(0, 0, 5), line(0, 4, 2)], twice=line(0, 4, 2), sel=dict(min_component_points=5),
                    want_kept=[0], want_reasons=[0, 3]))
    return out


def selection_case_calls(case):
    cells = [c for comp in case["comps"] for c in comp] + list(case.get("twice", []))
    return [(centres(cells, PAIR_LEAF), IDENTITY)]
