"""Pruning the world map restated in numpy (include/dsi_map_prune.h; DESIGN.md 7j "Pruning"), written from the header's
rule.  PruneReferenceMap is world_map_reference.ReferenceMap plus the per-key `stamp` (the serial of the last call that put
an accepted point into the cell); everything is by ascending key, integers and elementwise float64.

    reason (the FIRST that fails, 0 = kept)
      1  n < min_points                       2  windows < min_windows
      3  max_age is not None and calls - stamp > max_age
      4  box is not None and the float32 centroid of extract(), widened, lies outside [lo, hi] on some axis
      5  reach > 0 and fewer than min_neighbors OTHER cells with reason 0 after 1-4 among the cell indices c + o,
         |o| <= reach per axis, |c + o| <= 2^20 - 2 (one pass: a neighbour that 5 removes still counts)
"""
import itertools

import numpy as np

import world_map_reference as ref

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
DEFAULTS = dict(min_points=1, min_windows=1, max_age=None, box=None, reach=0, min_neighbors=0)


def shrunk_capacity(kept):
    """the smallest 2^k, k >= 8, with 4 kept <= 3 2^k"""
    k = 8
    while 4 * kept > 3 * (1 << k):
        k += 1
    return 1 << k


class PruneReferenceMap(ref.ReferenceMap):
    def reset(self):
        super().reset()
        self.stamp = np.zeros(0, np.uint64)

    def integrate(self, xyz, T_w_rv):
        xyz = np.asarray(xyz, np.float32)
        if xyz.ndim != 2:
            xyz = xyz.reshape(-1, 3)
        old_keys, old_stamp = self.keys, self.stamp
        rejected = super().integrate(xyz, T_w_rv)
        ok, c, _ = ref.cells(xyz, T_w_rv, self.leaf)
        stamp = np.zeros(len(self.keys), np.uint64)
        stamp[np.searchsorted(self.keys, old_keys)] = old_stamp
        stamp[np.searchsorted(self.keys, np.unique(ref.pack_key(c[ok])))] = np.uint64(self.calls)
        self.stamp = stamp
        return rejected

    def first_four(self, min_points=1, min_windows=1, max_age=None, box=None, **_):
        """per key: the first of criteria 1-4 that fails, 0 when none does"""
        r = np.zeros(len(self.keys), np.uint8)
        if box is not None:
            lo, hi = (np.asarray(b, np.float64).reshape(3) for b in box)
            p = self.extract(0, 0)["xyz"].astype(np.float64)
            r[((p < lo) | (p > hi)).any(axis=1)] = 4
        if max_age is not None:
            r[np.int64(self.calls) - self.stamp.astype(np.int64) > np.int64(max_age)] = 3
        r[self.windows < np.uint64(min_windows)] = 2                       # (written last = found first)
        r[self.n < np.uint64(min_points)] = 1
        return r

    def classify(self, **opts):
        """dict of keys, reason (uint8 per key), n_cells, n_kept, n_removed (5)"""
        o = dict(DEFAULTS, **opts)
        o.pop("shrink", None)
        r = self.first_four(**o)
        reach, need = int(o["reach"]), int(o["min_neighbors"])
        if reach > 0 and len(self.keys):
            alive = r == 0
            c = ref.unpack_key(self.keys)
            found = np.zeros(len(self.keys), np.int64)
            span = range(-reach, reach + 1)
            for off in itertools.product(span, span, span):
                if off == (0, 0, 0):
                    continue
                nb = c + np.asarray(off, np.int64)
                valid = (np.abs(nb) <= ref.CELL_MAX).all(axis=1)
                k = ref.pack_key(np.where(valid[:, None], nb, 0))
                j = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
                found += valid & (self.keys[j] == k) & alive[j]
            r[alive & (found < need)] = 5
        return {"keys": self.keys.copy(), "reason": r, "n_cells": len(r), "n_kept": int((r == 0).sum()),
                "n_removed": [int((r == q).sum()) for q in range(1, 6)]}

    def prune(self, **opts):
        out = self.classify(**opts)
        keep = out["reason"] == 0
        self.keys, self.n, self.S = self.keys[keep], self.n[keep], self.S[keep]
        self.windows, self.stamp = self.windows[keep], self.stamp[keep]
        return out


def brute_force(rm, **opts):
    """the reasons by a loop over all cell pairs: criteria 1-4 per cell in order, then criterion 5 by comparing every
    pair of cell indices (no keys, no search)"""
    o = dict(DEFAULTS, **opts)
    cells = rm.extract(0, 0)
    c = ref.unpack_key(rm.keys)
    first = []
    for i in range(len(rm.keys)):
        p = cells["xyz"][i].astype(np.float64)
        if int(rm.n[i]) < o["min_points"]:
            first.append(1)
        elif int(rm.windows[i]) < o["min_windows"]:
            first.append(2)
        elif o["max_age"] is not None and rm.calls - int(rm.stamp[i]) > o["max_age"]:
            first.append(3)
        elif o["box"] is not None and any(p[a] < o["box"][0][a] or p[a] > o["box"][1][a] for a in range(3)):
            first.append(4)
        else:
            first.append(0)
    out = list(first)
    if o["reach"] > 0:
        for i in range(len(out)):
            if first[i] == 0:
                near = sum(1 for j in range(len(out)) if j != i and first[j] == 0 and
                           max(abs(int(c[i][a]) - int(c[j][a])) for a in range(3)) <= o["reach"])
                if near < o["min_neighbors"]:
                    out[i] = 5
    return np.asarray(out, np.uint8)


# ---- the shared random scene: six uneven calls with empty calls in between, leaf 0.05 ----
LEAF = 0.05
SCENE_OPTS = dict(min_points=2, min_windows=2, max_age=4, box=((-0.7, -0.7, -0.2), (0.7, 0.38, 0.7)), reach=1, min_neighbors=2)


def scene_calls(seed=11):
    """list of (points float32 (N, 3) or an empty array, pose): a slab of surface cells sampled by every call (kept), its
    left part by the first two calls only (old), single noise points (few points), noise points repeated within one call
    (one window), the slab's far side (outside the box) and, well above the slab, lone cells and lines of three seen by
    the last calls (no support; a line's middle cell is kept by two cells that criterion 5 removes)."""
    rng = np.random.default_rng(seed)
    sizes = [900, 300, 1200, 150, 700, 500]
    empty = np.zeros((0, 3), np.float32)
    lone = np.column_stack([rng.integers(-4, 4, 60) * 3, rng.integers(-4, 3, 60) * 3, rng.integers(2, 5, 60) * 2])   # z cells 4, 6, 8
    lone = (lone + 0.5) * LEAF                                                    # three cells apart in x and y: no neighbours
    start = np.stack([np.arange(30) % 6 * 4 - 12, np.arange(30) // 6 * 4 - 12, np.full(30, 11)], axis=1)   # z cell 11: apart from `lone`
    lines = np.concatenate([(start + [d, 0, 0] + 0.5) * LEAF for d in range(3)])
    calls = []
    for k, n in enumerate(sizes):
        slab = np.column_stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(0.0, 0.1, n)])
        if k >= 2:
            slab = slab[slab[:, 0] > -0.25]                                       # the left part grows old
        noise = rng.uniform(-1.5, 1.5, (60, 3))
        twice = np.repeat(rng.uniform(-1.5, 1.5, (25, 3)) + [0, 0, 3.0], 2, axis=0)
        parts = [slab, noise, twice]
        if k >= 4:
            parts += [lone, lines]
        pts = np.concatenate(parts).astype(np.float32)
        calls.append((pts[rng.permutation(len(pts))], IDENTITY))
        if k in (1, 3):
            calls.append((empty, IDENTITY))
    return calls


def scene_map(seed=11):
    rm = PruneReferenceMap(LEAF)
    for pts, T in scene_calls(seed):
        rm.integrate(pts, T)
    return rm


def supported_only_by_removed(rm, **opts):
    """the number of kept cells all of whose supporters (cells that survive 1-4 within reach) are removed by criterion 5"""
    o = dict(DEFAULTS, **opts)
    out = rm.classify(**o)
    r, c = out["reason"], ref.unpack_key(rm.keys)
    first = rm.first_four(**o)
    count = 0
    for i in np.flatnonzero(r == 0):
        near = (np.abs(c - c[i]).max(axis=1) <= o["reach"]) & (first == 0)
        near[i] = False
        if near.any() and (r[near] == 5).all():
            count += 1
    return count


# ---- hand cases: a power-of-two leaf, single points at cell centres or exact offsets, so that every centroid is exact ----
def _centres(cells, leaf):
    return ((np.asarray(cells, np.float64).reshape(-1, 3) + 0.5) * leaf).astype(np.float32)


def hand_cases():
    """list of dicts: name, leaf, calls [(points, pose)], opts, want {cell index (cx, cy, cz): reason}"""
    inf = float("inf")
    f32 = np.float32
    empty = np.zeros((0, 3), f32)
    out = []
    # criterion 4: the closed box.  leaf 0.5: x = 0.25 and 0.75 are the centroids of cells 0 and 1, exactly; one float32
    # ulp below 0.25 and above 0.75 are exact centroids too
    below, above = np.nextafter(f32(0.25), f32(0.0)), np.nextafter(f32(0.75), f32(1.0))
    pts = f32([[0.25, 0.25, 0.25], [below, 1.25, 0.25], [0.75, 2.25, 0.25], [above, 3.25, 0.25]])
    out.append(dict(name="box edges", leaf=0.5, calls=[(pts, IDENTITY)], opts=dict(box=((0.25, -inf, -inf), (0.75, inf, inf))),
                    want={(0, 0, 0): 0, (0, 2, 0): 4, (1, 4, 0): 0, (1, 6, 0): 4}))
    out.append(dict(name="box of one point", leaf=0.5, calls=[(pts, IDENTITY)], opts=dict(box=((0.75, 2.25, 0.25), (0.75, 2.25, 0.25))),
                    want={(0, 0, 0): 4, (0, 2, 0): 4, (1, 4, 0): 0, (1, 6, 0): 4}))
    # criterion 3: age 0 is the last call; an empty call ages every cell by one
    p, q = _centres([[0, 0, 0]], 0.5), _centres([[5, 0, 0]], 0.5)
    out.append(dict(name="age 0 is the last call", leaf=0.5, calls=[(p, IDENTITY), (q, IDENTITY)], opts=dict(max_age=0),
                    want={(0, 0, 0): 3, (5, 0, 0): 0}))
    out.append(dict(name="an empty call ages", leaf=0.5, calls=[(p, IDENTITY), (q, IDENTITY), (empty, IDENTITY)], opts=dict(max_age=0),
                    want={(0, 0, 0): 3, (5, 0, 0): 3}))
    out.append(dict(name="age 1 after an empty call", leaf=0.5, calls=[(p, IDENTITY), (q, IDENTITY), (empty, IDENTITY)],
                    opts=dict(max_age=1), want={(0, 0, 0): 3, (5, 0, 0): 0}))
    # criteria 1 and 2, and their order: a cell with one point of one call fails criterion 1 first
    two = np.concatenate([p, p, q])
    out.append(dict(name="points before windows", leaf=0.5, calls=[(two, IDENTITY), (p, IDENTITY)], opts=dict(min_points=2, min_windows=2),
                    want={(0, 0, 0): 0, (5, 0, 0): 1}))
    out.append(dict(name="windows", leaf=0.5, calls=[(np.concatenate([two, q]), IDENTITY), (p, IDENTITY)],
                    opts=dict(min_points=2, min_windows=2), want={(0, 0, 0): 0, (5, 0, 0): 2}))
    # criterion 5
    line = _centres([[0, 0, 0], [1, 0, 0], [2, 0, 0]], 0.5)
    out.append(dict(name="a line keeps its middle", leaf=0.5, calls=[(line, IDENTITY)], opts=dict(reach=1, min_neighbors=2),
                    want={(0, 0, 0): 5, (1, 0, 0): 0, (2, 0, 0): 5}))
    block = [(x, y, z) for x in range(-1, 2) for y in range(-1, 2) for z in range(-1, 2)]
    out.append(dict(name="a block's centre has 26 neighbours", leaf=0.5, calls=[(_centres(block, 0.5), IDENTITY)],
                    opts=dict(reach=1, min_neighbors=26), want={c: 0 if c == (0, 0, 0) else 5 for c in block}))
    apart = _centres([[0, 0, 0], [2, -2, 1]], 0.5)
    out.append(dict(name="distance 2 is beyond reach 1", leaf=0.5, calls=[(apart, IDENTITY)], opts=dict(reach=1, min_neighbors=1),
                    want={(0, 0, 0): 5, (2, -2, 1): 5}))
    out.append(dict(name="distance 2 is within reach 2", leaf=0.5, calls=[(apart, IDENTITY)], opts=dict(reach=2, min_neighbors=1),
                    want={(0, 0, 0): 0, (2, -2, 1): 0}))
    # the outermost cells +-(2^20 - 2): the neighbours beyond them have no key and are skipped
    m = ref.CELL_MAX
    edge = _centres([[m, 0, 0], [m - 1, 0, 0], [-m, 3, -m], [0, m, 0], [0, m - 2, 0]], 1.0)
    for reach, last in ((1, 5), (2, 0)):
        out.append(dict(name="cells at the edge of the key range, reach %d" % reach, leaf=1.0, calls=[(edge, IDENTITY)],
                        opts=dict(reach=reach, min_neighbors=1),
                        want={(m, 0, 0): 0, (m - 1, 0, 0): 0, (-m, 3, -m): 5, (0, m, 0): last, (0, m - 2, 0): last}))
    return out


def run_hand_case(case, make_map):
    """the case's calls through make_map(leaf) (anything with integrate); returns the map"""
    mp = make_map(case["leaf"])
    for pts, T in case["calls"]:
        assert mp.integrate(pts, T) == 0
    return mp


def wanted_reasons(case):
    """(keys ascending, reasons) of the case's `want`"""
    cells = np.asarray(list(case["want"]), np.int64)
    keys = ref.pack_key(cells)
    order = np.argsort(keys)
    return keys[order], np.asarray(list(case["want"].values()), np.uint8)[order]
