"""The inputs of test_gpu_map_layouts.py, and the properties that test_map_layouts_cpu.py proves of them without a GPU
(DESIGN.md 7j): world maps laid out so that every strided kernel walks a second round, and so that a run of occupied slots
crosses the table's end.  Nothing here restates the map's arithmetic: the cells, renders, comparisons, verdicts and states
come from the existing restatements, and the home slot of a cell is pointcloud_reference.engine_bucket.

    table A   two scenes in tables created at 2^19 slots that never grow: 2,048 tiles of 256 slots for at most 1,024
              workgroups, so every workgroup walks two rounds; a cell sits at or just after its home slot
      dense   300,007 distinct cells, one point each, in two calls (57 % load: every tile of the table is occupied)
      sparse  a few thousand cells in five calls, with every count of windows from 1 to 5
    chains    cells of a lattice whose home slot lies in the last slots of the table: under linear probing they fill one
              run that crosses slot capacity - 1 -> 0, whatever the order of insertion
"""
import copy
import functools

import numpy as np

import map_eval_reference as eref
import map_merge_reference as mref
import map_prune_reference as pref
import pointcloud_reference as pcref
import world_map_reference as ref
import world_map_render_reference as rref

IDENTITY = pref.IDENTITY
LEAF = 0.05
LEAF_B = 0.04
BIG_LOG2 = 19
ROUND = 1 << 18                                                                # slots (items, pixels) of one round: 1,024 workgroups of 256
MARGIN = 1024                                                                  # at low load a cell sits at or just after its home: this far from slot 2^18 its round is certain


def home_slots(keys, capacity):
    """the slot pc_hash sends each packed key to in a table of `capacity` slots"""
    c = ref.unpack_key(np.asarray(keys, np.uint64)).reshape(-1, 3)
    return pcref.engine_bucket(c[:, 0], c[:, 1], c[:, 2], capacity)


def halves(keys, capacity=1 << BIG_LOG2):
    """(low, high): the keys whose home lies safely in the first round of a 2^19-slot table, and safely in the second"""
    h = home_slots(keys, capacity)
    return h < ROUND - MARGIN, h > ROUND + MARGIN


def subset(cells, keep):
    return {k: v[keep] for k, v in cells.items()}


def fresh(rm):
    """a copy of a cached restatement that a test may change"""
    return copy.deepcopy(rm)


# ---- table A: the dense scene ----
DENSE_CELLS = 300_007
DENSE_SIDE = 67


def _dense_points():
    idx = np.arange(DENSE_CELLS)
    cells = np.stack([idx % DENSE_SIDE - 33, idx // DENSE_SIDE % DENSE_SIDE - 33, idx // (DENSE_SIDE * DENSE_SIDE) + 10], axis=1)
    rng = np.random.default_rng(41)
    pts = ((cells + rng.uniform(0.1, 0.9, cells.shape)) * LEAF).astype(np.float32)
    return pts[rng.permutation(DENSE_CELLS)]


@functools.lru_cache(maxsize=None)
def dense_calls():
    """two calls, one point per cell of a 67 x 67 x 67 block (its first 300,007 cells) that overlaps the sparse scene"""
    pts = _dense_points()
    half = DENSE_CELLS // 2
    return ((pts[:half], IDENTITY), (pts[half:], IDENTITY))


@functools.lru_cache(maxsize=None)
def dense_reference():
    return mref.reference_of(dense_calls(), LEAF)


# ---- table A and part C: the sparse scene ----
@functools.lru_cache(maxsize=None)
def sparse_calls():
    """five calls that each see about 45 % of 7,000 surface points, with a little noise"""
    rng = np.random.default_rng(43)
    lo, hi = np.array([-2.0, -1.5, 1.0]), np.array([2.0, 1.5, 6.0])
    base = rng.uniform(lo, hi, size=(7000, 3))
    calls = []
    for _ in range(5):
        pick = rng.random(len(base)) < 0.45
        calls.append(((base[pick] + rng.normal(0.0, 0.004, (int(pick.sum()), 3))).astype(np.float32), IDENTITY))
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def sparse_reference():
    return mref.reference_of(sparse_calls(), LEAF)


@functools.lru_cache(maxsize=None)
def other_calls():
    """the map the sparse scene is compared and aligned with, at leaf 0.04: its points with x < 1, noisier, in two calls, and
    2,000 points anywhere in the scene's box"""
    rng = np.random.default_rng(47)
    pts = np.concatenate([p for p, _ in sparse_calls()])
    pts = pts[pts[:, 0] < 1]
    noisy = (pts.astype(np.float64) + rng.normal(0.0, 0.02, pts.shape)).astype(np.float32)
    half = len(noisy) // 2
    anywhere = rng.uniform([-2.0, -1.5, 1.0], [2.0, 1.5, 6.0], size=(2000, 3)).astype(np.float32)
    return ((noisy[:half], IDENTITY), (noisy[half:], IDENTITY), (anywhere, IDENTITY))


@functools.lru_cache(maxsize=None)
def other_reference():
    return mref.reference_of(other_calls(), LEAF_B)


# the views: (T_v_w, width, height, fx, fy, cx, cy, min_depth, max_depth), as WorldMap.render and the restatement take them
SMALL_VIEW = (rref.scene_pose(), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 5.0)
WIDE_W, WIDE_H = 523, 503                                                      # 263,069 pixels: a second round of 925 pixels, the last 157 of them a partial workgroup
WIDE_VIEW = (rref.scene_pose(), WIDE_W, WIDE_H, 200.0, 400.0, 261.0, 251.0, 0.5, 5.0)
RENDER_CASES = [(0, 1), (2, 1), (0, 2), (2, 2)]                                # (splat, min_windows)
EXTRACT_FILTERS = [(0, 0), (1, 1), (2, 1), (1, 2), (2, 3), (3, 4)]             # (min_points, min_windows)
SPARSE_PRUNE = dict(min_points=2, min_windows=3, max_age=1, box=((-1.8, -1.4, 1.1), (1.9, 1.2, 5.5)), reach=1, min_neighbors=1)
ALIGN_RADIUS = 0.08
ALIGN_POSE = np.array([1, 0, 0, 0.01, 0, 1, 0, -0.02, 0, 0, 1, 0.015], np.float64)


@functools.lru_cache(maxsize=None)
def sparse_render(view, splat, min_windows):
    """the restatement's render of the sparse scene; view: "small" or "wide" """
    v = SMALL_VIEW if view == "small" else WIDE_VIEW
    return rref.render(sparse_reference().extract(1, min_windows), *v, splat=splat)


@functools.lru_cache(maxsize=None)
def sparse_compare(forward, radius):
    """the restatement's compare of the sparse scene with the other map (forward), or of the other map with it"""
    a, b = sparse_reference().extract(), other_reference().extract()
    if forward:
        return eref.compare(a, b, LEAF_B, radius, eref.N_BINS)
    return eref.compare(b, a, LEAF, radius, eref.N_BINS)


# the states that k_map_import_build's counters [0] to [5] refuse, every bad cell at an index of the second round: the first
# item of that round, two that share a wave, the last item of a full workgroup, and the last item of all (a partial workgroup)
BAD_INDICES = (ROUND, ROUND + 5, ROUND + 6, ROUND + 255, ROUND + 256, ROUND + 20_000, DENSE_CELLS - 1)


def second_round_bad_states(whole):
    """(counter, the word the refusal names, state); as map_merge_reference.bad_states builds its states"""
    idx = np.asarray(BAD_INDICES)
    assert (idx >= ROUND).all() and (idx < len(whole["keys"])).all()

    def vary(**kw):
        s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in whole.items()}
        for k, v in kw.items():
            s[k][idx] = v
        return s
    n = whole["n"][idx].astype(np.uint64)
    over = whole["S"][idx].copy()
    over[:, 1] = (n << np.uint64(32)) + np.uint64(1)
    return [(0, "keys", vary(keys=np.uint64(0))),
            (1, "keys", vary(keys=whole["keys"][:len(idx)])),                 # duplicates of cells of the first round
            (2, "n", vary(n=np.uint32(0))),
            (3, "windows", vary(windows=np.uint32(0))),
            (4, "stamp", vary(stamp=np.uint32(whole["calls"] + 1))),
            (5, "sums", vary(S=over))]


# ---- part B: runs of occupied slots that cross the table's end ----
CHAIN_LEAF = 0.5
CHAIN_RADIUS = 0.6                                                             # reach 2 at leaf 0.5
CHAIN_PRUNE = dict(reach=1, min_neighbors=1)
CHAINS = {"2^8": dict(log2=8, half=8, tail=16, take=120), "2^19": dict(log2=19, half=56, tail=64, take=100)}


def linear_probing(homes, capacity):
    """the slots occupied after inserting keys with these home slots by linear probing (bool [capacity]); the set does not
    depend on the order of insertion"""
    occ = np.zeros(capacity, bool)
    for h in homes:
        h = int(h)
        while occ[h]:
            h = (h + 1) & (capacity - 1)
        occ[h] = True
    return occ


def run_across_the_end(occ):
    """(first slot, length) of the run of occupied slots that holds slot capacity - 1 and slot 0; None without one"""
    cap = len(occ)
    if not (occ[cap - 1] and occ[0]) or occ.all():
        return None
    back = 0
    while occ[cap - 1 - back]:
        back += 1
    fwd = 0
    while occ[fwd]:
        fwd += 1
    return cap - back, back + fwd


def in_run(slots, run, capacity):
    first, length = run
    return ((np.asarray(slots, np.int64) - first) % capacity) < length


@functools.lru_cache(maxsize=None)
def chain(name):
    """dict of one chain's inputs: capacity, log2; cells (the chain, int64 (take, 3)), spare (further cells with a home in the
    tail, not inserted by `first`); the calls `first` (one point per chain cell) and `again` (40 chain cells once more, then
    the +x neighbours of 30 chain cells: at most 72 points, so a 2^8-slot table keeps its size); other_calls (a map of the
    chain shifted by one cell in x and of the -x neighbours of spare cells: compared with the chain it looks up present
    keys, and absent keys whose home lies in the run); guest_calls (a map of at most 40 cells, chain cells and spare ones:
    what is merged and integrated INTO the chain without growing it)"""
    p = CHAINS[name]
    cap = 1 << p["log2"]
    g = np.arange(-p["half"], p["half"])
    lattice = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], axis=1)
    tail = lattice[pcref.engine_bucket(lattice[:, 0], lattice[:, 1], lattice[:, 2], cap) >= cap - p["tail"]]
    cells, spare = tail[:p["take"]], tail[p["take"]:]
    rng = np.random.default_rng(53)
    pts = lambda c: ((c + rng.uniform(0.1, 0.9, c.shape)) * CHAIN_LEAF).astype(np.float32)
    x1 = np.array([1, 0, 0])
    first = pts(cells)
    again = np.concatenate([pts(cells[-40:]), pts(cells[:30] + x1)])
    other = np.unique(np.concatenate([cells + x1, spare[:40] - x1]), axis=0)
    guest = np.concatenate([cells[::4], spare[:10]])
    return dict(name=name, log2=p["log2"], capacity=cap, cells=cells, spare=spare, first=(first, IDENTITY), again=(again, IDENTITY),
                other_calls=((pts(other[::2]), IDENTITY), (pts(other[1::2]), IDENTITY), (pts(other[::3]), IDENTITY)),
                guest_calls=((pts(guest), IDENTITY), (pts(guest[5:25]), IDENTITY)))


def chain_reference(name, calls=("first", "again")):
    ch = chain(name)
    return mref.reference_of([ch[k] for k in calls], CHAIN_LEAF)


def chain_run(name):
    """(occupancy of `first` under linear probing, its run across the end)"""
    ch = chain(name)
    occ = linear_probing(home_slots(ref.pack_key(ch["cells"]), ch["capacity"]), ch["capacity"])
    return occ, run_across_the_end(occ)


def duplicated(state, keys, take):
    """`state` with `take` of its cells -- those of `keys`, the last ones -- listed a second time"""
    again = np.flatnonzero(np.isin(state["keys"], keys))[-take:]
    assert len(again) == take
    out = {k: (np.concatenate([v, v[again]]) if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    out["accepted"] = int(out["n"].astype(np.uint64).sum())                    # (so that only the keys are wrong)
    return out


# ---- part C: one map, five layouts ----
def grown_from(calls, leaf, log2):
    """the capacity of a table created at 2^log2 slots after these calls, by the 3/4 rule"""
    cap, rm = 1 << log2, mref.MergeReferenceMap(leaf)
    for pts, T in calls:
        cap, _ = mref.grown_capacity(cap, len(rm.keys), len(pts))
        rm.integrate(pts, T)
    return cap


LAYOUTS = ("grown from 2^8", "2^16", "2^19", "2^20", "2^19 shrunk")
