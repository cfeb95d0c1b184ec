"""Call sequences for ONE long-lived mapper, and their exact expected outputs (CPU only; no GPU, no engine).

A mapper carries per-object device scratch that is grown, never cleared, and shared by entry points with different table
layouts.  test_gpu_mapper_reuse.py runs the sequences below on one mapper each and holds every step to the exact
reference; test_mapper_sequences_cpu.py checks, against the reference alone, that the sequences cover what they claim and
that a stale result of the previous step could not pass.

A step is (state class, knobs, freshly drawn input).  The state classes are the distinct things a call leaves behind:

    W   VOTE_LDS_BANDS, lane mapping 0 (per-packet waves)
    P   lane mapping 1, 3 or 7 (packed lanes; the class rotates through them)
    G   lane mapping 2 or 4 (packet groups: spk, gcuts, the groups' rowstart)
    Vt  lane mapping 5 or 6 with the cut table (set_inline_cuts(-1))
    Vi  lane mapping 5 or 6 with set_inline_cuts(0): `cuts` holds the transposed u16 row table
    A   VOTE_GLOBAL_ATOMIC
    Z   a call with 0 packets (evaluateDSI_batch of an empty batch: fillVoxelGrid returns before the vote when it has none)
    F   the mapper is camera 0 of a two-camera computeDepthMapOfEvents (halo-row tables, pair_work)

Knobs, all in fixed order and PER CLASS: every class rotates through its lane mappings, through BANDS where it has bands,
and through PACKETS (each class from another entry, so that neighbouring steps differ in size); every third banded step
is an accumulate step (two fillVoxelGrid calls without a reset between them, two inputs, expected fl32(old + new));
kernel timing is toggled every fourth step of a sequence.

Sequences: an Eulerian circuit of the complete directed graph on the eight classes (56 ordered pairs), cut into pieces of
at most 12 steps, each starting with the last step of the piece before (TRANSITIONS, 96 x 72 x 12); six seeded random
sequences of eight steps (RANDOM, 131 x 97 x 7: odd width, ragged last band); and, since a class meets a piece of the
circuit only once or twice, one sequence per banded class in which that class ALONE walks PACKETS there and back
(CYCLES: 40 1 13 70 5 64 2 64 5 70 13 1 40, the shapes alternating): every change of the list in both directions on one
mapper under one table layout, scratch that shrinks after it grew, and for Vi the transposed table's stride going
64 -> 128 -> 64 (twice).  Z is never next to Z.

Input: exact_case of test_exact_reference.py (multiplicity-1024 bursts, dead packets, special coordinates and centres);
with fewer than its 8 packets, a random packet first (so that even one packet is new input), then the hostile ones
(burst, 7-location pool, dead, one-row).  An F step has events instead: random pixels, one single-pixel packet (half a
packet where the camera has only one), small random poses.

Not included: the 32-bit record-offset fallback (from 349,525 packets in one call on) and lane mapping 8 (paired cells,
not exact) cannot be reached at a test's size.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import oracle as orc
from oracle_pipeline import OracleMapper
from test_exact_reference import exact_case

CLASSES = ("W", "P", "G", "Vt", "Vi", "A", "Z", "F")
BANDED = ("W", "P", "G", "Vt", "Vi")
MAPPINGS = {"W": (0,), "P": (1, 3, 7), "G": (2, 4), "Vt": (5, 6), "Vi": (5, 6), "F": (1, 3, 5, 6)}
BANDS = [None, (5, 1, 256), (7, 3, 512), (16, 8, 1024)]          # BANDS of test_gpu_exact_voxels.py
PACKETS = (40, 1, 13, 70, 5, 64, 2)
FUSE_OPS = (1, 2, 3, 4, 5, 6)
MIN_DEPTH, MAX_DEPTH = 1.0, 6.5
TRANSITION_SHAPE = (96, 72, 12)
RANDOM_SHAPE = (131, 97, 7)
MAX_STEPS = 12
PACKET = 1024

# mapping: lane mapping asked for (None: A and Z); band: (rows, chunks, block) or None; n_packets: camera 0's;
# n_packets1 / op: camera 1's packets and the fusion op of an F step
Step = namedtuple("Step", "cls mapping band n_packets accumulate timing n_packets1 op")
Sequence = namedtuple("Sequence", "name shape seed steps")


def camera(shape):
    nx, ny, _ = shape
    return (nx, ny, 0.8 * max(nx, 4), 0.8 * max(nx, 4), 0.5 * nx, 0.5 * ny)


def grid(shape):
    """(planes, virtual camera) a mapper of camera(shape) has."""
    nx, ny, nz = shape
    cam = camera(shape)
    return orc.depth_planes(MIN_DEPTH, MAX_DEPTH, nz), np.array([cam[2], cam[3], cam[4], cam[5]], np.float32)


def euler_circuit(n):
    """Hierholzer on the complete directed graph without loops: n (n - 1) + 1 vertices, every ordered pair once."""
    unused = {v: [w for w in range(n) if w != v] for v in range(n)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop(0))
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


class _Knobs:
    """The fixed-order rotations (one object per build of all the sequences)."""

    def __init__(self):
        self.map_i = dict.fromkeys(CLASSES, 0)
        self.band_i = dict.fromkeys(CLASSES, 0)
        # each class starts at an entry of its own; Vi at the one with which the piece of the circuit that holds three Vi
        # steps (other classes between them) takes 13, 70, 5 packets: stride 64, 128, 64
        self.packet_i = {"W": 0, "P": 4, "G": 5, "Vt": 6, "Vi": 4, "A": 1, "Z": 0, "F": 3}
        self.banded = 0
        self.ops = 0

    def step(self, cls, index, n_packets=None):
        """The class's next step; n_packets: given by the sequence (CYCLES) instead of the class's own rotation."""
        timing = (index // 4) % 2 == 1
        if cls == "Z":
            return Step(cls, None, None, 0, False, timing, 0, 0)
        mapping = band = None
        if cls in MAPPINGS:
            mapping = MAPPINGS[cls][self.map_i[cls] % len(MAPPINGS[cls])]
            self.map_i[cls] += 1
        if cls in BANDED or cls == "F":
            band = BANDS[self.band_i[cls] % len(BANDS)]
            self.band_i[cls] += 1
        n = n_packets
        if n is None:
            n = PACKETS[self.packet_i[cls] % len(PACKETS)]
            self.packet_i[cls] += 1
        if cls == "F":
            self.ops += 1
            return Step(cls, mapping, band, n, False, timing, PACKETS[(self.ops * 3) % len(PACKETS)],
                        FUSE_OPS[self.ops % len(FUSE_OPS)])
        accumulate = False
        if cls in BANDED:
            self.banded += 1
            accumulate = self.banded % 3 == 0
        return Step(cls, mapping, band, n, accumulate, timing, 0, 0)


PACKET_WALK = PACKETS + PACKETS[-2::-1]                             # there and back


def build_sequences():
    """(TRANSITIONS, RANDOM, CYCLES): deterministic."""
    knobs = _Knobs()
    circuit = [CLASSES[v] for v in euler_circuit(len(CLASSES))]
    transitions, start = [], 0
    while start < len(circuit) - 1:
        piece = circuit[start:start + MAX_STEPS]
        steps = tuple(knobs.step(c, i) for i, c in enumerate(piece))
        transitions.append(Sequence("transitions-%d" % len(transitions), TRANSITION_SHAPE, 9100 + len(transitions), steps))
        start += MAX_STEPS - 1
    random = []
    for k in range(6):
        rng = np.random.default_rng(4400 + k)
        classes = []
        while len(classes) < 8:
            c = CLASSES[int(rng.integers(len(CLASSES)))]
            if not (c == "Z" and classes and classes[-1] == "Z"):
                classes.append(c)
        steps = tuple(knobs.step(c, i) for i, c in enumerate(classes))
        random.append(Sequence("random-%d" % k, RANDOM_SHAPE, 9200 + k, steps))
    cycles = []
    for k, c in enumerate(BANDED):
        steps = tuple(knobs.step(c, i, n) for i, n in enumerate(PACKET_WALK))
        cycles.append(Sequence("cycle-%s" % c, (TRANSITION_SHAPE, RANDOM_SHAPE)[k % 2], 9300 + k, steps))
    return tuple(transitions), tuple(random), tuple(cycles)


TRANSITIONS, RANDOM, CYCLES = build_sequences()
ALL = TRANSITIONS + RANDOM + CYCLES

# exact_case: a random packet (centre between two planes), then burst, pool of 7, dead, one row, then the rest
SMALL_ORDER = (3, 6, 7, 4, 5, 0, 1, 2)


def draw_fill(rng, shape, n_packets):
    """(xy [n * 1024][2], centres [n][3]) for fillVoxelGrid."""
    nx, ny, _ = shape
    planes, _ = grid(shape)
    xy, centers = exact_case(rng, nx, ny, max(n_packets, 8), planes)
    if n_packets < 8:
        keep = np.array(SMALL_ORDER[:n_packets])
        xy = xy.reshape(8, PACKET, 2)[keep].reshape(-1, 2)
        centers = centers[keep]
    return np.ascontiguousarray(xy, np.float32), np.ascontiguousarray(centers, np.float32)


def draw_events(rng, shape, n_packets, offset_x):
    """(x, y uint16 [n * 1024], Rt [n][12]) of one camera of an F step: random pixels, the last packet one pixel (1024
    events of one location; the last HALF packet where the camera has only one, so that its volume is still drawn),
    poses a few hundredths of a radian and of a metre from the reference view."""
    nx, ny, _ = shape
    x = rng.integers(0, nx, n_packets * PACKET).astype(np.uint16)
    y = rng.integers(0, ny, n_packets * PACKET).astype(np.uint16)
    burst = PACKET if n_packets > 1 else PACKET // 2
    x[-burst:], y[-burst:] = nx // 3, ny // 2
    Rt = np.empty((n_packets, 12), np.float32)
    for k in range(n_packets):
        a, b, c = rng.normal(0.0, 0.01, 3)
        R = np.array([[1, -c, b], [c, 1, -a], [-b, a, 1]], np.float64)
        u, _, vt = np.linalg.svd(R)
        Rt[k, :9] = (u @ vt).reshape(-1)
        Rt[k, 9:] = rng.normal(0.0, 0.05, 3) + (offset_x, 0.0, 0.0)
    return x, y, Rt


def draw_inputs(seq):
    """One input per step, in order, all from the sequence's generator.  fill steps: [(xy, centres)] (two for an
    accumulate step); Z: []; F: [(x, y, Rt) of camera 0, of camera 1]."""
    rng = np.random.default_rng(seq.seed)
    out = []
    for s in seq.steps:
        if s.cls == "Z":
            out.append([])
        elif s.cls == "F":
            out.append([draw_events(rng, seq.shape, s.n_packets, 0.0), draw_events(rng, seq.shape, s.n_packets1, 0.12)])
        else:
            out.append([draw_fill(rng, seq.shape, s.n_packets) for _ in range(2 if s.accumulate else 1)])
    return out


Expected = namedtuple("Expected", "dsi acc count conf idx")


def expected_step(shape, step, inputs):
    """The exact reference's output of one step.  dsi: what the mapper's DSI holds (F: what camera 0's events vote, the
    volume the fused kernel never writes); acc / count: the Q33.31 sums and vote counts (the global-atomic bound);
    conf / idx: the fused depth map of an F step."""
    nx, ny, nz = shape
    planes, Kv = grid(shape)
    if step.cls == "Z":
        zero = np.zeros((nz, ny, nx), np.float32)
        return Expected(zero, zero.astype(np.uint64), zero.astype(np.uint32), None, None)
    if step.cls == "F":
        vols = []
        for x, y, Rt in inputs:
            r = OracleMapper(camera(shape), dimZ=nz, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, exact=True)
            assert np.array_equal(r.planes, planes) and np.array_equal(r.Kv, Kv)
            r.evaluate_packets(x, y, np.arange(Rt.shape[0], dtype=np.int64) * PACKET, Rt)
            vols.append(r)
        fused = orc.fuse2(orc.accumulate(np.zeros_like(vols[0].dsi), vols[0].dsi, 0), vols[1].dsi, step.op)
        conf, idx = orc.collapse_max_z(fused)
        return Expected(vols[0].dsi, vols[0].acc, vols[0].count, conf, idx)
    dsi = acc = count = None
    for xy, centers in inputs:
        a, c = orc.fill_voxel_grid_q31(xy, centers, planes, Kv, nx, ny)
        new = orc.q31_to_float(a)
        dsi = new if dsi is None else dsi + new            # numpy fp32 +: one IEEE rounding
        acc = a if acc is None else acc + a
        count = c if count is None else count + c
    return Expected(dsi, acc, count, None, None)


@functools.lru_cache(maxsize=None)
def inputs_and_expected(name):
    """(inputs, expected) per step of the named sequence; computed once, shared, never changed by a test."""
    seq = next(s for s in ALL if s.name == name)
    inputs = draw_inputs(seq)
    return inputs, [expected_step(seq.shape, s, i) for s, i in zip(seq.steps, inputs)]
