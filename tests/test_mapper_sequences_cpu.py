"""The mapper call sequences of mapper_sequence_cases.py, checked against the reference alone (CPU only): they cover what
test_gpu_mapper_reuse.py relies on, and no step's expected output could be met by what an earlier step left behind."""
import numpy as np

import mapper_sequence_cases as msc

MEASURED_MIN_FRACTION = 0.8226   # what test_consecutive_expected_outputs_differ printed
FLOOR = 0.5 * MEASURED_MIN_FRACTION


def _pairs(seqs, key=lambda s: s.cls):
    return {(key(a), key(b)) for q in seqs for a, b in zip(q.steps, q.steps[1:])}


def _contains(seq, run):
    return any(list(seq[k:k + len(run)]) == list(run) for k in range(len(seq) - len(run) + 1))


def test_every_ordered_pair_of_state_classes_occurs():
    pairs = _pairs(msc.TRANSITIONS)
    want = {(a, b) for a in msc.CLASSES for b in msc.CLASSES if a != b}
    assert len(want) == 56 and want <= pairs, sorted(want - pairs)
    assert all(len(q.steps) <= msc.MAX_STEPS for q in msc.TRANSITIONS)
    for a, b in zip(msc.TRANSITIONS, msc.TRANSITIONS[1:]):
        assert a.steps[-1].cls == b.steps[0].cls        # each piece starts with the last step of the piece before
    assert len(msc.RANDOM) == 6 and all(len(q.steps) == 8 for q in msc.RANDOM)
    assert all(q.shape == msc.TRANSITION_SHAPE for q in msc.TRANSITIONS) and all(q.shape == msc.RANDOM_SHAPE for q in msc.RANDOM)
    assert {q.shape for q in msc.CYCLES} == {msc.TRANSITION_SHAPE, msc.RANDOM_SHAPE}
    assert len({q.name for q in msc.ALL}) == len(msc.ALL)


def test_every_band_plan_under_every_banded_class_and_every_mapping():
    steps = [s for q in msc.ALL for s in q.steps]
    for cls in msc.BANDED:
        assert {s.band for s in steps if s.cls == cls} == set(msc.BANDS), cls
    for cls, mappings in msc.MAPPINGS.items():
        assert {s.mapping for s in steps if s.cls == cls} == set(mappings), cls
    assert {s.band for s in steps if s.cls == "F"} == set(msc.BANDS)
    assert {s.op for s in steps if s.cls == "F"} == set(msc.FUSE_OPS)
    # accumulate steps with one chunk and with several, under timing on and off
    acc = [s for s in steps if s.accumulate]
    assert {s.cls for s in acc} == set(msc.BANDED)
    assert any(s.band and s.band[1] == 1 for s in acc) and any(s.band and s.band[1] > 1 for s in acc)
    assert {s.timing for s in steps} == {False, True}


def test_every_class_cycles_through_the_packet_counts_itself():
    """Each class takes its packet counts from PACKETS in the list's order, whatever the other classes do between."""
    for cls in msc.CLASSES:
        if cls == "Z":
            continue
        own = [s.n_packets for q in msc.TRANSITIONS + msc.RANDOM for s in q.steps if s.cls == cls]
        start = msc.PACKETS.index(own[0])
        assert own == [msc.PACKETS[(start + k) % len(msc.PACKETS)] for k in range(len(own))], cls
        assert set(own) == set(msc.PACKETS), cls


def test_every_packet_count_change_occurs_in_both_directions():
    changes = list(zip(msc.PACKETS, msc.PACKETS[1:]))
    for cls in msc.BANDED:
        # ONE sequence (one mapper) in which consecutive steps of this class, nothing between, make every change of the
        # list in both directions: scratch of this layout that shrinks after it grew, and grows after it shrank
        ok = False
        for q in msc.ALL:
            got = {(a.n_packets, b.n_packets) for a, b in zip(q.steps, q.steps[1:]) if a.cls == b.cls == cls}
            ok = ok or all((a, b) in got and (b, a) in got for a, b in changes)
        assert ok, cls
    # the transposed u16 row table (only a Vi step writes `cuts` in that layout; its stride is roundup(np, 64)): stride 64,
    # then 128, then 64 again, in this order, on ONE mapper -- with nothing between the Vi steps, and with other classes between
    stride = lambda s: (s.n_packets + 63) // 64 * 64
    adjacent = [[stride(s) if s.cls == "Vi" else None for s in q.steps] for q in msc.ALL]
    assert any(_contains(v, (64, 128, 64)) for v in adjacent)
    apart = [[stride(s) for s in q.steps if s.cls == "Vi"] for q in msc.TRANSITIONS + msc.RANDOM]
    assert any(_contains(v, (64, 128, 64)) for v in apart)
    # and, on one mapper, a Vi step reads FEWER packets than the Vi step before it within one stride (a reader past np)
    vi = next(q for q in msc.CYCLES if q.name == "cycle-Vi")
    assert all(s.cls == "Vi" for s in vi.steps) and [s.n_packets for s in vi.steps] == list(msc.PACKET_WALK)
    assert (40, 1) in _pairs([vi], key=lambda s: s.n_packets) and (64, 2) in _pairs([vi], key=lambda s: s.n_packets)


def test_zero_packet_steps_are_never_adjacent():
    assert ("Z", "Z") not in _pairs(msc.ALL)
    assert sum(s.cls == "Z" for q in msc.ALL for s in q.steps) >= 7


def test_the_sequences_are_repeatable():
    again = msc.build_sequences()
    assert again == (msc.TRANSITIONS, msc.RANDOM, msc.CYCLES)
    for q in (msc.RANDOM[0], msc.CYCLES[-1]):
        a, b = msc.draw_inputs(q), msc.draw_inputs(q)
        for sa, sb in zip(a, b):
            assert len(sa) == len(sb)
            for ia, ib in zip(sa, sb):
                assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(ia, ib))


def test_small_inputs_are_freshly_drawn():
    """A one-packet fill step is a random packet, not the fixed burst: two draws differ; so does a one-packet camera."""
    rng = np.random.default_rng(5)
    a, b = (msc.draw_fill(rng, msc.TRANSITION_SHAPE, 1) for _ in range(2))
    assert a[0].shape == (msc.PACKET, 2) and len(np.unique(a[0], axis=0)) > 900 and not np.array_equal(a[0], b[0])
    x, y, _ = msc.draw_events(rng, msc.TRANSITION_SHAPE, 1, 0.0)
    assert len(np.unique(np.stack([x, y], 1), axis=0)) > 400


def _fraction(a, b, either=None):
    if either is None:
        either = (a != 0) | (b != 0)
    return float(((a != b) & either).sum()) / max(1, int(either.sum()))


def test_consecutive_expected_outputs_differ(capsys):
    """For every step, the fraction of voxels (of those non-zero in either) in which its expected output differs from
    what the mappers could still hold from before:
      * the expected DSI of the step before (every consecutive pair; an F step's is what camera 0's events vote);
      * for a voting step, the DSI camera 0 HELD before it -- after F steps, which leave that DSI alone, the one of the
        last voting step before them;
      * for an F step, the confidence and the index map of the previous F step of the sequence, which the long-lived
        output mapper still holds (index: over the pixels with a confidence in either).
    Measured minimum over all 158 consecutive pairs and the 169 further comparisons: 0.8226 (MEASURED_MIN_FRACTION, an index
    map against the previous F step's at random-2 step 7; the smallest among the DSIs is 0.9966); the
    floor asserted is half of it, so a result left over from an earlier step cannot pass for the step's own.  No
    expected DSI is all zero except a Z step's.  (A Z step whose mapper already held zeros -- Z, F, Z -- has nothing
    to tell apart and is not measured; the Z steps that follow a vote are.)"""
    worst, where, n_pairs, n_more = 1.0, None, 0, 0
    for q in msc.ALL:
        _, exp = msc.inputs_and_expected(q.name)
        held, maps = np.zeros_like(exp[0].dsi), None
        for k, (s, e) in enumerate(zip(q.steps, exp)):
            assert e.dsi.any() == (s.cls != "Z"), (q.name, k)
            found = []
            if k:
                found.append(("the step before", _fraction(exp[k - 1].dsi, e.dsi)))
                n_pairs += 1
            if s.cls == "F":
                assert e.conf.any() and len(np.unique(e.idx)) > 1, (q.name, k)
                if maps is not None:
                    found.append(("the previous F step's confidence", _fraction(maps[0], e.conf)))
                    found.append(("the previous F step's index", _fraction(maps[1], e.idx, (maps[0] != 0) | (e.conf != 0))))
                maps = (e.conf, e.idx)
            else:
                if held.any() or e.dsi.any():
                    found.append(("the DSI held before", _fraction(held, e.dsi)))
                held = e.dsi
            n_more += len(found) - (1 if k else 0)
            for name, f in found:
                assert f >= FLOOR, (q.name, k, name, f)
                if f < worst:
                    worst, where = f, (q.name, k, name)
    with capsys.disabled():
        print("\nsmallest fraction of voxels differing from a stale result: %.4f at %s (floor %.4f; %d consecutive pairs, "
              "%d further comparisons)" % (worst, where, FLOOR, n_pairs, n_more))
    assert worst >= FLOOR
