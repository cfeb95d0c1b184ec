"""Merging world maps restated in numpy (include/dsi_map_merge.h; DESIGN.md 7j "Merging"), written from the header's rule.
MergeReferenceMap is map_prune_reference.PruneReferenceMap plus export_state / import_state / merge; everything is by
ascending key and integer.

    merge(src) into dst, off = dst.calls before:  per cell of src (a cell dst lacks starts from zeros)
        n += n_src, S += S_src, windows += windows_src, stamp = max(stamp, stamp_src + off)
    then calls += src.calls, accepted += src.accepted, rejected += src.rejected
"""
import math

import numpy as np

import map_prune_reference as pref
import world_map_reference as ref

U32_MAX = (1 << 32) - 1
MAX_LOG2 = 27
PACKED_MAX = 2 * ref.CELL_MAX + 1                                              # a packed coordinate lies in [1, 2^21 - 3]


class Refused(ValueError):
    """what the engine refuses with DSI_ERR_INVALID; args[0] names the offending thing"""


def grown_capacity(capacity, occupied, n):
    """(capacity, doublings) of map_grow_for: doubled until occupied + n <= 3/4 of the slots"""
    g = 0
    while (occupied + n) * 4 > 3 * (capacity << g):
        g += 1
    return capacity << g, g


class MergeReferenceMap(pref.PruneReferenceMap):
    def export_state(self):
        return {"leaf": self.leaf, "calls": int(self.calls), "accepted": int(self.accepted), "rejected": int(self.rejected),
                "keys": self.keys.copy(), "n": self.n.astype(np.uint32), "S": self.S.copy().reshape(-1, 3),
                "windows": self.windows.astype(np.uint32), "stamp": self.stamp.astype(np.uint32)}

    def _check_counters(self, cells, calls, accepted):
        if calls > U32_MAX or self.calls + calls > U32_MAX:
            raise Refused("calls")
        if accepted > U32_MAX or self.accepted + accepted > U32_MAX:
            raise Refused("accepted")
        if cells > (1 << MAX_LOG2) or (len(self.keys) + cells) * 4 > (3 << MAX_LOG2):
            raise Refused("cells")

    def merge(self, other):
        """appends `other`; returns dict of n_src_cells, n_new, n_common"""
        if other is self:
            raise Refused("same map")
        if np.float64(self.leaf).tobytes() != np.float64(other.leaf).tobytes():
            raise Refused("leaf")
        self._check_counters(len(other.keys), other.calls, other.accepted)
        return self._append(other.keys, other.n, other.S, other.windows, other.stamp, other.calls, other.accepted, other.rejected)

    def _append(self, keys, n, S, windows, stamp, calls, accepted, rejected):
        off = np.uint64(self.calls)
        allk = np.union1d(self.keys, keys)
        out_n, out_w, out_s = (np.zeros(len(allk), np.uint64) for _ in range(3))
        out_S = np.zeros((len(allk), 3), np.uint64)
        old = np.searchsorted(allk, self.keys)
        out_n[old], out_S[old], out_w[old], out_s[old] = self.n, self.S, self.windows, self.stamp
        idx = np.searchsorted(allk, keys)                                      # (keys are distinct: plain indexed adds)
        out_n[idx] += n.astype(np.uint64)
        out_S[idx] += S.astype(np.uint64).reshape(-1, 3)
        out_w[idx] += windows.astype(np.uint64)
        out_s[idx] = np.maximum(out_s[idx], stamp.astype(np.uint64) + off)
        n_common = int(np.isin(keys, self.keys).sum())
        self.keys, self.n, self.S, self.windows, self.stamp = allk, out_n, out_S, out_w, out_s
        self.calls += int(calls)
        self.accepted += int(accepted)
        self.rejected += int(rejected)
        return {"n_src_cells": len(keys), "n_new": len(keys) - n_common, "n_common": n_common}

    def import_state(self, state):
        """merge() with an exported state as the source, validated as dsx_map_import validates it"""
        leaf = float(state["leaf"])
        if not (math.isfinite(leaf) and leaf > 0.0):
            raise Refused("leaf")
        keys = np.asarray(state["keys"], np.uint64).reshape(-1)
        m = len(keys)
        if m > (1 << MAX_LOG2):
            raise Refused("n_cells")
        if np.float64(self.leaf).tobytes() != np.float64(leaf).tobytes():
            raise Refused("leaf")
        calls, accepted, rejected = int(state["calls"]), int(state["accepted"]), int(state["rejected"])
        self._check_counters(m, calls, accepted)
        n, w, s = (np.asarray(state[k], np.uint32).reshape(-1).astype(np.uint64) for k in ("n", "windows", "stamp"))
        S = np.asarray(state["S"], np.uint64).reshape(-1, 3)
        packed = np.stack([(keys >> np.uint64(21 * a)) & np.uint64(0x1FFFFF) for a in range(3)], axis=-1)
        if ((keys == 0) | (keys >> np.uint64(63) != 0) | ((packed < 1) | (packed > PACKED_MAX)).any(axis=-1)).any():
            raise Refused("keys")
        if len(np.unique(keys)) != m:
            raise Refused("keys")
        if (n == 0).any():
            raise Refused("n")
        if ((w == 0) | (w > n) | (w > s)).any():
            raise Refused("windows")
        if ((s == 0) | (s > np.uint64(calls))).any():
            raise Refused("stamp")
        if (S > (n << np.uint64(32))[:, None]).any():
            raise Refused("sums")
        if accepted < int(n.sum()):
            raise Refused("accepted")
        return self._append(keys, n, S, w, s, calls, accepted, rejected)


def assert_states_equal(got, want):
    """array_equal on every array of two exported states, and equal headers"""
    for k in ("leaf", "calls", "accepted", "rejected"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("keys", "n", "S", "windows", "stamp"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def reference_of(calls, leaf=pref.LEAF):
    rm = MergeReferenceMap(leaf)
    for pts, T in calls:
        rm.integrate(pts, T)
    return rm


# ---- states that an import must refuse: the CPU and the GPU tests run the same list ----
def bad_states(whole):
    """(name, the word the refusal names, state): one violated bound each"""
    def vary(**kw):
        s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in whole.items()}
        for k, (i, v) in kw.items():
            if i is None:
                s[k] = v
            else:
                s[k][i] = v
        return s
    k0 = int(whole["keys"][0])
    big = int(np.argmax(whole["n"]))                                           # a cell with n >= 2
    assert whole["n"][big] >= 2
    return [
        ("key 0", "keys", vary(keys=(5, 0))),
        ("x coordinate 0", "keys", vary(keys=(0, k0 & ~0x1FFFFF))),
        ("y coordinate 2^21 - 2", "keys", vary(keys=(0, (k0 & ~(0x1FFFFF << 21)) | (((1 << 21) - 2) << 21)))),
        ("z coordinate 2^21 - 1", "keys", vary(keys=(0, (k0 & ~(0x1FFFFF << 42)) | (0x1FFFFF << 42)))),
        ("bit 63", "keys", vary(keys=(0, k0 | (1 << 63)))),
        ("duplicate key", "keys", vary(keys=(7, int(whole["keys"][8])))),
        ("n 0", "n", vary(n=(3, 0), windows=(3, 0))),
        ("windows 0", "windows", vary(windows=(3, 0))),
        ("windows > n", "windows", vary(windows=(3, int(whole["n"][3]) + 1), stamp=(3, 8))),
        ("windows > stamp", "windows", vary(windows=(big, 2), stamp=(big, 1))),
        ("stamp 0", "windows", vary(stamp=(3, 0))),                            # (windows >= 1 > stamp: named first)
        ("stamp > calls", "stamp", vary(stamp=(3, whole["calls"] + 1))),
        ("S > n 2^32", "sums", vary(S=((3, 1), (int(whole["n"][3]) << 32) + 1))),
        ("accepted < sum n", "accepted", vary(accepted=(None, int(whole["n"].sum()) - 1))),
        ("leaf nan", "leaf", vary(leaf=(None, float("nan")))),
        ("leaf 0", "leaf", vary(leaf=(None, 0.0))),
        ("leaf inf", "leaf", vary(leaf=(None, float("inf")))),
        ("leaf one ulp off", "leaf", vary(leaf=(None, float(np.nextafter(whole["leaf"], 1.0))))),
    ]


def header_states(leaf, dst_calls, dst_accepted):
    """states without cells whose counters alone are out of bounds for a destination with the given counters"""
    empty = {"keys": np.zeros(0, np.uint64), "n": np.zeros(0, np.uint32), "S": np.zeros((0, 3), np.uint64),
             "windows": np.zeros(0, np.uint32), "stamp": np.zeros(0, np.uint32), "leaf": leaf, "rejected": 0}
    top = U32_MAX
    return [("calls sum", "calls", dict(empty, calls=top - dst_calls + 1, accepted=0)),
            ("calls alone", "calls", dict(empty, calls=1 << 40, accepted=0)),
            ("accepted sum", "accepted", dict(empty, calls=0, accepted=top - dst_accepted + 1)),
            ("accepted alone", "accepted", dict(empty, calls=0, accepted=1 << 40))], \
           [dict(empty, calls=top - dst_calls, accepted=top - dst_accepted)]    # the bounds themselves are legal
