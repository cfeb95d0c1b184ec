"""Creation and destruction of every kind of engine object on the MI355X.  The host layer frees device memory, events and
streams through owning members (dvs_mcemvs_amd/csrc/dsi_owned.hpp); here each kind is created, made to allocate its scratch
with the smallest call that does (tests/lifecycle_cases.py: 32 x 24 sensor, 8 planes, two packets) and destroyed, three
times over in one process, and the last round must give the first round's bits.  Communicators hold no device resource of
the engine's own and are left to tests/test_gpu_multirank.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import lifecycle_cases as cases
from dvs_mcemvs_amd import engine as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def code_of(fn):
    try:
        fn()
    except d.DsiError as e:
        return e.code
    return E.OK


@pytest.mark.parametrize("kind", sorted(cases.CASES))
def test_three_rounds_of_create_use_destroy(built, kind):
    rounds = []
    for _ in range(3):
        ctx = d.Context(0)  # (the context is one of the kinds: a fresh one per round)
        objs, out = cases.CASES[kind](ctx)
        for o in objs:
            o.close()
        assert d.load_library().dsi_context_destroy(ctx._h) == E.OK
        ctx._h = C.c_void_p()
        rounds.append(out)
    first, last = rounds[0], rounds[-1]
    assert sorted(first) == sorted(last)
    for k in first:
        a, b = np.asarray(first[k]), np.asarray(last[k])
        assert a.size > 0 and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (kind, k)


def test_failed_creates_leave_the_context_destroyable(built):
    ctx = d.Context(0)
    cam = cases.rig()["cam"]
    assert code_of(lambda: d.MapperEMVS(ctx, cam, d.ShapeDSI(0, 0, 0, 4.0, 200.0, 0.0))) == E.ERR_INVALID      # no plane
    assert code_of(lambda: d.MapperEMVS(ctx, cam, d.ShapeDSI(0, 0, 8, 4.0, 2.0, 0.0))) == E.ERR_INVALID        # max < min depth
    K = [[cam[2], 0, cam[4]], [0, cam[3], cam[5]], [0, 0, 1]]
    bad_lens = d.Lens("plumb_bob", K, (0.1, 0.2, 0.3))                                                         # three coefficients
    assert code_of(lambda: d.MapperEMVS(ctx, cam, cases.shape(), lens=bad_lens)) == E.ERR_INVALID
    for log2 in (7, 28):                                                                                       # 8..27
        assert code_of(lambda: d.WorldMap(ctx, 0.05, log2)) == E.ERR_INVALID
    assert d.load_library().dsi_context_destroy(ctx._h) == E.OK
    ctx._h = C.c_void_p()


@pytest.mark.parametrize("kind", sorted(cases.CASES))
def test_a_context_goes_only_after_its_children(built, kind):
    L = d.load_library()
    ctx = d.Context(0)
    objs, _ = cases.CASES[kind](ctx)
    for o in objs:
        assert L.dsi_context_destroy(ctx._h) == E.ERR_CONTEXT
        assert b"still alive" in L.dsi_last_error()
        o.close()
    assert L.dsi_context_destroy(ctx._h) == E.OK
    ctx._h = C.c_void_p()


def test_objects_left_open_at_interpreter_exit(built):
    r = subprocess.run([sys.executable, os.path.join(HERE, "lifecycle_child.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LIFECYCLE_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
