"""The oracle's side of tests/tie_run_cases.py: its DSI of a case, computed once per session and shared by
tests/test_tie_run_cases_cpu.py and tests/test_gpu_tie_runs.py.  TEST INFRASTRUCTURE (imports oracle/)."""
import functools

import numpy as np

import tie_run_cases as T
from oracle_pipeline import OracleMapper


def oracle_mapper(case, exact=False):
    nz, lo, hi = case.shape
    r = OracleMapper(case.cam, dimZ=nz, min_depth=lo, max_depth=hi, exact=exact)
    if case.first.size:                                     # (no whole packet: nothing votes, the DSI stays zero)
        r.evaluate_packets(case.x, case.y, case.first.astype(np.int64), case.Rt)
    elif exact:
        r.acc, r.count = np.zeros(r.dsi.shape, np.uint64), np.zeros(r.dsi.shape, np.uint32)
    return r


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's fp32 event-order DSI of a case [nz][ny][nx]; never written to."""
    dsi = oracle_mapper(T.case(name)).dsi
    dsi.setflags(write=False)
    return dsi
