"""Child process of tests/test_gpu_lifecycle.py: one object of every kind is created and used, and main returns without
closing any -- the interpreter's exit (engine.py's atexit hook: children first, then contexts) has to take them down."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dvs_mcemvs_amd as d  # noqa: E402
import lifecycle_cases as cases  # noqa: E402

KEEP = []


def main():
    ctx = d.Context(0)
    KEEP.append(ctx)
    for name in sorted(cases.CASES):
        objs, out = cases.CASES[name](ctx)
        KEEP.extend(objs)
        assert out
    ctx.synchronize()
    print("LIFECYCLE_CHILD_OK %d objects left open" % len(KEEP), flush=True)


if __name__ == "__main__":
    main()
