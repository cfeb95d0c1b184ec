#!/usr/bin/env python
"""Generates tests/golden/grid3d_ops.npz: 8,192 input pairs and what the GENUINE members subtractTwoGrids,
ratioTwoGrids, quadraticMeanTwoGrids and cubicMeanTwoGrids of the reference's cartesian3dgrid.h make of them.

    python tests/golden/make_grid3d_ops.py <path of the reference tree>

compiles make_grid3d_ops.cpp (beside this file) with g++ against the reference header, included by path from the
given tree, and a stand-in <opencv2/core/core.hpp> written to a temporary directory; runs it; stores inputs and
outputs.  No -march flag: baseline x86-64 has no FMA, so the header's fp32 expressions round per operation.  The
binary, the stand-in and the raw files are temporary.  The fixture also records which overload the header's
unqualified fabs() resolved to (`fabs_is_double`) and which pairs tell the two readings of ratioTwoGrids apart.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import grid3d_reference as ref  # noqa: E402

F = np.float32
N = 8192

STANDIN = """#pragma once
// stand-in for <opencv2/core/core.hpp>: the members of cv::Mat that cartesian3dgrid.h touches
// <cmath>: the reference header uses std::sqrt / std::cbrt / fabs and includes no math header of its own; OpenCV's
// core headers supply <cmath> (opencv2/core/cvstd.hpp).  <math.h> is NOT included: with libstdc++ that wrapper would
// add the float overloads of fabs to the global namespace and flip the reading of ratioTwoGrids (DESIGN.md 7d).
#include <cmath>
#include <cstddef>
#include <vector>
#define CV_8U 0
#define CV_32FC1 5
namespace cv {
class Mat {
public:
    int rows = 0, cols = 0;
    Mat() {}
    Mat(int r, int c, int) : rows(r), cols(c), buf_((std::size_t)r * c * 4) {}
    template <typename T> T& at(int y, int x) { return reinterpret_cast<T*>(buf_.data())[(std::size_t)y * cols + x]; }
    template <typename T> const T& at(int y, int x) const { return reinterpret_cast<const T*>(buf_.data())[(std::size_t)y * cols + x]; }
private:
    std::vector<unsigned char> buf_;
};
}
"""


def inputs():
    rng = np.random.default_rng(20261017)
    parts = []

    def pairs(a, g):
        parts.append(np.stack([np.asarray(a, F), np.asarray(g, F)], 1))

    # vote-like magnitudes in [0, 50): sums of bilinear weights
    pairs(rng.random(5632) * 50, rng.random(5632) * 50)
    # coarse values (quarters): many exact results and ties
    pairs(rng.integers(0, 200, 256) / 4.0, rng.integers(0, 200, 256) / 4.0)
    # exact zeros in either or both operands
    z = rng.random(256) * 50
    pairs(np.concatenate([np.zeros(112), z[:112], np.zeros(32)]), np.concatenate([z[112:224], np.zeros(112), np.zeros(32)]))
    # negatives
    pairs(rng.random(512) * 100 - 50, rng.random(512) * 100 - 50)
    # subnormals (and the smallest normals)
    sub = (rng.integers(1, 1 << 24, 256).astype(np.uint32)).view(F)
    pairs(sub[:128] * np.where(rng.random(128) < 0.5, -1, 1), np.where(rng.random(128) < 0.5, sub[128:], rng.random(128)))
    # +-inf, NaN, +-0 against each other and against ordinary values
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.5, -2.25, 3.0e38], F)
    aa, gg = np.meshgrid(sp, sp, indexing="ij")
    pairs(aa.ravel(), gg.ravel())
    # near FLT_MAX: squares and cubes overflow in fp32
    big = (np.finfo(F).max * (1 - rng.random(128) * 0.5)).astype(F)
    pairs(big * np.where(rng.random(128) < 0.3, -1, 1), np.where(rng.random(128) < 0.5, big[::-1], rng.random(128) * 1e20))
    # pairs on which the two readings of ratioTwoGrids (all fp32 / sum and quotient in double) give different floats
    have = sum(p.shape[0] for p in parts)
    want = N - have
    found = []
    while sum(f.shape[0] for f in found) < want:
        a = (rng.random(1 << 18) * 50).astype(F)
        g = (rng.random(1 << 18) * 50).astype(F)
        d = ref.binary_op(a, g, ref.OP_RATIO, True).view(np.uint32) != ref.binary_op(a, g, ref.OP_RATIO, False).view(np.uint32)
        found.append(np.stack([a[d], g[d]], 1))
    parts.append(np.concatenate(found)[:want])
    ag = np.concatenate(parts).astype(F)
    assert ag.shape == (N, 2), ag.shape
    return ag, have


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    inc = os.path.join(sys.argv[1], "cartesian3dgrid", "include")
    assert os.path.exists(os.path.join(inc, "cartesian3dgrid", "cartesian3dgrid.h")), inc
    ag, first_ratio_pair = inputs()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "standin", "opencv2", "core"))
        with open(os.path.join(tmp, "standin", "opencv2", "core", "core.hpp"), "w") as f:
            f.write(STANDIN)
        exe = os.path.join(tmp, "gen")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(tmp, "standin"), "-I", inc,
                               os.path.join(HERE, "make_grid3d_ops.cpp"), "-o", exe])
        ag.tofile(os.path.join(tmp, "pairs.bin"))
        said = subprocess.run([exe, os.path.join(tmp, "pairs.bin"), os.path.join(tmp, "out.bin")], check=True,
                              capture_output=True, text=True).stdout
        print(said.strip())
        out = np.fromfile(os.path.join(tmp, "out.bin"), F).reshape(4, N)
    fabs_is_double = "double overload" in said
    np.savez_compressed(os.path.join(HERE, "grid3d_ops.npz"), a=ag[:, 0].copy(), g=ag[:, 1].copy(), subtract=out[0],
                        ratio=out[1], quadratic_mean=out[2], cubic_mean=out[3], fabs_is_double=np.int32(fabs_is_double),
                        first_ratio_pair=np.int32(first_ratio_pair))
    for k, name in enumerate(("subtract", "ratio", "quadratic_mean", "cubic_mean")):
        mine = ref.binary_op(ag[:, 0], ag[:, 1], k + 1, fabs_is_double)
        bad = np.flatnonzero(~ref.same_bits(mine, out[k]))
        print("%-15s restatement differs on %d of %d" % (name, bad.size, N))
        for i in bad[:8]:
            print("    a=%r g=%r header=%r restatement=%r" % (ag[i, 0], ag[i, 1], out[k][i], mine[i]))


if __name__ == "__main__":
    main()
