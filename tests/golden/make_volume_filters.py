#!/usr/bin/env python
"""Generates tests/golden/volume_filters.npz: seeded volumes and what the GENUINE 3-sigma gaussianiir3d of the
reference's cartesian3dgrid/src/gaussianiir3d.cpp makes of them.

    python tests/golden/make_volume_filters.py <path of the reference tree>

writes a two-line declaration header (the source includes "cartesian3dgrid/gaussianiir3d.h", whose original drags in
the OpenCV-dependent Grid3D header) and a small driver into a temporary directory, compiles the reference source from
the given tree, unmodified, with g++ -O3 -fopenmp (the reference's flags; no -march, so no FMA), runs it and stores
inputs, sigmas and outputs.  The binary, the header, the driver and the raw files are temporary.

The file also holds diffusion and Laplacian outputs of tests/volume_filters_reference.py, keys `restated_*`: those
are RESTATED, not compiled (the reference's diffuse / laplacian3D live in a file that needs OpenCV to compile).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import volume_filters_reference as vf  # noqa: E402

F = np.float32

HEADER = """#pragma once
void gaussianiir3d(float *volume, long width, long height, long depth, float sigma, int numsteps);
void gaussianiir3d(float *volume, long width, long height, long depth, float sigma_x, float sigma_y, float sigma_z, int numsteps);
"""

DRIVER = """#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cartesian3dgrid/gaussianiir3d.h"
// argv: in out width height depth sigma_x sigma_y sigma_z numsteps
int main(int argc, char** argv)
{
    if (argc != 10) return 2;
    const long w = std::atol(argv[3]), h = std::atol(argv[4]), d = std::atol(argv[5]);
    std::vector<float> v((size_t)(w * h * d));
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(v.data(), 4, v.size(), f) != v.size()) return 3;
    std::fclose(f);
    gaussianiir3d(v.data(), w, h, d, (float)std::atof(argv[6]), (float)std::atof(argv[7]), (float)std::atof(argv[8]),
                  std::atoi(argv[9]));
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(v.data(), 4, v.size(), f) != v.size()) return 4;
    std::fclose(f);
    return 0;
}
"""

# (name, (z, y, x), (sigma_x, sigma_y, sigma_z), numsteps, impulse position or None)
CASES = [
    ("a", (3, 5, 7), (0.7, 1.3, 2.0), 3, None),
    ("b", (5, 12, 35), (0.7, 1.3, 2.0), 3, None),
    ("c", (1, 4, 65), (0.5, 0.5, 0.5), 3, None),
    ("b1", (5, 12, 35), (0.7, 1.3, 2.0), 1, None),
    ("b4", (5, 12, 35), (0.7, 1.3, 2.0), 4, None),
    ("impulse", (3, 5, 70), (0.5, 0.5, 0.5), 3, (1, 2, 3)),
]


def volume_of(rng, shape, impulse):
    if impulse is not None:
        v = np.zeros(shape, F)
        v[impulse] = 1
        return v
    return (rng.random(shape) * 50).astype(F)      # vote-like magnitudes


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(sys.argv[1], "cartesian3dgrid", "src", "gaussianiir3d.cpp")
    assert os.path.exists(src), src
    rng = np.random.default_rng(20261019)
    out = {"names": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "inc", "cartesian3dgrid"))
        with open(os.path.join(tmp, "inc", "cartesian3dgrid", "gaussianiir3d.h"), "w") as f:
            f.write(HEADER)
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "gen")
        subprocess.check_call(["g++", "-O3", "-fopenmp", "-I", os.path.join(tmp, "inc"), src, os.path.join(tmp, "driver.cpp"),
                               "-o", exe])
        for name, shape, sig, steps, impulse in CASES:
            v = volume_of(rng, shape, impulse)
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            v.tofile(fin)
            subprocess.check_call([exe, fin, fout, str(shape[2]), str(shape[1]), str(shape[0])] +
                                  [repr(float(F(s))) for s in sig] + [str(steps)])
            got = np.fromfile(fout, F).reshape(shape)
            mine = vf.iir3(v, *sig, numsteps=steps)
            print("%-8s %-12s sigma %s steps %d: restatement differs on %d of %d voxels, %d subnormal outputs" %
                  (name, shape, sig, steps, int((~vf.same_bits(mine, got)).sum()), v.size,
                   int(((got != 0) & (np.abs(got) < np.finfo(F).tiny)).sum())))
            out["in_" + name] = v
            out["sigma_" + name] = np.array(sig, F)
            out["steps_" + name] = np.int32(steps)
            out["iir_" + name] = got
    # restated (NOT compiled): diffusion and Laplacian of two of the inputs
    for name, sigma in (("a", 1.0), ("b", 0.5)):
        out["restated_laplacian_" + name] = vf.laplacian(out["in_" + name])
        out["restated_diffuse_" + name], n = vf.diffuse(out["in_" + name], sigma)
        out["restated_diffuse_sigma_" + name] = F(sigma)
        out["restated_diffuse_steps_" + name] = np.int32(n)
    path = os.path.join(HERE, "volume_filters.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
