"""The gfx950 assembly of dsi_kernels.hip for the static audits (no GPU needed): compiled once per test process and
shared by every test module that reads register counts, scratch sizes or instructions out of it."""
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@functools.lru_cache(maxsize=None)
def kernel_asm_text():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dsi_kernels.s")
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-x", "hip",
                               "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "dvs_mcemvs_amd", "csrc", "dsi_kernels.hip"), "-o", out],
                              stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()
