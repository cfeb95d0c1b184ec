"""The owning types of the host layer (dvs_mcemvs_amd/csrc/dsi_owned.hpp) under the address and undefined-behaviour
sanitizers (no GPU needed): tests/cpp/test_owned.cpp is a stand-alone program with counting fakes of the HIP runtime
calls the header makes; it is built with a plain host compiler, linked against no HIP runtime, and run as a child."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owning_types_free_everything_exactly_once(tmp_path):
    exe = str(tmp_path / "test_owned")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           # (the runtimes linked into the program: a dynamically linked one refuses to start wherever the
                           #  dynamic loader is told to load some other library first)
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_owned.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("ok") and "ERROR" not in r.stderr, r.stdout + r.stderr
