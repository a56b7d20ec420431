"""The host helpers the serving cores share (csrc/serve_util.hpp: cut_batches, slots_of, first_outside) are pure host
functions: tests/serve_util_driver.cpp includes the header and checks them in a program of its own, built here with the
address and undefined-behaviour sanitizers linked into it (a stand-alone executable: nothing is preloaded)."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "matrixfactorizationsgd.java_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")


def test_serve_util_helpers_in_a_sanitized_program(tmp_path):
    exe = str(tmp_path / "serve_util_driver")
    build = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "serve_util_driver.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout)
