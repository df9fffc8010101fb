"""The ledger that owns what an engine holds (eftpipe_amd/csrc/eftb_own.hpp: hold, release, mark / release_to, the destructor) against
hand-written release orders: tests/own_host_test.cpp, built by the host compiler alone with the address and undefined-behaviour sanitizers
and run as a program of its own -- a handle released twice is a double free there, one never released a leak.  No GPU, nothing loaded into
this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_own_host_header(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = tmp_path / "own_host_test"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "eftpipe_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "own_host_test.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "all checks passed" in ran.stdout
