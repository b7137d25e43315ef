"""lgm_amd/csrc/work_split.h on the host (no GPU): tests/work_split_check.cpp, a program with its own main, is built
against the header with the address and undefined-behaviour sanitizers and run. It asserts that xcd_item is a bijection
on [0, M) for M = 1 .. 300 with xcd_group as its group map, and that split_range (int and long long) tiles [0, n) in
order for n = 0 .. 70 and S = 1 .. 17, counts within one of each other, the longer ranges first."""
import os
import shutil
import subprocess

import pytest

from lgm_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))


def host_compiler():
    """The system's C++ compiler, else the clang++ of the HIP toolchain."""
    hipcc = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which(B.HIPCC)
    near = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++") if hipcc \
        else None
    for cxx in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), near):
        if cxx and os.path.exists(cxx):
            return cxx
    pytest.fail("no host C++ compiler")


def test_work_split_host_program(tmp_path):
    exe = str(tmp_path / "work_split_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(B.HERE, "csrc"), os.path.join(HERE, "work_split_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "work_split ok" in r.stdout
