"""lgm_amd/csrc/render_layout.h on the host (no GPU): tests/render_layout_check.cpp, a program with its own main, is
built against the header with the address and undefined-behaviour sanitizers and run. Over B = 1..2, V = 1..3, N in
{0, 1, 2, 3, 5} and the four (deterministic, antialias) combinations it asserts that the accumulator block's regions are
ordered, disjoint, aligned and end at the block's total; that every device index function is a bijection onto exactly
its region; that the repeated backward's clear range is the accumulator regions without the factors; that the forward's
16-byte-rounded zero range covers the main records, overruns them by less than 16 bytes and stays inside the block's
reservation; that the workspace's regions are 256-byte aligned, ordered and disjoint with `total` the last end, and that
the regions the inspection entry points read do not move with the options; that make_layout's totals equal the values
recorded from the commit before the header; and that the diagnostics counter map's record ranges are back to back and end
at the word count -- the count lgm_amd._native.render_counter_words returns."""
import os
import subprocess

import pytest

from lgm_amd import _native
from lgm_amd import build as B
from tests.test_work_split import host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("render_layout") / "render_layout_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(B.HERE, "csrc"), "-I", os.path.join(B.ROOT, "include"),
           os.path.join(HERE, "render_layout_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_render_layout_host_program(check_program):
    r = subprocess.run([check_program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "render_layout ok" in r.stdout


@pytest.mark.parametrize("shape", [(1, 2, 1, 16, 16), (2, 3, 1000, 40, 24), (8, 6, 100000, 256, 256)])
def test_counter_words_match_the_header(check_program, shape):
    r = subprocess.run([check_program, "words"] + [str(x) for x in shape], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert int(r.stdout) == _native.render_counter_words(*shape)
