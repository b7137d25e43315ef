"""Registers, scratch and LDS of the compositing kernels' pool instantiations, read from the compiler (no GPU).

k_render_bwd runs four 4-wave workgroups per CU on the headline pool. That rests on three figures which the next
edit to the kernel would otherwise lose silently:
  - at most 128 VGPRs (AGPRs included: one register file), i.e. 4 waves per SIMD;
  - no private segment;
  - at most 40,960 B of static LDS (a quarter of the CU's 160 KiB).
k_render_fwd<false, 4> (every launch that fills the chip) runs 7 waves per SIMD: at most 72 VGPRs.
The figures are clang's kernel-resource-usage remarks for render_bwd.hip and render_fwd.hip compiled with
lgm_amd/build.py's own line (as tests/test_bin_resources.py does for k_bin).
"""
import os
import re
import shutil
import subprocess

import pytest

from lgm_amd import build as B

# the pool's instantiations: no depth gradient, no fused loss, float atomics, no antialiasing, no SH
BWD_POOL = "12k_render_bwdILb0ELb0ELb0ELb0ELb0EE"
FWD_POOL = "12k_render_fwdILb0ELi4ELb0EE"


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{mangled kernel name: {remark field: int}} of every kernel of render_bwd.hip and render_fwd.hip."""
    if not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)):
        pytest.fail(f"no HIP compiler at {B.HIPCC}")
    tmp = tmp_path_factory.mktemp("bwd_resources")
    runs = [subprocess.Popen(B.compile_cmd(os.path.join(B.HERE, "csrc", name + ".hip"), str(tmp / (name + ".o"))) +
                             ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"],
                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            for name in ("render_bwd", "render_fwd")]
    remarks = ""
    for r in runs:  # (the two sources compile side by side)
        err = r.communicate()[1]
        assert r.returncode == 0, err[-2000:]
        remarks += err
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: (?:[^ ]+: )?\s*([A-Za-z][^:]*): (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and val.isdigit():
            cur[re.sub(r" \[.*", "", key)] = int(val)
    return out


def _one(usage, mangled):
    hits = [v for k, v in usage.items() if mangled in k]
    assert len(hits) == 1, f"{mangled}: {len(hits)} kernels in {sorted(usage)}"
    return hits[0]


def test_pool_backward_keeps_four_workgroups_per_cu(usage):
    u = _one(usage, BWD_POOL)
    print("k_render_bwd (pool)", u)
    assert u["VGPRs"] + u["AGPRs"] <= 128
    assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0
    assert u["LDS Size"] <= 40960


def test_pool_forward_keeps_seven_waves_per_simd(usage):
    u = _one(usage, FWD_POOL)
    print("k_render_fwd<false, 4> (pool)", u)
    assert u["VGPRs"] + u["AGPRs"] <= 72
    assert u["Occupancy"] == 7
