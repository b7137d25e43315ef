"""Registers, scratch and LDS of the binning kernel, read from the compiler (no GPU).

k_bin's production instantiations (no pair statistics, no phase stamps; slot and packed emission) run three 8-wave
workgroups per CU. That rests on three figures, which the next edit to preprocess_view or to the kernel's LDS arrays
would otherwise lose silently:
  - no private segment (both earlier builds that spilled were slower);
  - at most 80 VGPRs (AGPRs included: one register file), i.e. 6 waves per SIMD;
  - static LDS plus the 12 * T bytes of dynamic LDS at LGM's 512^2 renders (T = 1,024 tiles) within a third of the
    CU's 160 KiB.
The figures are clang's kernel-resource-usage remarks for render_bin.hip compiled with lgm_amd/build.py's own line.
"""
import os
import re
import shutil
import subprocess

import pytest

from lgm_amd import build as B

MODES = {0: "count", 1: "slot", 2: "packed"}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{(mode, stats, stamps): {remark field: int}} of every k_bin instantiation."""
    if not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)):
        pytest.fail(f"no HIP compiler at {B.HIPCC}")
    src = os.path.join(B.HERE, "csrc", "render_bin.hip")
    obj = str(tmp_path_factory.mktemp("bin_resources") / "render_bin.o")
    cmd = B.compile_cmd(src, obj) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:[^ ]+: )?\s*([A-Za-z][^:]*): (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            k = re.search(r"5k_binILi(\d)ELb([01])ELb([01])EE", val)
            cur = out.setdefault((MODES[int(k.group(1))], k.group(2) == "1", k.group(3) == "1"), {}) if k else None
        elif cur is not None and val.isdigit():
            cur[re.sub(r" \[.*", "", key)] = int(val)
    return out


def test_every_instantiation_is_compiled(usage):
    assert set(usage) == {(m, s, t) for m in MODES.values() for s in (False, True) for t in (False, True)}


@pytest.mark.parametrize("mode", ["slot", "packed"])
def test_production_fits_three_workgroups_per_cu(usage, mode):
    u = usage[(mode, False, False)]
    print(mode, u)
    assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0
    assert u["VGPRs"] + u["AGPRs"] <= 80
    assert u["LDS Size"] + 12 * 1024 <= 160 * 1024 // 3


@pytest.mark.parametrize("key", [(m, s, t) for m in MODES.values() for s in (False, True) for t in (False, True)],
                         ids=lambda k: f"{k[0]}-stats{int(k[1])}-stamps{int(k[2])}")
def test_no_instantiation_spills(usage, key):
    """The count pass and the diagnostic builds have no occupancy target, but none may use scratch."""
    assert usage[key]["ScratchSize"] == 0
