"""Per-kernel registers, scratch, occupancy and static LDS of one source, from the compiler (no GPU):
python scripts/kernel_resources.py csrc/mvattn.hip > table.txt
Compiles with lgm_amd/build.py's own line plus clang's kernel-resource-usage remarks (as tests/test_bin_resources.py)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lgm_amd import build as B  # noqa: E402

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "Occupancy", "LDS Size"]


def usage(src):
    """[(demangled kernel, {field: int})] in the compiler's order."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = B.compile_cmd(src, os.path.join(tmp, "k.o")) + ["--cuda-device-only",
                                                              "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-2000:])
    out = []
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            out.append((m.group(2), {}))
        elif out and m.group(2).isdigit():
            out[-1][1][m.group(1)] = int(m.group(2))
    names = subprocess.run(["c++filt"], input="\n".join(n for n, _ in out), capture_output=True,
                           text=True).stdout.split("\n")
    short = [re.sub(r"^(?:void )?lgm::\(anonymous namespace\)::|\(.*", "", n) for n in names]
    return [(s, u) for s, (_, u) in zip(short, out)]


if __name__ == "__main__":
    rows = usage(os.path.join(B.HERE, sys.argv[1]))
    print(f"# {sys.argv[1]}: {len(rows)} kernels;", " | ".join(FIELDS))
    for name, u in sorted(rows, key=lambda row: row[0]):  # (two kernels may demangle to one short name)
        print(name, *(u[f] for f in FIELDS), sep="\t")
