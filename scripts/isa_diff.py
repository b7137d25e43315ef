"""Do two sets of sources compile to the same device code? Per kernel symbol, on hipcc -S --cuda-device-only listings
(lgm_amd/build.py's own line) with comments and assembler directives dropped and the function index in .LBB<n>_ /
.Ltmp<n> labels normalised. Text only, no GPU:
    python scripts/isa_diff.py [-DNAME ...] A.hip|A.s ... -- B.hip|B.s ...
A source's quoted includes resolve next to it first, so an older revision's source is compared from a directory that
holds that revision's headers. Prints the kernels only in A, only in B, and those whose instructions differ (each with
a short unified diff); exits non-zero if there are any, or if one side defines a kernel twice."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lgm_amd import build as B  # noqa: E402


def listing(path, defines, tmp):
    if path.endswith(".s"):
        return open(path).read()
    out = os.path.join(tmp, re.sub(r"\W", "_", os.path.abspath(path)) + ".s")
    cmd = [a for a in B.compile_cmd(os.path.abspath(path), out, defines) if a != "-c"] + ["-S", "--cuda-device-only"]
    subprocess.run(cmd, check=True)
    return open(out).read()


def kernels(text):
    """{symbol: [instruction and label lines]} of every function of one listing."""
    out, name, tmps = {}, None, {}
    for line in text.split("\n"):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, tmps = m.group(1), {}
            out[name] = []
        elif re.match(r"\.Lfunc_end\d+:", line):
            name = None
        elif name:
            s = line.split(";")[0].strip()
            if not s or s == name + ":" or (s.startswith(".") and not s.endswith(":")):
                continue  # comment, the symbol's own label, directive
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            out[name].append(re.sub(r"\.Ltmp\d+", lambda t: tmps.setdefault(t.group(0), f".Ltmp#{len(tmps)}"), s))
    return out


def side(paths, defines, tmp):
    every, twice = {}, []
    for p in paths:
        for k, v in kernels(listing(p, defines, tmp)).items():
            if k in every:
                twice.append(k)
            every[k] = v
    return every, twice


if __name__ == "__main__":
    args = sys.argv[1:]
    defines = [a for a in args if a.startswith("-D")]
    args = [a for a in args if not a.startswith("-D")]
    with tempfile.TemporaryDirectory() as tmp:
        (a, a2), (b, b2) = (side(s, defines, tmp) for s in (args[:args.index("--")], args[args.index("--") + 1:]))
    differ = [k for k in sorted(a) if k in b and a[k] != b[k]]
    lists = {"defined twice in A": a2, "defined twice in B": b2, "only in A": sorted(set(a) - set(b)),
             "only in B": sorted(set(b) - set(a)), "instructions differ": differ}
    print(f"{' '.join(defines) or '(no defines)'}: {len(a)} kernels in A, {len(b)} in B, "
          f"{len(set(a) & set(b)) - len(differ)} identical")
    for title, names in lists.items():
        print(f"{title}: {len(names)}")
        for k in names:
            print("  ", k)
            if title == "instructions differ":
                print("\n".join(list(difflib.unified_diff(a[k], b[k], "A", "B", n=2, lineterm=""))[:40]))
    sys.exit(1 if any(lists.values()) else 0)
