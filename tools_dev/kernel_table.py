#!/usr/bin/env python3
"""Per-kernel table of one or more HIP translation units, and the difference
of two such tables: the check that a change of host or launch code left every
remaining kernel as it was.

    tools_dev/kernel_table.py make OUT.json [--extra=-DBWAGPU_OCC_DIAG] [--root DIR] csrc/spec.hip ...
    tools_dev/kernel_table.py diff PARENT.json RESULT.json

`make` compiles each file device-only for gfx950 with the Makefile's flags
(from DIR/bwa-flow_amd, default this checkout), unbundles the code object and
reads its symbol table (llvm-readelf -sW: code bytes per kernel) and its
metadata note (llvm-readelf --notes: VGPR / AGPR / SGPR counts, private
segment, static LDS, spill counts).  It reads no instruction.  `diff` prints
the kernels only one table has and every row that differs among the kernels
both have; its exit status is 1 if such a row differs.  Raw bytes are not
compared: kernels that call an out-of-line function or read a __device__
variable embed PC-relative offsets that move with the layout."""
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FIELDS = {"agpr_count": ".agpr_count", "vgpr_count": ".vgpr_count", "sgpr_count": ".sgpr_count",
          "private_segment": ".private_segment_fixed_size", "static_lds": ".group_segment_fixed_size",
          "sgpr_spills": ".sgpr_spill_count", "vgpr_spills": ".vgpr_spill_count"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True,
                         check=True).stdout.splitlines()
    # the name with its template arguments, without the parameter list
    return {m: re.sub(r"^void ", "", d).split("(")[0].replace("bwagpu::", "") for m, d in zip(names, out)}


def table_of(src, root, extra, tmp):
    base = os.path.join(tmp, os.path.basename(src))
    cwd = os.path.join(root, "bwa-flow_amd")
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=gfx950", "--offload-device-only", "-O3", *extra,
                    "-fPIC", "-std=c++17", "-I../include", "-Icsrc", "-Ihost", "-c", src, "-o", base + ".co"],
                   cwd=cwd, check=True)
    llvm = os.path.join(ROCM, "llvm", "bin")
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--input=" + base + ".co",
                    "--targets=hip-amdgcn-amd-amdhsa--gfx950", "--output=" + base + ".elf", "--unbundle"], check=True)
    syms = subprocess.run([os.path.join(llvm, "llvm-readelf"), "-sW", base + ".elf"], capture_output=True, text=True,
                          check=True).stdout
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", base + ".elf"], capture_output=True,
                           text=True, check=True).stdout
    rows = {}
    for block in re.split(r"\n  - (?=\.agpr_count|\.args)", notes)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        row = {"code_bytes": size[name]}
        for k, key in FIELDS.items():
            row[k] = int(re.search(r"^\s*" + re.escape(key) + r":\s+(\d+)", block, re.M).group(1))
        rows[name] = row
    short = demangle(sorted(rows))
    assert len(set(short.values())) == len(short), "two kernels with one demangled name"
    return {short[m]: dict(rows[m], file=os.path.basename(src)) for m in rows}


def make(argv):
    out, extra, root, srcs = argv[0], [], REPO, []
    it = iter(argv[1:])
    for a in it:
        if a.startswith("--extra="):
            extra.append(a[len("--extra="):])
        elif a == "--root":
            root = next(it)
        else:
            srcs.append(a)
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for s in srcs:
            t = table_of(s, root, extra, tmp)
            assert not set(t) & set(kernels), "a kernel in two files"
            kernels.update(t)
    with open(out, "w") as f:
        json.dump({"arch": "gfx950", "flags": ["-O3", *extra], "files": srcs,
                   "kernels": dict(sorted(kernels.items()))}, f, indent=1)
        f.write("\n")
    print(f"{out}: {len(kernels)} kernels, {sum(k['code_bytes'] for k in kernels.values())} code bytes")


def diff(argv):
    a, b = (json.load(open(p))["kernels"] for p in argv[:2])
    for k in sorted(set(a) - set(b)):
        print(f"only in {argv[0]}: {k} ({a[k]['code_bytes']} bytes)")
    for k in sorted(set(b) - set(a)):
        print(f"only in {argv[1]}: {k} ({b[k]['code_bytes']} bytes)")
    bad = 0
    for k in sorted(set(a) & set(b)):
        ra, rb = ({f: v for f, v in r.items() if f != "file"} for r in (a[k], b[k]))
        if ra != rb:
            bad += 1
            print(f"differs: {k}: " + ", ".join(f"{f} {ra[f]} -> {rb[f]}" for f in ra if ra[f] != rb[f]))
    print(f"{len(set(a) & set(b))} kernels in both, {bad} with a different row")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "make":
        make(sys.argv[2:])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2:]))
    else:
        sys.exit(__doc__)
