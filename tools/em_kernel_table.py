#!/usr/bin/env python3
"""Per-kernel table of the device code of some .hip units (gfx950).

    tools/em_kernel_table.py [--check BASELINE] UNIT.hip ... > table.txt

Each unit's device side is compiled alone with the Makefile's CXXFLAGS
(--cuda-device-only --no-gpu-bundle-output: a plain ELF).  One row per kernel:
symbol, sha256 prefix of its encoded instruction bytes (llvm-objdump -d, the
address column left out: branches are relative), .vgpr_count .agpr_count
.sgpr_count .group_segment_fixed_size .private_segment_fixed_size
.max_flat_workgroup_size of its metadata note, and the unit.  A symbol in two
units is an error.  --check compares symbols, hashes and numbers (not units)
with an earlier table, e.g. profiles/em_split_kernels.txt, and fails on any
difference: a refactor that only moves kernels must leave the table alone.
"""
import argparse, concurrent.futures, hashlib, os, re, subprocess, sys, tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pyfasst_amd", "csrc")
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".max_flat_workgroup_size"]

def makefile_var(name):
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"{name}\s*\??=\s*(.*)", line)
        if m:
            return m.group(1).strip()
    raise SystemExit(f"no {name} in the Makefile")

def unit_rows(unit):
    flags = makefile_var("CXXFLAGS").replace("$(ARCH)", makefile_var("ARCH")).split()
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "dev.elf")
        subprocess.check_call([makefile_var("HIPCC"), *flags, "--cuda-device-only", "--no-gpu-bundle-output",
                               "-c", unit, "-o", elf], cwd=os.path.dirname(os.path.abspath(unit)) or ".")
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", elf], text=True)
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], text=True)
        syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", elf], text=True)
    size = {f[7]: int(f[2]) for f in map(str.split, syms.splitlines()) if len(f) == 8 and f[3] == "FUNC"}
    code, sym, left = {}, None, 0
    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym, left = m.group(1), size[m.group(1)]   # (the padding behind a function is not its code)
            code[sym] = hashlib.sha256()
        elif sym and left > 0 and "//" in line:   # "\tinsn   // ADDRESS: WORD WORD ..."
            words = line.rsplit("//", 1)[1].split(":", 1)[1].split()
            code[sym].update(" ".join(words).encode())
            left -= 4 * len(words)
    meta, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"(\s*)(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(2) and len(m.group(1)) == 2:   # a new entry of amdhsa.kernels
            cur = {}
        if cur is not None and len(m.group(1)) + len(m.group(2) or "") == 4:
            cur[m.group(3)] = m.group(4).strip("'\"")
            if m.group(3) == ".name":
                meta[cur[".name"]] = cur
    if set(meta) != set(code):
        raise SystemExit(f"{unit}: code symbols and kernel notes differ: {sorted(set(meta) ^ set(code))[:5]}")
    return {s: (code[s].hexdigest()[:16], *[meta[s][k] for k in KEYS], os.path.basename(unit)) for s in code}

def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", metavar="BASELINE")
    ap.add_argument("units", nargs="+")
    a = ap.parse_args()
    rows = {}
    with concurrent.futures.ThreadPoolExecutor(len(a.units)) as ex:
        for unit, r in zip(a.units, ex.map(unit_rows, a.units)):
            dup = set(rows) & set(r)
            if dup:
                raise SystemExit(f"kernel in two units: {sorted(dup)[:5]} ({unit})")
            rows.update(r)
    print("# symbol sha256[:16] vgpr agpr sgpr lds scratch max_wg unit")
    for s in sorted(rows):
        print(s, *rows[s])
    if a.check:
        base = {l.split()[0]: tuple(l.split()[1:8]) for l in open(a.check) if l.strip() and l[0] != "#"}
        now = {s: tuple(map(str, v[:7])) for s, v in rows.items()}
        bad = sorted(s for s in set(base) | set(now) if base.get(s) != now.get(s))
        for s in bad:
            print(f"DIFFERS {s}: {base.get(s)} -> {now.get(s)}", file=sys.stderr)
        print(f"{len(now)} kernels, {len(bad)} differ from {a.check}", file=sys.stderr)
        sys.exit(1 if bad else 0)

if __name__ == "__main__":
    main()
