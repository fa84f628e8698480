"""Instruction counts by class of one .hip file's gfx950 device code (host
only, no GPU):

    python scripts/isa_counts.py [--tree DIR] [-DNAME[=V] ...] [--kernel SUBSTR] [--min-mfma N] als.hip

The file is compiled as scripts/device_asm_digest.py compiles it (the
library's flags, --cuda-device-only -S). Per kernel it prints the static
count of every class, then one line per basic block (label or branch to the
next branch) that holds at least --min-mfma matrix instructions: the 16
unrolled step bodies of the rank-64 Gramian loop and the trailing updates of
the solve are such blocks. Last comes the scripts/kregs.py resource line.

Classes, by mnemonic prefix only: v_mfma*, f64 VALU (v_*_f64, conversions to
or from f64 included), other v_*, ds_*, buffer_* / global_* / flat_*,
scratch_*, s_*. A count says nothing about time: s_waitcnt and s_nop are
scalar-class lines like any other."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from device_asm_digest import device_asm, entry_flags  # noqa: E402

CLASSES = ("mfma", "valu_f64", "valu", "ds", "vmem", "scratch", "salu")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu_f64" if "_f64" in op else "valu"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("buffer_", "global_", "flat_")):
        return "vmem"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("s_"):
        return "salu"
    return None


def kernels(asm):
    """name -> [(line number, mnemonic or None for a block boundary)]."""
    out, name, body = {}, None, []
    for no, raw in enumerate(asm.splitlines(), 1):
        ln = raw.split(";")[0].strip()
        if name is None:
            m = re.match(r"^(\w+):\s*;\s*@\1", raw)
            if m:
                name, body = m.group(1), []
            continue
        if ln.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        if not ln or (ln.startswith(".") and not ln.endswith(":")):
            continue
        if ln.endswith(":"):
            body.append((no, None))
            continue
        op = ln.split()[0]
        body.append((no, op))
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            body.append((no, None))
    return out


def count(ops):
    c = dict.fromkeys(CLASSES, 0)
    for op in ops:
        k = classify(op)
        if k:
            c[k] += 1
    return c


def fmt(c):
    return " ".join(f"{k} {c[k]:5d}" for k in CLASSES)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="repository root to compile (default: this one)")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra -D for a diagnostic build")
    ap.add_argument("--kernel", default="", help="only kernels whose (mangled) name contains this")
    ap.add_argument("--min-mfma", type=int, default=8, help="list basic blocks with at least this many MFMAs")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("file", help="name of a .hip file in the tree's csrc/")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as fh:
            asm = fh.read()
    else:
        flags, csrc = entry_flags(os.path.abspath(a.tree))
        flags += ["-D" + d for d in a.defines]
        asm = device_asm(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), flags, os.path.join(csrc, a.file))
    for name, body in kernels(asm).items():
        if a.kernel not in name:
            continue
        print(name)
        print(f"  whole kernel          {fmt(count(op for _, op in body if op))}")
        blocks, cur = [], []
        for no, op in body:
            if op is None:
                if cur:
                    blocks.append(cur)
                cur = []
            else:
                cur.append((no, op))
        if cur:
            blocks.append(cur)
        for b in blocks:
            c = count(op for _, op in b)
            if c["mfma"] >= a.min_mfma:
                print(f"  block at line {b[0][0]:6d}  {fmt(c)}")
    with tempfile.NamedTemporaryFile("w", suffix=".s") as fh:
        fh.write(asm)
        fh.flush()
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(HERE, "kregs.py"), fh.name, a.kernel], check=True)


if __name__ == "__main__":
    main()
