"""Digest of the gfx950 device assembly of csrc/*.hip files, to show that a
source change leaves the device code as it was (host only, no GPU):

    python scripts/device_asm_digest.py [--tree DIR] [-DNAME[=V] ...] als.hip als_wide.hip

Each file of DIR's csrc/ (default: this tree) is compiled with the build's own
flags (HIPCC_FLAGS of DIR's __graft_entry__.py minus -shared) plus
--cuda-device-only -S. Lines that contain __hip_cuid_ are dropped: that symbol
is a hash of the translation unit's text, so it differs whenever a comment
does. Prints one sha256 per file and the per-kernel resource lines of
scripts/kregs.py. Two trees have the same device code exactly when their
outputs are equal; --keep DIR also writes the filtered assembly there, for a
diff when they are not."""
import argparse
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def entry_flags(tree):
    spec = importlib.util.spec_from_file_location("_entry", os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [f for f in mod.HIPCC_FLAGS if f != "-shared"], mod.CSRC


def device_asm(hipcc, flags, src):
    out = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", "-"], check=True,
                         stdout=subprocess.PIPE).stdout.decode()
    return "".join(ln for ln in out.splitlines(keepends=True) if "__hip_cuid_" not in ln)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="repository root to compile (default: this one)")
    ap.add_argument("--keep", help="directory that receives the filtered assembly (<file>.s)")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra -D for a diagnostic build")
    ap.add_argument("files", nargs="+", help="names of .hip files in the tree's csrc/")
    a = ap.parse_args()
    flags, csrc = entry_flags(os.path.abspath(a.tree))
    flags += ["-D" + d for d in a.defines]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for name in a.files:
        asm = device_asm(hipcc, flags, os.path.join(csrc, name))
        print(f"{name}  sha256 {hashlib.sha256(asm.encode()).hexdigest()}  lines {asm.count(chr(10))}")
        with tempfile.NamedTemporaryFile("w", suffix=".s") as fh:
            fh.write(asm)
            fh.flush()
            sys.stdout.flush()
            subprocess.run([sys.executable, os.path.join(HERE, "kregs.py"), fh.name], check=True)
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
            with open(os.path.join(a.keep, name + ".s"), "w") as fh:
                fh.write(asm)


if __name__ == "__main__":
    main()
