"""Per-kernel comparison of the gfx950 ISA of two builds of one object file (dev tool, CPU only): unbundles both
code objects as tools/kernel_resources.py does, disassembles them with llvm-objdump and compares every kernel whose
mangled name contains SUBSTR instruction for instruction (addresses and encodings left out).

usage: python tools/kernel_isa_diff.py OLD.hip.o NEW.hip.o [--filter SUBSTR]"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.kernel_resources import LLVM, TARGET, demangle  # noqa: E402


def disassemble(obj):
    """{mangled symbol: [instruction text]} of one object file's gfx950 code object."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat"), os.path.join(d, "co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "o")],
                       check=True, capture_output=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        f"--targets={TARGET}", f"--output={co}"], check=True, capture_output=True)
        text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
                              capture_output=True, text=True).stdout
    funcs, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:", ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and ln.strip() and ln.strip() != "...":  # ("...": the padding behind a section's last kernel)
            cur.append(re.sub(r"\s*//.*$", "", ln).strip())
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--filter", default="")
    args = ap.parse_args()
    old, new = disassemble(args.old), disassemble(args.new)
    names = sorted(k for k in old if args.filter in k and old[k])
    differ = 0
    for k, shown in zip(names, demangle(names)):
        if k not in new:
            print(f"GONE       {shown}")
            differ += 1
        elif old[k] == new[k]:
            print(f"IDENTICAL  {shown} ({len(old[k])} instructions)")
        else:
            differ += 1
            print(f"DIFFERENT  {shown} ({len(old[k])} -> {len(new[k])} instructions)")
            for ln in list(difflib.unified_diff(old[k], new[k], lineterm="", n=0))[2:22]:
                print("    " + ln)
    for k, shown in zip(*(lambda ks: (ks, demangle(ks)))(sorted(k for k in new if args.filter in k and k not in old))):
        print(f"NEW        {shown} ({len(new[k])} instructions)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
