#!/usr/bin/env python3
"""Resource lines (VGPRs, SGPRs, spills, scratch, code size in bytes) of every k_sdtw instantiation in a built object or
shared library -- kernel_resources.py's figures plus the size of the kernel's code from the code object's symbol table.
With two files: the lines of the second, and a verdict on the kernels both hold (a change to the kernel template must
leave the existing instantiations as they were).
usage: pairs_kernel_resources.py after.o|after.so [before.o|before.so] [name-filter, default k_sdtw<]"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402


def code_sizes(co):
    """{mangled kernel name: bytes of code} from the FUNC symbols of a code object"""
    txt = subprocess.run([os.path.join(kr.LLVM, "llvm-readelf"), "-s", "-W", co], capture_output=True, text=True).stdout
    out = {}
    for line in txt.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            out[f[7]] = int(f[2], 0)
    return out


def lines_of(path, flt):
    out = {}
    for co in kr.code_objects(path):
        sizes = code_sizes(co)
        for k in kr.kernels(co):
            raw = k["name"]
            name = kr.demangle(raw).replace("(anonymous namespace)::", "")
            name = re.sub(r"\(.*\)$", "", name).replace("void ", "")
            if flt not in name or name in out:
                continue
            out[name] = "%-34s %5s %5s %7s %7s %8s %8d" % (name, k.get("vgpr_count"), k.get("sgpr_count"),
                                                          k.get("vgpr_spill_count"), k.get("sgpr_spill_count"),
                                                          k.get("private_segment_fixed_size"), sizes.get(raw, -1))
    return out


def key(name):
    return [int(v) for v in re.findall(r"\d+", name)][::-1]


def main():
    args = sys.argv[1:]
    files = [a for a in args if os.path.exists(a)]
    flt = ([a for a in args if not os.path.exists(a)] or ["k_sdtw<"])[0]
    after = lines_of(files[0], flt)
    print("%-34s %5s %5s %7s %7s %8s %8s" % ("kernel", "vgpr", "sgpr", "v_spill", "s_spill", "scratch", "code"))
    for name in sorted(after, key=key):
        print(after[name])
    if len(files) > 1:
        before = lines_of(files[1], flt)
        changed = [n for n in before if after.get(n) != before[n]]
        print("# %d kernels before, %d after, %d new; of the %d both hold, %d differ%s" % (
            len(before), len(after), len(set(after) - set(before)), len(set(after) & set(before)), len(changed),
            "" if not changed else ": " + ", ".join(sorted(changed, key=key))))
        sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
