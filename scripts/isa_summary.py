#!/usr/bin/env python3
"""Per-kernel table of two directories of device listings (`make isa`).

  make -C trik-media-sensors-dsp_amd/csrc isa BUILD=/tmp/before   # at the parent
  make -C trik-media-sensors-dsp_amd/csrc isa BUILD=/tmp/after    # at the result
  python scripts/isa_summary.py /tmp/before/isa /tmp/after/isa [--pairs FILE]

--pairs: a file of OLD=NEW lines, kernel names as the table prints them; a
kernel NEW that the parent does not have is compared with the parent's OLD,
whichever listing held it (a renamed kernel, a kernel moved to another file).

For every kernel symbol: instruction count, VGPRs, SGPRs, static LDS bytes and
scratch bytes before -> after, and how the instruction stream compares:
  same   identical text (the function number of local labels, .LBB<n>_, aside:
         it is the kernel's position in its file)
  regs   identical once register numbers are masked
  kernarg  identical once, besides, the immediate operands of scalar loads and
         scalar adds are masked: the kernel arguments moved (a member added to
         or reordered in the argument struct), the code did not
  DIFF   anything else
"""
import glob
import os
import re
import subprocess
import sys

INFO = {"NumVgprs": "vgpr", "TotalNumSgprs": "sgpr", "ScratchSize": "scratch", "LDSByteSize": "lds"}
REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")
IMM = re.compile(r"(?<![\w#])(0x[0-9a-f]+|-?\d+)\b")
LABEL = re.compile(r"\.LBB\d+_")
SCALAR = ("s_load_dword", "s_add_u32", "s_addc_u32", "s_add_i32", ".amdhsa_kernarg_size")


def masked(ins, kernarg):
    """The instruction without its register numbers, and, for the kernarg
    class, without the immediates of a scalar load or add."""
    out = REG.sub(r"\1#", ins)
    return IMM.sub("#", out) if kernarg and out.startswith(SCALAR) else out


def kernels(path):
    """{symbol: {"ins": [...], vgpr, sgpr, lds, scratch}} of one listing."""
    out, cur, body = {}, None, False
    for line in open(path):
        m = re.match(r"^(\w+):\s+; @", line)
        if m:
            cur, body = {"ins": []}, True
            out[m.group(1)] = cur
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            body = False
        elif body and line.startswith("\t") and not line.startswith("\t.") and not line.startswith("\t;"):
            cur["ins"].append(LABEL.sub(".LBB_", line.split(";")[0].strip()))
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and m.group(1) in INFO:
            cur[INFO[m.group(1)]] = int(m.group(2))
    return {k: v for k, v in out.items() if "vgpr" in v}  # kernels carry the info block


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, res.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = name.replace("trik_hsv::", "").replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*$", "", name)  # the template arguments tell instantiations apart


def main():
    before, after = sys.argv[1], sys.argv[2]
    pairs, old = {}, {}  # NEW -> OLD; the parent's kernels by printed name
    if sys.argv[3:4] == ["--pairs"]:
        pairs = dict(reversed(ln.strip().split("=")) for ln in open(sys.argv[4]) if "=" in ln)
        for fb in glob.glob(os.path.join(before, "*.s")):
            kb = kernels(fb)
            old.update((short(n), kb[sym]) for sym, n in demangle(list(kb)).items())
    print("%-72s %-13s %-9s %-9s %-13s %-7s %s" % ("kernel", "instructions", "VGPR", "SGPR", "LDS", "scratch", "stream"))
    for fa in sorted(glob.glob(os.path.join(after, "*.s"))):
        fb = os.path.join(before, os.path.basename(fa))
        ka, kb = kernels(fa), kernels(fb) if os.path.exists(fb) else {}
        names = demangle(list(ka))
        print("# " + os.path.basename(fa).replace(".s", ".hip"))
        for sym, a in ka.items():
            b = kb.get(sym) or old.get(pairs.get(short(names[sym])))
            if b is None:
                print("%-72s (not in the parent)" % short(names[sym]))
                continue
            if a["ins"] == b["ins"]:
                stream = "same"
            elif [masked(i, False) for i in a["ins"]] == [masked(i, False) for i in b["ins"]]:
                stream = "regs"
            elif [masked(i, True) for i in a["ins"]] == [masked(i, True) for i in b["ins"]]:
                stream = "kernarg"
            else:
                stream = "DIFF"
            cols = ["%d->%d" % (b[k], a[k]) if b[k] != a[k] else "%d" % a[k] for k in ("vgpr", "sgpr", "lds", "scratch")]
            n = "%d->%d" % (len(b["ins"]), len(a["ins"])) if len(b["ins"]) != len(a["ins"]) else "%d" % len(a["ins"])
            print("%-72s %-13s %-9s %-9s %-13s %-7s %s" % (short(names[sym])[:72], n, *cols, stream))
        gone = demangle([sym for sym in kb if sym not in ka])
        for sym in gone:
            if short(gone[sym]) not in pairs.values():
                print("%-72s (gone)" % sym)


if __name__ == "__main__":
    main()
