#!/usr/bin/env python
"""Static instruction census of one kernel: compiles a translation unit of setk_amd/csrc with
the flags setk_amd/build.py gives it (device code only, to assembly) and prints, per basic block
of the named kernel, how many instructions of each class it holds:
    python tools/isa_census.py pass1.hip "stft_covar_kernel<8, false, false>"
    python tools/isa_census.py pass2_mc.hip "beamform_istft_mc_kernel<8, false>" --sum LBB7_12,LBB7_13
Classes: VALU (by mnemonic family), MFMA, LDS, global (global / flat / buffer), scratch, SMEM,
SALU (everything else scalar: arithmetic, waits, barriers, branches).  The kernel is chosen by a
substring of its demangled name (the first match; --list prints all).  --sum adds up the named
blocks, e.g. the blocks of a steady-state loop.  --asm FILE reads an assembly file instead of
compiling.  A count of what the compiler emitted, not of what a wave executes: a block inside a
branch counts whether or not it is taken."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from setk_amd import build  # noqa: E402

SUFFIX = re.compile(r"_(e32|e64|dpp|sdwa|e64_dpp)$")


def classify(mn):
    """(class, family) of one mnemonic."""
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "MFMA", mn
    if mn.startswith("v_"):
        base = SUFFIX.sub("", mn).split("_")
        fam = "_".join(base[:3] if base[1] in ("pk", "cvt", "cmp", "cmpx") else base[:2])
        return "VALU", fam
    if mn.startswith("ds_"):
        return "LDS", mn
    if mn.startswith(("global_", "flat_", "buffer_")):
        return "global", mn
    if mn.startswith("scratch_"):
        return "scratch", mn
    if mn.startswith(("s_load", "s_buffer_load")):
        return "SMEM", mn
    if mn.startswith("s_"):
        return "SALU", mn
    return "other", mn


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return r.stdout.split("\n")[:len(names)]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def kernels(text):
    """{mangled name: list of body lines} for every .amdgpu_hsa_kernel of the file."""
    lines = text.split("\n")
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for n in names:
        i = next((k for k, ln in enumerate(lines) if ln.startswith(n + ":")), None)
        if i is None:
            continue
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            j += 1
        out[n] = lines[i + 1:j]
    return out


def census(body):
    """[(block label, Counter of classes, Counter of VALU families)] in program order."""
    blocks = [("entry", collections.Counter(), collections.Counter())]
    for ln in body:
        ln = ln.split(";")[0].rstrip()
        if not ln:
            continue
        m = re.match(r"^\.?(LBB\d+_\d+):", ln)
        if m:
            blocks.append((m.group(1), collections.Counter(), collections.Counter()))
            continue
        ln = ln.strip()
        if ln.startswith(".") or ln.endswith(":"):
            continue
        mn = ln.split()[0]
        cls, fam = classify(mn)
        blocks[-1][1][cls] += 1
        if cls == "VALU":
            blocks[-1][2][fam] += 1
    return blocks


CLASSES = ("VALU", "MFMA", "LDS", "global", "scratch", "SMEM", "SALU", "other")


def fmt(label, cls, fam):
    head = f"{label:>10} " + " ".join(f"{c} {cls[c]:4d}" for c in CLASSES if c != "other" or cls[c])
    fams = " ".join(f"{k}:{v}" for k, v in sorted(fam.items(), key=lambda kv: (-kv[1], kv[0])))
    return head + ("\n" + " " * 11 + fams if fams else "")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", help="translation unit under setk_amd/csrc, e.g. pass1.hip")
    ap.add_argument("kernel", nargs="?", default="", help="substring of the demangled kernel name")
    ap.add_argument("--arch", default=build.ARCH)
    ap.add_argument("--asm", help="read this assembly file instead of compiling the unit")
    ap.add_argument("--list", action="store_true", help="print the kernels of the unit and exit")
    ap.add_argument("--min", type=int, default=1, help="hide blocks with fewer instructions")
    ap.add_argument("--sum", default="", help="comma-separated block labels to add up")
    a = ap.parse_args()

    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "unit.s")
            cmd = [build._hipcc()] + build.unit_flags(a.unit, a.arch) + \
                ["-S", "--cuda-device-only", os.path.join(build.CSRC, a.unit), "-o", out]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr)
            text = open(out).read()
    ks = kernels(text)
    names = list(ks)
    dem = demangle(names)
    if a.list:
        print("\n".join(dem))
        return
    pick = [n for n, d in zip(names, dem) if a.kernel in d]
    if not pick:
        sys.exit(f"no kernel matches {a.kernel!r}; --list prints the names")
    name = pick[0]
    print(f"# {dem[names.index(name)]}  ({a.unit}, {a.arch})")
    blocks = census(ks[name])
    tot_c, tot_f = collections.Counter(), collections.Counter()
    sum_c, sum_f = collections.Counter(), collections.Counter()
    want = [w.lstrip(".") for w in a.sum.split(",") if w]
    for label, cls, fam in blocks:
        tot_c.update(cls)
        tot_f.update(fam)
        if label in want:
            sum_c.update(cls)
            sum_f.update(fam)
        if sum(cls.values()) >= a.min:
            print(fmt(label, cls, fam))
    print(fmt("kernel", tot_c, tot_f))
    if want:
        print(fmt("sum", sum_c, sum_f) + "\n" + " " * 11 + "(" + " + ".join(want) + ")")


if __name__ == "__main__":
    main()
