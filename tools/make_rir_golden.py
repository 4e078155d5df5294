#!/usr/bin/env python
"""
Writes tests/golden/ref_rir.npz: the reference's image-method RIR generator on the cases of
tests/rir_model.py.

The reference's rir-simulate needs Kaldi, but include/rir-generator.{h,cc} use a handful of its
names only.  With the stand-in headers of tools/kaldistub the UNMODIFIED rir-generator.cc compiles
with the host g++ as one translation unit behind tools/kaldistub/rir_driver.cc -- into a temporary
directory outside the repository: nothing compiled from the reference and none of its text is kept.

Per case the fixture holds the parameters, the reference's RIR, e_ref = max |reference - float64
model| / peak (the reference's own float32 noise, the unit of the device test's bounds) and the
reference's seconds per channel on the machine that ran this tool.

Condition on the inputs: an image whose distance lies within float32 rounding of num_samples can fall
on either side of the inclusion test floor(dist) < num_samples in float32 and in float64, and its left
half-window is not small.  The tool asserts with the model that no image of any case lies within 1e-3
samples of that boundary (move a position by a millimetre where one does).

    python tools/make_rir_golden.py [--reference DIR] [--check]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import rir_model  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_rir.npz")
STUB = os.path.join(ROOT, "tools", "kaldistub")


def build_driver(reference, workdir):
    """The reference generator behind rir_driver.cc, compiled into `workdir`; the program's path."""
    exe = os.path.join(workdir, "rir-driver")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-w", "-I", STUB, "-I", reference,
           os.path.join(STUB, "rir_driver.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("compiling the reference generator failed:\n" + r.stdout + r.stderr)
    return exe


def _num(v):
    """A float32 value as text that parses back to the same float32."""
    return "{:.9g}".format(float(np.float32(v)))


def driver_args(c):
    """rir-simulate's options for a case."""
    vec = lambda p: ",".join(_num(v) for v in p)  # noqa: E731
    return ["--sound-velocity=" + _num(c["c"]), "--samp-frequency=" + _num(c["fs"]),
            "--hp-filter=" + ("true" if c["hp"] else "false"), "--number-samples=%d" % c["num_samples"],
            "--order=%d" % c["order"], "--microphone-type=" + c["mic_type"], "--angle=" + vec(c["angle"]),
            "--beta=" + (vec(c["beta"]) if c["beta"] is not None else _num(c["rt60"])),
            "--room-topo=" + vec(c["room"]), "--source-location=" + vec(c["src"]),
            "--receiver-location=" + ";".join(vec(m) for m in c["mics"])]


def run_reference(exe, c, workdir):
    """(the reference's [n_mics][num_samples] float32, seconds per channel)"""
    dest = os.path.join(workdir, "rir.bin")
    r = subprocess.run([exe] + driver_args(c) + [dest], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        raise RuntimeError("the reference generator failed: " + r.stderr)
    raw = np.fromfile(dest, dtype=np.uint8)
    rows, cols = np.frombuffer(raw[:8], dtype=np.int32)
    rir = np.frombuffer(raw[8:], dtype=np.float32).reshape(rows, cols).copy()
    return rir, float(r.stdout.split()[-1]) / rows


# The reference's command lines, run unmodified with `random` seeded: what they sample (rir.json) and
# what their rir-simulate calls compute.  Small on purpose: 2 rooms x 2 RIRs of 800 taps.
CLI_SEED = 20181
CLI_ARGS = {
    "rir_generate_1d": ["2", "--num-rirs", "2", "--rir-dur", "0.05", "--dump-dir", "rir_1d", "--room-dim",
                        "4,6;5,7;2.4,3", "--rt60", "0.2,0.5", "--array-topo", "0,0.05,0.1,0.15",
                        "--speaker-height", "1.2,1.9"],
    "rir_generate_2d": ["2", "--num-rirs", "2", "--rir-dur", "0.05", "--dump-dir", "rir_2d", "--room-dim",
                        "4,6;5,7;2.4,3", "--absorption-coefficient-range", "0.3,0.6", "--rt60", "",
                        "--speaker-height", "1.2,1.9"],
}

# stands in for rir-simulate on PATH: the compiled driver behind rir-simulate's flags.  Beside the wave
# file (16-bit, for the script's sake) it keeps the generator's float32 matrix as <dest>.f32.
FAKE_RIR_SIMULATE = """#!{python}
import subprocess, sys
import numpy as np
import scipy.io.wavfile
args, dest = sys.argv[1:-1], sys.argv[-1]
subprocess.run([{driver!r}] + args + [dest + ".f32"], check=True, stdout=subprocess.DEVNULL)
raw = np.fromfile(dest + ".f32", dtype=np.uint8)
rows, cols = np.frombuffer(raw[:8], dtype=np.int32)
rir = np.frombuffer(raw[8:], dtype=np.float32).reshape(rows, cols)
fs = [float(a.split("=")[1]) for a in args if a.startswith("--samp-frequency=")][0]
scipy.io.wavfile.write(dest, int(fs), np.trunc(rir.T * 32767.0).astype(np.int16))
"""

RUN_REFERENCE_SCRIPT = """import random, runpy, sys
sys.path.insert(0, {root!r})
from oracle import ref_harness as rh
rh.load()
random.seed({seed})
script = rh.REF_SPTK + "/{name}.py"
sys.argv = [script] + {args!r}
runpy.run_path(script, run_name="__main__")
"""


def record_cli(exe, tmp, reference):
    """The unmodified rir_generate_{1d,2d}.py as __main__ in a child process, through the compat
    shims of oracle/ref_harness.py: rir.json and the first RIR's matrix per script."""
    import json
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir)
    fake = os.path.join(bindir, "rir-simulate")
    with open(fake, "w") as f:
        f.write(FAKE_RIR_SIMULATE.format(python=sys.executable, driver=exe))
    os.chmod(fake, 0o755)
    out = {}
    for name, args in CLI_ARGS.items():
        work = os.path.join(tmp, "work_" + name)
        os.makedirs(work)
        runner = os.path.join(tmp, name + "_runner.py")
        with open(runner, "w") as f:
            f.write(RUN_REFERENCE_SCRIPT.format(root=ROOT, seed=CLI_SEED, name=name, args=args))
        env = dict(os.environ, PATH=bindir + os.pathsep + os.environ.get("PATH", ""), SETK_REFERENCE=reference)
        r = subprocess.run([sys.executable, runner], cwd=work, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"the reference's {name}.py failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
        dump = os.path.join(work, args[args.index("--dump-dir") + 1])
        text = open(os.path.join(dump, "rir.json")).read()
        cfg = json.loads(text)
        assert len(cfg) == 2 and all(len(room["spk"]) == 2 for room in cfg), name
        raw = np.fromfile(os.path.join(dump, "Room1-1.wav.f32"), dtype=np.uint8)
        rows, cols = np.frombuffer(raw[:8], dtype=np.int32)
        out[f"cli/{name}/args"] = np.frombuffer(json.dumps(args).encode(), dtype=np.uint8)
        out[f"cli/{name}/seed"] = np.int64(CLI_SEED)
        out[f"cli/{name}/rir_json"] = np.frombuffer(text.encode(), dtype=np.uint8)
        out[f"cli/{name}/room1_1"] = np.frombuffer(raw[8:], dtype=np.float32).reshape(rows, cols).copy()
        print(f"{name}: rir.json {len(text)} bytes, Room1-1 {rows} x {cols}, "
              f"{sorted(os.listdir(dump))}")
    return out


def record(reference):
    out = {}
    with tempfile.TemporaryDirectory(prefix="setk_rir_") as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep), "the build directory must lie outside the repository"
        exe = build_driver(reference, tmp)
        out.update(record_cli(exe, tmp, reference))
        for name, c in rir_model.cases().items():
            bnd = []
            model = rir_model.generate(c, boundary=bnd)
            assert min(bnd) >= 1e-3, f"{name}: an image lies {min(bnd):.2e} samples from the inclusion boundary"
            ref, sec = run_reference(exe, c, tmp)
            assert ref.shape == model.shape, (name, ref.shape, model.shape)
            peak = float(np.max(np.abs(ref)))
            e_ref = float(np.max(np.abs(ref - model))) / peak
            print(f"{name:24s} {ref.shape[0]:2d} x {ref.shape[1]:5d}  peak {peak:.4e}  e_ref {e_ref:.3e}  "
                  f"boundary {min(bnd):.2e}  {sec:.4f} s / channel")
            for k in ("room", "src", "mics", "angle"):
                out[f"{name}/{k}"] = c[k]
            out[f"{name}/beta"] = rir_model.beta_of(c)
            out[f"{name}/rt60"] = np.float32(-1.0 if c["rt60"] is None else c["rt60"])
            out[f"{name}/ints"] = np.array([c["num_samples"], c["order"], int(c["hp"]),
                                            rir_model.MIC_TYPES[c["mic_type"]]], np.int32)
            out[f"{name}/fs_c"] = np.array([c["fs"], c["c"]], np.float32)
            out[f"{name}/rir"] = ref
            out[f"{name}/e_ref"] = np.float64(e_ref)
            out[f"{name}/sec_per_channel"] = np.float64(sec)
    return out


def main():
    from oracle import ref_harness as rh
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=rh.REF_ROOT, help="the reference tree")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture, write nothing")
    args = ap.parse_args()
    out = record(args.reference)
    if args.check:
        old = np.load(GOLDEN)
        bad = [k for k in out if "sec_per" not in k and not np.array_equal(np.asarray(out[k]), old[k])]
        print("reproduced" if not bad else f"differs: {bad}")
        return 1 if bad else 0
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
