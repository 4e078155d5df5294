"""
Builds libsetk_hip.so (hand-written HIP for gfx950 + the C ABI of
include/setk_hip.h) in-tree with hipcc.  No CPU fallback exists: importing
the python mirror without this library raises.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libsetk_hip.so")
# The one list of translation units (`python setk_amd/build.py --units` prints it for the shell
# recipes under tools/): the kernel units, then the C ABI front end by feature (capi.h).
SOURCES = ["pass1.hip", "pass1_mc.hip", "pass2.hip", "pass2_mc.hip", "solve.hip", "modular.hip", "cgmm.hip", "cgmm_bin.hip", "cgmm_k.hip", "cacgmm.hip", "wpe.hip", "auxiva.hip", "ssl.hip", "spatial.hip", "ns.hip", "simu.hip", "online.hip", "wide.hip", "metric.hip", "rir.hip", "tfmask.hip", "comm.hip", "hostio.hip",
           "capi_support.hip", "capi_handle.hip", "capi_stft.hip", "capi_modular.hip", "capi_fused.hip", "capi_cgmm.hip", "capi_cacgmm.hip", "capi_wpe.hip", "capi_auxiva.hip", "capi_ssl.hip", "capi_spatial.hip", "capi_ns.hip", "capi_simu.hip", "capi_online.hip", "capi_metric.hip", "capi_rir.hip", "capi_tfmask.hip"]
HEADERS = ["common.h", "fft512.h", "dpp.h", "covar_fold.h", "mcdft.h", "mcdft_tables.h", "jacobi_herm.h", "capi.h", os.path.join("..", "..", "include", "setk_hip.h")]
ARCH = "gfx950"


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=False):
    """Compile every HIP translation unit for gfx950 and link the shared
    library.  Returns the library path."""
    os.makedirs(OBJ, exist_ok=True)
    # one builder at a time (the ranks of a torchrun launch all come through here)
    import fcntl
    with open(os.path.join(OBJ, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        return _build_locked(force, verbose)


def unit_flags(src, arch=ARCH):
    """The hipcc flags of one translation unit (everything but -c / -o): what the build uses and
    what tools/isa_census.py compiles with."""
    flags = ["--offload-arch=" + arch, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast",
             # SLP packing into v_pk_* costs more moves than it saves here (measured:
             # stft_covar 2.27 -> 1.86 ms, beamform_istft 1.46 -> 1.30 ms)
             "-fno-slp-vectorize",
             "-Wno-unused-result"] + os.environ.get("SETK_HIPCC_FLAGS", "").split()
    # pass 2 is one long straight-line block per frame: the max-ILP machine
    # scheduler measured 1-2 % faster there.  Pass 1 runs at a 128-VGPR budget
    # where the same scheduler spills (measured 1.14 vs 1.03 ms), so it keeps the
    # default.
    # Round 5 re-measured the strategies on the current sources (profiles/round5_sched_strategy_ab.txt):
    # pass 1 no longer spills under max-ilp / max-memory-clause and gains 0.7 % (0.929 against 0.936
    # ms), the matrix-core pass 2 0.6 % under max-ilp; iterative-maxocc costs pass 1 44 %.
    extra = {"pass1.hip": ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"],
             "pass2_mc.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
             "pass2.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
             "solve.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
             "modular.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
             "cgmm.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
             # (round 5: 16.5 - 16.7 ms per configs[4] batch against 17.0 - 17.4 with the default
             #  strategy, profiles/round5_cgmm_sched_ab.txt)
             "cgmm_bin.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"],
             "cgmm_k.hip": [],
             "cacgmm.hip": [],
             "wpe.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
             "auxiva.hip": [],
             "ssl.hip": [],
             "spatial.hip": [],
             "ns.hip": [],
             "simu.hip": [],
             "online.hip": [],
             "wide.hip": [],
             "metric.hip": [],
             "rir.hip": [],
             "tfmask.hip": [],
             "comm.hip": []}   # (the capi_*.hip units hold no kernel)
    # solve.hip and modular.hip hold a kernel each that must round like numpy operation by operation
    # (lu_refusal_kernel's LAPACK-order elimination; the Kaldi compressed-matrix decode) behind
    # `#pragma clang fp contract(off)`.  Plain `fast` lets the BACKEND fuse across the pragma (round 5's
    # lu_refusal_kernel was compiled with fused multiply-adds although its comment says otherwise);
    # `fast-honor-pragmas` honours it.  Every other kernel of the two units compiles to the same ISA
    # under both (diffed); cgmm.hip / cgmm_k.hip do not (float64 builtins lose the contract flag), so
    # the switch stays per unit.
    honor = {"solve.hip", "modular.hip"}
    fl = [f if f != "-ffp-contract=fast" or src not in honor else "-ffp-contract=fast-honor-pragmas"
          for f in flags]
    return fl + extra.get(src, [])


def _build_locked(force, verbose):
    hdrs = [os.path.normpath(os.path.join(CSRC, h)) for h in HEADERS]
    jobs = []
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([_hipcc()] + unit_flags(src) + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    if "--units" in sys.argv:
        print(" ".join(s[:-len(".hip")] for s in SOURCES))
        sys.exit(0)
    print(build_library(force="--force" in sys.argv, verbose=True))
