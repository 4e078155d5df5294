#!/usr/bin/env python
"""AuxIVA (setk_auxiva_batch) at the per-GPU shard of BASELINE configs[2]: 125 utterances x 8
channels x 30 s, 16 kHz, audio resident in HBM, 20 epochs.  One GPU.  Prints one JSON line:
wall time per batch (warm-up, then >= 10 timed repeats: median / min / max; a host clock around
a call that ends in a stream synchronise), HIP-event time per stage (STFT, epochs with their
projections, transposition + inverse STFT, renorm), the time as a multiple of the float64 floor
derived in DESIGN.md and as x real time, and -- beside it, on one core of the host -- the numpy
model of tests/auxiva_model.py on ONE utterance ("model": the reference's python loop itself is
1 - 4 x slower than the model and does not travel).  Kernel times come from a separate run:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_auxiva.py --repeats 3 --model 0

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 76.8e12  # measured on the matrix pipe, tools/ubench/mfma_f64_layout.hip
HBM_PEAK = 8.0e12    # spec


def flops_per_bin_frame(C):
    """float64 operations an epoch needs per (bin, frame): C weighted covariances of
    C (C + 1) / 2 Hermitian entries (a complex multiply-add = 8), the weighting, the projection."""
    return C * (C * (C + 1) // 2) * 8 + 2 * C * C + C * C * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--model", type=int, default=1, help="time the numpy model on one utterance")
    a = ap.parse_args()
    import torch
    from setk_amd import _ffi, synth
    from setk_amd.libs.utils import stft_window
    if not torch.cuda.is_available():
        raise SystemExit("bench_auxiva needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    C, N = a.channels, int(a.seconds * 16000)
    ctx = _ffi.Context(0)
    ctx.stft_plan(512, 256, 512, True, stft_window("hann", 512))
    T = ctx.num_frames(N)
    L = ctx.istft_num_samples(T)
    F = 257
    host = [synth.synth_scene(i, C, N) for i in range(min(4, a.utts))]
    distinct = [torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(dev) for h in host]
    audio = [distinct[i % len(distinct)].clone() for i in range(a.utts)]
    waves = [torch.empty((C, L), dtype=torch.int16, device=dev) for _ in range(a.utts)]
    status = np.zeros(a.utts, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        ctx.auxiva_batch(C, [t.data_ptr() for t in audio], [N] * a.utts, a.epochs,
                         [w.data_ptr() for w in waves], status=status, flags=_ffi.FLAG_OUT_PCM16,
                         stream=stream)
        torch.cuda.synchronize()

    for _ in range(a.warmup):
        step()
    assert not status.any(), status
    ctx.set_profiling(True)
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    stage = ctx.last_stage_ms()
    ctx.set_profiling(False)
    times.sort()
    med = times[len(times) // 2]
    flops = flops_per_bin_frame(C) * F * T * a.utts * a.epochs
    spec_bytes = 8 * F * C * T * a.utts
    floor_ms = max(flops / FP64_PEAK, spec_bytes * a.epochs / HBM_PEAK) * 1e3
    rec = {
        "workload": f"AuxIVA {a.epochs} epochs, {a.utts} x {C} ch x {a.seconds:g} s (T = {T}), audio resident, PCM16 out",
        "ms_per_batch": {"median": round(med * 1e3, 2), "min": round(times[0] * 1e3, 2),
                         "max": round(times[-1] * 1e3, 2), "repeats": a.repeats, "warmup": a.warmup},
        "stage_ms": {"stft_maxabs": round(stage[0], 3), "epochs": round(stage[1], 3),
                     "transpose_istft": round(stage[2], 3), "renorm": round(stage[3], 3)},
        "x_real_time": round(a.utts * a.seconds / med, 1),
        "fp64_flop_per_batch": flops,
        "fp64_floor_ms": round(floor_ms, 2),
        "floor_bound": "fp64 matrix pipe" if flops / FP64_PEAK > spec_bytes * a.epochs / HBM_PEAK else "HBM",
        "epochs_over_floor": round(stage[1] / floor_ms, 2),
        "epochs_fp64_tflops": round(flops / (stage[1] * 1e-3) / 1e12, 2),
    }
    if a.model:
        # a child of its own with the BLAS pools pinned to one thread (set before numpy loads)
        import subprocess
        code = ("import sys, time, numpy as np\n"
                f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
                "import auxiva_model\n"
                "from oracle import np_oracle as o\n"
                "from setk_amd import synth\n"
                f"x = synth.synth_scene(0, {C}, {N})\n"
                "X = np.stack([o.forward_stft(c, frame_len=512, frame_hop=256, center=True, window='hann',"
                " transpose=True) for c in x])\n"
                "t0 = time.perf_counter()\n"
                f"auxiva_model.auxiva(X, {a.epochs})\n"
                "print(time.perf_counter() - t0)\n")
        env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1200)
        if r.returncode != 0:
            raise SystemExit("model run failed:\n" + r.stderr[-2000:])
        dt = float(r.stdout.strip().splitlines()[-1])
        rec["model_one_utterance_s"] = round(dt, 2)
        rec["model_threads"] = 1
        rec["model_x_real_time"] = round(a.seconds / dt, 2)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
