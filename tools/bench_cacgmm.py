#!/usr/bin/env python
"""CACGMM (setk_cacgmm_estimate_batch) at the per-GPU shard of BASELINE configs[2]: 125
utterances x 8 channels x 30 s, 16 kHz, audio and starts resident in HBM, K = 3, 50 iterations.
One GPU.  Prints one JSON line: wall time per batch (warm-up, then timed repeats: median / min /
max; a host clock around a call that ends in a stream synchronise), HIP-event time per stage
(STFT into the bin-major layout, the EM launch), the EM as a multiple of the floor derived in
DESIGN.md section 5 -- the K covariances at the fp64 matrix rate, the quadratic forms at the
fp64 vector rate, one HBM read of the spectrogram -- and, beside it, the nearest existing
arithmetic: the general CGMM EM (setk_cgmm_masks_k, K = 3, csrc/cgmm_k.hip, the same kernel as
before this tool existed) on ONE utterance of the same shape with the same number of iterations,
scaled to the batch.  Kernel times come from a separate run:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_cacgmm.py --repeats 2

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MATRIX = 76.8e12  # measured on the matrix pipe, tools/ubench/mfma_f64_layout.hip
FP64_VECTOR = 78.6e12  # spec
HBM_PEAK = 8.0e12      # spec


def flops_per_bin_frame(C, K):
    """float64 operations an iteration needs per (bin, frame): (matrix, vector).  Matrix: K weighted
    covariances of C (C + 1) / 2 Hermitian entries (a complex multiply-add = 8).  Vector: K
    quadratic forms in the eigenbasis (C projections of C complex multiply-adds, |.|^2 / w)."""
    return K * (C * (C + 1) // 2) * 8, K * (C * C * 8 + 4 * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cgmm-k", type=int, default=1, help="time setk_cgmm_masks_k on one utterance")
    a = ap.parse_args()
    import torch
    from setk_amd import _ffi, synth
    from setk_amd.libs.utils import stft_window
    if not torch.cuda.is_available():
        raise SystemExit("bench_cacgmm needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    C, K, N = a.channels, a.classes, int(a.seconds * 16000)
    ctx = _ffi.Context(0)
    ctx.stft_plan(512, 256, 512, True, stft_window("hann", 512))
    T, F = ctx.num_frames(N), 257
    host = [synth.synth_scene(i, C, N) for i in range(min(4, a.utts))]
    distinct = [torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(dev) for h in host]
    audio = [distinct[i % len(distinct)] for i in range(a.utts)]
    g = torch.rand((K, F, T), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(777))
    g0 = (g / g.sum(0, keepdim=True)).contiguous()
    masks = [torch.empty((K, T, F), dtype=torch.float32, device=dev) for _ in range(a.utts)]
    status = np.zeros(a.utts, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        ctx.cacgmm_estimate_batch(C, [t.data_ptr() for t in audio], [N] * a.utts, K, a.iters,
                                  [g0.data_ptr()] * a.utts, [m.data_ptr() for m in masks], stream=stream,
                                  status=status)
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
    fm, fv = flops_per_bin_frame(C, K)
    cells = F * T * a.utts * a.iters
    spec_bytes = 8 * F * C * T * a.utts
    floor_ms = (fm * cells / FP64_MATRIX + fv * cells / FP64_VECTOR + spec_bytes / HBM_PEAK) * 1e3
    rec = {
        "workload": f"CACGMM K = {K}, {a.iters} iterations, {a.utts} x {C} ch x {a.seconds:g} s (T = {T}), "
                    "audio and starts resident",
        "ms_per_batch": {"median": round(med * 1e3, 2), "min": round(times[0] * 1e3, 2),
                         "max": round(times[-1] * 1e3, 2), "repeats": a.repeats, "warmup": a.warmup},
        "stage_ms": {"stft": round(stage[0], 3), "em": round(stage[1], 3)},
        "x_real_time": round(a.utts * a.seconds / med, 1),
        "floor_ms": {"matrix": round(fm * cells / FP64_MATRIX * 1e3, 2),
                     "vector": round(fv * cells / FP64_VECTOR * 1e3, 2),
                     "hbm": round(spec_bytes / HBM_PEAK * 1e3, 2), "sum": round(floor_ms, 2)},
        "em_over_floor": round(stage[1] / floor_ms, 2),
    }
    if a.cgmm_k:
        spec = torch.empty((C, T, F), dtype=torch.complex64, device=dev)
        ctx.stft(audio[0], spec)
        gam = torch.empty((K, T, F), dtype=torch.float32, device=dev)
        ks = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.cgmm_masks_k(spec, C, T, F, K, a.iters, g0, None, gam, update_alpha=True)
            torch.cuda.synchronize()
            ks.append(time.perf_counter() - t0)
        one = min(ks[1:])
        rec["cgmm_masks_k_one_utterance_ms"] = round(one * 1e3, 2)
        rec["cgmm_masks_k_scaled_to_batch_ms"] = round(one * a.utts * 1e3, 1)
        rec["cgmm_masks_k_over_cacgmm_em"] = round(one * a.utts * 1e3 / stage[1], 2)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
