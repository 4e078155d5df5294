#!/usr/bin/env python
"""Oracle TF masks and oracle separation on 125 utterances of 30 s, 16 kHz, samples resident in
HBM.  One GPU.  Two workloads, one record each:

  masks    setk_tf_mask_batch, irm, 125 (clean, noisy) pairs -> 125 masks [T][257] float32
  oracle   setk_oracle_separate_batch, irm, K = 2: 125 mixtures + 250 references -> 250 waves

Per record: wall time per batch (warm-up, then timed repeats: median / min / max; a host clock
around a call that ends in a stream synchronise), HIP-event time per stage (setk_last_stage_ms),
and the byte floor of the workload (what must cross HBM once, at the 6.3 TB/s copy rate DESIGN.md
section 5 uses) with the stage's multiple of it.

The A/B the fused forward answers to: in the same process, interleaved repeat by repeat, the
fused forward launch of the masks workload against the TWO setk_stft_batch launches that the
unfused chain (setk_stft_batch x 2 -> setk_tf_mask) cannot avoid, on the same batch, both by HIP
events; medians.  Writes profiles/tfmask/bench_tfmask.json (--out).  No pass / fail time.

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_RATE = 6.3e12


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "tfmask", "bench_tfmask.json"))
    a = ap.parse_args()
    import torch
    import tfmask_cases as tc
    from setk_amd import _ffi
    from setk_amd.libs.utils import stft_window
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfmask needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    N, F, U = int(a.seconds * 16000), 257, a.utts
    ctx = _ffi.Context(0)
    ctx.stft_plan(512, 256, 512, True, stft_window("hann", 512))
    T = ctx.num_frames(N)
    L = ctx.istft_num_samples(T)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    parts = [[tc.coloured(rng, N).astype(np.float32), (0.7 * tc.coloured(rng, N)).astype(np.float32)] for _ in range(4)]
    tgt = [torch.from_numpy(p[0]).to(dev) for p in parts]
    oth = [torch.from_numpy(p[1]).to(dev) for p in parts]
    mix = [torch.from_numpy(p[0] + p[1]).to(dev) for p in parts]
    pick = lambda v: [v[i % 4].data_ptr() for i in range(U)]  # noqa: E731
    ns = [N] * U
    status = np.zeros(U, dtype=np.int32)
    records = []

    # ---- masks, and the A/B against two setk_stft_batch launches ----
    masks = [torch.empty((T, F), dtype=torch.float32, device=dev) for _ in range(U)]
    spec_a = [torch.empty((1, T, F), dtype=torch.complex64, device=dev) for _ in range(U)]
    spec_b = [torch.empty((1, T, F), dtype=torch.complex64, device=dev) for _ in range(U)]
    mptr, aptr, bptr = [m.data_ptr() for m in masks], [s.data_ptr() for s in spec_a], [s.data_ptr() for s in spec_b]

    def fused():
        ctx.tf_mask_batch("irm", pick(tgt), pick(mix), ns, mptr, status=status, want_stats=True, stream=stream)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def two_stft():
        e0.record()
        ctx.stft_batch(1, pick(tgt), ns, aptr, stream=stream)
        ctx.stft_batch(1, pick(mix), ns, bptr, stream=stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        fused()
        two_stft()
    ctx.set_profiling(True)
    wall, stages, chain = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        fused()
        wall.append(time.perf_counter() - t0)
        stages.append(ctx.last_stage_ms())
        ctx.set_profiling(False)
        chain.append(two_stft())
        ctx.set_profiling(True)
    ctx.set_profiling(False)
    fwd = median([s[0] for s in stages])
    floor = U * (2 * 4 * N + 4 * T * F) / COPY_RATE * 1e3
    chain_bytes = U * (2 * 4 * N + 2 * 2 * 8 * T * F + 4 * T * F)
    rec = {
        "workload": f"setk_tf_mask_batch irm, {U} pairs x {a.seconds:g} s (T = {T}, F = {F}), samples resident, "
                    "masks float32 out",
        "ms_per_batch": {"median": round(median(wall) * 1e3, 3), "min": round(min(wall) * 1e3, 3),
                         "max": round(max(wall) * 1e3, 3), "repeats": a.repeats, "warmup": a.warmup},
        "stage_ms": {"fused_forward": round(fwd, 3), "statistics": round(median([s[1] for s in stages]), 3)},
        "byte_floor_ms": round(floor, 3),
        "byte_floor_assumes": f"two signals read, one mask written, once each, at {COPY_RATE / 1e12:g} TB/s",
        "fused_forward_over_floor": round(fwd / floor, 2),
        "ab_two_stft_batch_launches_ms": {"median": round(median(chain), 3), "min": round(min(chain), 3),
                                          "max": round(max(chain), 3)},
        "ab_fused_forward_ms": {"median": round(fwd, 3), "min": round(min(s[0] for s in stages), 3),
                                "max": round(max(s[0] for s in stages), 3)},
        "ab_interleaved_repeats": a.repeats,
        "fused_forward_beats_two_stft_launches": bool(fwd < median(chain)),
        "bytes_fused_MB_per_utt": round((2 * 4 * N + 4 * T * F) / 1e6, 2),
        "bytes_chain_MB_per_utt": round(chain_bytes / U / 1e6, 2),
        "status_ok": bool((status == 0).all()),
        "finite": bool(torch.isfinite(masks[0]).all().item()),
    }
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del masks, spec_a, spec_b

    # ---- oracle separation, K = 2 ----
    K = 2
    waves = [torch.empty(L, dtype=torch.float32, device=dev) for _ in range(U * K)]
    tptr = [p for i in range(U) for p in (tgt[i % 4].data_ptr(), oth[i % 4].data_ptr())]

    def step():
        ctx.oracle_separate_batch("irm", K, pick(mix), tptr, ns, [w.data_ptr() for w in waves], status=status,
                                  stream=stream)

    for _ in range(a.warmup):
        step()
    ctx.set_profiling(True)
    wall, stages = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        step()
        wall.append(time.perf_counter() - t0)
        stages.append(ctx.last_stage_ms())
    ctx.set_profiling(False)
    st = [median([s[i] for s in stages]) for i in range(4)]
    fwd_floor = U * ((K + 1) * 4 * N + K * 8 * T * F) / COPY_RATE * 1e3
    inv_floor = U * (K * 8 * T * F + K * 4 * L) / COPY_RATE * 1e3
    rec = {
        "workload": f"setk_oracle_separate_batch irm, K = {K}, {U} mixtures x {a.seconds:g} s (T = {T}, F = {F}), "
                    "samples resident, float32 waveforms out",
        "ms_per_batch": {"median": round(median(wall) * 1e3, 3), "min": round(min(wall) * 1e3, 3),
                         "max": round(max(wall) * 1e3, 3), "repeats": a.repeats, "warmup": a.warmup},
        "x_real_time": round(U * a.seconds / median(wall), 1),
        "stage_ms": {"fused_forward": round(st[0], 3), "istft": round(st[1], 3), "scale": round(st[2], 3)},
        "byte_floor_ms": {"fused_forward": round(fwd_floor, 3), "istft": round(inv_floor, 3)},
        "byte_floor_assumes": f"K + 1 signals read and K masked spectra written; those read and K waves written; "
                              f"once each, at {COPY_RATE / 1e12:g} TB/s",
        "fused_forward_over_floor": round(st[0] / fwd_floor, 2),
        "istft_over_floor": round(st[1] / inv_floor, 2),
        "status_ok": bool((status == 0).all()),
        "finite": bool(torch.isfinite(waves[0]).all().item()),
    }
    records.append(rec)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump(records, fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
