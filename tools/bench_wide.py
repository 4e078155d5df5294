#!/usr/bin/env python
"""The batched call for 9 to 16 channels (setk_enhance_batch's wide path, csrc/wide.hip) on 125
utterances x 10 s, 16 kHz, at 12 and 16 channels, MVDR.  One GPU.  Per channel count:

  resident   samples and masks in HBM, float32 waves out: wall time per batch (warm-up, then timed
             repeats: median / min / max; a host clock around a call that ends in a stream
             synchronise) and HIP-event time per stage (STFT + covariances; weights; beamform +
             iSTFT; renorm) from setk_last_stage_ms;
  engine     BatchEnhancer.enhance on the same utterances as host arrays (upload, the batched call,
             download) at batches of 1, 8 and all of them;
  unfused    BatchEnhancer._run_unfused, the path these channel counts took before (one utterance at
             a time through the stand-alone operators, same host arrays in and out), same batches.

DERIVED, not measured: the bytes of spectra that make the round trip through HBM (8 F C Tp per
utterance, written once and read twice) and the scratch of the call.

Writes profiles/wide/bench_wide.json (--out).  No pass / fail time.

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(step, warmup, repeats):
    for _ in range(warmup):
        step()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    times.sort()
    return {"median": round(times[len(times) // 2] * 1e3, 3), "min": round(times[0] * 1e3, 3),
            "max": round(times[-1] * 1e3, 3), "repeats": repeats, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--channels", type=str, default="12,16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--engine-repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "wide", "bench_wide.json"))
    a = ap.parse_args()
    import torch
    from setk_amd import _ffi, synth
    from setk_amd.engine import BatchEnhancer
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    U, N = a.utts, int(a.seconds * 16000)
    recs = []
    for C in [int(v) for v in a.channels.split(",")]:
        ctx = _ffi.Context(0)
        ctx.stft_plan(512, 256, 512, True)
        stream = torch.cuda.current_stream().cuda_stream
        T = ctx.num_frames(N)
        L = ctx.istft_num_samples(T)
        base = [synth.synth_utterance(500 + k, C, N).astype(np.float32) for k in range(5)]
        rng = np.random.default_rng(5)
        hmask = [(0.1 + 0.8 * rng.random((T, 257))).astype(np.float32) for _ in range(5)]
        audio = [torch.from_numpy(base[u % 5]).to(dev).clone() for u in range(U)]
        masks = [torch.from_numpy(hmask[u % 5]).to(dev).clone() for u in range(U)]
        waves = [torch.empty(L, dtype=torch.float32, device=dev) for _ in range(U)]
        aptr, mptr, wptr, ns = [t.data_ptr() for t in audio], [t.data_ptr() for t in masks], \
            [t.data_ptr() for t in waves], [N] * U
        opts = _ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK, pmwf_ref=-1)
        status = []

        def resident():
            status[:] = ctx.enhance_batch(opts, C, aptr, ns, mptr, None, wptr, want_status=True, stream=stream)
            torch.cuda.synchronize()

        for _ in range(a.warmup):
            resident()
        ctx.set_profiling(True)
        times, stages = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            resident()
            times.append(time.perf_counter() - t0)
            stages.append(ctx.last_stage_ms())
        ctx.set_profiling(False)
        times.sort()
        stage = [round(sorted(s[i] for s in stages)[len(stages) // 2], 3) for i in range(4)]
        med = times[len(times) // 2] * 1e3
        Tp = (T + 3) & ~3
        slabs = -(-T // 128)
        rec = {"workload": f"{U} utterances x {C} ch x {a.seconds:g} s, 16 kHz (T = {T} frames), MVDR, float32 out",
               "resident": {"ms_per_batch": {"median": round(med, 3), "min": round(times[0] * 1e3, 3),
                                             "max": round(times[-1] * 1e3, 3), "repeats": a.repeats, "warmup": a.warmup},
                            "ms_per_utterance": round(med / U, 4),
                            "stage_ms": dict(zip(("stft_covariances", "weights", "beamform_istft", "renorm"), stage)),
                            "x_real_time": round(U * a.seconds / (med * 1e-3), 1),
                            "status_ok": all(s == 0 for s in status),
                            "spectra_mb_derived": round(U * 8 * 257 * C * Tp / 1e6, 1),
                            "slabs_mb_derived": round(U * slabs * 257 * 824 * 4 / 1e6, 1)},
               "host_arrays": {}}
        # release the resident copies before the engine makes its own
        del audio, masks, waves
        torch.cuda.empty_cache()
        eng = BatchEnhancer(beamformer="mvdr", ctx=ctx)
        for n in sorted({1, min(8, U), U}):
            utts = [(base[u % 5], hmask[u % 5], None) for u in range(n)]
            out = [None] * n

            def fused():
                out[:] = eng.enhance(utts)

            def unfused():
                eng._run_unfused(utts, list(range(n)), C, False, out)

            f = wall(fused, 1, a.engine_repeats)
            ok_f = all(s == 0 for _, s in out)
            g = wall(unfused, 1, a.engine_repeats)
            ok_u = all(s == 0 for _, s in out)
            rec["host_arrays"][str(n)] = {
                "engine_ms": f, "unfused_ms": g, "status_ok": ok_f and ok_u,
                "engine_ms_per_utterance": round(f["median"] / n, 3),
                "unfused_ms_per_utterance": round(g["median"] / n, 3),
                "speed_up": round(g["median"] / f["median"], 2)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump(recs, fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
