#!/usr/bin/env python
"""OM-LSA noise suppression (setk_ns_batch) on 125 single-channel utterances of 30 s, 16 kHz:
samples resident in HBM, waveforms out (float32), both noise trackers.  One GPU.  Per tracker one
record: wall time per batch (warm-up, then timed repeats: median / min / max; a host clock around a
call that ends in a stream synchronise), HIP-event time per stage (STFT, the recursion, inverse
STFT), the recursion per frame, and a DERIVED floor for it: the recursion is one workgroup per
utterance walking T frames, so its time is T x the dependent float64 chain of a frame, whatever
the batch size up to the number of CUs.  The chain is counted from csrc/ns.hip (series branch of
E1: about 250 dependent float64 operations with log, exp, two pow and six divisions expanded) at 8
cycles per dependent float64 operation and 2.4 GHz -- an assumption, not a measurement.  Beside
it, on one core of the host, the numpy model of tests/ns_model.py on ONE utterance, and the
reference's own measured rate per spectrogram cell (0.28 ms iMCRA, 0.34 ms MCRA: its numerical
integral).  Writes profiles/ns/bench_ns.json (--out).  No pass / fail time.

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHAIN_OPS, CYCLES_PER_OP, CLOCK_HZ = 250, 8, 2.4e9
REFERENCE_MS_PER_CELL = {"imcra": 0.28, "mcra": 0.34}


def model_seconds(kind, N):
    """tests/ns_model.py on one utterance, one thread (set before numpy loads)."""
    code = ("import sys, time, numpy as np\n"
            f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import ns_model\n"
            "from oracle import np_oracle as o\n"
            f"x = ns_model.synth_samples({N}, 0).astype(np.float32)\n"
            "X = o.forward_stft(x, frame_len=512, frame_hop=256, center=True, window='hann', transpose=True)\n"
            "t0 = time.perf_counter()\n"
            f"ns_model.run({kind!r}, X)\n"
            "print(time.perf_counter() - t0)\n")
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1200)
    if r.returncode != 0:
        raise SystemExit("model run failed:\n" + r.stderr[-2000:])
    return float(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--kinds", type=str, default="imcra,mcra")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--model", type=int, default=1, help="time the numpy model on one utterance")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ns", "bench_ns.json"))
    a = ap.parse_args()
    import torch
    import ns_model
    from setk_amd import _ffi
    from setk_amd.libs import ns
    from setk_amd.libs.utils import stft_window
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    N, F = int(a.seconds * 16000), 257
    ctx = _ffi.Context(0)
    ctx.stft_plan(512, 256, 512, True, stft_window("hann", 512))
    T, L = ctx.num_frames(N), ctx.istft_num_samples(ctx.num_frames(N))
    stream = torch.cuda.current_stream().cuda_stream
    distinct = [torch.from_numpy(ns_model.synth_samples(N, i).astype(np.float32)).to(dev) for i in range(min(4, a.utts))]
    audio = [distinct[i % len(distinct)] for i in range(a.utts)]
    waves = [torch.empty(L, dtype=torch.float32, device=dev) for _ in range(a.utts)]
    status = np.zeros(a.utts, dtype=np.int32)
    floor_ms = T * CHAIN_OPS * CYCLES_PER_OP / CLOCK_HZ * 1e3
    records = []
    for kind in a.kinds.split(","):
        opts = (ns.MCRA() if kind == "mcra" else ns.iMCRA()).opts(gain=False, spec=True)

        def step():
            ctx.ns_batch(opts, [t.data_ptr() for t in audio], [N] * a.utts, wave_ptrs=[w.data_ptr() for w in waves],
                         status=status, stream=stream)
            torch.cuda.synchronize()

        for _ in range(a.warmup):
            step()
        ctx.set_profiling(True)
        times, stages = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            step()
            times.append(time.perf_counter() - t0)
            stages.append(ctx.last_stage_ms())
        ctx.set_profiling(False)
        times.sort()
        med = times[len(times) // 2]
        stage = [sorted(s[i] for s in stages)[len(stages) // 2] for i in range(4)]
        rec = {
            "workload": f"setk_ns_batch {kind}, {a.utts} x 1 ch x {a.seconds:g} s (T = {T}, F = {F}), samples "
                        "resident, float32 waveforms out",
            "ms_per_batch": {"median": round(med * 1e3, 2), "min": round(times[0] * 1e3, 2),
                             "max": round(times[-1] * 1e3, 2), "repeats": a.repeats, "warmup": a.warmup},
            "x_real_time": round(a.utts * a.seconds / med, 1),
            "stage_ms": {"stft": round(stage[0], 3), "recursion": round(stage[1], 3), "istft": round(stage[2], 3)},
            "recursion_us_per_frame": round(stage[1] * 1e3 / T, 3),
            "recursion_ns_per_cell": round(stage[1] * 1e6 / (a.utts * T * F), 3),
            "derived_floor_ms": round(floor_ms, 3),
            "derived_floor_assumes": f"{CHAIN_OPS} dependent float64 operations per frame x {CYCLES_PER_OP} cycles at "
                                     f"{CLOCK_HZ / 1e9:g} GHz, one workgroup per utterance",
            "recursion_over_floor": round(stage[1] / floor_ms, 2),
            "reference_ms_per_cell": REFERENCE_MS_PER_CELL[kind],
            "reference_batch_s": round(REFERENCE_MS_PER_CELL[kind] * 1e-3 * a.utts * T * F, 0),
            "status_ok": bool((status == 0).all()),
            "finite": bool(torch.isfinite(waves[0]).all().item()),
        }
        if a.model:
            dt = model_seconds(kind, N)
            rec["model_one_utterance_s"] = round(dt, 2)
            rec["model_threads"] = 1
            rec["model_x_real_time"] = round(a.seconds / dt, 2)
        records.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump(records, fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
