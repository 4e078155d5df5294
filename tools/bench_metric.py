#!/usr/bin/env python
"""SI-SNR scoring with permutation alignment (setk_si_snr_batch) on 125 utterances of 30 s, 16 kHz,
at K = 2 and K = 8 sources, float32 and 16-bit samples resident in HBM (every signal in memory of
its own: nothing is served twice out of a cache).  One GPU.  Per workload one record: wall time
per batch (warm-up, then timed repeats: median / min / max; a host clock around a call that ends
in a stream synchronise), HIP-event time per phase from the profile marks (means, centred Gram
sums, residuals, table + search + copies), and two DERIVED floors per phase:
  byte floor    the bytes the phase must read (every sample of the 2 K signals once) / 6.3 TB/s,
                the achievable HBM rate
  launch floor  its dependent launches (means 2, Gram 2, residual 1, search 1) x 1.8 us, the
                boundary between real streaming kernels
Beside it, on the host, the float64 numpy statement tests/metric_model.py on ONE utterance.
Writes profiles/metric/bench_metric.json (--out).  No pass / fail time.

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

HBM_BYTES_PER_S, BOUNDARY_US = 6.3e12, 1.8
LAUNCHES = {"means": 2, "gram": 2, "residual": 1, "search": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sources", type=str, default="2,8")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--model", type=int, default=1, help="time the numpy statement on one utterance")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "metric", "bench_metric.json"))
    a = ap.parse_args()
    import torch
    import metric_model as model
    from setk_amd import _ffi
    if not torch.cuda.is_available():
        raise SystemExit("bench_metric needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    L = int(a.seconds * 16000)
    ctx = _ffi.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    records = []
    for K in [int(k) for k in a.sources.split(",")]:
        est, ref = [], []
        for n in range(K):  # estimate n on reference (n + 1) % K, 5 to 26 dB
            x, s = model.planted(rng, L, 5.0 + 3.0 * n)
            est.append(x)
            ref.append(s)
        ref = ref[-1:] + ref[:-1]
        want = (np.arange(K) + 1) % K
        host_s = None
        if a.model:
            t0 = time.perf_counter()
            model.permute_si_snr(est, ref, align=True)
            host_s = time.perf_counter() - t0
        for form in ("float32", "pcm16"):
            def device_copies(v):
                if form == "pcm16":
                    v = np.clip(np.rint(v.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
                first = torch.from_numpy(v).to(dev)
                return [first] + [first.clone() for _ in range(a.utts - 1)]
            e_dev, r_dev = [device_copies(v) for v in est], [device_copies(v) for v in ref]
            eptr = [e_dev[n][u].data_ptr() for u in range(a.utts) for n in range(K)]
            rptr = [r_dev[n][u].data_ptr() for u in range(a.utts) for n in range(K)]
            pair = torch.empty(a.utts * K * K, dtype=torch.float64, device=dev)
            best = torch.empty(a.utts, dtype=torch.float64, device=dev)
            perm = torch.empty(a.utts * K, dtype=torch.int32, device=dev)
            status = np.zeros(a.utts, dtype=np.int32)
            flags = _ffi.FLAG_IN_PCM16 if form == "pcm16" else 0

            def step():
                ctx.si_snr_batch([K] * a.utts, eptr, [1] * len(eptr), rptr, [1] * len(rptr), [L] * a.utts,
                                 pair.data_ptr(), best=best.data_ptr(), perm=perm.data_ptr(), status=status,
                                 flags=flags, stream=stream)

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
            stage = dict(zip(LAUNCHES, [sorted(s[i] for s in stages)[len(stages) // 2] for i in range(4)]))
            phase_bytes = a.utts * 2 * K * L * (2 if form == "pcm16" else 4)
            byte_floor = {p: (phase_bytes / HBM_BYTES_PER_S * 1e3 if p != "search" else 0.0) for p in LAUNCHES}
            launch_floor = {p: n * BOUNDARY_US * 1e-3 for p, n in LAUNCHES.items()}
            rec = {
                "workload": f"setk_si_snr_batch, {a.utts} utterances x {a.seconds:g} s, K = {K} ({2 * K} signals, "
                            f"{K * K} pairs, {int(np.prod(np.arange(1, K + 1)))} orders), {form} samples resident",
                "ms_per_batch": {"median": round(med * 1e3, 3), "min": round(times[0] * 1e3, 3),
                                 "max": round(times[-1] * 1e3, 3), "repeats": a.repeats, "warmup": a.warmup},
                "x_real_time": round(a.utts * a.seconds / med, 1),
                "phase_ms": {p: round(v, 4) for p, v in stage.items()},
                "phase_bytes": phase_bytes,
                "byte_floor_ms": {p: round(v, 4) for p, v in byte_floor.items()},
                "launch_floor_ms": {p: round(v, 4) for p, v in launch_floor.items()},
                "binding_floor": {p: ("bytes" if byte_floor[p] >= launch_floor[p] else "launches") for p in LAUNCHES},
                "phase_over_floor": {p: round(stage[p] / max(byte_floor[p], launch_floor[p]), 2) for p in LAUNCHES},
                "sum_of_floors_ms": round(sum(max(byte_floor[p], launch_floor[p]) for p in LAUNCHES), 4),
                "floor_assumes": f"{HBM_BYTES_PER_S / 1e12:g} TB/s achievable HBM rate; {BOUNDARY_US} us per dependent "
                                 "launch",
                "status_ok": bool((status == 0).all()),
                "orders_recovered": bool((perm.cpu().numpy().reshape(a.utts, K) == want).all()),
            }
            if host_s is not None:
                rec["host_numpy_one_utterance_s"] = round(host_s, 3)
                rec["host_numpy_batch_s"] = round(host_s * a.utts, 1)
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del e_dev, r_dev
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump(records, fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
