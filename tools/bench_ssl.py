#!/usr/bin/env python
"""Sound source localisation (setk_ssl_batch) at the per-GPU shard of BASELINE configs[2]: 125
utterances x 8 channels x 30 s, 16 kHz, 360 directions, audio resident in HBM, offline (one
window per utterance).  One GPU.  Prints one JSON line per backend (ml, srp, music): wall time
per batch (warm-up, then >= 10 timed repeats: median / min / max; a host clock around a call
that ends in a stream synchronise), HIP-event time per stage (STFT, frame scores, window
reduction), the frame-score stage as a multiple of the fp32 floor derived in DESIGN.md, x real
time, and -- beside it, on one core of the host -- the numpy model of tests/ssl_model.py on ONE
utterance.  `--online CHUNK,LOOKBACK` times the online windows instead.  Kernel times come from
a separate run:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_ssl.py --repeats 3 --model 0

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_PEAK = 157.3e12  # vector fp32, spec (256 CUs x 128 lanes x 2 x 2.4 GHz)


def flops_per_cell(backend, C, P):
    """fp32 operations per (direction, frame, bin): ML a complex inner product over the channels
    (8 C), |.|^2, the subtraction and the masked accumulation (6; the logarithm runs on the
    transcendental unit); SRP one real part per pair (4 P) on every frame (online) -- offline the
    frames are folded first and the contraction is T times smaller."""
    return 8 * C + 6 if backend == "ml" else 4 * P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--doas", type=int, default=360)
    ap.add_argument("--backends", type=str, default="ml,srp,music")
    ap.add_argument("--online", type=str, default="", help="CHUNK,LOOKBACK frames: the online windows")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--model", type=int, default=1, help="time the numpy model on one utterance")
    a = ap.parse_args()
    import torch
    from setk_amd import _ffi, synth
    from setk_amd.libs.beamformer import circular_steer_vector
    from setk_amd.libs.utils import stft_window
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssl needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    C, N, A, F = a.channels, int(a.seconds * 16000), a.doas, 257
    ctx = _ffi.Context(0)
    ctx.stft_plan(512, 256, 512, True, stft_window("hann", 512))
    T = ctx.num_frames(N)
    sv = np.stack([circular_steer_vector(0.05, C, d, F, c=343, sr=16000) for d in np.arange(0, 360, 360 / A)])
    sv = np.ascontiguousarray(sv.transpose(0, 2, 1), dtype=np.complex64)
    d_sv = torch.from_numpy(sv).to(dev)
    pairs = (list(range(C // 2)), [i + C // 2 for i in range(C // 2)])
    host = [synth.synth_scene(i, C, N) for i in range(min(4, a.utts))]
    distinct = [torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(dev) for h in host]
    audio = [distinct[i % len(distinct)].clone() for i in range(a.utts)]
    mask = torch.rand((T, F), dtype=torch.float32, device=dev)
    if a.online:
        chunk, back = [int(v) for v in a.online.split(",")]
        wins = [(max(t - back, 0), min(t + chunk, T)) for t in range(0, T, chunk)]
    else:
        wins = [(0, T)]
    index = torch.empty(a.utts * len(wins), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for backend in a.backends.split(","):
        opts = _ffi.ssl_opts(backend, srp_pair=pairs, compression=-1, eps=float(np.finfo(np.float32).eps))
        status = np.zeros(a.utts, dtype=np.int32)

        def step():
            ctx.ssl_batch(opts, C, [t.data_ptr() for t in audio], [N] * a.utts, [mask.data_ptr()] * a.utts, d_sv, A,
                          [wins] * a.utts, index.data_ptr(), status=status, stream=stream)
            torch.cuda.synchronize()

        for _ in range(a.warmup):
            step()
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
        rec = {
            "workload": f"SSL {backend}, {a.utts} x {C} ch x {a.seconds:g} s (T = {T}) x {A} directions, "
                        f"{len(wins)} window(s) per utterance, masked, audio resident",
            "ms_per_batch": {"median": round(med * 1e3, 2), "min": round(times[0] * 1e3, 2),
                             "max": round(times[-1] * 1e3, 2), "repeats": a.repeats, "warmup": a.warmup},
            "stage_ms": {"stft": round(stage[0], 3), "frame_scores": round(stage[1], 3), "reduce": round(stage[2], 3)},
            "x_real_time": round(a.utts * a.seconds / med, 1),
            "worst_status": int(status.max()),
        }
        if backend == "ml" or (backend == "srp" and a.online):
            flops = flops_per_cell(backend, C, len(pairs[0])) * A * T * F * a.utts
            rec["fp32_flop_per_batch"] = flops
            rec["fp32_floor_ms"] = round(flops / FP32_PEAK * 1e3, 2)
            rec["frame_scores_over_floor"] = round(stage[1] / (flops / FP32_PEAK * 1e3), 2)
            rec["frame_scores_fp32_tflops"] = round(flops / (stage[1] * 1e-3) / 1e12, 2)
        if a.model:
            # a child of its own with the BLAS pools pinned to one thread (set before numpy loads)
            import subprocess
            code = ("import sys, time, numpy as np\n"
                    f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
                    "import ssl_model\n"
                    "from oracle import np_oracle as o\n"
                    "from setk_amd import synth\n"
                    f"x = synth.synth_scene(0, {C}, {N})\n"
                    "X = np.stack([o.forward_stft(c, frame_len=512, frame_hop=256, center=True, window='hann',"
                    " transpose=True) for c in x])\n"
                    f"sv = ssl_model.steer_vectors('circular', {A}, 257, around={C}, radius=0.05)\n"
                    "mask = np.random.default_rng(0).uniform(size=X.shape[1:])\n"
                    "t0 = time.perf_counter()\n"
                    f"for t in range(0, X.shape[1], 256):\n"   # (the model's A x T x F arrays, a block of frames at a time)
                    f"    ssl_model.get_doa({backend!r}, X[:, t:t + 256], sv, mask[t:t + 256], "
                    f"{pairs!r} if {backend!r} == 'srp' else None)\n"
                    "print(time.perf_counter() - t0)\n")
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1200)
            if r.returncode != 0:
                raise SystemExit("model run failed:\n" + r.stderr[-2000:])
            dt = float(r.stdout.strip().splitlines()[-1])
            rec["model_one_utterance_s"] = round(dt, 2)
            rec["model_threads"] = 1
            rec["model_x_real_time"] = round(a.seconds / dt, 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
