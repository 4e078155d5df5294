#!/usr/bin/env python
"""Geometry-driven spatial features (setk_spatial_batch) at the per-GPU shard of BASELINE
configs[2]: 125 utterances x 8 channels x 30 s, 16 kHz, spectrograms resident in HBM (one
setk_stft_batch in front, timed on its own).  One GPU.  Four kinds: the linear SRP-PHAT spectrum
(28 pairs, 181 DoA), the circular one (3 diagonal pairs of 6 microphones, 121 DoA), cos+sin IPD
(4 pairs) and DF over 4 directions (4 pairs).  Per kind one record: wall time per batch (warm-up,
then timed repeats: median / min / max; a host clock around a call that ends in a stream
synchronise), HIP-event time per stage (SRP: observation tiles, pair contraction, combination),
for SRP the contraction as a multiple of the fp32 floor (4 operations per pair, frame, bin and
direction over the 157 TFLOP/s vector peak DESIGN.md section 5 uses) and -- beside it, on one
core of the host -- the numpy model of tests/spatial_model.py on ONE utterance.  The batch runs
in chunks of --chunk utterances, as the engine bounds its scratch.  Writes
profiles/spatial/bench_spatial.json (--out).  No pass / fail time.

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

FP32_PEAK = 157.3e12  # vector fp32, spec (256 CUs x 128 lanes x 2 x 2.4 GHz)


def model_seconds(kind, C, N, spec):
    """tests/spatial_model.py on one utterance, one thread (set before numpy loads)."""
    code = ("import sys, time, numpy as np\n"
            f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import spatial_model as sm\n"
            "from oracle import np_oracle as o\n"
            "from setk_amd import synth\n"
            f"x = synth.synth_scene(0, {C}, {N})\n"
            "X = np.stack([o.forward_stft(c, frame_len=512, frame_hop=256, center=True, window='hann',"
            " transpose=True) for c in x])\n"
            f"spec = {spec!r}\n"
            "sv = (np.random.default_rng(0).standard_normal((8, X.shape[0], 257)) + 1j).astype(np.complex64)\n"
            "t0 = time.perf_counter()\n"
            f"kind = {kind!r}\n"
            "if kind == 'srp_linear': sm.srp_linear(X, spec['topo'], 181)\n"
            "elif kind == 'srp_circular': sm.srp_circular(X, spec['pairs'], 6, 0.07, 121)\n"
            "elif kind == 'ipd': sm.ipd(X, spec['pairs'], cos=True, sin=True)\n"
            "else: sm.geometry_df(X, sv, [0, 2, 4, 6], spec['pairs'])\n"
            "print(time.perf_counter() - t0)\n")
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1200)
    if r.returncode != 0:
        raise SystemExit("model run failed:\n" + r.stderr[-2000:])
    return float(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--chunk", type=int, default=25, help="utterances per setk_spatial_batch call")
    ap.add_argument("--kinds", type=str, default="srp_linear,srp_circular,ipd,df")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--model", type=int, default=1, help="time the numpy model on one utterance")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "spatial", "bench_spatial.json"))
    a = ap.parse_args()
    import torch
    from setk_amd import _ffi, synth
    from setk_amd.libs import spatial as sp
    from setk_amd.libs.utils import stft_window
    if not torch.cuda.is_available():
        raise SystemExit("bench_spatial needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    C, N, F = a.channels, int(a.seconds * 16000), 257
    ctx = _ffi.Context(0)
    ctx.stft_plan(512, 256, 512, True, stft_window("hann", 512))
    T = ctx.num_frames(N)
    stream = torch.cuda.current_stream().cuda_stream
    host = [synth.synth_scene(i, C, N) for i in range(min(4, a.utts))]
    distinct = [torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(dev) for h in host]
    audio = [distinct[i % len(distinct)] for i in range(a.utts)]
    specs = [torch.empty((C, T, F, 2), dtype=torch.float32, device=dev) for _ in range(a.utts)]

    def stft():
        ctx.stft_batch(C, [t.data_ptr() for t in audio], [N] * a.utts, [s.data_ptr() for s in specs], stream=stream)
        torch.cuda.synchronize()

    stft()
    t_stft = []
    for _ in range(3):
        t0 = time.perf_counter()
        stft()
        t_stft.append(time.perf_counter() - t0)
    topo = tuple(0.04 * i for i in range(C))
    rng = np.random.default_rng(0)
    sv = (rng.standard_normal((8, C, F)) + 1j * rng.standard_normal((8, C, F))).astype(np.complex64)
    half = [(i, i + C // 2) for i in range(C // 2)]
    circ_pairs = [(0, 3), (1, 4), (2, 5)]
    setups = {}
    pairs, table, weight = sp.linear_srp_tables(topo, num_bins=F, num_doa=181)
    setups["srp_linear"] = (pairs, 181, table, weight, dict(topo=topo))
    pairs, table, weight = sp.circular_srp_tables(circ_pairs, 6, 0.07, num_bins=F, num_doas=121)
    setups["srp_circular"] = (pairs, 121, table, weight, dict(pairs=circ_pairs))
    setups["ipd"] = (half, 2 * len(half) * F, None, None, dict(pairs=half))
    setups["df"] = (half, 4 * F, None, None, dict(pairs=half))
    records = [{"workload": f"setk_stft_batch, {a.utts} x {C} ch x {a.seconds:g} s (T = {T})",
                "ms_per_batch": {"median": round(sorted(t_stft)[1] * 1e3, 2), "repeats": 3}}]
    for kind in a.kinds.split(","):
        pairs, width, table, weight, spec = setups[kind]
        d_const = None
        if kind.startswith("srp"):
            d_const = torch.from_numpy(table.view(np.float32)).to(dev)
        elif kind == "df":
            d_const = torch.from_numpy(sv.view(np.float32)).to(dev)
        outs = [torch.empty((T, width), dtype=torch.float32, device=dev) for _ in range(a.chunk)]
        chunks = [list(range(i, min(i + a.chunk, a.utts))) for i in range(0, a.utts, a.chunk)]

        def opts_for(n):
            if kind.startswith("srp"):
                return _ffi.spatial_opts("srp", pairs, table=d_const.data_ptr(), num_doas=width, pair_weight=weight)
            if kind == "df":
                return _ffi.spatial_opts("df", pairs, steer_vector=d_const.data_ptr(), num_sv=8,
                                         doa_index=[[0, 2, 4, 6]] * n)
            return _ffi.spatial_opts("cos_sin_ipd", pairs)

        def step():
            for chunk in chunks:
                ctx.spatial_batch(opts_for(len(chunk)), C, [specs[i].data_ptr() for i in chunk], [T] * len(chunk), F,
                                  [outs[k].data_ptr() for k in range(len(chunk))], stream=stream)
            torch.cuda.synchronize()

        for _ in range(a.warmup):
            step()
        ctx.set_profiling(True)
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            step()
            times.append(time.perf_counter() - t0)
        stage = [v * len(chunks) for v in ctx.last_stage_ms()]  # (the mean per call x calls per batch)
        ctx.set_profiling(False)
        times.sort()
        med = times[len(times) // 2]
        rec = {
            "workload": f"spatial {kind}, {a.utts} x {C} ch x {a.seconds:g} s (T = {T}), {len(pairs)} pairs, "
                        f"width {width}, spectrograms resident, {len(chunks)} calls of {a.chunk} utterances",
            "ms_per_batch": {"median": round(med * 1e3, 2), "min": round(times[0] * 1e3, 2),
                             "max": round(times[-1] * 1e3, 2), "repeats": a.repeats, "warmup": a.warmup},
            "x_real_time": round(a.utts * a.seconds / med, 1),
            "finite": bool(torch.isfinite(outs[0]).all().item()),
        }
        if kind.startswith("srp"):
            rec["stage_ms"] = {"obs_tiles": round(stage[0], 3), "pair_contraction": round(stage[1], 3),
                               "combine": round(stage[2], 3)}
            flops = 4.0 * len(pairs) * T * F * width * a.utts
            rec["fp32_flop_per_batch"] = flops
            rec["fp32_floor_ms"] = round(flops / FP32_PEAK * 1e3, 3)
            rec["contraction_over_floor"] = round(stage[1] / (flops / FP32_PEAK * 1e3), 2)
            rec["contraction_fp32_tflops"] = round(flops / (stage[1] * 1e-3) / 1e12, 2)
        else:
            rec["stage_ms"] = {"kernel": round(stage[0], 3)}
            moved = a.utts * (8.0 * C * T * F + 4.0 * T * width)  # one read of the spectrogram, one write
            rec["hbm_gb_per_s"] = round(moved / (stage[0] * 1e-3) / 1e9, 1)
        if a.model:
            dt = model_seconds(kind, C, N, spec)
            rec["model_one_utterance_s"] = round(dt, 2)
            rec["model_threads"] = 1
            rec["model_x_real_time"] = round(a.seconds / dt, 2)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del outs, d_const
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump(records, fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
