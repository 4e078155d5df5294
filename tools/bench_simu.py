#!/usr/bin/env python
"""Data simulation (setk_simu_batch) on 125 mixtures of 30 s, 16 kHz: two speakers and one point
noise, each reverberated with its own 8-channel RIR of 8000 taps (32 partitions), mixed at an SDR
/ SNR and peak-normalised; sources and RIRs resident in HBM, float32 mixtures and references out.
One GPU.  One record: wall time per batch (warm-up, then timed repeats: median / min / max; a host
clock around a call that ends in a stream synchronise), HIP-event time per stage (transforms,
convolutions, powers + coefficients + peak, scaling), and DERIVED floors beside the convolution
and the mixing:

  convolution, per source: K = 1875 frames x N = 8 channels x P = 32 partitions x 256 complex
  multiply-adds x 8 flop = 0.98 GFLOP, plus 1875 forward and 15000 inverse 512-point transforms at
  about 5 n log2 n = 23 kflop = 0.39 GFLOP; compulsory traffic 1.9 MB of samples in, 15.4 MB of
  images out, 3.8 MB of spectra out and in = about 25 MB.  At the card's 157 Tflop/s of float32
  vector arithmetic (256 CUs x 128 lanes x 2 x 2.4 GHz) and 8 TB/s the arithmetic bounds it.
  mixing, per mixture: the three images read once (46 MB), the mixture and three references
  written (15.4 + 5.8 MB) at 8 TB/s.  The kernels read the images twice (peak, output) and channel
  0 twice more (powers).

Both are assumptions about the card's peak rates, not measurements.  Beside them, on one core of
the host, the float64 numpy model of tests/simu_model.py (FFT convolution) on ONE mixture of the
same shape.  Writes profiles/simu/bench_simu.json (--out).  No pass / fail time.

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

PEAK_FLOPS, PEAK_BYTES = 256 * 128 * 2 * 2.4e9, 8e12


def model_seconds(N, S, R):
    """tests/simu_model.py on one mixture, one thread (set before numpy loads)."""
    code = ("import sys, time, numpy as np\n"
            f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import simu_model as sm\n"
            "rng = np.random.default_rng(0)\n"
            f"N, S, R = {N}, {S}, {R}\n"
            "case = dict(spk=[sm._speech(rng, S), sm._speech(rng, S)], spk_begin=[0, 0], sdr=[3.0],\n"
            "            spk_rir=[sm._rir(rng, N, R), sm._rir(rng, N, R)], noise=[sm._speech(rng, S)], noise_begin=[0],\n"
            "            noise_snr=[5.0], noise_rir=[sm._rir(rng, N, R)], repeat=False, dump_channel=-1, norm_factor=0.9)\n"
            "t0 = time.perf_counter()\n"
            "sm.run_simu(case, conv=sm.fftconvolve64)\n"
            "print(time.perf_counter() - t0)\n")
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1200)
    if r.returncode != 0:
        raise SystemExit("model run failed:\n" + r.stderr[-2000:])
    return float(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixtures", type=int, default=125)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--taps", type=int, default=8000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", type=int, default=1, help="time the numpy model on one mixture")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "simu", "bench_simu.json"))
    a = ap.parse_args()
    import torch
    import simu_model as sm
    from setk_amd import _ffi
    if not torch.cuda.is_available():
        raise SystemExit("bench_simu needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    S, N, R, M = int(a.seconds * 16000), a.channels, a.taps, a.mixtures
    ctx = _ffi.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    srcs = [torch.from_numpy(sm.pcm_to_float(sm._speech(rng, S))).to(dev) for _ in range(6)]
    rirs = [torch.from_numpy(sm.pcm_to_float(sm._rir(rng, N, R))).to(dev) for _ in range(3 * M)]  # every source its own
    mix = [torch.empty((N, S), dtype=torch.float32, device=dev) for _ in range(M)]
    refs = [[torch.empty(S, dtype=torch.float32, device=dev) for _ in range(3)] for _ in range(M)]
    recipes = []
    for u in range(M):
        def src(k, **kw):
            return _ffi.simu_source(srcs[(3 * u + k) % len(srcs)].data_ptr(), S, rir=rirs[3 * u + k].data_ptr(),
                                    rir_channels=N, rir_taps=R, **kw)
        r = _ffi.simu_recipe([src(0), src(1, snr=3.0)], [src(2, snr=5.0)])
        _ffi.simu_recipe_outputs(r, mix[u].data_ptr(), [refs[u][0].data_ptr(), refs[u][1].data_ptr()],
                                 refs[u][2].data_ptr())
        recipes.append(r)
    status = np.zeros(M, dtype=np.int32)

    def step():
        ctx.simu_batch(recipes, status=status, stream=stream)
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
    K, P, n_src = -(-S // 256), -(-R // 256), 3 * M
    mac_flop = K * N * P * 256 * 8
    fft_flop = (K + K * N) * 5 * 512 * 9
    conv_bytes = 4 * S + 4 * N * S + 2 * K * 2048
    conv_floor = n_src * max((mac_flop + fft_flop) / PEAK_FLOPS, conv_bytes / PEAK_BYTES) * 1e3
    mix_bytes = M * (3 * 4 * N * S + 4 * N * S + 3 * 4 * S)
    mix_floor = mix_bytes / PEAK_BYTES * 1e3
    peak = float(mix[0].abs().max().item())
    rec = {
        "workload": f"setk_simu_batch, {M} mixtures x (2 speakers + 1 point noise) x {N} ch x {a.seconds:g} s, "
                    f"{R}-tap RIRs (K = {K} frames, P = {P} partitions), sources and RIRs resident, float32 out",
        "ms_per_batch": {"median": round(med * 1e3, 2), "min": round(times[0] * 1e3, 2),
                         "max": round(times[-1] * 1e3, 2), "repeats": a.repeats, "warmup": a.warmup},
        "x_real_time": round(M * a.seconds / med, 1),
        "stage_ms": {"transforms": round(stage[0], 3), "convolutions": round(stage[1], 3),
                     "powers_coefficients_peak": round(stage[2], 3), "scaling": round(stage[3], 3)},
        "per_source": {"gflop": round((mac_flop + fft_flop) / 1e9, 3), "compulsory_mb": round(conv_bytes / 1e6, 1),
                       "convolution_us": round((stage[0] + stage[1]) * 1e3 / n_src, 2)},
        "convolution_tflops": round(n_src * (mac_flop + fft_flop) / ((stage[0] + stage[1]) * 1e-3) / 1e12, 2),
        "derived_floor_ms": {"convolution": round(conv_floor, 3), "mixing": round(mix_floor, 3)},
        "derived_floor_assumes": "157 Tflop/s float32 vector arithmetic, 8 TB/s HBM; see the tool's header",
        "convolution_over_floor": round((stage[0] + stage[1]) / conv_floor, 2),
        "mixing_over_floor": round((stage[2] + stage[3]) / mix_floor, 2),
        "reference_s_per_mixture": 0.1,
        "status_ok": bool((status == 0).all()),
        "peak_of_first_mixture": round(peak, 7),
    }
    if a.model:
        dt = model_seconds(N, S, R)
        rec["model_one_mixture_s"] = round(dt, 2)
        rec["model_threads"] = 1
        rec["model_batch_s"] = round(dt * M, 1)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump([rec], fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
