#!/usr/bin/env python
"""Block-online MVDR beamforming (setk_enhance_online_batch) on 125 utterances x 8 channels x 30 s,
16 kHz, at chunk sizes 32, 64 and 128 frames: samples and masks resident in HBM, float32 waves out.
One GPU.  Per chunk size: wall time per batch (warm-up, then timed repeats: median / min / max; a
host clock around a call that ends in a stream synchronise) and HIP-event time per stage (STFT +
chunk covariances; smoothing + weights + BAN; beamform + iSTFT; renorm).  Beside them, in the same
run: the offline step (setk_enhance_batch) of the same batch, and the per-utterance host loop the
CLI used before (libs.beamformer.OnlineMvdrBeamformer under do_online_beamform, with its STFT and
inverse STFT) on ONE utterance of the batch at chunk size 32.

DERIVED, not measured: the weight solve sees utterances x chunks x 257 problems (125 x 59 x 257 =
1.9 M at chunk 32 against 32 k offline), and the chunk scratch is (slabs + planes + weights) x
1056 bytes x chunks.  Both are printed beside the measurements.

Writes profiles/online/bench_online.json (--out).  No pass / fail time.

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(step, warmup, repeats, ctx):
    for _ in range(warmup):
        step()
    ctx.set_profiling(True)
    times, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
        stages.append(ctx.last_stage_ms())
    ctx.set_profiling(False)
    times.sort()
    stage = [sorted(s[i] for s in stages)[len(stages) // 2] for i in range(4)]
    return {"median": round(times[len(times) // 2] * 1e3, 3), "min": round(times[0] * 1e3, 3),
            "max": round(times[-1] * 1e3, 3), "repeats": repeats, "warmup": warmup}, [round(v, 3) for v in stage]


def host_loop_seconds(mix, mask, chunk, alpha):
    """The per-utterance loop of run_online on one utterance: host STFT, the chunk loop of
    operator calls, host inverse STFT."""
    from setk_amd.libs import utils
    from setk_amd.libs.beamformer import OnlineMvdrBeamformer
    from setk_amd.sptk.apply_adaptive_beamformer import do_online_beamform
    kw = dict(frame_len=512, frame_hop=256, window="hann", center=True, transpose=False)
    args = argparse.Namespace(chunk_size=chunk, alpha=alpha, ban=False)
    bf = OnlineMvdrBeamformer(257, mix.shape[0], alpha)

    def once():
        obs = np.stack([utils.forward_stft(x, round_power_of_two=True, **kw) for x in mix])
        enh = do_online_beamform(bf, mask, None, obs, args)
        return utils.inverse_stft(enh, norm=float(np.max(np.abs(mix))), **kw)

    once()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        once()
        times.append(time.perf_counter() - t0)
    return sorted(times)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=125)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--chunks", type=str, default="32,64,128")
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-loop", type=int, default=1, help="time the per-utterance host loop on one utterance")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "online", "bench_online.json"))
    a = ap.parse_args()
    import torch
    from setk_amd import _ffi, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_online needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    U, C, N = a.utts, a.channels, int(a.seconds * 16000)
    ctx = _ffi.Context(0)
    ctx.stft_plan(512, 256, 512, True)
    stream = torch.cuda.current_stream().cuda_stream
    T = ctx.num_frames(N)
    L = ctx.istft_num_samples(T)
    # a few distinct utterances, every one of the batch its own copy in HBM
    base = [synth.synth_utterance(500 + k, C, N).astype(np.float32) for k in range(5)]
    audio = [torch.from_numpy(base[u % len(base)]).to(dev).clone() for u in range(U)]
    gen = torch.Generator(device=dev).manual_seed(5)
    masks = [(0.1 + 0.8 * torch.rand((T, 257), generator=gen, device=dev, dtype=torch.float32)).contiguous()
             for _ in range(U)]
    waves = [torch.empty(L, dtype=torch.float32, device=dev) for _ in range(U)]
    aptr, mptr, wptr, ns = [t.data_ptr() for t in audio], [t.data_ptr() for t in masks], \
        [t.data_ptr() for t in waves], [N] * U
    opts = _ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK, pmwf_ref=-1)
    status = np.zeros(U, dtype=np.int32)

    def offline():
        ctx.enhance_batch(opts, C, aptr, ns, mptr, None, wptr, want_status=True, stream=stream)
        torch.cuda.synchronize()

    wall, stage = timed(offline, a.warmup, a.repeats, ctx)
    rec = {"workload": f"{U} utterances x {C} ch x {a.seconds:g} s, 16 kHz (T = {T} frames), MVDR, alpha {a.alpha:g}, "
                       "samples and masks resident, float32 out",
           "offline": {"ms_per_batch": wall,
                       "stage_ms": dict(zip(("stft_covariances", "reduction_weights", "beamform_istft", "renorm"), stage)),
                       "problems": U * 257},
           "online": {}}
    NP = C * (C + 1) // 2
    for chunk in [int(v) for v in a.chunks.split(",")]:
        def online():
            ctx.enhance_online_batch(opts, chunk, a.alpha, C, aptr, ns, mptr, None, wptr, status=status, stream=stream)
            torch.cuda.synchronize()

        wall, stage = timed(online, a.warmup, a.repeats, ctx)
        K = ctx.online_num_chunks(N, chunk)
        slabs = -(-chunk // 64)
        rec["online"][str(chunk)] = {
            "ms_per_batch": wall,
            "stage_ms": dict(zip(("stft_chunk_covariances", "smoothing_weights", "beamform_istft", "renorm"), stage)),
            "x_real_time": round(U * a.seconds / (wall["median"] * 1e-3), 1),
            "chunks_per_utterance": K, "problems_derived": U * K * 257,
            "scratch_mb_derived": round(U * K * 1056 * (slabs * (4 * NP + 2) + 4 * NP + 2 * C) / 1e6, 1),
            "status_ok": bool((status == 0).all()),
            "over_offline": round(wall["median"] / rec["offline"]["ms_per_batch"]["median"], 2)}
    if a.host_loop:
        dt = host_loop_seconds(base[0], masks[0].cpu().numpy(), 32, a.alpha)
        rec["host_loop_one_utterance_chunk32_s"] = round(dt, 3)
        rec["host_loop_batch_s_derived"] = round(dt * U, 1)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump([rec], fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
