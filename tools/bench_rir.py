#!/usr/bin/env python
"""Image-method RIR generation (setk_rir_generate_batch) at the reference's example shape: 8 rooms x
40 RIRs x 6 microphones x 8000 taps (rir_generate_1d.py:369-384, --rir-dur 0.5), outputs resident in
HBM.  One GPU.  One record:
  MEASURED   wall time per batch (warm-up, then timed repeats: median / min / max; a host clock
             around a call that ends in a stream synchronise) and HIP-event time per stage from the
             profile marks (tables, images, fold + high-pass, copies)
  DERIVED    the tap contributions of the batch (counted in numpy on the first RIR of every room and
             scaled by the RIRs per room) x the vector instructions per 64 taps of the kernel's tap
             loop (tools/isa_census.py on rir.hip) at the VALU issue rate of DESIGN.md section 5
             (2.24 cycles per instruction and SIMD, 1024 SIMDs, 1.89 GHz).  That rate was measured on
             float32 code; the tap loop is float64, which issues slower, so the floor is optimistic.
  RECORDED   the reference's CPU seconds per channel on the `workload` case of
             tests/golden/ref_rir.npz (8000 taps, 7 x 8 x 3 m; one core of the machine that wrote the
             fixture), times the channels of the batch.
Writes profiles/rir/bench_rir.json (--out).  No pass / fail time.

(Side measurement for DESIGN.md; bench.py is the contract benchmark.)"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CYCLES_PER_INSTR, SIMDS, HZ = 2.24, 1024, 1.89e9


def sample_rooms(rooms, rirs, mics, rng):
    """Rooms of 4-6 x 8-10 x 2.4-3 m at T60 0.2-0.7 s with a linear array of 5 cm pitch and `rirs`
    speakers each, the ranges of the reference's example."""
    from setk_amd.libs.rir import three_decimals
    out = []
    for _ in range(rooms):
        size = [rng.uniform(4, 6), rng.uniform(8, 10), rng.uniform(2.4, 3)]
        V, S = size[0] * size[1] * size[2], 2 * (size[0] * size[1] + size[0] * size[2] + size[1] * size[2])
        rt60 = rng.uniform(max(0.2, 24 * V * np.log(10) / (340 * S) * 1.05), 0.7)
        cx, cy, cz = size[0] * rng.uniform(0.4, 0.6), size[1] * rng.uniform(0.05, 0.1), rng.uniform(1.2, 1.8)
        array = [three_decimals((cx + 0.05 * (m - (mics - 1) / 2), cy, cz)) for m in range(mics)]
        for _ in range(rirs):
            d, doa = rng.uniform(1, 4), rng.uniform(0.1, np.pi - 0.1)
            src = (min(max(cx + np.cos(doa) * d, 0.2), size[0] - 0.2), min(cy + np.sin(doa) * d, size[1] - 0.2),
                   rng.uniform(1, 2))
            out.append(dict(room=three_decimals(size), src=three_decimals(src), mics=array, beta_or_rt60=round(rt60, 3)))
    return out


def count_taps(setting, ns, fs=16000.0, c=340.0):
    """(images that pass, their taps inside [0, ns)) of one setting, summed over its microphones."""
    cts = c / fs
    T, S = np.float64(setting["room"]) / cts, np.float64(setting["src"]) / cts
    Tw = 2 * int(0.004 * fs + 0.5)
    images = taps = 0
    for mic in np.float64(setting["mics"]) / cts:
        comp = []
        for a in range(3):
            n = int(np.ceil(ns / (2 * T[a])))
            cell = np.repeat(np.arange(-n, n + 1), 2)
            mirror = np.tile(np.arange(2), 2 * n + 1)
            comp.append((1 - 2 * mirror) * S[a] - mic[a] + 2 * cell * T[a])
        fd = np.floor(np.sqrt(comp[0][:, None, None]**2 + comp[1][None, :, None]**2 + comp[2][None, None, :]**2))
        pos = fd[fd < ns] - Tw // 2 + 1
        images += pos.size
        taps += int(np.sum(np.minimum(pos + Tw, ns) - np.maximum(pos, 0)))
    return images, taps


def tap_loop_instructions():
    """Vector instructions of the tap loop per trip (64 taps): the census block with the reciprocal
    and the two LDS operations (the table read and the 64-bit add)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_census.py"), "rir.hip", "rir_images"],
                       capture_output=True, text=True, timeout=600)
    best = None
    lines = r.stdout.splitlines()
    for head, body in zip(lines, lines[1:]):
        f = head.split()
        if len(f) >= 7 and f[1] == "VALU" and f[5] == "LDS" and f[6] == "2" and "v_rcp:1" in body and "v_cvt_f64:1" in body:
            best = max(best or 0, int(f[2]))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=8)
    ap.add_argument("--rirs", type=int, default=40)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--taps", type=int, default=8000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "rir", "bench_rir.json"))
    a = ap.parse_args()
    import torch
    import rir_model as rm
    from setk_amd import _ffi
    from setk_amd.libs.rir import make_spec
    if not torch.cuda.is_available():
        raise SystemExit("bench_rir needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    ctx = _ffi.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    settings = sample_rooms(a.rooms, a.rirs, a.mics, random.Random(0))
    specs = [make_spec(rir_nsamps=a.taps, **s) for s in settings]
    outs = [torch.empty((a.mics, a.taps), dtype=torch.float32, device=dev) for _ in specs]
    status = torch.zeros(len(specs), dtype=torch.int32, device=dev)
    ptrs = [o.data_ptr() for o in outs]

    def step(flags=0):
        ctx.rir_generate_batch(specs, ptrs, status=status.data_ptr(), flags=flags, stream=stream)

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
    names = ("tables", "images", "fold_highpass", "copies")
    stage = dict(zip(names, [sorted(s[i] for s in stages)[len(stages) // 2] for i in range(4)]))
    first = outs[0].cpu().numpy()
    # one RIR alone (split over workgroups) for the latency of a single call
    one = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.rir_generate_batch(specs[:1], ptrs[:1], status=status.data_ptr(), stream=stream)
        one.append(time.perf_counter() - t0)
    same = bool(np.array_equal(first, outs[0].cpu().numpy()))

    counted = [count_taps(settings[r * a.rirs], a.taps) for r in range(a.rooms)]
    images, taps = (sum(c[i] for c in counted) * a.rirs for i in range(2))
    per_trip = tap_loop_instructions()
    channels = len(specs) * a.mics
    ref_sec = rm.load_fixture()["workload"][3]
    rec = {
        "workload": f"setk_rir_generate_batch, {a.rooms} rooms x {a.rirs} RIRs x {a.mics} microphones x {a.taps} taps "
                    f"({channels} channels), 16 kHz, rooms 4-6 x 8-10 x 2.4-3 m, T60 0.2-0.7 s, outputs resident",
        "measured": {
            "ms_per_batch": {"median": round(med * 1e3, 3), "min": round(times[0] * 1e3, 3),
                             "max": round(times[-1] * 1e3, 3), "repeats": a.repeats, "warmup": a.warmup},
            "stage_ms": {k: round(v, 4) for k, v in stage.items()},
            "ms_per_channel": round(med * 1e3 / channels, 4),
            "one_rir_alone_ms": round(min(one) * 1e3, 3),
            "one_rir_alone_has_the_batch_bits": same,
            "status_ok": bool((status.cpu().numpy() == 0).all()),
        },
        "derived": {
            "images_that_pass": images, "tap_contributions": taps,
            "counted_on": f"the first RIR of each of the {a.rooms} rooms, x {a.rirs}",
            "valu_instructions_per_64_taps": per_trip,
            "floor_ms": None if not per_trip else round(taps / 64 * per_trip * CYCLES_PER_INSTR / SIMDS / HZ * 1e3, 3),
            "floor_assumes": f"{CYCLES_PER_INSTR} cycles per vector instruction and SIMD (DESIGN.md section 5, measured "
                             f"on float32 code), {SIMDS} SIMDs, {HZ / 1e9:g} GHz; float64 instructions issue slower, "
                             "and the per-image set-up is not counted: optimistic",
        },
        "recorded_reference": {
            "cpu_seconds_per_channel": round(ref_sec, 4),
            "cpu_core_seconds_for_the_batch": round(ref_sec * channels, 1),
            "source": "tests/golden/ref_rir.npz, case `workload` (8000 taps, 7 x 8 x 3 m): the reference's "
                      "GenerateRir on one core of the machine that wrote the fixture, not this one",
        },
    }
    if rec["derived"]["floor_ms"]:
        rec["images_stage_over_floor"] = round(stage["images"] / rec["derived"]["floor_ms"], 2)
    rec["batch_against_the_recorded_reference"] = round(ref_sec * channels / med, 1)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fd:
        json.dump([rec], fd, indent=1)
        fd.write("\n")


if __name__ == "__main__":
    main()
