#!/usr/bin/env python
"""
Generate tests/golden/ref_ns.npz by running the UNMODIFIED reference (funcwj/setk
scripts/sptk/libs/ns.py and apply_ns.py through oracle/ref_harness.py).
Build container only: the reference tree does not exist where the GPU tests run.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***

    python tools/make_ns_golden.py            # from the repo root   (about a minute: the
                                              # reference integrates E1 numerically per cell)

  <case>_stft    the input of a case of tests/ns_model.py CASES, complex64 T x F (the reference
                 gets it as complex128, so that it computes in float64 as its own STFT would)
  <case>_gain    MCRA(**conf).run / iMCRA(**conf).run of the reference, float64 T x F
  <case>_seed, <case>_margin, <case>_model_err
                 the seed used, the decision margin of the run (ns_model) and the worst relative
                 gain error of the model against the reference
  cli_pcm        one 1.2 s utterance, 16-bit PCM
  cli_wav        apply_ns.py --output wave on it (512 / 256 / hann, iMCRA defaults): the PCM_16 file
  cli_gain       apply_ns.py --output gain on it: the .npy file
Only inputs and recorded results are stored.  A case whose decision margin is below 1e-9 gets
another seed HERE (the tool tries the next ones): no fixture sits on a threshold.
"""
import argparse
import os
import sys
import tempfile
import warnings

import numpy as np
import scipy.io.wavfile as wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness as rh  # noqa: E402
import ns_model  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STFT = dict(frame_len=512, frame_hop=256, window="hann", center=True, round_power_of_two=True)
CLI_SAMPLES, CLI_SEED = 19200, 5


def main():
    if not rh.available():
        raise SystemExit("the reference tree is not present")
    import importlib
    rh.load()
    ref_ns = importlib.import_module("libs.ns")
    cli = rh.load_cli("apply_ns")
    out = {}
    worst = 0.0
    for name, (kind, T, F, seed0, conf) in ns_model.CASES.items():
        cls = ref_ns.MCRA if kind == "mcra" else ref_ns.iMCRA
        for seed in range(seed0, seed0 + 1000, 100):
            stft = ns_model.synth_spectrogram(T, F, seed)
            info = {}
            model, margin = ns_model.run(kind, stft, **conf) if kind == "mcra" else \
                ns_model.imcra(stft, info=info, **conf)
            if margin >= ns_model.MIN_MARGIN and not info.get("clamped", 0):
                break
            print(f"  {name}: seed {seed} has margin {margin:.2e}, clamped {info.get('clamped', 0)}: next seed")
        else:
            raise SystemExit(f"{name}: no seed with a margin of {ns_model.MIN_MARGIN}")
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # (the reference's quadrature warns where it diverges)
            gain = cls(**conf).run(stft.astype(np.complex128))
        assert gain.shape == (T, F) and gain.dtype == np.float64 and np.isfinite(gain).all()
        err = float(np.max(np.abs(model - gain) / np.abs(gain)))
        worst = max(worst, err)
        print(f"{name}: T {T} F {F} seed {seed}  model vs reference {err:.2e}  margin {margin:.2e}")
        out[name + "_stft"], out[name + "_gain"] = stft, gain
        out[name + "_seed"], out[name + "_margin"], out[name + "_model_err"] = np.int64(seed), margin, err
    out["model_err_worst"] = np.float64(worst)
    print(f"worst model-versus-reference figure {worst:.2e} -> device bound max(1e-8, 30 x) = "
          f"{max(1e-8, 30 * worst):.2e}")

    # ---- the command line on one utterance ----
    pcm = np.rint(ns_model.synth_samples(CLI_SAMPLES, CLI_SEED) * 32767.0).astype(np.int16)
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "u0.wav")
        wavfile.write(wav, 16000, pcm)
        scp = os.path.join(tmp, "wav.scp")
        with open(scp, "w") as fd:
            fd.write(f"u0 {wav}\n")
        for output in ("wave", "gain"):
            dst = os.path.join(tmp, output)
            cli.run(argparse.Namespace(wav_scp=scp, dst_dir=dst, conf="", output=output, sr=16000, **STFT))
        sr, ref_wav = wavfile.read(os.path.join(tmp, "wave", "u0.wav"))
        ref_gain = np.load(os.path.join(tmp, "gain", "u0.npy"))
    assert sr == 16000 and ref_wav.dtype == np.int16
    x = pcm.astype(np.float32) / np.float32(32768.0)
    libs = rh.load()
    X = libs.utils.forward_stft(x, **STFT, transpose=True)
    info = {}
    model, margin = ns_model.imcra(X, info=info)
    err = float(np.max(np.abs(model - ref_gain) / np.abs(ref_gain)))
    print(f"cli: stft {X.dtype} {X.shape}, gain {ref_gain.dtype}, wav {ref_wav.shape}; model (float64) vs the "
          f"command line's gain {err:.2e}, margin {margin:.2e}, clamped {info['clamped']}")
    out["cli_pcm"], out["cli_wav"], out["cli_gain"] = pcm, ref_wav, ref_gain
    out["cli_margin"], out["cli_model_err"] = margin, err
    path = os.path.join(GOLD, "ref_ns.npz")
    np.savez_compressed(path, **out)
    print("ref_ns.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
