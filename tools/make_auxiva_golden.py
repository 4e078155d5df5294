#!/usr/bin/env python
"""
Generate the AuxIVA fixtures under tests/golden/ by running the UNMODIFIED reference
(funcwj/setk scripts/sptk/apply_auxiva.py through oracle/ref_harness.py).  Build container
only: the reference tree does not exist where the GPU tests run.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***

    python tools/make_auxiva_golden.py            # from the repo root

  ref_auxiva.npz         the doc recording (the `egs` array of doc_adaptive_beamformer.npz,
                         5 channels) through the reference's command line with its defaults
                         (512 / 256 / hann, centred, 20 epochs): the five waves it wrote, int16.
  ref_auxiva_scenes.npz  three synthetic scenes (2, 4 and 8 channels; tests/auxiva_model.py
                         synth_scene, seeds below): the input as 16-bit PCM (x = pcm / 32768,
                         exact in float32) and the reference's auxiva() on the reference's own
                         STFT of it, as complex64.  The scenes are short because Y does not
                         compress and every committed file stays below 1 MiB.
Only samples and recorded outputs are stored.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import scipy.io.wavfile as wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness as rh  # noqa: E402
import auxiva_model  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STFT = dict(frame_len=512, frame_hop=256, window="hann", center=True, round_power_of_two=True)
# name, seed, channels, frames (samples = hop * (frames - 1))
SCENES = [("c2", 20, 2, 30), ("c4", 21, 4, 24), ("c8", 22, 8, 28)]
EPOCHS = 20


def main():
    if not rh.available():
        raise SystemExit("the reference tree is not present")
    cli = rh.load_cli("apply_auxiva")
    libs = rh.load()
    egs = np.load(os.path.join(GOLD, "doc_adaptive_beamformer.npz"))["egs"]  # N x 5 int16
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "egs.wav")
        wavfile.write(wav, 16000, egs)
        scp = os.path.join(tmp, "wav.scp")
        with open(scp, "w") as fd:
            fd.write(f"egs {wav}\n")
        dst = os.path.join(tmp, "out")
        os.makedirs(dst)
        args = argparse.Namespace(wav_scp=scp, dst_dir=dst, epochs=EPOCHS, sr=16000, **STFT)
        cli.run(args)
        waves = []
        for n in range(egs.shape[1]):
            sr, w = wavfile.read(os.path.join(dst, f"egs.src{n + 1}.wav"))
            assert sr == 16000 and w.dtype == np.int16 and w.ndim == 1
            waves.append(w)
    np.savez_compressed(os.path.join(GOLD, "ref_auxiva.npz"), egs_waves=np.stack(waves),
                        epochs=np.int32(EPOCHS))

    out = {"epochs": np.int32(EPOCHS), "names": np.array([s[0] for s in SCENES]),
           "seeds": np.array([s[1] for s in SCENES], dtype=np.int32)}
    for name, seed, C, T in SCENES:
        samps = auxiva_model.synth_scene(seed, C, 256 * (T - 1))
        pcm = np.rint(samps.astype(np.float64) * 32767.0).astype(np.int16)
        x = pcm.astype(np.float32) / np.float32(32768.0)
        # SpectrogramReader._load with transpose=True (libs/data_handler.py): N x T x F
        X = np.stack([libs.utils.forward_stft(c, **STFT, transpose=True) for c in x])
        assert X.shape == (C, T, 257) and X.dtype == np.complex64, (X.shape, X.dtype)
        Y = cli.auxiva(X, EPOCHS)
        Ym = auxiva_model.auxiva(X, EPOCHS)
        dev = np.sqrt(np.mean(np.abs(Ym - Y)**2, axis=(1, 2)) / np.mean(np.abs(Y)**2, axis=(1, 2)))
        print(f"{name}: model against reference, per source: {dev}")
        out[name + "_pcm"] = pcm
        out[name + "_Y"] = Y.astype(np.complex64)
    np.savez_compressed(os.path.join(GOLD, "ref_auxiva_scenes.npz"), **out)
    for f in ("ref_auxiva.npz", "ref_auxiva_scenes.npz"):
        print(f, os.path.getsize(os.path.join(GOLD, f)), "bytes")


if __name__ == "__main__":
    main()
