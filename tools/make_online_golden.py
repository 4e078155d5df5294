#!/usr/bin/env python
"""
Generate tests/golden/ref_online.npz by running the UNMODIFIED reference classes
(funcwj/setk scripts/sptk/libs/beamformer.py OnlineMvdrBeamformer / OnlineGevdBeamformer, through
oracle/ref_harness.py) chunk by chunk, the way do_online_beamform
(apply_adaptive_beamformer.py:25-47) drives them.  Build container only: the reference tree does
not exist where the GPU tests run.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***

    python tools/make_online_golden.py            # from the repo root

One 4-channel utterance (tests/online_model.py case_inputs(4, 16384): 65 frames), chunk size 32
(three chunks, the last a single frame), alpha 0.8, with and without BAN.  Per class:
  <kind>.weight      [chunks][F][N] complex128: weight(self.Rs, self.Rn) after each run()
  <kind>.enh         F x T complex64: the chunks' run() outputs side by side
  <kind>_ban.enh     the same with ban=True
The inputs are not stored: the test rebuilds them from the seeded generator.  The reference's
`reset` member is never cleared (:296-317), so these records follow phi_c = 1; the tool prints how
far the model (tests/online_model.py, reference_phi=True, gauge off, promote=False) is from each.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import np_oracle as o  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
import online_model as om  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CHANNELS, SAMPLES, CHUNK, ALPHA = 4, 16384, 32, 0.8


def main():
    libs = rh.load()
    mix, mask = om.case_inputs(CHANNELS, SAMPLES)
    obs = o.multichannel_stft(mix, round_power_of_two=True, transpose=False, **om.STFT_KW)
    mask = np.minimum(mask, 1)
    N, F, T = obs.shape
    out = {}
    for kind, cls in (("mvdr", libs.beamformer.OnlineMvdrBeamformer), ("gevd", libs.beamformer.OnlineGevdBeamformer)):
        for ban in (False, True):
            bf = cls(F, N, ALPHA)
            bf.reset_stats(ALPHA)
            enh, weights = [], []
            for t0 in range(0, T, CHUNK):
                sl = slice(t0, t0 + CHUNK)
                enh.append(bf.run(mask[sl], np.ascontiguousarray(obs[:, :, sl]), mask_n=None, ban=ban))
                weights.append(bf.weight(bf.Rs, bf.Rn))
            name = kind + ("_ban" if ban else "")
            out[f"{name}.enh"] = np.hstack(enh).astype(np.complex64)
            if not ban:
                out[f"{kind}.weight"] = np.stack(weights).astype(np.complex128)
            # (the reference sums a chunk's covariances in the spectrogram's complex64: promote=False)
            model = om.online_parts(obs, mask, CHUNK, ALPHA, kind=kind, ban=ban, gauge=False, reference_phi=True,
                                    promote=False)
            err = np.sqrt(np.mean(np.abs(model["enh"] - np.hstack(enh))**2) / np.mean(np.abs(np.hstack(enh))**2))
            print(f"{name}: model against the reference, rel rms {err:.3e}")
    path = os.path.join(GOLD, "ref_online.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
