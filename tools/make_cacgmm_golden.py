#!/usr/bin/env python
"""
Generate the CACGMM fixtures under tests/golden/ by running the UNMODIFIED reference
(funcwj/setk scripts/sptk/libs/cluster.py CacgmmTrainer and estimate_cacgmm_masks.py through
oracle/ref_harness.py).  Build container only: the reference tree does not exist where the GPU
tests run.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***

    python tools/make_cacgmm_golden.py            # from the repo root

  ref_cacgmm.npz       the synthetic cases of tests/cacgmm_model.py (CASES; five bins each): the
                       spectrogram (complex64), the start gamma0 and the reference's posteriors
                       after 0, 1, 2, 5 and the last iteration -- <case>_ref128_<n>: on the
                       spectrogram promoted to complex128 (the arithmetic of the model),
                       <case>_ref64_last: on the complex64 spectrogram as a user passes it (the
                       reference then normalises in complex64).
  ref_cacgmm_2spk.npz, ref_cacgmm_noisy.npz
                       the two doc recipes (files of their own: every committed file stays
                       below 1 MiB).
The doc recipes of doc/spatial_clustering/README.md on the two recordings of
doc_spatial_clustering.npz, through the reference's command line:
  2spk   --num-classes 3 --num-iters 20 (seed 777, aligner on)
  noisy  --num-classes 2 --cgmm-init true --update-alpha false --solve-permu false --num-iters 20
For each: <name>_post, the posteriors before alignment K x T x F float32 (CacgmmTrainer on the
reader's spectrogram with the same seed), and <name>_order uint8 K x F, the class of the
posteriors that the file written by the command line holds in slot k of bin f: the file is
np.take_along_axis(post, order[:, None, :], 0) bit for bit (asserted here), which is stored
instead of a second K x T x F array for the size limit.
Only inputs and recorded outputs are stored.  The tool prints how far the model
(tests/cacgmm_model.py, float64 normalisation) is from each record.
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
import cacgmm_model as cm  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STFT = dict(frame_len=512, frame_hop=256, window="hann", center=True, round_power_of_two=True)
RECIPES = {
    "2spk": dict(num_classes=3, num_iters=20, seed=777, cgmm_init=False, update_alpha=True, solve_permu=True),
    "noisy": dict(num_classes=2, num_iters=20, seed=777, cgmm_init=True, update_alpha=False, solve_permu=False),
}


def ref_snapshots(libs, x, g0, K, N, cgmm_init, ua):
    """The reference's posteriors after every iteration in cm.snapshots(N) (train(1) continues
    from the trainer's state, so N calls are train(N))."""
    tr = libs.cluster.CacgmmTrainer(x, K, gamma=None if g0 is None else g0.copy(), cgmm_init=cgmm_init,
                                    update_alpha=ua)
    out = {0: np.array(tr.gamma)}
    for n in range(1, N + 1):
        g = tr.train(1)
        if n in cm.snapshots(N):
            out[n] = np.array(g)
    return out


def doc_recipe(libs, cli, name, pcm, opts):
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, f"{name}.wav")
        wavfile.write(wav, 16000, pcm)
        scp = os.path.join(tmp, "wav.scp")
        with open(scp, "w") as fd:
            fd.write(f"{name} {wav}\n")
        dst = os.path.join(tmp, "out")
        args = argparse.Namespace(wav_scp=scp, dst_dir=dst, init_mask="", fmt="numpy", **STFT, **opts)
        cli.run(args)
        saved = np.load(os.path.join(dst, f"{name}.npy"))
        reader = libs.data_handler.SpectrogramReader(scp, **STFT, transpose=False)
        stft = reader[name]
    np.random.seed(opts["seed"])
    tr = libs.cluster.CacgmmTrainer(stft, opts["num_classes"], cgmm_init=opts["cgmm_init"],
                                    update_alpha=opts["update_alpha"])
    post = np.transpose(tr.train(opts["num_iters"]), (0, 2, 1)).astype(np.float32)
    K, T, F = post.shape
    assert saved.shape == post.shape and saved.dtype == np.float32
    order = np.zeros((K, F), dtype=np.uint8)
    for f in range(F):
        for k in range(K):
            hit = [j for j in range(K) if np.array_equal(saved[k, :, f], post[j, :, f])]
            assert len(hit) == 1, (name, f, k, hit)
            order[k, f] = hit[0]
    assert np.array_equal(np.take_along_axis(post, order[:, None, :].astype(np.int64), 0), saved)
    if not opts["solve_permu"]:
        assert (order == np.arange(K)[:, None]).all()
    # the model on the same spectrogram, for the record
    np.random.seed(opts["seed"])
    g0 = None if opts["cgmm_init"] else cm.random_start(K, F, T)
    m = cm.cacgmm_em(stft, K, opts["num_iters"], g0, cgmm_init=opts["cgmm_init"],
                     update_alpha=opts["update_alpha"])[-1]
    d = np.abs(np.transpose(m, (0, 2, 1)) - post)
    print(f"doc {name}: model (float64 normalisation) against the reference (complex64): max {d.max():.3e}, "
          f"mean {d.mean():.3e}; bins re-ordered by the aligner: {int((order != np.arange(K)[:, None]).any(0).sum())}")
    return post, order


def main():
    if not rh.available():
        raise SystemExit("the reference tree is not present")
    libs = rh.load()
    cli = rh.load_cli("estimate_cacgmm_masks")
    out = {"names": np.array(sorted(cm.CASES))}
    for name in sorted(cm.CASES):
        x, g0, K, N, cgmm_init, ua = cm.case_inputs(name)
        out[name + "_spec"] = x
        if g0 is not None:
            out[name + "_gamma0"] = g0
        model = cm.cacgmm_em(x, K, N, g0, cgmm_init=cgmm_init, update_alpha=ua)
        r128 = ref_snapshots(libs, x.astype(np.complex128), g0, K, N, cgmm_init, ua)
        r64 = ref_snapshots(libs, x, g0, K, N, cgmm_init, ua)
        for n, g in r128.items():
            out[f"{name}_ref128_{n}"] = g
        out[name + "_ref64_last"] = r64[N].astype(np.float64)
        d128 = max(np.abs(model[n] - g).max() for n, g in r128.items())
        d64 = np.abs(model[N] - r64[N])
        print(f"{name}: model against the reference, complex128 input (all snapshots): max {d128:.3e}; "
              f"complex64 input (last): max {d64.max():.3e}, mean {d64.mean():.3e}")
    doc = np.load(os.path.join(GOLD, "doc_spatial_clustering.npz"))
    files = {"ref_cacgmm.npz": out, "ref_cacgmm_2spk.npz": {}, "ref_cacgmm_noisy.npz": {}}
    for name, opts in RECIPES.items():
        post, order = doc_recipe(libs, cli, name, doc["pcm_" + name], opts)
        dst = files[f"ref_cacgmm_{name}.npz"]
        dst[name + "_post"] = post
        dst[name + "_order"] = order
    for fn, arrays in files.items():
        np.savez_compressed(os.path.join(GOLD, fn), **arrays)
        print(fn, os.path.getsize(os.path.join(GOLD, fn)), "bytes")


if __name__ == "__main__":
    main()
