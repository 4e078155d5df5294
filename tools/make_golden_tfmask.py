#!/usr/bin/env python
"""
tests/golden/ref_tfmask.npz: what the UNMODIFIED reference tools (scripts/sptk/compute_mask.py,
wav_separate.py, oracle_separate.py, loaded through oracle.ref_harness) return on the cases of
tests/tfmask_cases.py, for tests/test_tfmask_cases.py and tests/test_gpu_tfmask.py.

    python tools/make_golden_tfmask.py            (needs the reference tree; no GPU)
    python tools/make_golden_tfmask.py --check    reproduce the file, compare, print the figures

Recorded (inputs and outputs only):
  fn_*    compute_mask(tgt, mix, kind) of compute_mask.py and compute_mask(mixture, targets, kind)
          of oracle_separate.py on the complex64 rounding of the float64 spectra of the two smallest
          noise pairs and the K = 8 oracle pair
  cli_*   three 16-bit wav pairs (clean, other, noisy = clean + other) through run() of the three
          tools: the archives of compute_mask (irm; psm with --cutoff 2; crm), the waves of
          wav_separate on the irm archive and of oracle_separate (irm, two references)
On EVERY case the restatement of tests/tfmask_cases.py is held to the reference's functions bit
for bit, and the ibm waveform pairs are asserted to have an empty argmax band.

Figures printed (tests/PARITY_NOTES_TFMASK.md records them): the smallest rounding constant c that
covers the reference's own float32 arithmetic per kind, the share of cells left out per case, the
cells in the ibm band, the cells where the float32 and float64 ibm decisions differ.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import scipy.io.wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import tfmask_cases as tc  # noqa: E402

SR = 16000
STFT = dict(frame_len=512, frame_hop=256, round_power_of_two=True, window="hann", center=True)
CLI_MASKS = (("irm", -1.0), ("psm", 2.0), ("crm", -1.0))


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*args)


def build():
    cm = ref_harness.load_cli("compute_mask")
    ws = ref_harness.load_cli("wav_separate")
    osep = ref_harness.load_cli("oracle_separate")
    out = {"numpy_version": np.array(np.__version__)}
    figures = {"c": {}, "left_out": {}, "ibm_band": {}, "ibm_f32_f64": {}}

    # ---- the functions on stored spectra: the restatement bit for bit, the figures ----
    stored = ("noise512u/K2", "noise1000c/K2")
    for p in tc.mask_pairs() + tc.other_size_pairs():
        ts32, m32 = p.spectra(np.complex64)
        for kind in tc.KINDS:
            with np.errstate(all="ignore"):
                ref = quiet(cm.compute_mask, ts32[0], m32, kind)
            mine = tc.mask_formula(kind, ts32[0], m32)
            assert same(np.asarray(ref), np.asarray(mine)), f"{p.name}:{kind}: the restatement differs"
            if p.name in stored:
                out[f"fn_{p.name}_{kind}"] = np.asarray(ref, np.float32)
            if not p.judged:
                continue
            c = tc.smallest_c(kind, p)
            assert c is not None, f"{p.name}:{kind}: the yardstick is outside a cap"
            figures["c"][kind] = max(figures["c"].get(kind, 0), c)
            v = tc.judge_mask("yardstick", kind, tc.yardstick_mask(kind, p), p, c_round=tc.C_ROUND)
            figures["left_out"][f"{p.name}:{kind}"] = v.left_out
            if kind == "ibm":
                ts, m = p.spectra()
                figures["ibm_f32_f64"][p.name] = int((np.asarray(mine) != tc.mask_formula(kind, ts[0], m)).sum())
        if p.name in stored:
            out[f"fn_{p.name}_tgt"], out[f"fn_{p.name}_mix"] = p.pcm[0][0], p.pcm[1]
    for p in tc.oracle_pairs():
        ts32, m32 = p.spectra(np.complex64)
        figures["ibm_band"][p.name] = tc.ibm_band_cells(p)
        assert figures["ibm_band"][p.name] == 0, f"{p.name}: the ibm waveform case needs an empty band"
        for kind in tc.ORACLE_KINDS:
            with np.errstate(all="ignore"):
                ref = quiet(osep.compute_mask, m32, ts32, kind)
            mine = tc.oracle_formula(kind, m32, ts32)
            assert all(same(np.asarray(r), np.asarray(x)) for r, x in zip(ref, mine)), f"{p.name}:{kind}"
            c = tc.smallest_c(kind, p, oracle=True)
            assert c is not None, f"{p.name}:{kind} (oracle): the yardstick is outside a cap"
            figures["c"]["oracle " + kind] = max(figures["c"].get("oracle " + kind, 0), c)
            if len(ts32) == 8:
                out[f"fn_oracle8_{kind}"] = np.stack([np.asarray(r) for r in ref]).astype(
                    bool if kind == "ibm" else np.float32)
        if len(ts32) == 8:
            out["fn_oracle8_targets"], out["fn_oracle8_mix"] = np.stack(p.pcm[0]), p.pcm[1]

    # ---- the command lines on 16-bit files ----
    keys = ["utt_a", "utt_b", "utt_c"]
    rng = np.random.default_rng(20261021)
    files = {}
    for key, n in zip(keys, (2000, 3000, 4133)):
        clean = np.rint(32768 * tc.coloured(rng, n)).astype(np.int16)
        other = np.rint(32768 * 0.7 * tc.coloured(rng, n)).astype(np.int16)
        files[f"clean_{key}"], files[f"other_{key}"] = clean, other
        files[f"noisy_{key}"] = (clean.astype(np.int32) + other).astype(np.int16)
    out["cli_keys"] = np.array(keys)
    for name, v in files.items():
        out["cli_" + name] = v
    libs = ref_harness.load()
    with tempfile.TemporaryDirectory() as tmp:
        for name, v in files.items():
            scipy.io.wavfile.write(os.path.join(tmp, name + ".wav"), SR, v)
        for role in ("clean", "other", "noisy"):
            with open(os.path.join(tmp, role + ".scp"), "w") as f:
                f.writelines(f"{key}\t{os.path.join(tmp, role + '_' + key + '.wav')}\n" for key in keys)
        scp = {role: os.path.join(tmp, role + ".scp") for role in ("clean", "other", "noisy")}
        for kind, cutoff in CLI_MASKS:
            args = argparse.Namespace(clean_scp=scp["clean"], noisy_scp=scp["noisy"],
                                      mask_ark=os.path.join(tmp, kind + ".ark"), scp=os.path.join(tmp, kind + ".scp"),
                                      format="kaldi", mask=kind, cutoff=cutoff, **STFT)
            with np.errstate(all="ignore"):
                quiet(cm.run, args)
            reader = libs.data_handler.ScriptReader(args.scp)
            for key in keys:
                out[f"cli_{kind}_{key}"] = np.asarray(reader[key], np.float32)
        args = argparse.Namespace(wav_scp=scp["noisy"], mask_scp=os.path.join(tmp, "irm.scp"),
                                  dst_dir=os.path.join(tmp, "sep"), sr=SR, phase_ref="", fmt="kaldi", keep_length=False,
                                  mixed_norm=True, **STFT)
        quiet(ws.run, args)
        args = argparse.Namespace(mix_scp=scp["noisy"], ref_scp=scp["clean"] + "," + scp["other"],
                                  dump_dir=os.path.join(tmp, "ora"), mask="irm", sr=SR, keep_length=False, **STFT)
        quiet(osep.run, args)
        for key in keys:
            out[f"cli_sep_{key}"] = scipy.io.wavfile.read(os.path.join(tmp, "sep", key + ".wav"))[1]
            for k in (1, 2):
                out[f"cli_ora{k}_{key}"] = scipy.io.wavfile.read(os.path.join(tmp, "ora", f"spk{k}", key + ".wav"))[1]
    return out, figures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="reproduce the file, compare with it, print the figures")
    opts = ap.parse_args()
    out, fig = build()
    if opts.check:
        old = np.load(tc.GOLDEN)
        assert sorted(old.files) == sorted(out), "the golden file holds other entries"
        for name in out:
            if name == "numpy_version":
                continue
            a, b = np.asarray(out[name]), old[name]
            if a.dtype.kind == "f":
                assert a.shape == b.shape and np.allclose(a, b, rtol=1e-5, atol=1e-6, equal_nan=True), name
            else:
                assert np.array_equal(a, b), name
        print(f"{tc.GOLDEN}: reproduced (numpy {np.__version__}, recorded with {old['numpy_version']})")
    else:
        np.savez_compressed(tc.GOLDEN, **out)
        print(f"{tc.GOLDEN}: {os.path.getsize(tc.GOLDEN)} bytes; numpy {np.__version__}")
    c = max(fig["c"].values())
    print("smallest c that covers the reference's float32 arithmetic, per kind:", fig["c"])
    print(f"c = {c}; C_ROUND = m x max(c, 1) = {int(tc.M_BITS) * max(c, 1)} (tests/tfmask_cases.py has {tc.C_ROUND})")
    worst = {}
    for name, share in fig["left_out"].items():
        case, kind = name.rsplit(":", 1)
        worst[case] = max(worst.get(case, 0.0), share if kind != "ibm" else 0.0)
    print("cells left out (ratio kinds, worst kind), per case:",
          {k: f"{100 * v:.3f} %" for k, v in worst.items()})
    print("ibm cells inside the band, per case:",
          {n.rsplit(":", 1)[0]: f"{100 * s:.3f} %" for n, s in fig["left_out"].items() if n.endswith(":ibm")})
    print("ibm cells whose float32 and float64 decisions differ:", fig["ibm_f32_f64"])
    print("cells in the argmax band of the oracle pairs:", fig["ibm_band"])


if __name__ == "__main__":
    main()
