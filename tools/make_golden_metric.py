#!/usr/bin/env python
"""
tests/golden/ref_metric.npz: what the UNMODIFIED reference (scripts/sptk/libs/metric.py and
compute_si_snr.py, loaded through oracle.ref_harness) returns on small signals, for
tests/test_metric_model.py and tests/test_gpu_metric.py.

    python tools/make_golden_metric.py        (needs the reference tree; no GPU)

Recorded: si_snr on planted pairs up to 60 dB (float32 inputs, both remove_dc settings),
permute_si_snr(align=True) on K = 2, 3, 4, and the command line in both modes on 16-bit wave files
(their samples, the --per-utt / --utt-ali files, the report text, with and without --spk2class).
Every case stays at or below 60 dB: the reference computes in float32 and above that its own
rounding, not the metric, decides the figure (tests/PARITY_NOTES_METRIC.md).  The distance of the
reference from the float64 statement tests/metric_model.py is measured here and stored with the
numpy version (`ref_gap_db`); the model tests hold the reference to four times it.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import scipy.io.wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import metric_model as model  # noqa: E402

SR = 16000


def to_pcm(x):
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def main():
    # libs/metric.py imports editdistance for permute_ed, which nothing here calls
    sys.modules.setdefault("editdistance", types.ModuleType("editdistance"))
    cli = ref_harness.load_cli("compute_si_snr")
    metric = sys.modules["libs.metric"]
    rng = np.random.default_rng(20261020)
    out = {"numpy_version": np.array(np.__version__)}
    gaps = []

    # ---- si_snr on planted pairs ----
    pair_cases = [(1000, -20.0), (4001, 0.0), (8192, 20.0), (12000, 40.0), (20000, 60.0)]
    out["pair_db"] = np.array([db for _, db in pair_cases])
    for k, (L, db) in enumerate(pair_cases):
        x, s = model.planted(rng, L, db)
        out[f"pair{k}_x"], out[f"pair{k}_s"] = x, s
        for name, dc in (("dc", True), ("nodc", False)):
            ref = float(metric.si_snr(x, s, remove_dc=dc))
            out[f"pair{k}_{name}"] = np.array(ref, dtype=np.float64)
            gaps.append(abs(ref - model.si_snr(x, s, remove_dc=dc)))

    # ---- permute_si_snr(align=True) ----
    perm_cases = [(2, (1, 0)), (3, (2, 0, 1)), (4, (3, 1, 0, 2))]
    out["perm_k"] = np.array([K for K, _ in perm_cases])
    for k, (K, order) in enumerate(perm_cases):
        L = 2000 + 37 * k
        refs = [(0.1 * rng.standard_normal(L) + 0.01 * (j + 1)).astype(np.float32) for j in range(K)]
        ests = [(0.6 * refs[order[n]] + 0.1 * 10.0 ** (-(12.0 + 3 * n) / 20.0) * rng.standard_normal(L)).astype(np.float32)
                for n in range(K)]
        best, ali = metric.permute_si_snr(ests, refs, align=True)
        assert tuple(ali) == order, (ali, order)
        out[f"perm{k}_x"], out[f"perm{k}_s"] = np.stack(ests), np.stack(refs)
        out[f"perm{k}_best"], out[f"perm{k}_order"] = np.array(float(best)), np.array(ali, dtype=np.int32)
        gaps.append(abs(float(best) - model.permute_si_snr(ests, refs)))

    # ---- the command line on 16-bit files: two speakers, four utterances ----
    keys = ["utt_a", "utt_b", "utt_c", "utt_d"]
    swap = [False, True, False, True]          # whether the separated files are in the other order
    classes = ["MM", "FM", "MM", "FF"]
    files = {}
    for u, key in enumerate(keys):
        L = 4000 + 501 * u
        r = [0.1 * rng.standard_normal(L) + 0.01, 0.08 * rng.standard_normal(L) - 0.02]
        e = [0.8 * r[j] + 0.1 * 10.0 ** (-(8.0 + 4 * u + 3 * j) / 20.0) * rng.standard_normal(L) for j in range(2)]
        if swap[u]:
            e = e[::-1]
        e, r = [to_pcm(v) for v in e], [to_pcm(v) for v in r]
        if u == 1:   # the separated signals run 100 samples longer: both sides are cut (:82-85, :95-98)
            e = [np.concatenate([v, to_pcm(0.05 * rng.standard_normal(100))]) for v in e]
        if u == 2:   # the references run longer
            r = [np.concatenate([v, to_pcm(0.05 * rng.standard_normal(64))]) for v in r]
        if u == 3:   # a two-channel reference: channel 0 is scored (:34-36)
            r[1] = np.stack([r[1], to_pcm(0.05 * rng.standard_normal(r[1].size))], axis=1)
        for name, v in (("sep1", e[0]), ("sep2", e[1]), ("ref1", r[0]), ("ref2", r[1])):
            files[f"{name}_{key}"] = v
    out["cli_keys"] = np.array(keys)
    out["cli_classes"] = np.array(classes)
    for name, v in files.items():
        out["cli_" + name] = v
    with tempfile.TemporaryDirectory() as tmp:
        for name, v in files.items():
            scipy.io.wavfile.write(os.path.join(tmp, name + ".wav"), SR, v)
        for name in ("sep1", "sep2", "ref1", "ref2"):
            with open(os.path.join(tmp, name + ".scp"), "w") as f:
                f.writelines(f"{key}\t{os.path.join(tmp, name + '_' + key + '.wav')}\n" for key in keys)
        with open(os.path.join(tmp, "spk2class"), "w") as f:
            f.writelines(f"{key}\t{c}\n" for key, c in zip(keys, classes))
        runs = {"single": ("sep1.scp", "ref1.scp", ""), "multi": ("sep1.scp,sep2.scp", "ref1.scp,ref2.scp", ""),
                "multi_class": ("sep1.scp,sep2.scp", "ref1.scp,ref2.scp", "spk2class")}
        for tag, (sep, ref, s2c) in runs.items():
            join = lambda scps: ",".join(os.path.join(tmp, p) for p in scps.split(","))  # noqa: E731
            args = argparse.Namespace(sep_scp=join(sep), ref_scp=join(ref),
                                      spk2class=os.path.join(tmp, s2c) if s2c else "",
                                      per_utt=os.path.join(tmp, tag + ".snr"), utt_ali=os.path.join(tmp, tag + ".ali"))
            text = io.StringIO()
            with contextlib.redirect_stdout(text), contextlib.redirect_stderr(io.StringIO()):
                cli.run(args)
            out[f"cli_{tag}_report"] = np.array(text.getvalue())
            out[f"cli_{tag}_per_utt"] = np.array(open(args.per_utt).read())
            out[f"cli_{tag}_utt_ali"] = np.array(open(args.utt_ali).read())
    # the reference against the model on what the command line scored
    for u, key in enumerate(keys):
        e = [files[f"sep{j}_{key}"].astype(np.float32) / np.float32(32768) for j in (1, 2)]
        r = [files[f"ref{j}_{key}"].astype(np.float32) / np.float32(32768) for j in (1, 2)]
        r = [v if v.ndim == 1 else v[:, 0] for v in r]
        end = min(e[0].size, r[0].size)
        e, r = [v[:end] for v in e], [v[:end] for v in r]
        gaps.append(abs(float(metric.permute_si_snr(e, r)) - model.permute_si_snr(e, r)))
        gaps.append(abs(float(metric.si_snr(e[0], r[0])) - model.si_snr(e[0], r[0])))
    out["ref_gap_db"] = np.array(max(gaps), dtype=np.float64)
    dst = os.path.join(ROOT, "tests", "golden", "ref_metric.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {os.path.getsize(dst)} bytes; numpy {np.__version__}; "
          f"largest |reference - float64 model| = {max(gaps):.3e} dB over {len(gaps)} figures")


if __name__ == "__main__":
    main()
