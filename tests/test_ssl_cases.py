"""
ssl_cases.py on the CPU: the float64 reference reproduces the reference project's recorded indices
(tests/golden/ref_ssl.npz); its restatement with the per-cell terms kept equals it; the input
conditions of every case the GPU file runs hold (ML: delta >= 2^-10 x power; MUSIC: the eigenvalue
gaps; no cell without a bar); the float32 models of the ML and SRP kernels stay within the bar of
every cell of those cases, so the bar is attainable by honest float32 arithmetic; and seeded faults,
each at one place, all fail the judge -- the table says which of them the flat bar of test_gpu_ssl.py
(max_a |device - model| <= 1e-4 x spread, per spectrum) would have seen.  Figures: PARITY_NOTES_SSL.md.
"""
import functools

import numpy as np
import pytest

import ssl_cases as sc
import ssl_model
from conftest import load_golden
from oracle import np_oracle as o

WORST = {}


# ---------------------------------------------------------------- the reference against the recorded indices
@functools.lru_cache(maxsize=None)
def scene_inputs(name):
    g = load_golden("ref_ssl.npz")
    x = g[name + "_pcm"].astype(np.float32) / np.float32(32768.0)
    kw = ssl_model.scene_stft_kwargs(name)
    kw.pop("round_power_of_two")
    X = np.stack([o.forward_stft(c, transpose=True, **kw) for c in x]).astype(np.complex64)
    return X, ssl_model.scene_steer_vectors(name).astype(np.complex64), ssl_model.scene_masks(name)


@pytest.mark.parametrize("name", list(ssl_model.SCENES))
def test_reference_reproduces_the_recorded_indices(name):
    g = load_golden("ref_ssl.npz")
    X, sv, masks = scene_inputs(name)
    pairs = list(zip(*ssl_model.scene_pairs(name)))
    for tag, m in (("nomask", None), ("mask", masks[0])):
        for backend in sc.BACKENDS:
            idx, score = sc.reference(backend, X, sv, None, m, pairs, **(sc.ML_CLI if backend == "ml" else {}))
            print(f"{name} {backend} {tag}: index {idx[0]}")
            assert int(idx[0]) == int(g[f"{name}_{backend}_{tag}"]), (name, backend, tag)
            # the restatement with its terms kept is the same spectrum
            case = sc.Case(name, backend, "scene", X, sv, m, [(0, X.shape[1])], pairs if backend == "srp" else None,
                           dict(sc.ML_CLI) if backend == "ml" else None)
            own = sc.expected(case)["own"]
            assert np.abs(own - score).max() <= 1e-7 * np.abs(score).max(), (name, backend, tag)


# ---------------------------------------------------------------- the float32 model under the judge
@functools.lru_cache(maxsize=None)
def all_groups():
    """(group, list of cases): every case of test_gpu_ssl_conformance.py but the batch entry's, whose
    spectrograms come from the device's transform"""
    out = []
    for b in sc.BACKENDS:
        out.append((f"channels {b}", [c for C in range(1, 17) for c in sc.channel_cases(C, b)]))
        out.append((f"edges {b}", [c for ax, v in sc.EDGES for c in sc.edge_cases(ax, v, b)]))
        out.append((f"one-hot {b}", sc.onehot_cases(b)))
        out.append((f"families {b}", [c for C in (2, 5, 16) for c in sc.family_cases(b, C)]))
        out.append((f"ties {b}", [c for c, _, _ in sc.tie_cases(b)]))
        out.append((f"nan {b}", sc.nan_cases(b)))
    out.append(("fold srp", [c for pair in sc.fold_cases() for c in pair]))
    out.append(("options ml", sc.ml_option_cases()))
    out.append(("windows music", sc.music_window_cases()))
    return out


GROUPS = [g for g, _ in all_groups()]


@pytest.mark.parametrize("group", GROUPS)
def test_input_conditions_and_the_float32_model(group):
    """Per case: the conditions on the inputs, the restatement against ssl_model, and (ML, SRP) the
    float32 model under the judge.  A worst ratio above about one half would say that the allowance or
    the inputs are wrong."""
    cases = dict(all_groups())[group]
    tally = sc.Tally(f"model {group}")
    for c in cases:
        exp = sc.expected(c)
        with np.errstate(all="ignore"):
            scale = np.nanmax(np.abs(np.where(np.isfinite(exp["ref"]), exp["ref"], 0.0))) + 1.0
            assert np.nanmax(np.abs(exp["own"] - exp["ref"]), initial=0.0) <= (1e-6 if c.backend == "music" else 1e-9) * scale, c.name
        assert np.array_equal(np.isfinite(exp["own"]), np.isfinite(exp["ref"])), c.name
        if c.needs_delta:
            assert exp["delta_ratio"] >= sc.DELTA_FLOOR, (c.name, exp["delta_ratio"])
        if c.backend == "ml":
            assert c.needs_delta or c.rule == "range", c.name
        if c.backend == "music":
            assert exp["gap"] >= c.min_gap and tuple(exp["dead"]) == tuple(c.dead_bins), (c.name, exp["gap"], exp["dead"])
            continue
        idx, got = sc.run_model(c)
        sc.evaluate(c, exp, idx, got, tally)
    tally.report()
    for fam, (r, name, _) in tally.worst.items():
        key = fam.split()[0] + (" (range)" if "(range)" in fam else "")
        if r >= WORST.get(key, (0.0, ""))[0]:
            WORST[key] = (r, name)
    assert not tally.failures, "\n".join(tally.failures[:20])
    for fam, (r, name, where) in tally.worst.items():
        if "(range)" not in fam:
            assert r <= 0.5, (fam, r, name, where)


def test_worst_ratio_of_the_model_per_backend():
    for key, (r, name) in sorted(WORST.items()):
        print(f"float32 model, {key}: worst error/allowance {r:.3f} ({name})")


# ---------------------------------------------------------------- seeded faults
def base(backend, **kw):
    """4 channels, 65 frames (three tiles), 33 bins (two patches), 65 directions (one padding wave)"""
    return sc.make("faults", backend, "plane", 4, 65, 33, 65, sc.frames_and_whole(65), **kw)


def faults():
    """name -> (case, (index, scores) of the faulty model)"""
    ml, srp = base("ml"), base("srp")
    out = {}
    out["one bin dropped from one frame tile (ML)"] = (ml, sc.run_model(ml, "drop_bin"))
    out["frame 32 reads frame 31's observation (SRP)"] = (srp, sc.run_model(srp, "stale_frame"))
    out["the last pair skipped (SRP)"] = (srp, sc.run_model(srp, "last_pair"))
    out["imaginary sign of one pair flipped in one bin (SRP)"] = (srp, sc.run_model(srp, "imag_sign"))
    out["the neighbouring bin's mask at f = 32 (ML)"] = (ml, sc.run_model(ml, "mask_neighbour"))
    S = sc.model_pad_overwrite(sc.model_srp(srp.x, srp.sv, srp.pairs, srp.mask), 0.0)
    out["padding direction written over direction 0 of the next row (SRP)"] = (srp, sc.model_windows(S, srp.windows))
    e3 = base("ml", kw=dict(compression=0, eps=1e-3))
    out["1 / (1 + eps) omitted (ML, eps = 1e-3)"] = (e3, sc.run_model(e3, "no_inv1pe"))
    al = sc.make("faults", "ml", "aligned", 4, 65, 33, 65, sc.frames_and_whole(65))
    out["the eps clamp omitted (ML, aligned)"] = (al, sc.run_model(al, "no_clamp"))
    fold = sc.make("faults", "srp", "white", 4, 129, 33, 65, [(0, 129)])
    out["the frame at a 64-chunk boundary dropped from the fold (SRP)"] = (fold, sc.run_model(fold, "fold_boundary"))
    out["window t1 taken inclusive (SRP)"] = (srp, sc.run_model(srp, "t1_inclusive"))
    tie = sc.tie_cases("srp")[0][0]
    out["the tie rule returning the highest index (SRP)"] = (tie, sc.run_model(tie, "tie_highest"))
    nan = [c for c in sc.nan_cases("ml") if "nan in x" in c.name][0]
    out["a NaN swallowed by the clamp (ML)"] = (nan, sc.run_model(nan, "nan_clamp"))
    ex = [c for c in sc.family_cases("ml", 5) if c.family == "extreme"][0]
    out["|x| under norm without the rescaling (ML, extreme)"] = (ex, sc.run_model(ex, naive_modulus=True))
    return out


def test_seeded_faults_fail_the_judge():
    rows = []
    for name, (case, (idx, got)) in faults().items():
        exp = sc.expected(case)
        clean = sc.Tally("clean")
        sc.evaluate(case, exp, *sc.run_model(case), clean)
        assert not clean.failures, (name, clean.failures[:3])
        tally = sc.Tally(name)
        v = sc.evaluate(case, exp, idx, got, tally)
        whole = [w for w, (t0, t1) in enumerate(case.windows) if t1 - t0 == case.x.shape[1]]
        flat_all = sc.flat_bar_sees(got, exp["ref"])
        flat_whole = sc.flat_bar_sees(got[whole], exp["ref"][whole]) if whole else False
        if not np.isfinite(exp["ref"]).all():
            flat_whole = flat_all = None            # max |device - model| / spread is a NaN there
        rows.append((name, v.worst, len(tally.failures), flat_whole, flat_all))
        assert tally.failures, f"the judge does not see: {name}"
    print("\n| seeded fault | worst error / bar | flat bar on the whole utterance | flat bar on every window of the case |")
    print("|---|---|---|---|")
    say = {True: "sees it", False: "misses it", None: "not defined (NaN reference)"}
    for name, worst, n, fw, fa in rows:
        print(f"| {name} | {worst:.3g} | {say[fw]} | {say[fa]} |")
