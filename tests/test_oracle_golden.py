"""
Pins the CPU oracle (oracle/np_oracle.py) against
  (i)  the reference's stored doc vectors (doc/adaptive_beamformer/asset),
  (ii) vectors produced by the unmodified reference modules
       (oracle/make_golden.py -> tests/golden/*.npz),
  (iii) what the live reference answered on seeded cases, recorded once
       (oracle/make_golden.py gen_live -> tests/golden/ref_live.npz).
"""
import os

import numpy as np
import pytest

from conftest import load_golden, pcm16_rel_rms, rms, rel_rms
from oracle import np_oracle as o
from oracle import make_golden as mg

STFT_KW = dict(frame_len=512, frame_hop=256, window="hann", center=True)


def pcm_to_float(x):
    return x.astype(np.float64) / 32768.0


def float_to_pcm(x):
    return np.rint(np.asarray(x, dtype=np.float64) * 32767.0)


def per_bin_gain_fit(ours, stored):
    """Least-squares complex gain per frequency bin between two waveforms
    (gauge analysis).  Returns gains[F], residual rms after fit."""
    A = o.forward_stft(ours.astype(np.float32), transpose=False, **STFT_KW)
    B = o.forward_stft(stored.astype(np.float32), transpose=False, **STFT_KW)
    num = np.sum(B * np.conj(A), axis=1)
    den = np.maximum(np.sum(np.abs(A)**2, axis=1), 1e-30)
    g = num / den
    energy = np.sum(np.abs(B)**2, axis=1)
    g = np.where(energy > 1e-4 * np.max(energy), g, np.median(np.abs(g)))
    return g, rms(g[:, None] * A, B) / max(rms(B), 1e-30)


@pytest.fixture(scope="module")
def live():
    return load_golden("ref_live.npz")


@pytest.fixture(scope="module")
def doc():
    return load_golden("doc_adaptive_beamformer.npz")


DOC_CASES = [
    ("pmwf_0", "pmwf-0", {}),
    ("pmwf_0_eig", "pmwf-0", dict(rank1_appro="eig")),
    ("pmwf_0_gev", "pmwf-0", dict(rank1_appro="gev")),
]


@pytest.mark.parametrize("key,kind,kw", DOC_CASES)
def test_doc_gauge_free_goldens(doc, key, kind, kw):
    """PMWF outputs are gauge free: the oracle reproduces the reference's
    stored wav to PCM16 quantisation."""
    samps = (doc["egs"].astype(np.float32) / 32768.0).T.copy()
    wav = o.enhance_utterance(samps, doc["cgmm_mask"], kind=kind, **kw)
    assert wav.shape[0] == doc[key].shape[0] == 93952
    err = rms(float_to_pcm(wav) / 32768.0, pcm_to_float(doc[key]))
    assert err < 4e-5, err


def resolve_gauge(enh, norm, stored):
    """Find the per-bin +-1 pattern s_f for which istft(enh * s_f) (renormed)
    reproduces `stored`.  Candidates come from the per-bin
    correlation <STFT(stored)_f, enh_f> (a flipped bin also depresses its
    neighbours through window leakage), then a greedy coordinate search keeps
    the flips that lower the waveform error."""
    B = o.forward_stft(stored.astype(np.float32), transpose=False, **STFT_KW)
    c = (np.sum(B * np.conj(enh), axis=1) /
         np.maximum(np.sum(np.abs(enh)**2, axis=1), 1e-30)).real
    cand = [int(f) for f in np.argsort(c) if c[f] < 0.75 * np.median(c)]
    signs = np.ones(enh.shape[0])

    def err_of(sg):
        wav = o.inverse_stft(enh * sg[:, None], norm=norm, transpose=False,
                             **STFT_KW)
        return rms(float_to_pcm(wav) / 32768.0, stored)

    best = err_of(signs)
    improved = True
    while improved:
        improved = False
        for f in cand:
            signs[f] *= -1
            e = err_of(signs)
            if e < best:
                best, improved = e, True
            else:
                signs[f] *= -1
    return signs, best


@pytest.mark.parametrize("key,kind,kw", [("mvdr", "mvdr", {}),
                                         ("gevd", "gevd", {}),
                                         ("gevd_ban", "gevd", dict(ban=True))])
def test_doc_gauged_goldens(doc, key, kind, kw):
    """MVDR/GEV stored outputs equal ours up to a per-bin +-1 (LAPACK sign
    gauge): after resolving the sign pattern the stored wav is
    reproduced to PCM16 quantisation."""
    samps = (doc["egs"].astype(np.float32) / 32768.0).T.copy()
    _, parts = o.enhance_utterance(samps, doc["cgmm_mask"], kind=kind,
                                   return_parts=True, **kw)
    signs, err = resolve_gauge(parts["enh"], parts["norm"],
                               pcm_to_float(doc[key]))
    assert err < 4e-5, err
    assert int(np.sum(signs < 0)) < 0.1 * signs.shape[0]


def test_cgmm_mask_matches_reference(doc):
    samps = (doc["egs"].astype(np.float32) / 32768.0).T.copy()
    stft = o.multichannel_stft(samps, transpose=False, **STFT_KW)
    m = o.cgmm_masks(stft, 20)
    assert m.shape == doc["cgmm_mask"].shape == (368, 257)
    assert np.max(np.abs(m - doc["cgmm_mask"])) < 1e-4


def test_stft_goldens():
    g = load_golden("ref_stft.npz")
    for name, N, fl, hop, center, rp2, window in mg.STFT_CASES:
        x = g[f"{name}.x"]
        S = o.forward_stft(x, frame_len=fl, frame_hop=hop, center=center,
                           round_power_of_two=rp2, window=window,
                           transpose=False)
        assert S.shape == g[f"{name}.S"].shape
        assert S.dtype == np.complex64
        assert rel_rms(S, g[f"{name}.S"]) < 1e-6, name
        y = o.inverse_stft(S, frame_len=fl, frame_hop=hop, center=center,
                           window=window, transpose=False)
        assert y.shape == g[f"{name}.y"].shape
        assert rms(y, g[f"{name}.y"]) < 1e-6, name
        yn = o.inverse_stft(S, frame_len=fl, frame_hop=hop, center=center,
                            window=window, transpose=False, norm=0.5)
        assert rms(yn, g[f"{name}.y_norm"]) < 1e-6, name
        assert abs(np.max(np.abs(yn)) - 0.5) < 1e-5


def test_roundtrip_config0():
    """BASELINE config 0: 1-ch 16 kHz STFT -> iSTFT round trip on the CPU path."""
    x = o.synth_utterance(0, 1, 160000)[0]
    S = o.forward_stft(x, transpose=False, **STFT_KW)
    assert S.shape == (257, 626)
    y = o.inverse_stft(S, transpose=False, **STFT_KW)
    assert y.shape[0] == 256 * 625
    assert rms(y, x[:y.shape[0]]) / rms(x) < 1e-6


ORACLE_KINDS = {
    "mvdr": ("mvdr", {}), "mvdr_ban": ("mvdr", dict(ban=True)),
    "gevd": ("gevd", {}), "gevd_ban": ("gevd", dict(ban=True)),
    "pmwf0": ("pmwf-0", {}), "pmwf1": ("pmwf-1", {}),
    "pmwf0_ref1": ("pmwf-0", dict(pmwf_ref=1)),
    "pmwf0_eig": ("pmwf-0", dict(rank1_appro="eig")),
    "pmwf0_gev": ("pmwf-0", dict(rank1_appro="gev")),
    "mpdr": ("mpdr", {}), "mpdr_whiten": ("mpdr-whiten", {}),
    "mpdr_whiten_ban": ("mpdr-whiten", dict(ban=True)),
}


@pytest.mark.parametrize("case", mg.BF_CASES, ids=[c[0] for c in mg.BF_CASES])
def test_beamformer_goldens(case):
    g = load_golden("ref_beamformer.npz")
    name = case[0]
    mix, mask = mg.bf_inputs(case)
    obs = o.multichannel_stft(mix, transpose=False, **STFT_KW)
    Rs = o.compute_covar(obs, mask)
    Rn = o.compute_covar(obs, 1 - mask)
    assert rel_rms(Rs, g[f"{name}.Rs"]) < 1e-6
    assert rel_rms(Rn, g[f"{name}.Rn"]) < 1e-6
    # Hermitian property (the reference's only assertion, test-beamformer.cc:34-48)
    assert np.max(np.abs(Rs - np.conj(np.transpose(Rs, (0, 2, 1))))) < 1e-6
    # eigenvectors: equal up to gauge -> compare gauge-fixed
    pe = o.fix_gauge_evd(o.solve_pevd(Rs))
    assert rel_rms(pe, o.fix_gauge_evd(g[f"{name}.pevd"])) < 1e-4
    pg = o.fix_gauge_gev(o.solve_pevd(Rs, Rn), Rn)
    assert rel_rms(pg, o.fix_gauge_gev(g[f"{name}.pgevd"], Rn)) < 1e-4
    norm = float(np.max(np.abs(mix)))
    for kind, (okind, kw) in ORACLE_KINDS.items():
        enh = o.supervised_run(okind, mask, obs, **kw)
        wav = o.inverse_stft(enh, norm=norm, transpose=False, **STFT_KW)
        ref = g[f"{name}.{kind}.wav"]
        # same LAPACK in-process => same gauge; fall back to the gauge fit
        err = rms(wav, ref) / rms(ref)
        if err > 1e-3:
            _, err = per_bin_gain_fit(wav, ref)
        assert err < 1e-3, (name, kind, err)


def test_cli_goldens():
    g = load_golden("ref_cli.npz")
    for i in range(2):
        samps = (g[f"u{i}.pcm"].astype(np.float32) / 32768.0).T.copy()
        for bf in ("mvdr", "gevd", "pmwf-0"):
            wav = o.enhance_utterance(samps, g[f"u{i}.mask"], kind=bf)
            ref = pcm_to_float(g[f"u{i}.{bf}"])
            err = rms(float_to_pcm(wav) / 32768.0, ref) / rms(ref)
            if err > 1e-3:
                _, err = per_bin_gain_fit(wav, ref)
            assert err < 2e-3, (i, bf, err)


def test_live_reference_enhance(live):
    """Oracle == live reference on a fresh seeded case (incl. VAD + post-mask): the reference's
    MVDR output of that case as it recorded it (ref_live.npz), fed the oracle's STFT, which
    equals the reference's on a seeded sample of the spectrogram's bins."""
    mix, sp, nz = o.synth_utterance(42, 6, 7000, return_parts=True)
    mask = o.irm_mask(sp, nz)
    kw = dict(frame_len=512, frame_hop=256, window="hann", center=True,
              transpose=False)
    obs = np.stack([o.forward_stft(s, round_power_of_two=True, **kw) for s in mix])
    idx = live["mvdr.obs_index"]
    assert np.array_equal(idx, mg.live_obs_index(obs.shape))
    assert rel_rms(obs.reshape(-1)[idx], live["mvdr.obs_sample"]) < 1e-6
    ref = live["mvdr.enh"]
    ours = o.supervised_run("mvdr", mask, obs)
    assert ours.shape == ref.shape
    assert rel_rms(ours, ref) < 1e-5


def test_consumer_cli_goldens():
    """the oracle reproduces what the unmodified reference CLIs
    apply_fixed_beamformer.py and compute_df_on_mask.py wrote for the stored
    inputs (tests/golden/ref_consumers.npz, oracle/make_golden.py)."""
    g = load_golden("ref_consumers.npz")
    kw = dict(frame_len=512, frame_hop=256, center=True, window="hann")
    for k in ("u0", "u1"):
        samps = g[f"{k}.pcm"].T.astype(np.float32) / np.float32(32768)
        obs = np.stack([o.forward_stft(c, round_power_of_two=True, transpose=False, **kw)
                        for c in samps])                                   # M x F x T
        # fixed beamformer: beamform + inverse_stft, renorm to max |audio|, PCM16
        w = g["weights"][int(g[f"{k}.beam"])]
        enh = o.beamform(w, obs)
        wav = o.inverse_stft(enh, norm=float(np.max(np.abs(samps))), transpose=False, **kw)
        ref = g[f"{k}.fixed"].astype(np.float64) / 32768
        got = np.rint(wav.astype(np.float64) * 32767) / 32768
        assert wav.shape == ref.shape
        assert rms(got, ref) / rms(ref) < 2e-4
        # directional features (gauge free)
        mask = np.minimum(g[f"{k}.mask"], 1)
        sv = o.solve_pevd(o.compute_covar(obs, mask))
        df = o.directional_feats(obs, sv.T, df_pair=[(0, 1), (1, 3), (0, 2)])
        assert df.shape == g[f"{k}.df"].shape
        assert np.max(np.abs(df - g[f"{k}.df"])) < 2e-3


# ---------------------------------------------------------------------------
# WPE / facted WPD (libs/wpe.py)
# ---------------------------------------------------------------------------
def test_wpe_restatement_equals_reference_vectors():
    g = load_golden("ref_wpe.npz")
    rev, mix = mg.wpe_small_case()
    assert np.array_equal(o.compute_tap_mat(rev, 3, 1), g["small.tap"])
    assert np.allclose(o.compute_lambda(rev, ctx=2), g["small.lambda"], rtol=1e-12, atol=0)
    assert rel_rms(o.wpe(rev, taps=4, delay=2, context=1, num_iters=2), g["small.wpe"]) < 1e-10
    obs = o.multichannel_stft(mix, transpose=True, **STFT_KW)
    mask, enh = o.facted_wpd(obs, cgmm_iters=3, wpd_iters=2, taps=4, delay=2, context=1)
    assert np.max(np.abs(mask - g["small.wpd_mask"])) < 1e-5
    # per-bin sign of the steering vector is LAPACK's: compare up to it
    ref = g["small.wpd_enh"]
    sign = np.sign(np.real(np.sum(enh * np.conj(ref), axis=0)))
    assert rel_rms(enh * sign[None, :], ref) < 1e-6


def test_wpe_doc_assets():
    """doc/wpe: apply_wpe.py --frame-len 512 --frame-hop 128 (3 iterations, 10 taps,
    delay 3) and apply_wpd.py --frame-len 512 --wpd-iters 2 --cgmm-iters 10, against
    the wavs the reference's author stored."""
    g = load_golden("ref_wpe.npz")
    samps = (g["egs"].astype(np.float32) / 32768.0).T.copy()
    kw = dict(frame_len=512, frame_hop=128, window="hann", center=True)
    obs = o.multichannel_stft(samps, transpose=True, **kw)           # N x T x F
    der = o.wpe(np.transpose(obs, (2, 0, 1)), taps=10, delay=3, context=1, num_iters=3)
    wav = np.stack([o.inverse_stft(x, transpose=True, **kw) for x in np.transpose(der, (1, 2, 0))])
    stored = pcm_to_float(g["wpe_egs"]).T
    assert wav.shape == stored.shape == (4, 53248)
    assert rms(float_to_pcm(wav) / 32768.0, stored) / rms(stored) < 1e-3
    obs = o.multichannel_stft(samps, transpose=True, **STFT_KW)
    _, enh = o.facted_wpd(obs, cgmm_iters=10, wpd_iters=2, taps=10, delay=3, context=1)
    stored = pcm_to_float(g["wpd_egs"])
    _, best = resolve_gauge(enh.T, np.max(np.abs(samps)), stored)
    assert best / rms(stored) < 1e-3, best / rms(stored)


def test_cgmm_update_alpha_equals_live_reference(live):
    mix = o.synth_utterance(61, 4, 12000)
    obs = o.multichannel_stft(mix, transpose=False, **STFT_KW)
    for ua in (False, True):
        ref = mg.with_last_class(live[f"cgmm2.update_alpha{int(ua)}"])
        got = o.cgmm_gamma(obs, 5, update_alpha=ua)
        assert got.shape == ref.shape and np.max(np.abs(got - ref)) < 1e-9


def test_cgmm_three_classes_seeded_start_equals_live_reference(live):
    """num_classes != 2: the reference starts from np.random.uniform(size=[K, F, T]) of the legacy
    GLOBAL generator, which its CLI seeds with --seed (estimate_cgmm_masks.py:28, 95-98) -- a
    reproducible start (the round-3 text called it unseeded: wrong).  The oracle draws from the
    same generator in the same order: first utterance after the seed, then the second."""
    obs1 = o.multichannel_stft(o.synth_utterance(62, 4, 9000), transpose=False, **STFT_KW)
    obs2 = o.multichannel_stft(o.synth_utterance(63, 4, 7000), transpose=False, **STFT_KW)
    # after np.random.seed(777), in this order
    ref1, ref2 = (mg.with_last_class(live[k]) for k in ("cgmm3.first", "cgmm3.second"))
    got1 = o.cgmm_gamma(obs1, 4, num_classes=3, seed=777)
    got2 = o.cgmm_gamma(obs2, 4, num_classes=3, update_alpha=True)  # generator state carried over
    assert ref1.shape == got1.shape == (3,) + obs1.shape[1:] and ref2.shape == got2.shape
    assert np.max(np.abs(got1 - ref1)) < 1e-9 and np.max(np.abs(got2 - ref2)) < 1e-9


CLASSIC_RUNS = {
    "ds.circular": dict(kind="ds", geometry="circular", doa=77.5, num_arounded=4),
    "sd.circular.norm": dict(kind="sd", geometry="circular", doa=200.0, num_arounded=4, normalize=True),
    "ds.linear": dict(kind="ds", geometry="linear", doa=60.0, linear_topo=(0.0, 0.04, 0.08, 0.12)),
    "sd.linear": dict(kind="sd", geometry="linear", doa=135.0, linear_topo=(0.0, 0.05, 0.1, 0.2)),
    "sd.center.norm": dict(kind="sd", geometry="circular", doa=10.0, num_arounded=3,
                           circular_center=True, normalize=True),
    "ds.online": dict(kind="ds", geometry="circular", num_arounded=4, chunk_len=16),
}


def classic_online_doas(num_samples, chunk_len=16):
    T = 1 + num_samples // 256
    return [30.0 + 50.0 * k for k in range(-(-T // chunk_len))]


def test_classic_beamformer_goldens():
    """DS / SD: the oracle against the reference's stored doc outputs
    (doc/fixed_beamformer/asset: ds.wav = DS at 100 degrees with c = 340, sd.wav = SD
    with --normalize) and against files the unmodified reference CLI wrote."""
    g = load_golden("ref_classic.npz")
    egs = (g["doc.egs"].astype(np.float32) / 32768.0).T.copy()
    for name, kw in (("ds", dict(kind="ds")), ("sd", dict(kind="sd", normalize=True))):
        y = o.classic_enhance(egs, geometry="circular", doa=100.0, c=340, num_arounded=4,
                              radius=0.05, **kw)
        ref = g[f"doc.{name}"]
        assert y.shape == ref.shape
        assert pcm16_rel_rms(ref, y) < 1e-3, (name, pcm16_rel_rms(ref, y))
    for k in ("c0", "c1"):
        samps = (g[f"{k}.pcm"].astype(np.float32) / 32768.0).T.copy()
        for name, kw in CLASSIC_RUNS.items():
            kw = dict(kw)
            if name == "ds.online":
                kw["doa"] = classic_online_doas(samps.shape[1])
            y = o.classic_enhance(samps, c=343, **kw)
            ref = g[f"{k}.{name}"]
            assert y.shape == ref.shape, (k, name)
            assert pcm16_rel_rms(ref, y) < 2e-4, (k, name, pcm16_rel_rms(ref, y))


def test_spatial_clustering_doc_pipelines_on_real_recordings():
    """doc/spatial_clustering/README.md on the reference's two real recordings (first 4 s):
    K = 2 on noisy.wav (5 ch) and K = 3, seed 777, --solve-permu on 2spk.wav (7 ch), run through
    the UNMODIFIED reference by oracle/make_golden.py.  The oracle (and, for K = 3, the
    product's host-side aligner on the oracle's posteriors) reproduces what the reference CLI
    saves: T x F for two classes, K x T x F otherwise (estimate_cgmm_masks.py:62-64)."""
    from setk_amd.libs.cluster import permu_aligner
    g = load_golden("doc_spatial_clustering.npz")
    samps = (g["pcm_noisy"].astype(np.float32) / 32768.0).T.copy()
    stft = o.multichannel_stft(samps, transpose=False, **STFT_KW)
    m = o.cgmm_masks(stft, 20)
    assert m.shape == g["saved_noisy"].shape == (251, 257)
    d = np.abs(m - g["saved_noisy"])
    assert d.mean() < 1e-5 and d.max() < 1e-3, (d.mean(), d.max())
    samps = (g["pcm_2spk"].astype(np.float32) / 32768.0).T.copy()
    stft = o.multichannel_stft(samps, transpose=False, **STFT_KW)
    gamma = o.cgmm_gamma(stft, 20, num_classes=3, seed=777)           # K x F x T
    saved = permu_aligner(np.transpose(gamma, (0, 2, 1))).astype(np.float32)
    assert saved.shape == g["saved_2spk"].shape == (3, 251, 257)
    d = np.abs(saved - g["saved_2spk"])
    assert d.mean() < 1e-5 and d.max() < 1e-3, (d.mean(), d.max())


def test_wide_real_recording_through_the_reference_clis():
    """A real 16-channel recording (doc/ssl/asset/egs.wav, 2 s) through the unmodified
    estimate_cgmm_masks.py and apply_adaptive_beamformer.py --beamformer pmwf-0
    (make_golden.py wide): the oracle reproduces the saved mask and the saved wave file (PMWF is
    gauge free) to the PCM16 floor of this quiet recording."""
    g = load_golden("doc_wide_16ch.npz")
    samps = (g["pcm"].astype(np.float32) / 32768.0).T.copy()
    assert samps.shape == (16, 32000)
    stft = o.multichannel_stft(samps, transpose=False, **STFT_KW)
    m = o.cgmm_masks(stft, 20)
    d = np.abs(m - g["mask"])
    assert m.shape == g["mask"].shape == (126, 257) and d.mean() < 1e-5 and d.max() < 1e-3, (d.mean(), d.max())
    wav = o.enhance_utterance(samps, g["mask"], kind="pmwf-0")
    ref = pcm_to_float(g["pmwf0"])
    assert wav.shape == ref.shape
    # measured: every sample of the file equal (a quiet recording: one LSB is 3e-3 of its RMS)
    assert np.mean(float_to_pcm(wav) != g["pmwf0"]) < 1e-3


# ---- the reference's skip set on singular noise covariances ------------------------------
def _skipset_inputs():
    cases = dict(o.skipset_cases())
    cases.update(mg.skipset_real_recordings())
    return cases


def _oracle_outcome(samps, mask, spec, gauge):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            wav = o.enhance_utterance(samps, mask, gauge=gauge, **spec)
        except np.linalg.LinAlgError:
            return "LinAlgError"
    return "ok" if np.isfinite(wav).all() else "ok-nonfinite"


def test_oracle_skip_set_equals_the_reference():
    """Which (input, beamformer) pairs raise LinAlgError -- the utterances
    apply_adaptive_beamformer.py:170-172 skips.  tests/golden/ref_skipset.json is what the
    UNMODIFIED reference classes did (oracle/make_golden.py gen_skipset); the oracle must
    raise on exactly those, with and without the gauge (round 4's oracle raised from its own
    gauge Cholesky on `noisy` / the 16-channel recording under GEV, where the reference's
    scipy.linalg.eig fallback goes through: the reference skips NONE of its real
    recordings)."""
    import json
    table = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_skipset.json")))["table"]
    cases = _skipset_inputs()
    assert set(cases) == set(table)
    raised = 0
    for name, (samps, mask) in cases.items():
        for kname, spec in o.SKIPSET_KINDS.items():
            want = table[name][kname]
            for gauge in ((False, True) if samps.shape[0] <= 5 else (True,)):
                got = _oracle_outcome(samps, mask, spec, gauge)
                # a NaN result and a clean one are both "the reference writes a file"
                assert (got == "LinAlgError") == (want == "LinAlgError"), (name, kname, gauge, got, want)
            raised += want == "LinAlgError"
    assert raised >= 20
    for name in table:
        if name.startswith("real-"):
            assert all(v == "ok" for v in table[name].values()), name
        assert table[name]["gevd"] != "LinAlgError"  # the GEV path never raises (:54-59)


def test_skip_set_table_equals_the_live_reference(live):
    """The committed table against what the live reference answered on the same eight cases
    (ref_live.npz), and those cases' inputs byte for byte the ones it was asked about."""
    import json
    table = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_skipset.json")))["table"]
    cases = _skipset_inputs()
    names = [str(n) for n in live["skipset.names"]]
    kinds = [str(k) for k in live["skipset.kinds"]]
    assert names == list(mg.skipset_live_names()) and kinds == list(o.SKIPSET_KINDS)
    for i, name in enumerate(names):
        assert mg.skipset_input_sha256(*cases[name]) == live["skipset.input_sha256"][i], name
        for j, kname in enumerate(kinds):
            assert live["skipset.outcome"][i, j] == table[name][kname], (name, kname)
