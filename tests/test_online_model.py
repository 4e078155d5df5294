"""
The float64 statement of the block-online beamformer (tests/online_model.py) held to what is
known without a device: the unmodified reference classes (tests/golden/ref_online.npz, written by
tools/make_online_golden.py) under their phi = 1, the offline oracle where the two coincide, and the
recursion spelled out.
"""
import numpy as np
import pytest

import online_model as om
from conftest import load_golden, rel_rms
from oracle import np_oracle as o

CHUNK, ALPHA = 32, 0.8


@pytest.fixture(scope="module")
def case():
    mix, mask = om.case_inputs(4, 16384)
    obs = o.multichannel_stft(mix, round_power_of_two=True, transpose=False, **om.STFT_KW)
    assert obs.shape == (4, 257, 65)  # three chunks of 32, the last a single frame
    return mix, mask, obs


def _gauge_fit(a, ref):
    """rel rms of `a` against `ref` ([..., F, n]) after one unit phase per leading index and bin:
    the reference leaves its eigenvectors' phase to LAPACK."""
    ph = np.sum(ref * np.conj(a), axis=-1, keepdims=True)
    ph = np.where(np.abs(ph) > 0, ph / np.maximum(np.abs(ph), 1e-300), 1)
    return rel_rms(a * ph, ref)


@pytest.mark.parametrize("kind", ["mvdr", "gevd"])
def test_model_with_phi_one_reproduces_the_reference_classes(case, kind):
    g = load_golden("ref_online.npz")
    _, mask, obs = case
    mask = np.minimum(mask, 1)
    for ban in (False, True):
        # the reference sums a chunk's covariances in the spectrogram's complex64 (promote=False)
        m = om.online_parts(obs, mask, CHUNK, ALPHA, kind=kind, ban=ban, gauge=False, reference_phi=True,
                            promote=False)
        ref = g[f"{kind}{'_ban' if ban else ''}.enh"]
        assert m["enh"].shape == ref.shape
        chunks = [slice(t, t + CHUNK) for t in range(0, ref.shape[1], CHUNK)]
        for sl in chunks:  # (complex64 records: 6e-8)
            assert _gauge_fit(m["enh"][:, sl], ref[:, sl]) < 1e-6, (kind, ban, sl)
        if not ban:
            assert m["weight"].shape == g[f"{kind}.weight"].shape
            assert _gauge_fit(m["weight"], g[f"{kind}.weight"]) < 1e-9
    # the float64 statement itself (observations promoted): the same up to the complex64 sums
    m = om.online_parts(obs, mask, CHUNK, ALPHA, kind=kind, gauge=False, reference_phi=True)
    assert _gauge_fit(m["weight"], g[f"{kind}.weight"]) < 1e-4
    # and the stated rule (phi_c = 1 - alpha after the first chunk) is a different beamformer
    m = om.online_parts(obs, mask, CHUNK, ALPHA, kind=kind, gauge=False, promote=False)
    assert _gauge_fit(m["weight"][1:], g[f"{kind}.weight"][1:]) > 1e-3
    assert _gauge_fit(m["weight"][:1], g[f"{kind}.weight"][:1]) < 1e-9


def test_the_recursion_spelled_out(case):
    _, mask, obs = case
    m = om.online_parts(obs, mask, CHUNK, ALPHA)
    cuts = [slice(0, 32), slice(32, 64), slice(64, 65)]
    rs = [o.compute_covar(obs[:, :, sl].astype(np.complex128), mask[sl].astype(np.float64)) for sl in cuts]
    rn = [o.compute_covar(obs[:, :, sl].astype(np.complex128), 1 - mask[sl].astype(np.float64)) for sl in cuts]
    assert np.allclose(m["Rs"][0], rs[0], rtol=0, atol=0)
    assert np.allclose(m["Rs"][1], ALPHA * rs[0] + (1 - ALPHA) * rs[1], rtol=1e-14, atol=0)
    assert np.allclose(m["Rn"][2], ALPHA * (ALPHA * rn[0] + (1 - ALPHA) * rn[1]) + (1 - ALPHA) * rn[2],
                       rtol=1e-14, atol=0)
    assert np.array_equal(m["rn"][2], rn[2])


@pytest.mark.parametrize("kind", ["mvdr", "gevd"])
@pytest.mark.parametrize("opts", [dict(), dict(ban=True, post_mask=True), dict(itf=True)])
def test_one_chunk_is_the_offline_beamformer(case, kind, opts):
    mix, mask, obs = case
    opts = dict(opts)
    itf = np.random.default_rng(7).uniform(0.1, 0.9, size=mask.shape).astype(np.float32) if opts.pop("itf", 0) else None
    ref = o.enhance_utterance(mix, mask, kind=kind, itf_mask=itf, gauge=True, **opts)
    for chunk in (65, 1000):
        # The offline oracle keeps the spectrogram's complex64 through its covariances AND its
        # eigen-solves; the model's state is complex128 (as the reference's online class).  With
        # the same complex64 sums (promote=False) what is left is the complex64 solve: float32
        # eps (1.2e-7) x cond(Rn) (<= 1.5e3 on these inputs) = 2e-4 at worst.
        wav = om.enhance_online(mix, mask, chunk, ALPHA, kind=kind, itf_mask=itf, promote=False, **opts)
        assert wav.shape == ref.shape and rel_rms(wav, ref) < 2e-4
        # the float64 statement: the project's bar on waveforms
        wav = om.enhance_online(mix, mask, chunk, ALPHA, kind=kind, itf_mask=itf, **opts)
        assert rel_rms(wav, ref) < 1e-3


@pytest.mark.parametrize("kind", ["mvdr", "gevd"])
def test_alpha_zero_is_independent_chunks(case, kind):
    _, mask, obs = case
    mask = np.minimum(mask, 1).astype(np.float64)
    obs = obs.astype(np.complex128)
    for ban in (False, True):
        m = om.online_parts(obs, mask, 33, 0.0, kind=kind, ban=ban)
        for t0 in (0, 33):
            sl = slice(t0, t0 + 33)
            ref = o.supervised_run(kind, mask[sl], obs[:, :, sl], ban=ban, gauge=True)
            assert rel_rms(m["enh"][:, sl], ref) < 1e-12, (kind, ban, t0)
