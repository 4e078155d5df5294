"""
The streaming kernels load their prefetched samples where the transforms read them: stage 1's
interior frames through a wave-uniform branch of their own (fft512.h load_raw), stage 3's
channels through two sample buffers that swap roles from channel to channel, the channel loop
unrolled by two with its last one or two channels outside it (pass2_mc.hip: float32 input from
five channels up -- C = 5 is the odd and C = 8 the even tail here; fewer channels and PCM input
keep the one buffer).  What can go wrong
is a matter of parity and of ends: one tile, an odd tile count, a partial last tile, a single
group, an odd last group, odd channel counts and one channel, edge and interior groups in one
launch.  So: utterances of T in {1, 2, 3, 4, 5, 8, 9, 13} frames at the 512 / 256 geometry as ONE
ragged batch per channel count C in {1, 2, 3, 5, 8}, centre off (T = 1 exists) and on (T >= 2).

Checked per utterance, every case, at the bars of the other fused-path tests
(test_gpu_baseline_sizes.py):
  * the covariances of stage 1 against the oracle's, <= 1e-5, and max |x| exactly;
  * the waveform, <= 1e-3, against the oracle's STFT beamformed with the weights the launch
    itself solved (its `weight` tap) and put through the oracle's inverse STFT and peak scaling.
    That compares stage 3 -- transform, channel order, fold, inverse, overlap-add, renorm -- with
    the oracle sample by sample without passing through the solve: with fewer frames than
    channels the noise covariance is singular and the oracle's OWN weights move with the last
    digits of its covariances (or numpy refuses), which says nothing about stage 3.  The solve
    has its conformance tests elsewhere (test_gpu_solve.py).
Bit-level identities, every case: 16-bit PCM input against float32 input on pcm / 32768; an
utterance alone against the same utterance inside the ragged batch under two cuts of stage 3's
work list (SETK_MC_P2_ITEMS = 1 and 4096); and the covariances under SETK_P1_ITEMS = 1 and 4096
stay within the covariance bar.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_rms
from oracle import np_oracle as o

pytestmark = pytest.mark.gpu

FRAMES = [1, 2, 3, 4, 5, 8, 9, 13]
EXTRA = [0, 37, 255, 100, 1, 200, 77, 131]  # samples past the last whole hop: odd and even ends
CHANNELS = [1, 2, 3, 5, 8]
WAVE_TOL, COVAR_TOL = 1e-3, 1e-5
F = 257


def lengths(center):
    """Sample counts of the ragged batch, one per frame count."""
    if center:  # T = 1 + N // 256 and reflect padding needs N > 256
        return [(t, 256 * (t - 1) + 1 + min(e, 254)) for t, e in zip(FRAMES, EXTRA) if t >= 2]
    return [(t, 512 + 256 * (t - 1) + e) for t, e in zip(FRAMES, EXTRA)]


def stft_kw(center):
    return dict(frame_len=512, frame_hop=256, window="hann", center=center, transpose=False)


@functools.lru_cache(maxsize=None)
def case(C, T, N, center):
    """(mix C x N float32, mask T x F) of one synthetic utterance."""
    mix, sp, nz = o.synth_utterance(1300 + 17 * C + T, C, N, return_parts=True)
    mask = o.irm_mask(sp, nz, center=center)
    assert mask.shape in ((T, F), (F, T)), (mask.shape, T)
    return np.ascontiguousarray(mix, dtype=np.float32), np.ascontiguousarray(mask.reshape(T, F) if mask.shape == (T, F) else mask.T, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def reference(C, T, N, center):
    """The oracle's parts of one case, none of which involves a solve: its STFT, its two
    covariances and the peak the output is scaled to."""
    mix, mask = case(C, T, N, center)
    stft = o.multichannel_stft(mix, round_power_of_two=True, **stft_kw(center))
    m = np.minimum(mask, 1)
    return dict(stft=stft, Rs=o.compute_covar(stft, m), Rn=o.compute_covar(stft, 1 - m), norm=np.max(np.abs(mix)))


def new_ctx(center):
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, 256, 512, center)
    return c


def enhance(c, C, audio, ns, masks, pcm=False, taps=False):
    """One fused launch.  audio: float32 [C][N] arrays, or int16 [N][C] frames with pcm."""
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    n = len(ns)
    if pcm:
        src = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in audio]
        a = [torch.zeros((C, c.pcm16_channel_stride(k)), dtype=torch.int16, device=dev) for k in ns]
        c.pcm16_deinterleave_batch(C, [t.data_ptr() for t in src], ns, [t.data_ptr() for t in a])
    else:
        a = [torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(dev) for u in audio]
    m = [torch.from_numpy(x).to(dev) for x in masks]
    outs = [torch.empty(c.istft_num_samples(c.num_frames(k)), dtype=torch.float32, device=dev) for k in ns]
    tp = None
    if taps:
        tp = dict(Rs=torch.empty((n, F, C, C), dtype=torch.complex64, device=dev),
                  Rn=torch.empty((n, F, C, C), dtype=torch.complex64, device=dev),
                  weight=torch.empty((n, F, C), dtype=torch.complex64, device=dev),
                  maxabs=torch.empty(n, dtype=torch.float32, device=dev))
    opts = _ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK | (_ffi.FLAG_IN_PCM16 if pcm else 0))
    st = c.enhance_batch(opts, C, [t.data_ptr() for t in a], ns, [t.data_ptr() for t in m], None,
                         [t.data_ptr() for t in outs], taps=tp)
    torch.cuda.synchronize()
    if tp:
        tp = {k: v.cpu().numpy() for k, v in tp.items()}
    return [t.cpu().numpy() for t in outs], st, tp


def batch(C, center):
    ln = lengths(center)
    pairs = [case(C, t, n, center) for t, n in ln]
    return ln, [p[0] for p in pairs], [p[1] for p in pairs]


@functools.lru_cache(maxsize=None)
def fused(C, center):
    """The ragged batch of one channel count through the default handle, once per module run."""
    ln, utts, masks = batch(C, center)
    c = new_ctx(center)
    try:
        for (t, n) in ln:
            assert c.num_frames(n) == t, (n, t)
        return enhance(c, C, utts, [n for _, n in ln], masks, taps=True)
    finally:
        c.close()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("C", CHANNELS)
def test_covariances_and_max_match_oracle(C, center):
    waves, st, taps = fused(C, center)
    for i, (t, n) in enumerate(lengths(center)):
        parts = reference(C, t, n, center)
        es, en = rel_rms(taps["Rs"][i], parts["Rs"]), rel_rms(taps["Rn"][i], parts["Rn"])
        print(f"C={C} T={t} centre={center}: Rs {es:.2e} Rn {en:.2e}")
        assert es < COVAR_TOL and en < COVAR_TOL, (C, t, es, en)
        assert rel_rms(taps["Rs"][i][256], parts["Rs"][256]) < COVAR_TOL, (C, t)  # (the Nyquist side path)
        assert taps["maxabs"][i] == np.max(np.abs(case(C, t, n, center)[0])), (C, t)


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("C", CHANNELS)
def test_waveforms_match_oracle_beamformed_with_the_same_weights(C, center):
    waves, st, taps = fused(C, center)
    compared = 0
    for i, (t, n) in enumerate(lengths(center)):
        parts = reference(C, t, n, center)
        w = taps["weight"][i].astype(np.complex128)
        assert w.shape == (F, C) and np.isfinite(w).all(), (C, t, st[i])
        ref = o.inverse_stft(o.beamform(w, parts["stft"]), norm=parts["norm"], **stft_kw(center))
        assert waves[i].shape == ref.shape, (C, t, waves[i].shape, ref.shape)
        err = rel_rms(waves[i], ref)
        print(f"C={C} T={t} centre={center}: status {st[i]} max |w| {np.max(np.abs(w)):.2e} waveform rel rms {err:.2e}")
        assert err < WAVE_TOL, (C, t, err)
        compared += 1
    assert compared == len(lengths(center))


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("C", CHANNELS)
def test_pcm16_equals_float32_bit_for_bit(C, center):
    ln, utts, masks = batch(C, center)
    ns = [n for _, n in ln]
    frames = [np.ascontiguousarray(np.clip(np.rint(u.T * 32767.0 * 4.0), -32768, 32767).astype(np.int16)) for u in utts]
    floats = [np.ascontiguousarray(f.T.astype(np.float32) / 32768.0) for f in frames]
    c = new_ctx(center)
    try:
        ys, sts, tps = enhance(c, C, frames, ns, masks, pcm=True, taps=True)
        yf, stf, tpf = enhance(c, C, floats, ns, masks, taps=True)
    finally:
        c.close()
    assert sts == stf
    for k in ("Rs", "Rn", "weight", "maxabs"):
        assert np.array_equal(bits(tps[k]), bits(tpf[k])), (C, k)
    for i, (t, n) in enumerate(ln):
        assert np.array_equal(bits(ys[i]), bits(yf[i])), (C, t)


@pytest.mark.parametrize("C", CHANNELS)
def test_alone_and_in_the_batch_under_two_cuts_of_stage_3(monkeypatch, C):
    """SETK_P1_ITEMS = 1 gives every utterance one frame range in stage 1, alone and in the
    batch, so the weights are the same; stage 3 must then write the same bits however its work
    list is cut and whoever shares the launch."""
    center = False
    ln, utts, masks = batch(C, center)
    monkeypatch.setenv("SETK_P1_ITEMS", "1")
    got = {}
    for items in ("1", "4096"):
        monkeypatch.setenv("SETK_MC_P2_ITEMS", items)
        c = new_ctx(center)
        try:
            together, st, _ = enhance(c, C, utts, [n for _, n in ln], masks)
            alone = [enhance(c, C, [u], [n], [m])[0][0] for u, (_, n), m in zip(utts, ln, masks)]
        finally:
            c.close()
        for i, (t, n) in enumerate(ln):
            assert np.array_equal(bits(together[i]), bits(alone[i])), (C, t, items)
        got[items] = together
    for i, (t, n) in enumerate(ln):
        assert np.array_equal(bits(got["1"][i]), bits(got["4096"][i])), (C, t)


@pytest.mark.parametrize("C", CHANNELS)
def test_stage_1_cut_keeps_the_covariances(monkeypatch, C):
    center = True
    ln, utts, masks = batch(C, center)
    for items in ("1", "4096"):
        monkeypatch.setenv("SETK_P1_ITEMS", items)
        c = new_ctx(center)
        try:
            _, _, taps = enhance(c, C, utts, [n for _, n in ln], masks, taps=True)
        finally:
            c.close()
        for i, (t, n) in enumerate(ln):
            parts = reference(C, t, n, center)
            es, en = rel_rms(taps["Rs"][i], parts["Rs"]), rel_rms(taps["Rn"][i], parts["Rn"])
            assert es < COVAR_TOL and en < COVAR_TOL, (C, t, items, es, en)
