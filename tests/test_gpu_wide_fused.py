"""
setk_enhance_batch(_taps) for 9 to 16 channels (csrc/wide.hip: covariances on the fp32 matrix
cores, the beamformer on the bin-major spectra) against the oracle, and the engine's routing to it.
What is compared with what, and the measured errors: tests/PARITY_NOTES_WIDE.md.

The tolerances are the project's own for the same quantities: covariances rel_rms < 1e-5 and
exactly Hermitian (test_gpu_wide.py), weights < 2e-4 against the complex128 oracle (the same file's
kind table), waveforms < 1e-3, the two engine paths < 1e-4 (test_gpu_api.py).

Weights and waveforms are compared where the noise covariance is well posed, cond(Rn) < 1e4 in
float64.  The inputs (a point source in spatially white noise under an IRM mask kept inside
[0.05, 0.95]) make EVERY bin well posed as soon as there are more frames than channels, and the test
asserts that; with T = 1 or 3 frames Rn has rank <= T < C, no input can make a bin well posed, and
those sizes check the covariances, the status, finiteness and (below) bit-identity.
"""
import hashlib

import numpy as np
import pytest

from conftest import load_golden, rel_rms
from oracle import np_oracle as o

pytestmark = pytest.mark.gpu
F, HOP = 257, 256
STFT_KW = dict(frame_len=512, frame_hop=HOP, window="hann", center=True)


def samples_for(T, center=True):
    """A length with exactly T frames that is not a multiple of the hop.  The centred transform
    reflects n_fft / 2 samples at either end, so its shortest signal has two frames: T = 1 is a
    signal of one window under center = False."""
    return HOP * (T - 1) + 100 + (0 if center else 512)


def new_ctx(center):
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, HOP, 512, center)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_nc():
    c = new_ctx(False)
    yield c
    c.close()


def utterance(seed, C, T, center=True):
    assert center or T >= 1
    mix, sp, nz = o.synth_utterance(seed, C, samples_for(T, center), return_parts=True)
    mask = (0.05 + 0.9 * o.irm_mask(sp, nz, center=center)).astype(np.float32)
    assert mask.shape == (T, F), (mask.shape, T)
    return mix, mask


def run(c, opts, C, utts, itfs=None, taps=True, pcm16=False):
    """One batched call on device-resident inputs.  utts: [(mix C x N, mask T x F)].  Returns waves,
    status, taps (numpy)."""
    import torch
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    n = len(utts)
    a = [torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(dev) for m, _ in utts]
    ms = [torch.from_numpy(np.ascontiguousarray(k)).to(dev) for _, k in utts]
    mi = [torch.from_numpy(np.ascontiguousarray(k, dtype=np.float32)).to(dev) for k in itfs] if itfs else None
    ns = [m.shape[1] for m, _ in utts]
    outs = [torch.zeros(max(c.istft_num_samples(c.num_frames(k)), 1), dtype=torch.int16 if pcm16 else torch.float32,
                        device=dev) for k in ns]
    tp = None
    if taps:
        tp = dict(Rs=torch.zeros((n, F, C, C), dtype=torch.complex64, device=dev),
                  Rn=torch.zeros((n, F, C, C), dtype=torch.complex64, device=dev),
                  weight=torch.zeros((n, F, C), dtype=torch.complex64, device=dev),
                  maxabs=torch.zeros(n, dtype=torch.float32, device=dev))
    if pcm16:
        opts = _ffi.BfOpts(kind=opts.kind, flags=opts.flags | _ffi.FLAG_OUT_PCM16, pmwf_beta=opts.pmwf_beta,
                           pmwf_ref=opts.pmwf_ref, rank1=opts.rank1)
    st = c.enhance_batch(opts, C, [t.data_ptr() for t in a], ns, [t.data_ptr() for t in ms],
                         [t.data_ptr() for t in mi] if mi else None, [t.data_ptr() for t in outs], taps=tp)
    torch.cuda.synchronize()
    waves = [t.cpu().numpy()[:c.istft_num_samples(c.num_frames(k))] for t, k in zip(outs, ns)]
    return waves, st, ({k: v.cpu().numpy() for k, v in tp.items()} if tp else None)


def kind_table(C):
    from setk_amd import _ffi
    return [
        ("mvdr", _ffi.BF_MVDR, {}, dict(kind="mvdr"),
         lambda Rs, Rn, Ry: o.mvdr_weight(Rs, Rn, gauge=True)),
        ("gevd", _ffi.BF_GEVD, {}, dict(kind="gevd"),
         lambda Rs, Rn, Ry: o.gevd_weight(Rs, Rn, gauge=True)),
        ("pmwf0_ref0", _ffi.BF_PMWF, dict(pmwf_ref=0), dict(kind="pmwf-0", pmwf_ref=0),
         lambda Rs, Rn, Ry: o.pmwf_weight(Rs, Rn, beta=0, ref_channel=0)),
        ("pmwf1_ref", _ffi.BF_PMWF, dict(pmwf_beta=1.0, pmwf_ref=C - 2), dict(kind="pmwf-1", pmwf_ref=C - 2),
         lambda Rs, Rn, Ry: o.pmwf_weight(Rs, Rn, beta=1, ref_channel=C - 2)),
        ("mpdr", _ffi.BF_MPDR, {}, dict(kind="mpdr"),
         lambda Rs, Rn, Ry: o.mpdr_weight(Rs, Ry, gauge=True)),
        ("mpdr_whiten", _ffi.BF_MPDR_WHITEN, {}, dict(kind="mpdr-whiten"),
         lambda Rs, Rn, Ry: o.mpdr_weight(Rs, Ry, Rn=Rn, gauge=True)),
    ]


@pytest.mark.parametrize("T", [1, 3, 63, 64, 65, 129])
@pytest.mark.parametrize("C", [9, 12, 16])
def test_taps_weights_and_waveform(ctx, ctx_nc, C, T):
    """T: the odd frame of an instruction pair and 1 to 3 frames of pitch padding (1, 3, 63, 65, 129),
    both sides of the 64-frame transform tile (63, 64, 65) and the first frame of a second
    128-frame covariance slab (129).  T = 1 runs under center = False (samples_for)."""
    from setk_amd import _ffi
    center = T > 1
    if not center:
        ctx = ctx_nc
    kw_c = dict(STFT_KW, center=center)
    mix, mask = utterance(300 + 10 * C + T, C, T, center)
    obs = o.multichannel_stft(mix, transpose=False, **kw_c)
    assert obs.shape == (C, F, T)
    Rs_ref = o.compute_covar(obs, mask).astype(np.complex64)
    Rn_ref = o.compute_covar(obs, 1 - mask).astype(np.complex64)
    Ry_ref = o.compute_covar(obs, np.ones_like(mask)).astype(np.complex64)
    Rs128, Rn128, Ry128 = (m.astype(np.complex128) for m in (Rs_ref, Rn_ref, Ry_ref))
    ev = np.linalg.eigvalsh(Rn128)
    good = ev[:, 0] * 1e4 > ev[:, -1]
    if T > C:
        assert good.all(), (C, T, int(good.sum()))  # no bin is left out
    for kname, kind, kw, okw, ref_fn in kind_table(C):
        for ban in (False, True):
            if ban and kind == _ffi.BF_MPDR:
                continue
            opts = _ffi.BfOpts(kind=kind, flags=_ffi.FLAG_CLAMP_MASK | (_ffi.FLAG_BAN if ban else 0),
                               pmwf_beta=kw.get("pmwf_beta", 0.0), pmwf_ref=kw.get("pmwf_ref", -1), rank1=0)
            (wave,), st, tp = run(ctx, opts, C, [(mix, mask)])
            tag = (C, T, kname, ban)
            assert st == [0], tag
            Rs, Rn, w = tp["Rs"][0], tp["Rn"][0], tp["weight"][0]
            e_s, e_n = rel_rms(Rs, Rs_ref), rel_rms(Rn, Rn_ref)
            print(f"[wide {tag}] Rs {e_s:.2e} Rn {e_n:.2e}", end="")
            assert e_s < 1e-5 and e_n < 1e-5, tag
            assert np.max(np.abs(Rs - np.conj(np.transpose(Rs, (0, 2, 1))))) == 0, tag
            assert np.max(np.abs(Rn - np.conj(np.transpose(Rn, (0, 2, 1))))) == 0, tag
            assert tp["maxabs"][0] == np.max(np.abs(mix)), tag
            assert np.isfinite(w).all() and np.isfinite(wave).all(), tag
            assert wave.shape == (HOP * (T - 1) + (0 if center else 512),), tag
            if not good.any():
                print()
                continue
            # The complex128 oracle on the float32 matrices the solve read (the taps; Ry has no tap),
            # as test_wide_covar_pevd_weights evaluates its kind table on the matrices it hands to the
            # device.  On the ORACLE's covariances instead (printed as w*), the 2e-7 between the two
            # sets of covariances is multiplied by the pencil's eigenvalue gap for the eigenvector
            # kinds (GEVD, MPDR-whiten: up to 7e-4 measured), which says nothing about the solve.
            Rs_t, Rn_t = Rs.astype(np.complex128), Rn.astype(np.complex128)
            wref = ref_fn(Rs_t, Rn_t, Ry128)
            wfar = ref_fn(Rs128, Rn128, Ry128)
            if ban:
                wref, wfar = o.do_ban(wref, Rn_t), o.do_ban(wfar, Rn128)
            e_w = rel_rms(w[good], wref[good])
            print(f" w* {rel_rms(w[good], wfar[good]):.2e}", end="")
            ref = o.enhance_utterance(mix, mask, ban=ban, gauge=True, center=center, **okw)
            e_y = rel_rms(wave, ref) if good.all() else float("nan")
            print(f" w {e_w:.2e} wave {e_y:.2e}")
            assert e_w < 2e-4, (tag, e_w)
            if good.all():
                assert wave.shape == ref.shape and e_y < 1e-3, (tag, e_y)


def test_snr_selected_reference_and_rank1(ctx):
    """PMWF with the SNR-selected reference channel, plain and with either rank-1 approximation."""
    from setk_amd import _ffi
    C, T = 12, 65
    mix, mask = utterance(411, C, T)
    for name, rank1 in (("", _ffi.RANK1_NONE), ("eig", _ffi.RANK1_EIG), ("gev", _ffi.RANK1_GEV)):
        opts = _ffi.BfOpts(kind=_ffi.BF_PMWF, flags=_ffi.FLAG_CLAMP_MASK, pmwf_beta=0.0, pmwf_ref=-1, rank1=rank1)
        (wave,), st, _ = run(ctx, opts, C, [(mix, mask)])
        ref = o.enhance_utterance(mix, mask, kind="pmwf-0", pmwf_ref=-1, rank1_appro=name)
        print(f"[wide pmwf-0 ref=-1 rank1={name!r}] wave {rel_rms(wave, ref):.2e}")
        assert st == [0] and rel_rms(wave, ref) < 1e-3, (name, rel_rms(wave, ref))


def test_interferer_mask_and_post_mask(ctx):
    from setk_amd import _ffi
    C, T = 12, 70
    mix, mask = utterance(512, C, T)
    rng = np.random.default_rng(5)
    itf = np.clip(1 - mask + 0.05 * rng.standard_normal(mask.shape), 0.02, 1.5).astype(np.float32)
    obs = o.multichannel_stft(mix, transpose=False, **STFT_KW)
    for post in (False, True):
        opts = _ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_POST_MASK if post else 0, pmwf_ref=-1)
        (wave,), st, tp = run(ctx, opts, C, [(mix, mask)], itfs=[itf])
        assert st == [0]
        assert rel_rms(tp["Rs"][0], o.compute_covar(obs, mask)) < 1e-5
        assert rel_rms(tp["Rn"][0], o.compute_covar(obs, itf)) < 1e-5
        ref = o.enhance_utterance(mix, mask, kind="mvdr", itf_mask=itf, post_mask=post, gauge=True)
        print(f"[wide itf post={post}] wave {rel_rms(wave, ref):.2e}")
        assert rel_rms(wave, ref) < 1e-3, (post, rel_rms(wave, ref))


def test_ragged_batch_is_bit_identical_to_single_runs(ctx_nc):
    """Five utterances of different lengths and one of a single frame (hence center = False)."""
    from setk_amd import _ffi
    C, ctx = 16, ctx_nc
    utts = [utterance(600 + T, C, T, False) for T in (130, 1, 64, 257, 77, 5)]
    opts = _ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK, pmwf_ref=-1)
    for pcm16 in (False, True):
        waves, st, tp = run(ctx, opts, C, utts, pcm16=pcm16)
        assert st == [0] * len(utts)
        for u, utt in enumerate(utts):
            (w1,), st1, tp1 = run(ctx, opts, C, [utt], pcm16=pcm16)
            assert st1 == [0]
            assert w1.dtype == (np.int16 if pcm16 else np.float32)
            assert np.array_equal(w1, waves[u]), (u, pcm16)
            for k in ("Rs", "Rn", "weight", "maxabs"):
                assert tp1[k][0].tobytes() == tp[k][u].tobytes(), (u, k, pcm16)


def test_stale_scratch_does_not_matter():
    """A long utterance, then a short one on the same context: the short one finds the long one's
    spectra behind its last frame and the long one's slabs in the arena."""
    from setk_amd import _ffi
    C = 12
    long_utt, short_utt = utterance(700, C, 200), utterance(701, C, 13)
    opts = _ffi.BfOpts(kind=_ffi.BF_GEVD, flags=_ffi.FLAG_CLAMP_MASK, pmwf_ref=-1)
    res = []
    for warm in (True, False):
        c = _ffi.Context(0)
        c.stft_plan(512, HOP, 512, True)
        if warm:
            run(c, opts, C, [long_utt])
        res.append(run(c, opts, C, [short_utt]))
        c.close()
    (wa,), sta, ta = res[0]
    (wb,), stb, tb = res[1]
    assert sta == stb == [0] and np.array_equal(wa, wb)
    for k in ta:
        assert ta[k].tobytes() == tb[k].tobytes(), k


def test_engine_routes_wide_batches_to_the_batched_call(monkeypatch):
    from setk_amd.engine import BatchEnhancer
    C = 12
    utts = [utterance(800 + i, C, T) + (None,) for i, T in enumerate((40, 90, 33, 64, 150))]
    e = BatchEnhancer(beamformer="mvdr")
    calls = []
    real = e.ctx.enhance_batch
    monkeypatch.setattr(e.ctx, "enhance_batch", lambda *a, **k: (calls.append(len(a[2])), real(*a, **k))[1])
    fused = e.enhance(utts)
    assert calls == [len(utts)]
    unfused = [None] * len(utts)
    e._run_unfused(utts, list(range(len(utts))), C, False, unfused)
    for (wf, sf), (wu, su) in zip(fused, unfused):
        assert sf == su == 0 and wf.shape == wu.shape
        print(f"[wide engine] batched against unfused {rel_rms(wf, wu):.2e}")
        assert rel_rms(wf, wu) < 1e-4, rel_rms(wf, wu)
    # a byte cap that cuts the five utterances into three sub-batches: same bits, same order
    need = [e._wide_bytes(u[0], C) for u in utts]
    del calls[:]
    e.max_wide_bytes = max(need[0] + need[1], need[2] + need[3]) + 1
    assert need[0] + need[1] + need[2] > e.max_wide_bytes and need[2] + need[3] + need[4] > e.max_wide_bytes
    cut = e.enhance(utts)
    assert calls == [2, 2, 1]
    for (wf, _), (wc, sc) in zip(fused, cut):
        assert sc == 0 and np.array_equal(wf, wc)
    # the VAD filter needs the spectrogram on the host: unfused as before
    del calls[:]
    v = BatchEnhancer(beamformer="mvdr", vad_proportion=0.9, ctx=e.ctx)
    (wv, sv), = v.enhance(utts[:1])
    assert calls == [] and sv == 0 and np.isfinite(wv).all()


def test_sixteen_channel_doc_recording_through_the_batched_call(ctx):
    """tests/golden/doc_wide_16ch.npz with the reference's mask: finite, zero status, and weights
    against the oracle on the well-posed bins -- the selection and the bar of
    test_gpu_wide.py::test_sixteen_channel_real_recording_against_the_reference_clis."""
    from setk_amd import _ffi
    g = load_golden("doc_wide_16ch.npz")
    samps = (g["pcm"].astype(np.float32) / 32768.0).T.copy()
    mask = np.ascontiguousarray(g["mask"], dtype=np.float32)
    C = samps.shape[0]
    assert C == 16
    opts = _ffi.BfOpts(kind=_ffi.BF_PMWF, flags=_ffi.FLAG_CLAMP_MASK, pmwf_beta=0.0, pmwf_ref=0)
    (wave,), st, tp = run(ctx, opts, C, [(samps, mask)])
    assert st == [0] and np.isfinite(wave).all() and np.abs(wave).max() > 0
    w = tp["weight"][0]
    assert np.isfinite(w).all()
    stft = o.multichannel_stft(samps, transpose=False, **STFT_KW)
    Rs = o.compute_covar(stft, np.minimum(mask, 1)).astype(np.complex64)
    Rn = o.compute_covar(stft, 1 - np.minimum(mask, 1)).astype(np.complex64)
    ev = np.linalg.eigvalsh(Rn.astype(np.complex128))
    good = ev[:, 0] * 1e4 > ev[:, -1]
    wo = o.pmwf_weight(Rs.astype(np.complex128), Rn.astype(np.complex128), ref_channel=0)
    print(f"[16ch doc, batched] well-posed bins {int(good.sum())} of {F}: weights {rel_rms(w[good], wo[good]):.2e}")
    assert good.sum() >= 20
    assert rel_rms(w[good], wo[good]) < 1e-3
    assert np.abs(w).max() < 1e4


def test_eight_channels_keep_their_bits(ctx):
    """The call for up to 8 channels does not pass through the wide path: the same utterance gives
    the same bits alone and inside a batch that is followed by a 12-channel call on the same
    context (tools/ab_bits.py compares builds; its hashes are in tests/PARITY_NOTES_WIDE.md)."""
    from setk_amd import _ffi
    opts = _ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK, pmwf_ref=-1)
    narrow = [utterance(900 + i, 8, T) for i, T in enumerate((70, 33))]
    first = run(ctx, opts, 8, narrow)
    run(ctx, opts, 12, [utterance(910, 12, 50)])
    again = run(ctx, opts, 8, narrow)
    for a, b in zip(first[0], again[0]):
        assert np.array_equal(a, b)
    h = hashlib.sha256(b"".join(w.tobytes() for w in first[0])).hexdigest()[:24]
    print(f"[narrow C=8] {h}")
    for k in first[2]:
        assert first[2][k].tobytes() == again[2][k].tobytes(), k
