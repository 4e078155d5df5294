"""
GPU parity of the fused hot path (setk_enhance_batch) against the CPU oracle
and the reference's golden vectors.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, rms, rel_rms, rel_rms_outside_bins
from oracle import np_oracle as o
from oracle import make_golden as mg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, 256, 512, True)
    yield c
    c.close()


def run_batch(ctx, opts, utts, masks, itf=None, pcm16=False):
    """utts: list of C x N float32, masks: list of T x F float32."""
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    C = utts[0].shape[0]
    a = [torch.from_numpy(np.ascontiguousarray(u)).to(dev) for u in utts]
    m = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in masks]
    it = None
    if itf is not None:
        it = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in itf]
    outs = []
    for u in utts:
        T = ctx.num_frames(u.shape[1])
        L = ctx.istft_num_samples(T)
        outs.append(torch.empty(L, dtype=torch.int16 if pcm16 else torch.float32, device=dev))
    if pcm16:
        opts.flags |= _ffi.FLAG_OUT_PCM16
    st = ctx.enhance_batch(opts, C, [t.data_ptr() for t in a], [u.shape[1] for u in utts],
                           [t.data_ptr() for t in m],
                           None if it is None else [t.data_ptr() for t in it],
                           [t.data_ptr() for t in outs])
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], st


def run_one_with_weights(ctx, opts, samps, mask):
    """One utterance through setk_enhance_batch_taps: (wave, status, weights F x C)."""
    dev = torch.device("cuda:0")
    C, N = samps.shape
    a = torch.from_numpy(np.ascontiguousarray(samps)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev)
    out = torch.empty(ctx.istft_num_samples(ctx.num_frames(N)), dtype=torch.float32, device=dev)
    w = torch.empty((1, 257, C), dtype=torch.complex64, device=dev)
    st = ctx.enhance_batch(opts, C, [a.data_ptr()], [N], [m.data_ptr()], None, [out.data_ptr()],
                           taps=dict(weight=w))
    torch.cuda.synchronize()
    return out.cpu().numpy(), st, w[0].cpu().numpy()


def well_posed_weight_errors(w, parts, cond_max=1e4):
    """Per-bin relative deviation of the device weights from the oracle's, over the bins whose
    noise covariance is well conditioned (cond(Rn) < cond_max: the float32 covariances carry a
    relative noise of ~1e-7, a solve amplifies it by the condition number).  A real recording
    has a few bins beyond that -- for GEV LAPACK's hegvd even refuses some and the reference's
    scipy.linalg.eig fallback answers with rounding noise of arbitrary size (libs/beamformer.py:
    54-59), which then dominates the WAVEFORM (and its max-abs renorm) -- so the comparison is
    made where it means something: on the weights, bin by bin."""
    Rn = parts["Rn"].astype(np.complex128)
    cond = np.linalg.cond(Rn)
    sel = cond < cond_max
    ref = parts["weight"]
    err = np.linalg.norm(w - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-30)
    return err[sel], int(sel.sum()), cond


KINDS = {
    "mvdr": dict(kind=0), "gevd": dict(kind=1),
    "pmwf-0": dict(kind=2, pmwf_beta=0.0, pmwf_ref=-1),
    "pmwf-1": dict(kind=2, pmwf_beta=1.0, pmwf_ref=-1),
    "mpdr": dict(kind=3), "mpdr-whiten": dict(kind=4),
}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("C,N", [(4, 16000), (8, 20000), (5, 9001), (2, 7000), (1, 6000),
                                  (3, 8000), (7, 10001), (6, 5000)])
def test_enhance_matches_oracle(ctx, kind, C, N):
    from setk_amd import _ffi
    if C == 1 and kind not in ("mvdr", "pmwf-0"):
        pytest.skip("single channel: covered by mvdr/pmwf")
    mix, sp, nz = o.synth_utterance(20 + C, C, N, return_parts=True)
    mask = o.irm_mask(sp, nz)
    opts = _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind])
    (wav,), st = run_batch(ctx, opts, [mix], [mask])
    assert st == [0]
    ref = o.enhance_utterance(mix, mask, kind=kind, gauge=True)
    assert wav.shape == ref.shape
    assert rms(wav, ref) / rms(ref) < 1e-3, rms(wav, ref) / rms(ref)


@pytest.mark.parametrize("switch", ["SETK_MC_PASS1=1", "SETK_MC_PASS2=0", "SETK_LEGACY_FFT=1"])
@pytest.mark.parametrize("kind,C,N", [("mvdr", 8, 20000), ("gevd", 4, 16000), ("pmwf-0", 2, 7000),
                                      ("mvdr", 1, 6000), ("mpdr", 8, 9001)])
def test_alternative_kernel_forms_hold_the_same_bar(ctx, switch, kind, C, N):
    """The forms behind the environment switches are products too: pass 1 with its transforms
    on the matrix cores (opt-in: slower), pass 2 as fp32 butterflies, both
    passes as butterflies.  Each against the oracle at the 1e-3 bar, and against the default
    form at 1e-5 (the two transform arithmetics differ by 1e-7 per spectrum)."""
    import os
    from setk_amd import _ffi
    mix, sp, nz = o.synth_utterance(60 + C, C, N, return_parts=True)
    mask = o.irm_mask(sp, nz)
    opts = lambda: _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK | _ffi.FLAG_POST_MASK, **KINDS[kind])
    (base,), st = run_batch(ctx, opts(), [mix], [mask])
    assert st == [0]
    name, val = switch.split("=")
    old = os.environ.get(name)
    os.environ[name] = val
    try:
        # (SETK_LEGACY_FFT is read when the transform is planned: its own handle)
        c2 = _ffi.Context(0)
        c2.stft_plan(512, 256, 512, True)
        (wav,), st = run_batch(c2, opts(), [mix], [mask])
        c2.close()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old
    assert st == [0]
    ref = o.enhance_utterance(mix, mask, kind=kind, gauge=True, post_mask=True)
    assert rms(wav, ref) / rms(ref) < 1e-3, rms(wav, ref) / rms(ref)
    assert rms(wav, base) / rms(base) < 1e-5, rms(wav, base) / rms(base)


@pytest.mark.parametrize("flags", ["ban", "post", "itf", "pcm16"])
def test_enhance_flags(ctx, flags):
    from setk_amd import _ffi
    mix, sp, nz = o.synth_utterance(31, 6, 12000, return_parts=True)
    mask = o.irm_mask(sp, nz)
    f = _ffi.FLAG_CLAMP_MASK
    kw = {}
    itf = None
    if flags == "ban":
        f |= _ffi.FLAG_BAN
        kw["ban"] = True
    if flags == "post":
        f |= _ffi.FLAG_POST_MASK
        kw["post_mask"] = True
    if flags == "itf":
        itf = np.random.default_rng(3).uniform(0.1, 0.9, size=mask.shape).astype(np.float32)
        f = 0
        kw["itf_mask"] = itf
    opts = _ffi.BfOpts(kind=0, flags=f)
    (wav,), st = run_batch(ctx, opts, [mix], [mask], itf=None if itf is None else [itf],
                           pcm16=(flags == "pcm16"))
    ref = o.enhance_utterance(mix, mask, kind="mvdr", gauge=True, **kw)
    if flags == "pcm16":
        assert wav.dtype == np.int16
        assert np.max(np.abs(wav - np.rint(ref.astype(np.float64) * 32767))) <= 1
    else:
        assert rms(wav, ref) / rms(ref) < 1e-3


def test_enhance_ragged_batch(ctx):
    """Several utterances of different length in one call; results equal the
    one-at-a-time results bit for bit (utterances are independent)."""
    from setk_amd import _ffi
    lens = [5000, 16000, 7777, 30001, 12000]
    utts, masks = [], []
    for i, n in enumerate(lens):
        mix, sp, nz = o.synth_utterance(50 + i, 4, n, return_parts=True)
        utts.append(mix)
        masks.append(o.irm_mask(sp, nz))
    opts = _ffi.BfOpts(kind=0, flags=_ffi.FLAG_CLAMP_MASK)
    outs, st = run_batch(ctx, opts, utts, masks)
    assert st == [0] * len(lens)
    for i in range(len(lens)):
        ref = o.enhance_utterance(utts[i], masks[i], kind="mvdr", gauge=True)
        assert rms(outs[i], ref) / rms(ref) < 1e-3
        (single,), _ = run_batch(ctx, opts, [utts[i]], [masks[i]])
        assert rms(single, outs[i]) / rms(ref) < 1e-5


def test_enhance_zero_noise_mask_reports_singular(ctx):
    from setk_amd import _ffi
    mix, sp, nz = o.synth_utterance(1, 4, 8000, return_parts=True)
    mask = np.ones((32, 257), np.float32)  # noise mask 1 - m == 0 everywhere
    opts = _ffi.BfOpts(kind=0, flags=_ffi.FLAG_CLAMP_MASK)
    _, st = run_batch(ctx, opts, [mix], [mask])
    assert st == [_ffi.NUM_SINGULAR]


def resolve_gauge(enh, norm, stored):
    from test_oracle_golden import resolve_gauge as rg
    return rg(enh, norm, stored)


def test_doc_goldens_on_gpu(ctx):
    """The reference's stored doc outputs (doc/adaptive_beamformer/asset)."""
    from setk_amd import _ffi
    doc = load_golden("doc_adaptive_beamformer.npz")
    samps = (doc["egs"].astype(np.float32) / 32768.0).T.copy()
    mask = doc["cgmm_mask"]
    cases = [("pmwf_0", dict(kind=2, pmwf_ref=-1), "pmwf-0", {}),
             ("pmwf_0_eig", dict(kind=2, pmwf_ref=-1, rank1=1), "pmwf-0", dict(rank1_appro="eig")),
             ("pmwf_0_gev", dict(kind=2, pmwf_ref=-1, rank1=2), "pmwf-0", dict(rank1_appro="gev"))]
    for key, kw, okind, okw in cases:
        opts = _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **kw)
        (wav,), st = run_batch(ctx, opts, [samps], [mask])
        assert st == [0]
        stored = doc[key].astype(np.float64) / 32768.0
        err = rms(np.rint(wav.astype(np.float64) * 32767) / 32768.0, stored)
        assert err / rms(stored) < 1e-3, (key, err)
    # gauge-carrying kinds: compare with the gauge-fixed oracle (the stored wavs
    # carry LAPACK's arbitrary signs, pinned by tests/test_oracle_golden.py)
    for kind, kid in (("mvdr", 0), ("gevd", 1)):
        opts = _ffi.BfOpts(kind=kid, flags=_ffi.FLAG_CLAMP_MASK)
        (wav,), st = run_batch(ctx, opts, [samps], [mask])
        ref = o.enhance_utterance(samps, mask, kind=kind, gauge=True)
        assert rms(wav, ref) / rms(ref) < 1e-3, kind


@pytest.mark.parametrize("N,hop,center", [(300, 256, True), (513, 256, True), (700, 256, True),
                                          (512, 256, False), (1100, 256, False),
                                          (6000, 128, True), (6000, 64, True), (6000, 512, True),
                                          (6000, 384, True), (6000, 160, False), (6001, 100, True)])
def test_enhance_edge_geometries(N, hop, center):
    """Very short utterances (1-3 frames), hops from 64 to n_fft, center on/off:
    the fused kernels against the oracle (MVDR needs T >= C for a full-rank
    noise covariance, so short cases use 2 channels and PMWF)."""
    from setk_amd import _ffi
    C = 2
    c2 = _ffi.Context(0)
    try:
        c2.stft_plan(512, hop, 512, center)
        mix, sp, nz = o.synth_utterance(100 + hop, C, N, return_parts=True)
        kw = dict(frame_len=512, frame_hop=hop, center=center, window="hann")
        mask = o.irm_mask(sp, nz, frame_len=512, frame_hop=hop, center=center)
        mask = (0.1 + 0.8 * mask).astype(np.float32)
        T = mask.shape[0]
        assert T == c2.num_frames(N)
        kind = "mvdr" if T >= 8 else "pmwf-0"
        opts = _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind])
        (wav,), st = run_batch(c2, opts, [mix], [mask])
        ref = o.enhance_utterance(mix, mask, kind=kind, gauge=True, **kw)
        assert wav.shape == ref.shape
        if T >= 3:
            assert st == [0]
            err = rms(wav, ref) / max(rms(ref), 1e-12)
            assert err < 1e-3, (N, hop, center, err)
        else:
            # 1-2 frames: rank-deficient covariances (and, without centring, samples
            # divided by window^2 ~ 1e-9): nothing meaningful to compare, but the
            # kernels must run and produce finite output of the right length
            assert np.all(np.isfinite(wav))
    finally:
        c2.close()


def test_randomised_geometry_sweep():
    """tools/stress.py: 30 random draws of channels (1-8), ragged batch, hop
    (64..512), centring and beamformer against the oracle."""
    import subprocess
    import sys
    from conftest import ROOT
    import os
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stress.py"), "30", "7"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "CHECK" not in r.stdout


def test_batch_is_deterministic(ctx):
    """The fused path has no order-dependent reductions for MVDR / GEV (partial
    slabs are summed in a fixed order, the only atomics are max): two runs of a
    ragged batch return bit-identical waveforms."""
    from setk_amd import _ffi
    utts, masks = [], []
    for i, (C, N) in enumerate([(8, 40000), (8, 23001), (8, 61000)]):
        mix, sp, nz = o.synth_utterance(70 + i, C, N, return_parts=True)
        utts.append(mix)
        masks.append(o.irm_mask(sp, nz))
    # pmwf-0 with the SNR-selected reference channel: the per-bin SNR terms are summed
    # in bin order (an atomic accumulation could flip the argmax between runs)
    for kind in ("mvdr", "gevd", "pmwf-0"):
        opts = _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind])
        a, st_a = run_batch(ctx, opts, utts, masks)
        b, st_b = run_batch(ctx, opts, utts, masks)
        assert st_a == [0, 0, 0] and st_b == [0, 0, 0]
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_full_size_properties(ctx):
    """BASELINE configs[2] utterance size (8 ch x 30 s): size-independent properties
    of the fused path on top of the direct oracle comparison at this size
    (tests/test_gpu_baseline_sizes.py) --
    scale equivariance, channel-permutation invariance of PMWF with a fixed physical
    reference microphone, independence of the batch an utterance travels in, and
    the single-channel identity."""
    from setk_amd import _ffi
    N = 480000
    mix, sp, nz = o.synth_utterance(5, 8, N, return_parts=True)
    c2 = ctx
    T = c2.num_frames(N)
    rng = np.random.default_rng(3)
    mask = rng.uniform(0.05, 0.95, size=(T, 257)).astype(np.float32)
    opts = lambda: _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS["mvdr"])  # noqa: E731
    (y,), st = run_batch(c2, opts(), [mix], [mask])
    assert st == [0] and y.shape == (N,) and np.all(np.isfinite(y))
    # output is renormalised to max |input|
    assert abs(np.max(np.abs(y)) - np.max(np.abs(mix))) < 1e-4 * np.max(np.abs(mix))
    # scale equivariance
    (y2,), _ = run_batch(c2, opts(), [0.5 * mix], [mask])
    assert rms(y2, 0.5 * y) / rms(y) < 1e-4
    # channel permutation: PMWF referenced to the same physical microphone (MVDR's
    # output is referenced to the gauge channel 0, so it is not permutation invariant)
    perm = np.array([3, 0, 7, 1, 6, 2, 5, 4])
    pm = lambda ref: _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, kind=2, pmwf_beta=0.0,  # noqa: E731
                                 pmwf_ref=ref)
    (ya,), sa = run_batch(c2, pm(2), [mix], [mask])
    (yb,), sb = run_batch(c2, pm(int(np.where(perm == 2)[0][0])),
                          [np.ascontiguousarray(mix[perm])], [mask])
    assert sa == [0] and sb == [0]
    assert rms(yb, ya) / rms(ya) < 1e-4
    # same utterance inside a ragged batch (different work split)
    others = [o.synth_utterance(6, 8, 200000), o.synth_utterance(7, 8, 333333)]
    masks = [rng.uniform(0.05, 0.95, size=(c2.num_frames(u.shape[1]), 257)).astype(np.float32)
             for u in others]
    ys, st = run_batch(c2, opts(), [others[0], mix, others[1]], [masks[0], mask, masks[1]])
    assert st == [0, 0, 0]
    assert rms(ys[1], y) / rms(y) < 1e-5
    # one channel: the beamformer is the identity up to the renorm
    (y1,), st = run_batch(c2, opts(), [mix[:1]], [mask])
    assert st == [0]
    x = mix[0, :y1.shape[0]]
    assert rms(y1, x * (np.max(np.abs(mix[0])) / np.max(np.abs(x)))) / rms(x) < 1e-4


@pytest.mark.parametrize("kind", ["pmwf-0", "mvdr", "gevd"])
def test_rank_deficient_real_recording_through_the_fused_path(ctx, kind):
    """The first 8 channels of doc/ssl/asset/egs.wav (two or three coherent sources: the noise
    covariance is singular to float32 in ~100 bins).  The reference goes through on LAPACK's
    noise-level pivots and its output is a rounding artefact there (it moves by O(1) under a
    1e-7 input perturbation); the fused path must go through too -- no status, nothing
    non-finite, bounded weights (the floored-pivot Cholesky of rounds 1 - 3 grew |L| by 1e10 on
    this input) -- agree with the oracle where the problem is well posed, and stay within the
    reference's own sensitivity elsewhere."""
    from setk_amd import _ffi
    g = load_golden("doc_wide_16ch.npz")
    samps = np.ascontiguousarray((g["pcm"][:, :8].astype(np.float32) / 32768.0).T)
    mask = g["mask"]
    opts = _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind])
    (wav,), st = run_batch(ctx, opts, [samps], [mask])
    assert st == [0] and np.isfinite(wav).all()
    assert np.abs(wav).max() > 1e-4
    ref, parts = o.enhance_utterance(samps, mask, kind=kind, gauge=True, return_parts=True)
    if kind == "gevd":
        # 94 of the 257 pencils are singular for LAPACK's hegvd and the reference's
        # scipy.linalg.eig fallback answers with rounding noise (it does NOT skip the utterance:
        # tests/golden/ref_skipset.json); the 146 well-conditioned bins are compared on the weights
        _, st2, w = run_one_with_weights(ctx, _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind]), samps, mask)
        err, n_sel, cond = well_posed_weight_errors(w, parts)
        print(f"[8ch real, gevd] {n_sel} bins with cond(Rn) < 1e4: weight error max {err.max():.3g}, "
              f"median {np.median(err):.3g}; cond(Rn) up to {cond.max():.3g} elsewhere")
        assert st2 == [0] and n_sel > 120 and err.max() < 2e-3 and np.median(err) < 1e-4
        return
    rng = np.random.default_rng(1)
    moved = o.enhance_utterance(samps * (1 + 1e-7 * rng.standard_normal(samps.shape)).astype(np.float32),
                                mask, kind=kind, gauge=True)
    sens = rms(moved, ref) / rms(ref)
    err = rms(wav, ref) / rms(ref)
    print(f"[8ch real, {kind}] vs oracle {err:.3g}; oracle under a 1e-7 input perturbation {sens:.3g}")
    assert err < max(1e-3, 3.0 * sens)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ["noisy", "2spk"])
def test_real_recordings_with_the_reference_masks(ctx, name, kind):
    """The reference's spatial-clustering recordings (5 and 7 channels, 4 s) with the masks the
    unmodified reference estimated for them (tests/golden/doc_spatial_clustering.npz), through
    every beamformer of the fused path against the oracle.  Real rooms are not the synthetic
    scenes of the other tests: a few bins of `noisy` have a noise covariance at the float32
    rank floor, where the bar is the oracle's own sensitivity to a 1e-7 input perturbation."""
    from setk_amd import _ffi
    g = load_golden("doc_spatial_clustering.npz")
    samps = np.ascontiguousarray((g["pcm_" + name].astype(np.float32) / 32768.0).T)
    mask = g["saved_" + name] if name == "noisy" else g["saved_2spk"][0]
    opts = _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind])
    (wav,), st = run_batch(ctx, opts, [samps], [mask])
    assert st == [0] and np.isfinite(wav).all()
    ref, parts = o.enhance_utterance(samps, mask, kind=kind, gauge=True, return_parts=True)
    if kind in ("gevd", "mpdr-whiten") and len(o.gev_fallback_bins(parts["Rs"], parts["Rn"])):
        # `noisy`: two pencils (bins 2, 4) are singular for LAPACK's hegvd; the reference's
        # scipy.linalg.eig fallback answers there with rounding noise that dominates the wave
        # (and does NOT skip the utterance: tests/golden/ref_skipset.json).  The other bins --
        # 252 of 257 have cond(Rn) < 1e4 -- are compared on the weights.
        _, st2, w = run_one_with_weights(ctx, _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind]), samps, mask)
        err, n_sel, cond = well_posed_weight_errors(w, parts)
        print(f"[real {name}, {kind}] {n_sel} bins with cond(Rn) < 1e4: weight error max {err.max():.3g}, "
              f"median {np.median(err):.3g}")
        assert st2 == [0] and n_sel > 240 and err.max() < 2e-3 and np.median(err) < 1e-4
        return
    err = rms(wav, ref) / rms(ref)
    bar = 1e-3
    if err >= bar:
        rng = np.random.default_rng(2)
        moved = o.enhance_utterance(samps * (1 + 1e-7 * rng.standard_normal(samps.shape)).astype(np.float32),
                                    mask, kind=kind, gauge=True)
        bar = 3.0 * rms(moved, ref) / rms(ref)
    print(f"[real {name}, {kind}] vs oracle {err:.3g} (bar {bar:.3g})")
    assert err < bar


@pytest.mark.parametrize("kind", ["mvdr", "gevd", "mpdr", "mpdr-whiten", "pmwf-1"])
def test_fused_partial_reduction_equals_the_finalize_kernel(ctx, kind):
    """With few partial slabs per utterance the solve sums pass 1's slabs itself
    (covar_finalize_kernel's launch falls away); SETK_FUSED_REDUCE=0 keeps the separate kernel.
    Same sums, same order, same float32 expressions: the waveforms are equal bit for bit."""
    import os
    from setk_amd import _ffi
    outs = []
    for sw in (None, "0"):
        if sw is None:
            os.environ.pop("SETK_FUSED_REDUCE", None)
        else:
            os.environ["SETK_FUSED_REDUCE"] = sw
        try:
            utts, masks = [], []
            for i, (C, N) in enumerate([(8, 40000), (8, 9000)]):
                mix, sp, nz = o.synth_utterance(300 + i, C, N, return_parts=True)
                utts.append(mix)
                masks.append(o.irm_mask(sp, nz))
            opts = _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind])
            wavs, st = run_batch(ctx, opts, utts, masks)
            assert st == [0, 0]
            outs.append(wavs)
        finally:
            os.environ.pop("SETK_FUSED_REDUCE", None)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    ref = o.enhance_utterance(utts[0], masks[0], kind=kind, gauge=True)
    assert rms(outs[0][0], ref) / rms(ref) < 1e-3


def _skipset_table():
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_skipset.json")))["table"]


@pytest.mark.parametrize("strict", [True, False])
def test_skip_set_on_singular_noise_covariances(strict):
    """Which utterances are refused (status != 0 -> LinAlgError -> the CLI's log-and-skip).
    tests/golden/ref_skipset.json is what the UNMODIFIED reference does on structurally
    singular, nearly singular and real inputs.  strict_reference=True (SETK_FLAG_STRICT_REFERENCE,
    --strict-reference true) must refuse exactly the pairs numpy.linalg.solve raises on -- and
    none of the real recordings, and never under GEV; the only tolerated difference is the
    pairs where the reference WRITES A FILE OF NaNs ('ok-nonfinite'), which the product refuses.
    The default refuses only what no regularisation can solve: an all-zero covariance."""
    from setk_amd.engine import BatchEnhancer
    table = _skipset_table()
    cases = dict(o.skipset_cases())
    cases.update(mg.skipset_real_recordings())
    zero_rn = ("ones-mask", "mask-above-one", "silence")
    wrong = []
    for kname, spec in o.SKIPSET_KINDS.items():
        eng = BatchEnhancer(beamformer=spec["kind"], rank1_appro=spec.get("rank1_appro", ""),
                            strict_reference=strict)
        for name, (samps, mask) in cases.items():
            (wav, status), = eng.enhance([(samps, mask, None)])
            refused = status != 0
            want = table[name][kname]
            if not refused:
                assert np.isfinite(wav).all(), (name, kname)
            if strict:
                ok = refused == (want == "LinAlgError") or (want == "ok-nonfinite" and refused)
            else:
                ok = refused == (name in zero_rn and not (kname == "mpdr" and name != "silence"))
            if not ok:
                wrong.append((name, kname, int(status), want))
    assert not wrong, wrong


def test_strict_reference_leaves_the_weights_alone():
    """The refusal is a status only: an utterance that passes is enhanced bit for bit as in
    the default mode (the float64 Cholesky's weights), in the batch next to a refused one."""
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, 256, 512, True)
    try:
        cases = o.skipset_cases()
        utts = [cases["plain"][0], cases["dup-channel"][0], cases["channel-x0.3"][0]]
        masks = [cases["plain"][1], cases["dup-channel"][1], cases["channel-x0.3"][1]]
        for kind in ("mvdr", "pmwf-0", "mpdr"):
            y0, st0 = run_batch(c, _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind]), utts, masks)
            y1, st1 = run_batch(c, _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK | _ffi.FLAG_STRICT_REFERENCE,
                                               **KINDS[kind]), utts, masks)
            assert st0 == [0, 0, 0] and st1 == [0, _ffi.NUM_SINGULAR, 0], (kind, st0, st1)
            assert np.array_equal(y0[0], y1[0]) and np.array_equal(y0[2], y1[2])
    finally:
        c.close()


def _enhance_pcm16(ctx, opts, frames_list, masks):
    """frames_list: int16 [N][C] arrays (a wave file's frames).  De-interleaved on the device
    (setk_pcm16_deinterleave_batch) and enhanced with SETK_FLAG_IN_PCM16: no float32 copy."""
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    C = frames_list[0].shape[1]
    src = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames_list]
    ns = [f.shape[0] for f in frames_list]
    planar = [torch.full((C, ctx.pcm16_channel_stride(n)), 12345, dtype=torch.int16, device=dev) for n in ns]
    power = torch.zeros(len(ns), dtype=torch.float64, device=dev)
    ctx.pcm16_deinterleave_batch(C, [t.data_ptr() for t in src], ns, [t.data_ptr() for t in planar],
                                 power0=power.data_ptr())
    m = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in masks]
    outs = [torch.empty(ctx.istft_num_samples(ctx.num_frames(n)), dtype=torch.float32, device=dev) for n in ns]
    opts.flags |= _ffi.FLAG_IN_PCM16
    st = ctx.enhance_batch(opts, C, [t.data_ptr() for t in planar], ns, [t.data_ptr() for t in m], None,
                           [t.data_ptr() for t in outs])
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], st, [t.cpu().numpy() for t in planar], power.cpu().numpy()


@pytest.mark.parametrize("kind", ["mvdr", "gevd", "pmwf-0", "mpdr-whiten"])
@pytest.mark.parametrize("C,lens", [(8, [20000, 9001, 33333]), (4, [16000, 5003]), (5, [7001]), (1, [6000]),
                                    (2, [12345, 4097, 8190]), (6, [10007])])
def test_pcm16_input_is_the_float_path_bit_for_bit(ctx, kind, C, lens):
    """SETK_FLAG_IN_PCM16 (SURVEY 8f-3 'int16 ingest on device'): both streaming kernels read
    the wave file's 16-bit samples (planar int16, 2 bytes per sample) and scale by 2^-15 inside
    their transforms.  Reference: read_wav's dtype='float32' read, int16 / 32768
    (libs/utils.py:80-90).  Because the scale is a power of two folded into the window tables,
    the waveform equals the float32 call on pcm / 32768 BIT FOR BIT -- and so holds the same
    1e-3 bar against the oracle on the dequantised samples.  Ragged batches, odd lengths (the
    channel stride is padded to a multiple of 8), every channel count class."""
    from setk_amd import _ffi
    if C == 1 and kind not in ("mvdr", "pmwf-0"):
        pytest.skip("single channel: covered by mvdr/pmwf")
    frames, floats, masks = [], [], []
    for i, n in enumerate(lens):
        mix, sp, nz = o.synth_utterance(700 + 10 * C + i, C, n, return_parts=True)
        pcm = np.ascontiguousarray(np.clip(np.rint(mix.T * 32767.0 * 4.0), -32768, 32767).astype(np.int16))  # [N][C]
        frames.append(pcm)
        floats.append(np.ascontiguousarray(pcm.T.astype(np.float32) / 32768.0))
        masks.append(o.irm_mask(sp, nz))
    ys, st, planar, power = _enhance_pcm16(ctx, _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind]), frames, masks)
    yf, stf = run_batch(ctx, _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind]), floats, masks)
    assert st == [0] * len(lens) and stf == st
    for i, n in enumerate(lens):
        # the planar copy: the file's samples, channel major, the padding zeroed
        assert np.array_equal(planar[i][:, :n], frames[i].T) and not planar[i][:, n:].any()
        assert abs(power[i] - float(np.sum(floats[i][0].astype(np.float64) ** 2))) <= 1e-4 * max(power[i], 1e-9)
        assert np.array_equal(ys[i], yf[i]), (kind, C, n, rms(ys[i], yf[i]) / rms(yf[i]))
    ref = o.enhance_utterance(floats[0], masks[0], kind=kind, gauge=True)
    assert rms(ys[0], ref) / rms(ref) < 1e-3


def test_pcm16_input_flags_edges_and_taps(ctx):
    """The same identity with BAN + post-mask, an interferer mask, PCM16 output, a batch that
    is cut into several frame ranges per utterance (partial slabs, carries across ranges), and
    the taps: covariances, weights and max |x| equal those of the float call."""
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    C, lens = 8, [160000, 40000]
    frames, floats, masks, itf = [], [], [], []
    for i, n in enumerate(lens):
        mix, sp, nz = o.synth_utterance(760 + i, C, n, return_parts=True)
        pcm = np.ascontiguousarray(np.rint(mix.T * 32767.0 * 2.0).astype(np.int16))  # [N][C], frame major
        frames.append(pcm)
        floats.append(np.ascontiguousarray(pcm.T.astype(np.float32) / 32768.0))
        m = o.irm_mask(sp, nz)
        masks.append(m)
        itf.append((1 - m) ** 2)
    for flags, use_itf in ((_ffi.FLAG_CLAMP_MASK | _ffi.FLAG_BAN | _ffi.FLAG_POST_MASK, False), (0, True)):
        src = [torch.from_numpy(f).to(dev) for f in frames]
        planar = [torch.empty((C, ctx.pcm16_channel_stride(n)), dtype=torch.int16, device=dev) for n in lens]
        ctx.pcm16_deinterleave_batch(C, [t.data_ptr() for t in src], lens, [t.data_ptr() for t in planar])
        fl = [torch.from_numpy(f).to(dev) for f in floats]
        m = [torch.from_numpy(x).to(dev) for x in masks]
        it = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in itf] if use_itf else None
        res = {}
        for name, aud, extra in (("pcm", planar, _ffi.FLAG_IN_PCM16), ("f32", fl, 0)):
            outs = [torch.empty(ctx.istft_num_samples(ctx.num_frames(n)), dtype=torch.int16, device=dev) for n in lens]
            taps = dict(Rs=torch.empty((2, 257, C, C), dtype=torch.complex64, device=dev),
                        Rn=torch.empty((2, 257, C, C), dtype=torch.complex64, device=dev),
                        weight=torch.empty((2, 257, C), dtype=torch.complex64, device=dev),
                        maxabs=torch.empty(2, dtype=torch.float32, device=dev))
            st = ctx.enhance_batch(_ffi.BfOpts(flags=flags | extra | _ffi.FLAG_OUT_PCM16, **KINDS["mvdr"]), C,
                                   [t.data_ptr() for t in aud], lens, [t.data_ptr() for t in m],
                                   None if it is None else [t.data_ptr() for t in it],
                                   [t.data_ptr() for t in outs], taps=taps)
            torch.cuda.synchronize()
            assert st == [0, 0]
            res[name] = [t.cpu().numpy() for t in outs] + [v.cpu().numpy() for v in taps.values()]
        for a, b in zip(res["pcm"], res["f32"]):
            assert np.array_equal(a, b)
        assert res["pcm"][-1][0] == np.abs(floats[0]).max()


def test_pcm16_input_needs_the_half_overlap_geometry():
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, 128, 512, True)
    try:
        dev = torch.device("cuda:0")
        a = torch.zeros((2, 8000), dtype=torch.int16, device=dev)
        m = torch.full((c.num_frames(8000), 257), 0.5, dtype=torch.float32, device=dev)
        out = torch.empty(c.istft_num_samples(c.num_frames(8000)), dtype=torch.float32, device=dev)
        with pytest.raises(Exception) as e:
            c.enhance_batch(_ffi.BfOpts(flags=_ffi.FLAG_IN_PCM16, kind=0), 2, [a.data_ptr()], [8000],
                            [m.data_ptr()], None, [out.data_ptr()])
        assert "hop" in str(e.value)
    finally:
        c.close()


@pytest.mark.parametrize("scale", [32768.0, 3.0, 1e4, 2.0 ** 40])
@pytest.mark.parametrize("kind", ["mvdr", "gevd"])
def test_float_samples_beyond_unit_range(ctx, kind, scale):
    """The reference's STFT / iSTFT is scale free (libs/utils.py:96-173): float wave files,
    WaveReader(normalize=False)'s int16-range floats or any C-API caller may hand in |x| >> 1.
    The matrix-core transforms of pass 2 split window x sample x 2^10 into fp16 operands (65504
    ends that range); they take the utterance's max |x| from pass 1 and scale by a power of two
    (round 4 assumed |x| <= 1 and produced inf / NaN beyond ~64).  The beamformer is linear and
    the renorm targets max |x|: the output scales with the input."""
    from setk_amd import _ffi
    mix, sp, nz = o.synth_utterance(41, 4, 24000, return_parts=True)
    mask = o.irm_mask(sp, nz)
    opts = lambda: _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS[kind])  # noqa: E731
    (y1,), st1 = run_batch(ctx, opts(), [mix], [mask])
    (ys,), sts = run_batch(ctx, opts(), [(mix * np.float32(scale))], [mask])
    assert st1 == [0] and sts == [0] and np.isfinite(ys).all()
    assert rms(ys / scale, y1) / rms(y1) < 1e-4  # (a scale that is no power of two moves roundings)
    ref = o.enhance_utterance(mix * np.float32(scale), mask, kind=kind, gauge=True)
    assert rms(ys, ref) / rms(ref) < 1e-3


@pytest.mark.parametrize("C", [8, 4])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_nonfinite_utterance_does_not_mark_its_neighbours(ctx, C, value):
    """The per-utterance status is the worst of its own 257 bins.  Bins of three utterances share
    wavefronts of the solve (257 is no multiple of the 8 / 16 problems a wavefront holds), so one
    NaN or inf sample in the middle utterance must report SETK_NUM_NONFINITE there and leave the
    outer two alone: status 0 and the waveform of the same batch with a clean middle utterance,
    bit for bit (the streaming CLI drops every wav whose status is not 0)."""
    from setk_amd import _ffi
    utts, masks = [], []
    for i in range(3):
        mix, sp, nz = o.synth_utterance(70 + i, C, 12000, return_parts=True)
        utts.append(mix)
        masks.append(o.irm_mask(sp, nz))
    opts = lambda: _ffi.BfOpts(flags=_ffi.FLAG_CLAMP_MASK, **KINDS["mvdr"])  # noqa: E731
    clean, st = run_batch(ctx, opts(), utts, masks)
    assert st == [0, 0, 0]
    bad = [u.copy() for u in utts]
    bad[1][C // 2, 5000] = value
    got, st = run_batch(ctx, opts(), bad, masks)
    assert st == [0, _ffi.NUM_NONFINITE, 0], st
    for k in (0, 2):
        assert np.array_equal(got[k].view(np.uint32), clean[k].view(np.uint32)), k
