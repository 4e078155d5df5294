"""
Conformance of every device form of the STFT / iSTFT -- the fp32 radix-16 butterflies (fft512.h,
pass2.hip), the matrix-core fp16-split DFT of the default stage 3 (mcdft.h in pass2_mc.hip: float32
and PCM input, one and two sample buffers), the opt-in matrix-core pass 1 (pass1_mc.hip) and the
generic radix-2 and Bluestein kernels (modular.hip) -- on the constructed signals and spectrograms
of stft_cases.py, frame by frame and bin by bin.

Every frame (every block of hop output samples) of every case is held to m (u_t ||X_t|| + floor):
u_t is what a plain float32 implementation of the same operation loses on that very frame, m = 4,
floor = 0 for the fp32 forms and the documented subnormal quantum of the fp16 lo halves for the
matrix-core forms (stft_cases.judge / mc_floor; the lane model meets the same bars in
test_stft_cases.py).  The fused forms are judged against their own tapped weights applied in
float64: the transform answers, not the solver.  Measured figures: PARITY_NOTES_STFT.md.
"""
import os

import numpy as np
import pytest

import covar_cases as cc
import stft_cases as sc
from conftest import rel_rms

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
CASES = sc.signal_cases()
HANN = [c for c in CASES if c.window == "hann"]
RECT = [c for c in CASES if c.window == "rect"]
INV = sc.inverse_cases()
_REF = {}


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def spectra_of(case, C, geo):
    """(x [C][N] float32, reference [C][T][F], yardstick) of `channels(case.x, C)`; computed once."""
    def make():
        x = sc.channels(case.x, C)
        return x, sc.ref_stft(x, geo), sc.f32_stft(x, geo)
    return cached(("fw", case.id, C, repr(geo)), make)


class Tally:
    """Verdicts of one test: the worst figures per family, printed, and every failure."""

    def __init__(self, form):
        self.form, self.worst, self.failures = form, {}, []

    def add(self, family, v):
        f, b, rel = v.worst()
        w = self.worst.setdefault(family, [0.0, 0.0, 0.0, ""])
        if f >= w[0]:
            w[3] = v.name
        w[0], w[1], w[2] = max(w[0], f), max(w[1], b), max(w[2], rel)
        self.failures += v.failures

    def finish(self):
        for fam, (f, b, rel, name) in sorted(self.worst.items()):
            print(f"[{self.form}] {fam:10s} worst frame {f:.3f}, worst bin {b:.3f} of the allowance; "
                  f"worst relative frame error {rel:.2e} ({name})")
        assert not self.failures, f"{len(self.failures)} failures:\n" + "\n".join(self.failures[:25])


def new_ctx(geo=None):
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(*(geo or sc.Geom()).plan_args())
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    c.close()


class switched:
    """A fresh handle under an environment switch (read when the transform is planned / called)."""

    def __init__(self, switch, geo=None):
        self.switch, self.geo = switch, geo

    def __enter__(self):
        self.old = {}
        for kv in filter(None, self.switch.split(",")):
            k, v = kv.split("=")
            self.old[k] = os.environ.get(k)
            os.environ[k] = v
        self.ctx = new_ctx(self.geo)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def dev_stft(c, x, geo):
    x = np.ascontiguousarray(x, np.float32)
    out = np.full((x.shape[0], c.num_frames(x.shape[1]), geo.F), np.nan, np.complex64)
    c.stft(x, out)
    return out


def dev_istft(c, S, nsamps=None):
    S = np.ascontiguousarray(S[None], np.complex64)
    y = np.full((1, c.istft_num_samples(S.shape[1], nsamps)), np.nan, np.float32)
    c.istft(S, 1, S.shape[1], nsamps, None, y)
    return y[0]


# ---------------------------------------------------------------- butterfly forward (fft512.h)
@pytest.mark.parametrize("C", [1, 3, 8, 11])
def test_butterfly_forward(ctx, C):
    """setk_stft, n_fft = 512: every family, Hann and rectangular; 11 channels = 8 + 3 in two launches."""
    tally = Tally(f"butterfly forward C={C}")
    for case in HANN + RECT:
        geo = sc.geom_of(case)
        ctx.stft_plan(*geo.plan_args())
        x, ref, yard = spectra_of(case, C, geo)
        tally.add(case.family, sc.judge(case.id, dev_stft(ctx, x, geo), ref, yard))
    ctx.stft_plan(*sc.Geom().plan_args())
    tally.finish()


@pytest.mark.parametrize("center", [True, False])
def test_butterfly_forward_batched(ctx, center):
    """setk_stft_batch: a ragged batch in one launch with spec_pitch 272 > 257; the padding of
    every row stays untouched."""
    import torch
    dev = torch.device("cuda:0")
    C, pitch = 3, 272
    tally = Tally(f"butterfly forward, batched, center={center}")
    for cases in (HANN, RECT):
        cases = [c for c in cases if c.x.shape[0] >= 512 or center]
        geos = [sc.geom_of(c, center=center) for c in cases]
        ctx.stft_plan(*geos[0].plan_args())
        parts = [spectra_of(c, C, g) for c, g in zip(cases, geos)]
        a = [torch.from_numpy(p[0]).to(dev) for p in parts]
        s = [torch.full((C, p[1].shape[1], pitch), float("nan"), dtype=torch.complex64, device=dev) for p in parts]
        ctx.stft_batch(C, [t.data_ptr() for t in a], [p[0].shape[1] for p in parts], [t.data_ptr() for t in s],
                       spec_pitch=pitch)
        torch.cuda.synchronize()
        for c, p, t in zip(cases, parts, s):
            got = t.cpu().numpy()
            assert np.isnan(got[..., 257:]).all(), c.id
            tally.add(c.family, sc.judge(c.id, got[..., :257], p[1], p[2]))
    ctx.stft_plan(*sc.Geom().plan_args())
    tally.finish()


# ---------------------------------------------------------------- butterfly inverse
@pytest.mark.parametrize("hop", [256, 128, 64])
def test_butterfly_inverse(ctx, hop):
    """setk_istft on spectrograms given directly; natural length, and nsamps shorter / longer."""
    tally = Tally(f"butterfly inverse hop={hop}")
    for ic in INV:
        geo = sc.Geom(hop=hop, window=ic.window)
        ctx.stft_plan(*geo.plan_args())
        natural = hop * (ic.S.shape[0] - 1)
        lengths = [None] if ic.name.startswith("cell") and "k=16" not in ic.name else \
            [None, natural - 3 * hop - 7, natural + hop + 5]
        for nsamps in lengths:
            ref, yard = cached(("inv", ic.name, hop, nsamps), lambda: (
                sc.ref_istft(ic.S, geo, nsamps), sc.f32_istft(ic.S, geo, nsamps)))
            got = dev_istft(ctx, ic.S, nsamps)
            assert got.shape == ref.shape, (ic.name, nsamps)
            tally.add("inverse" if nsamps is None else "inverse/nsamps",
                      sc.judge(f"{ic.name} nsamps={nsamps}", sc.blocks(got, hop), sc.blocks(ref, hop),
                               sc.blocks(yard, hop)))
    ctx.stft_plan(*sc.Geom().plan_args())
    tally.finish()


# ---------------------------------------------------------------- butterfly forward + inverse
def roundtrip_of(case, geo):
    """istft(stft(x)) is x itself over the hop (T - 1) samples the centred inverse returns (Hann
    and rectangular windows at hop = n_fft / 2 overlap-add to a constant): the reference is exact,
    silent blocks included; the yardstick is the float32 round trip."""
    def make():
        yard = sc.f32_istft(sc.f32_stft(case.x, geo), geo)
        return case.x[:yard.shape[0]].astype(np.float64), yard
    return cached(("rt", case.id, repr(geo)), make)


@pytest.mark.parametrize("C", [1, 4, 8])
def test_butterfly_forward_and_inverse(ctx, C):
    """setk_apply_weights_batch with one-hot weights and SETK_FLAG_NO_RENORM: the output is
    channel c itself, through pass 2's butterfly transforms (pass2.hip)."""
    import torch
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    tally = Tally(f"butterfly forward + inverse C={C}")
    w = np.zeros((C, 257, C), np.complex64)
    for c in range(C):
        w[c, :, c] = 1
    rng = np.random.default_rng(C)
    for cases in (HANN, RECT):
        cases = [c for c in cases if c.name != "uncentred"]
        geo = sc.geom_of(cases[0])
        ctx.stft_plan(*geo.plan_args())
        utts, pick = [], []
        for i, case in enumerate(cases):
            x = (rng.uniform(-1, 1, (C, case.x.shape[0])) * case.peak).astype(np.float32)
            pick.append(i % C)
            x[pick[-1]] = case.x
            utts.append(x)
        a = [torch.from_numpy(u).to(dev) for u in utts]
        outs = [torch.full((ctx.istft_num_samples(ctx.num_frames(u.shape[1])),), float("nan"), dtype=torch.float32,
                           device=dev) for u in utts]
        ctx.apply_weights_batch(C, [t.data_ptr() for t in a], [u.shape[1] for u in utts], w, C, pick,
                                [t.data_ptr() for t in outs], flags=_ffi.FLAG_NO_RENORM)
        torch.cuda.synchronize()
        for case, t in zip(cases, outs):
            ref, yard = roundtrip_of(case, geo)
            got = t.cpu().numpy()
            assert got.shape == ref.shape, case.id
            # (a silent block beside a loud one is not silent on the way out of any float32 round
            #  trip: it answers to the yardstick's own error there, not to exact zero)
            tally.add(case.family, sc.judge(case.id, sc.blocks(got, 256), sc.blocks(ref, 256), sc.blocks(yard, 256),
                                            exact_zero=False))
    ctx.stft_plan(*sc.Geom().plan_args())
    tally.finish()


# ---------------------------------------------------------------- the fused call (stage 3)
def fused_utterance(case, C, index, pcm=False):
    """C channels for the fused call: the case in channel index % C, independent noise of at most
    the case's peak in the others (rotated copies of one signal have a rank-one covariance: no
    beamformer is defined there).  max |x| is the case's peak."""
    def make():
        rng = np.random.default_rng(1000 + index)
        if pcm:
            top = int(np.abs(case.pcm.astype(np.int64)).max())
            x = rng.integers(-min(top, 32767), min(top, 32767) + 1, (C, case.pcm.shape[0])).astype(np.int16)
            x[index % C] = case.pcm
            return x
        x = (rng.uniform(-1, 1, (C, case.x.shape[0])) * case.peak).astype(np.float32)
        x[index % C] = case.x
        return x
    return cached(("fu", case.id, C, index, pcm), make)


def mask_of(T, index, post=False):
    if post:       # 1 on one cell per frame pair, 2^-20 elsewhere
        m = np.full((T, 257), 2.0 ** -20, np.float32)
        for t in range(0, T, 2):
            m[t, (37 * t + 5 * index) % 257] = 1
        return m
    return np.random.default_rng(index).uniform(0.2, 0.8, (T, 257)).astype(np.float32)


def run_fused(c, C, utts, masks, flags, pcm=False):
    """One setk_enhance_batch_taps launch (MVDR): waves, statuses, weights [n][257][C]."""
    import torch
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    ns = [u.shape[1] for u in utts]
    if pcm:
        a = [torch.zeros((C, c.pcm16_channel_stride(n)), dtype=torch.int16, device=dev) for n in ns]
        for t, u in zip(a, utts):
            t[:, :u.shape[1]] = torch.from_numpy(u).to(dev)
        flags |= _ffi.FLAG_IN_PCM16
    else:
        a = [torch.from_numpy(u).to(dev) for u in utts]
    m = [torch.from_numpy(x).to(dev) for x in masks]
    outs = [torch.full((c.istft_num_samples(c.num_frames(n)),), float("nan"), dtype=torch.float32, device=dev)
            for n in ns]
    w = torch.zeros((len(utts), 257, C), dtype=torch.complex64, device=dev)
    st = c.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR, flags=flags | _ffi.FLAG_CLAMP_MASK), C,
                         [t.data_ptr() for t in a], ns, [t.data_ptr() for t in m], None,
                         [t.data_ptr() for t in outs], taps=dict(weight=w))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], st, w.cpu().numpy()


def fused_judge(tally, c, C, cases, geo, flags=0, post=False, pcm=False, mc=True, quiet_bar=False):
    """The cases as one ragged batch through the fused call; every block of hop samples judged.
    mc: the stage-3 transforms run on the matrix cores (their floor applies).  Returns the waves
    and the statuses."""
    from setk_amd import _ffi
    c.stft_plan(*geo.plan_args())
    utts = [fused_utterance(case, C, i, pcm) for i, case in enumerate(cases)]
    xs = [u.astype(np.float32) / np.float32(32768) for u in utts] if pcm else utts
    masks = [mask_of(c.num_frames(u.shape[1]), i, post) for i, u in enumerate(utts)]
    waves, st, w = run_fused(c, C, utts, masks, flags | (_ffi.FLAG_POST_MASK if post else 0), pcm)
    refused = []
    for i, case in enumerate(cases):
        # 2^60: |X|^2 leaves float32 in stage 1's covariances -- the solver's range, reported
        if case.peak > 2.0 ** 50:
            assert st[i] == _ffi.NUM_NONFINITE, (case.id, st[i])
            continue
        # one channel: a line spectrum (DC, alternation, a tone on the bin grid) leaves whole bins at
        # exact zero, there is no covariance to solve with and the solver refuses the utterance
        # as numpy.linalg.solve does for the reference -- no wave is defined; such a signal is
        # judged at C >= 2, where the other channels keep every bin alive
        if C == 1 and st[i] == _ffi.NUM_SINGULAR and not np.isfinite(w[i]).all():
            assert case.family == "fullscale" or case.name.startswith("alt"), (case.id, st[i])
            refused.append(case.id)
            continue
        assert st[i] == 0, (case.id, st[i])
        ref, yard, inp = sc.fused_reference(xs[i], w[i], masks[i], geo, post, case.peak if mc else None)
        assert waves[i].shape == ref.shape, case.id
        tally.add(case.family, sc.judge(case.id, sc.blocks(waves[i], geo.hop), sc.blocks(ref, geo.hop),
                                        sc.blocks(yard, geo.hop), floor=inp, exact_zero=False))
        if quiet_bar and case.family == "quiet":
            rel = rel_rms(waves[i], ref)
            print(f"[{tally.form}] {case.id}: wave relative RMS {rel:.2e} (bar 1e-3)")
            if not rel < 1e-3:
                tally.failures.append(f"{case.id}: wave relative RMS {rel:.2e} misses the 1e-3 waveform bar")
    if refused:
        print(f"[{tally.form}] refused by the solver (singular, one channel): {', '.join(refused)}")
    # (under the rectangular window every full-scale signal is a line spectrum)
    assert len(refused) < len(cases) // 2 or geo.window == "rect"
    return waves, st


FUSED_HANN = [c for c in HANN if c.name != "uncentred"]
FUSED_RECT = RECT


@pytest.mark.parametrize("C", [1, 2, 4, 5, 8])
def test_matrix_core_stage3_float32(ctx, C):
    """The default fused path: mcdft.h in pass2_mc.hip, one sample buffer (C <= 4) and two
    (C >= 5).  A quiet utterance must also meet the project's own 1e-3 waveform bar: float
    samples of any magnitude are accepted (setk_hip.h)."""
    tally = Tally(f"matrix-core stage 3 C={C}")
    fused_judge(tally, ctx, C, FUSED_HANN, sc.Geom(), quiet_bar=True)
    fused_judge(tally, ctx, C, FUSED_RECT, sc.Geom(window="rect"))
    ctx.stft_plan(*sc.Geom().plan_args())
    tally.finish()


@pytest.mark.parametrize("C", [1, 5])
def test_matrix_core_stage3_post_mask(ctx, C):
    tally = Tally(f"matrix-core stage 3, post mask C={C}")
    fused_judge(tally, ctx, C, FUSED_HANN, sc.Geom(), post=True)
    fused_judge(tally, ctx, C, FUSED_RECT, sc.Geom(window="rect"), post=True)
    ctx.stft_plan(*sc.Geom().plan_args())
    tally.finish()


@pytest.mark.parametrize("C", [1, 5, 8])
def test_matrix_core_stage3_pcm_input(ctx, C):
    """SETK_FLAG_IN_PCM16: judged like the float form, and bit-identical to the float call."""
    cases = [c for c in HANN if c.pcm is not None]
    tally = Tally(f"matrix-core stage 3, PCM in C={C}")
    got, st_pcm = fused_judge(tally, ctx, C, cases, sc.Geom(), pcm=True)
    utts = [fused_utterance(case, C, i, True).astype(np.float32) / np.float32(32768) for i, case in enumerate(cases)]
    masks = [mask_of(ctx.num_frames(u.shape[1]), i) for i, u in enumerate(utts)]
    waves, st, _ = run_fused(ctx, C, utts, masks, 0)
    assert st == st_pcm
    for case, a, b in zip(cases, got, waves):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), case.id
    tally.finish()


@pytest.mark.parametrize("switch,hop", [("SETK_MC_PASS2=0", 256), ("SETK_LEGACY_FFT=1", 256), ("", 128)])
@pytest.mark.parametrize("C", [2, 8])
def test_butterfly_stage3_inside_the_fused_call(switch, hop, C):
    """pass2.hip behind the fused call: by switch, and by geometry (hop 128 has no matrix-core form)."""
    tally = Tally(f"butterfly stage 3 {switch or 'hop=128'} C={C}")
    geo = sc.Geom(hop=hop)
    with switched(switch, geo) as c:
        fused_judge(tally, c, C, FUSED_HANN, geo, mc=False)
        fused_judge(tally, c, C, FUSED_RECT, geo.with_(window="rect"), mc=False)
    tally.finish()


# ---------------------------------------------------------------- matrix-core pass 1 (opt-in)
@pytest.mark.parametrize("C", [4, 8])
def test_matrix_core_pass1_covariances(C):
    """SETK_MC_PASS1=1: the tapped Rs / Rn against float64 covariances of the float64 spectra, on
    every family under both windows.

    Two measures.  The utterance: as a bin of a spectrum answers to its frame's norm, an entry of
    a covariance answers to the norm of the utterance's covariances: ||R - R_ref|| over all bins
    against m (u ||R_ref|| + floor), u from float32 covariances of the float32 yardstick spectra
    and at least 3 x 2^-24 (an entry is a product of two float32 spectra, each rounded, and is
    rounded itself; pocketfft's spectra of on-grid lines are exact to 2e-8 and say nothing of it),
    floor = 2 sqrt(C) q ||max_t |X_f,t| ||_f, q = 2^-34 sqrt(n_fft) fullscale the per-bin quantum of
    the forward (dR = X dX^H + dX X^H).  The bin: ||R_f - R_ref,f|| against m (the yardstick's error
    in that bin + sum_t m_t 2 ||X_f,t|| a_t / sum_t m_t), a_t = sqrt(sum_c (u_c,t ||X_c,t|| +
    floor)^2) the forward's own promise for any bin of frame t -- a fault confined to weak bins
    answers here.

    This form has no per-utterance exponent: its operands are window x sample x 2^10 whatever
    max |x| is (the maximum comes out of the same launch).  Below 2^-15 the absolute floor is all
    that is promised, and it is what the measure allows.  Above 1 a stage-1 sum may leave fp16:
    such an utterance must come back refused (SETK_NUM_NONFINITE), never with covariances that
    miss the bars under status 0 (setk_hip.h states the limit)."""
    import torch
    from setk_amd import _ffi
    from oracle import np_oracle as o
    dev = torch.device("cuda:0")
    tally = Tally(f"matrix-core pass 1 C={C}")
    outcome = {}
    for cases, geo in ((FUSED_HANN, sc.Geom()), (FUSED_RECT, sc.Geom(window="rect"))):
        with switched("SETK_MC_PASS1=1", geo) as c:
            utts = [fused_utterance(case, C, i) for i, case in enumerate(cases)]
            masks = [mask_of(c.num_frames(u.shape[1]), i) for i, u in enumerate(utts)]
            a = [torch.from_numpy(u).to(dev) for u in utts]
            m = [torch.from_numpy(x).to(dev) for x in masks]
            outs = [torch.empty(c.istft_num_samples(c.num_frames(u.shape[1])), dtype=torch.float32, device=dev)
                    for u in utts]
            taps = dict(Rs=torch.zeros((len(utts), 257, C, C), dtype=torch.complex64, device=dev),
                        Rn=torch.zeros((len(utts), 257, C, C), dtype=torch.complex64, device=dev))
            st = c.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK), C,
                                 [t.data_ptr() for t in a], [u.shape[1] for u in utts], [t.data_ptr() for t in m], None,
                                 [t.data_ptr() for t in outs], taps=taps)
            torch.cuda.synchronize()
            Rs, Rn = taps["Rs"].cpu().numpy(), taps["Rn"].cpu().numpy()
        for i, case in enumerate(cases):
            key = f"{case.name.split('@')[-1]}" if case.family == "fullscale" else case.family
            if case.peak > 1.0 and st[i] == _ffi.NUM_NONFINITE:
                outcome.setdefault(key, []).append("refused")
                continue
            assert st[i] == 0, (case.id, st[i])
            outcome.setdefault(key, []).append("conforms")
            X = np.transpose(sc.ref_stft(utts[i], geo), (0, 2, 1))                 # C x F x T
            X32 = np.transpose(sc.f32_stft(utts[i], geo), (0, 2, 1))
            q = 2.0 ** -34 * np.sqrt(512) * sc.fullscale_of(case.peak)
            floor = 2 * np.sqrt(C) * q * np.linalg.norm(np.abs(X).max(axis=(0, 2)))
            at = np.sqrt((cc.forward_promise(X, X32, floor=sc.mc_floor(case.peak), axis=1) ** 2)
                         .sum(axis=0))                                             # [T]
            xf = np.linalg.norm(X, axis=0)                                         # [F][T]
            for name, got, mk in (("Rs", Rs[i], masks[i]), ("Rn", Rn[i], 1 - masks[i])):
                ref = o.compute_covar(X, mk.astype(np.float64)).reshape(257, -1)
                yard = o.compute_covar(X32, mk).astype(np.complex64).reshape(257, -1)
                got = got.reshape(257, -1)
                tally.add(case.family, sc.judge(f"{case.id} {name}", got.reshape(1, -1), ref.reshape(1, -1),
                                                yard.reshape(1, -1), floor=floor, exact_zero=False,
                                                u_min=3 * sc.U32))
                mk64 = mk.astype(np.float64).T                                     # [F][T]
                per_bin = cc.bin_forward_term(mk64, xf, at)
                err = np.linalg.norm(got - ref, axis=1)
                allow = sc.M_BITS * (np.linalg.norm(yard - ref, axis=1) + per_bin)
                worst = int(np.argmax(err / allow))
                if not (err <= allow).all():
                    tally.failures.append(f"{case.id} {name}: bin {worst} error {err[worst]:.3e} > {allow[worst]:.3e}")
    for key, v in outcome.items():
        print(f"[{tally.form}] {key}: {v.count('conforms')} conform, {v.count('refused')} refused (SETK_NUM_NONFINITE)")
    tally.finish()


# ---------------------------------------------------------------- generic radix-2 and Bluestein (modular.hip)
GENERIC_FAMILIES = ("impulses", "fullscale", "coloured", "zeros")


def generic_form(name, geos):
    tally = Tally(name)
    c = new_ctx(geos[0])
    try:
        for g0 in geos:
            cases = sc.signal_cases(g0.n_fft, g0.hop, GENERIC_FAMILIES, peaks=(1.0, 65504.0, 2.0 ** 60))
            for case in sorted(cases, key=lambda k: k.window):      # (one plan per window)
                geo = g0.with_(window=case.window)
                if geo.frame_len != geo.n_fft and case.window == "rect":
                    continue      # (a rectangular window shorter than n_fft: no such case is set)
                c.stft_plan(*geo.plan_args())
                x = sc.channels(case.x, 2)
                ref, yard = sc.ref_stft(x, geo), sc.f32_stft(x, geo)
                got = dev_stft(c, x, geo)
                tally.add(f"{case.family}/{g0!r}"[:40], sc.judge(f"{case.id} {geo!r}", got, ref, yard))
            # inverse: where the hop divides n_fft.  Otherwise a block of hop samples holds a sliver
            # of a frame (n_fft mod hop samples at the window's tail, 190 dB down): its error answers to
            # the frame it came from, not to the sliver, and the per-block measure does not apply.
            for ic in sorted(sc.inverse_cases(g0.n_fft), key=lambda k: k.window) if g0.n_fft % g0.hop == 0 else []:
                gi = g0.with_(window=ic.window)
                if gi.frame_len != gi.n_fft and ic.window == "rect":
                    continue      # (a rectangular window shorter than n_fft: no such case is set)
                c.stft_plan(*gi.plan_args())
                ref, yard = sc.ref_istft(ic.S, gi), sc.f32_istft(ic.S, gi)
                got = dev_istft(c, ic.S)
                assert got.shape == ref.shape, (ic.name, gi)
                tally.add(f"inverse/{g0!r}"[:40], sc.judge(f"{ic.name} {gi!r}", sc.blocks(got, gi.hop),
                                                           sc.blocks(ref, gi.hop), sc.blocks(yard, gi.hop)))
    finally:
        c.close()
    tally.finish()


@pytest.mark.parametrize("n_fft,frame_len", [(64, 64), (1024, 1024), (1024, 400), (4096, 4096)])
def test_generic_radix2(n_fft, frame_len):
    generic_form(f"radix-2 n_fft={n_fft} frame_len={frame_len}",
                 [sc.Geom(n_fft=n_fft, hop=n_fft // 4, frame_len=frame_len),
                  sc.Geom(n_fft=n_fft, hop=n_fft // 2, frame_len=frame_len, center=False)])


@pytest.mark.parametrize("n_fft", [18, 250, 600, 4094])
def test_bluestein(n_fft):
    hop4 = max(1, n_fft // 4)
    generic_form(f"Bluestein n_fft={n_fft}",
                 [sc.Geom(n_fft=n_fft, hop=n_fft // 2), sc.Geom(n_fft=n_fft, hop=hop4),
                  sc.Geom(n_fft=n_fft, hop=n_fft // 2, center=False), sc.Geom(n_fft=n_fft, hop=hop4, center=False)])
