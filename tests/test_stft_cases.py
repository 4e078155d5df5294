"""The transform conformance cases on the CPU (stft_cases.py): the float64 reference against the
oracle's goldens, the float32 yardstick against the reference, and the lane model of the
matrix-core DFT (mcdft_model.py, the blueprint of csrc/mcdft.h) through the very helper, m and
floor the device is held to in test_gpu_stft_conformance.py.  Figures: PARITY_NOTES_STFT.md."""
import numpy as np
import pytest

import mcdft_model
import stft_cases as sc
from conftest import load_golden, rel_rms, rms
from oracle import make_golden as mg
from oracle import np_oracle as o

CASES = sc.signal_cases()
INV = sc.inverse_cases()
EPS32 = float(np.finfo(np.float32).eps)


def by_family(*families):
    return [c for c in CASES if c.family in families]


def test_the_case_list_is_what_the_suite_promises():
    fams = {c.family for c in CASES}
    assert fams == {"impulses", "fullscale", "ladder", "quiet", "coloured", "pcm", "zeros", "shortest"}
    T = {sc.geom_of(c).num_frames(c.x.shape[0]) for c in CASES if c.family not in ("shortest", "ladder")}
    assert min(T) >= 10 and max(T) <= 19 and {t % 2 for t in T} == {0, 1}
    assert {c.x.shape[0] for c in by_family("shortest")} == {257, 512}
    assert len(by_family("fullscale")) == 9 * 2 * len(sc.PEAKS)
    for c in by_family("fullscale"):
        assert np.abs(c.x).max() in [np.float32(p) for p in sc.PEAKS]
    for c in CASES:
        if c.pcm is not None:
            assert c.pcm.dtype == np.int16 and np.array_equal(c.pcm.astype(np.float32) / 32768, c.x)
    imp = by_family("impulses")[0].x
    assert imp[1] == 1 and imp[-2] == 1 and set(np.unique(imp)) == {0.0, 1.0}
    hit = {(i + 256) % 256 + 256 * h for i in np.flatnonzero(imp) for h in (0, 1)}
    assert set(sc.POS512) <= hit
    z = by_family("zeros")[0]
    X = sc.ref_stft(z.x, sc.geom_of(z))
    dead = np.flatnonzero(np.abs(X).max(axis=1) == 0)
    assert list(dead) == [0, 1, 2, X.shape[0] - 2, X.shape[0] - 1]


def test_reference_reproduces_the_oracle_goldens():
    g = load_golden("ref_stft.npz")
    for name, N, fl, hop, center, rp2, window in mg.STFT_CASES:
        n_fft = o.nextpow2(fl) if rp2 else fl
        geo = sc.Geom(n_fft=n_fft, hop=hop, frame_len=fl, center=center, window=window)
        x = g[f"{name}.x"]
        S = sc.ref_stft(x, geo)
        assert S.shape == g[f"{name}.S"].T.shape and S.dtype == np.complex128
        # the oracle's own bars against the reference's stored outputs (test_oracle_golden.py)
        assert rel_rms(S.astype(np.complex64), g[f"{name}.S"].T) < 1e-6, name
        # and bit for bit what the oracle's wrapper rounds to complex64
        assert np.array_equal(S.astype(np.complex64).T, o.forward_stft(
            x, frame_len=fl, frame_hop=hop, center=center, round_power_of_two=rp2, window=window, transpose=False))
        y = sc.ref_istft(g[f"{name}.S"].T, geo)
        # (the golden wave is float32; center=False divides its first samples by window^2 ~ 1e-9,
        # ill conditioned in float32: the bars test_gpu_ops.py holds the device to on these files)
        assert y.shape == g[f"{name}.y"].shape and rms(y, g[f"{name}.y"]) < (1e-6 if center else 1e-4), name


@pytest.mark.parametrize("n_fft,hop", [(512, 256), (64, 32), (1024, 256), (4096, 2048), (18, 9), (250, 125),
                                       (600, 150), (4094, 2047)])
def test_yardstick_stays_within_a_few_eps_of_the_reference(n_fft, hop):
    """Otherwise a case would be ill posed.  pocketfft's documented bound is O(eps log n); the
    chirp-z adds two transforms of length M >= 2 n and three complex multiplications."""
    few = (4 if n_fft & (n_fft - 1) == 0 else 16) * EPS32
    fams = None if n_fft == 512 else ("impulses", "fullscale", "coloured", "zeros")
    peaks = sc.PEAKS if n_fft == 512 else (1.0, 65504.0)
    worst = 0.0
    for c in sc.signal_cases(n_fft, hop, fams, peaks):
        geo = sc.geom_of(c, n_fft, hop)
        ref = sc.ref_stft(c.x, geo)
        u = sc.yardstick_health(ref, sc.f32_stft(c.x, geo))
        worst = max(worst, u)
        assert u < few, (c.id, u)
    for ic in sc.inverse_cases(n_fft):
        geo = sc.Geom(n_fft=n_fft, hop=hop, window=ic.window)
        ref = sc.blocks(sc.ref_istft(ic.S, geo), hop)
        u = sc.yardstick_health(ref, sc.blocks(sc.f32_istft(ic.S, geo), hop))
        worst = max(worst, u)
        assert u < few, (ic.name, u)
    print(f"[yardstick n_fft={n_fft} hop={hop}] worst per-frame relative error {worst:.2e} (bar {few:.2e})")


def model_verdict(c, model=None):
    geo = sc.geom_of(c)
    ref = sc.ref_stft(c.x, geo)
    return sc.judge(c.id, sc.model_stft(c.x, geo, model=model), ref, sc.f32_stft(c.x, geo),
                    floor=sc.mc_floor(c.peak), exact_zero=True)


@pytest.mark.parametrize("family", ["impulses", "fullscale", "ladder", "quiet", "coloured", "pcm", "zeros",
                                    "shortest"])
def test_model_forward_meets_the_device_bar(family):
    """The blueprint through judge() with the device's m and floor: a bar it cannot meet is wrong."""
    bad, worst = [], (0.0, 0.0, "")
    for c in by_family(family):
        v = model_verdict(c)
        f, b, _ = v.worst()
        worst = max(worst, (f, b, c.id))
        bad += v.failures
    print(f"[model forward {family}] worst frame {worst[0]:.3f}, bin {worst[1]:.3f} of the allowance ({worst[2]})")
    assert not bad, "\n".join(bad[:20])


def test_model_inverse_meets_the_device_bar():
    bad, worst = [], (0.0, "")
    for ic in INV:
        geo = sc.Geom(window=ic.window)
        ref = sc.blocks(sc.ref_istft(ic.S, geo), 256)
        got = sc.blocks(sc.model_istft(ic.S, geo), 256)
        v = sc.judge(ic.name, got, ref, sc.blocks(sc.f32_istft(ic.S, geo), 256), exact_zero=True)
        worst = max(worst, (v.worst()[0], ic.name))
        bad += v.failures
    print(f"[model inverse] worst block {worst[0]:.3f} of the allowance ({worst[1]})")
    assert not bad, "\n".join(bad[:20])


def frame_rel(got, ref):
    n = np.linalg.norm(ref, axis=1)
    e = np.linalg.norm(got - ref, axis=1)
    return e[n > 0] / n[n > 0], n[n > 0]


def test_quiet_and_ladder_follow_the_floor_law():
    """Without a negative exponent the model's per-frame error is the absolute floor: relative
    error x frame level stays near one constant of the order 2^-34 sqrt(n_fft) over 2^-4 .. 2^-40,
    i.e. the relative error doubles whenever the level halves.  With the exponent (peak below 2^-15) a quiet
    utterance is back at the float32 class."""
    lad = by_family("ladder")[0]
    geo = sc.geom_of(lad)
    ref = sc.ref_stft(lad.x, geo)
    rel, norm = frame_rel(sc.model_stft(lad.x, geo), ref)
    burst = slice(1, None, 2)          # frame 2 j + 1 lies inside burst j alone
    rel, norm = rel[burst], norm[burst]
    levels = 2.0 ** -np.arange(0, 41, 4)
    absf = rel * norm / np.sqrt(257)   # per-bin absolute error
    print("[floor law: ladder] level, relative frame error, per-bin absolute error / (2^-34 sqrt(512))")
    for lv, r, a in zip(levels, rel, absf):
        print(f"    2^{int(np.log2(lv)):4d}  {r:.2e}  {a / (2.0 ** -34 * np.sqrt(512)):.3f}")
    assert (rel[:2] < 4e-7).all()                      # 2^0, 2^-4: the float32 class
    low = absf[4:9]                                    # 2^-16 .. 2^-32: the floor rules
    assert low.max() < 4 * low.min()
    assert 0.05 < low.mean() / (2.0 ** -34 * np.sqrt(512)) < 1.0
    assert np.all(rel[5:9] / rel[4:8] > 4)             # x16 in level: at least x4 in relative error
    print("[floor law: quiet] peak, relative frame error without / with the negative exponent, float32 FFT")
    for c in by_family("quiet"):
        geo = sc.geom_of(c)
        ref = sc.ref_stft(c.x, geo)
        old = frame_rel(sc.model_stft(c.x, geo, negative=False), ref)[0].max()
        new = frame_rel(sc.model_stft(c.x, geo, negative=True), ref)[0].max()
        f32 = frame_rel(sc.f32_stft(c.x, geo), ref)[0].max()
        print(f"    {c.name:6s}  {old:.2e}  {new:.2e}  {f32:.2e}")
        if c.peak < 2.0 ** -15:
            assert new < 4e-7 and old > 10 * new, (c.name, old, new)
        else:
            assert new == old


class LostLoHalf:
    """mcdft_model with the lo half of the stage-2 real tile gone (the tile is rounded to fp16
    before it is split): the broken transform the suite must catch."""

    def __getattr__(self, k):
        return getattr(mcdft_model, k)

    @staticmethod
    def forward(xw, scale=1024.0):
        orig = mcdft_model.stage2_tiles

        def broken():
            ar, ai = orig()
            return ar.astype(np.float16).astype(np.float64), ai
        mcdft_model.stage2_tiles = broken
        try:
            return mcdft_model.forward(xw, scale)
        finally:
            mcdft_model.stage2_tiles = orig


def test_a_lost_lo_half_of_one_tile_is_caught():
    """... on `coloured` and `fullscale`, by the per-frame / per-bin measure; the global relative
    RMS over broadband noise that the older bars use (3e-7, test_mcdft_model.py) moves too, but
    stays five hundred times below the 1e-4 the device tests assert."""
    broken = LostLoHalf()
    for fam in ("coloured", "fullscale"):
        cases = by_family(fam)
        failed = [c.id for c in cases if not model_verdict(c, model=broken).ok]
        print(f"[lost lo half] {fam}: {len(failed)} of {len(cases)} cases fail")
        assert len(failed) > len(cases) // 2, (fam, failed)
    rng = np.random.default_rng(11)
    xw = np.clip(rng.standard_normal((24, 512)) * 0.2, -1, 1).astype(np.float32)
    xw *= (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(512) / 512)).astype(np.float32)
    ref = np.fft.rfft(xw.astype(np.float64), axis=1)
    rel = rel_rms(broken.forward(xw), ref)
    print(f"[lost lo half] global relative RMS on broadband noise {rel:.2e} (sound model: "
          f"{rel_rms(mcdft_model.forward(xw), ref):.2e}; the device tests assert < 1e-4)")
    assert 3e-7 < rel < 1e-4


def chained(case, C, seed, model=None):
    """Model forward of every channel -> the oracle's MVDR weights (complex64, as the device's
    taps are) -> model inverse -> max-abs renorm, judged as the fused device forms are: with the
    input-referred term of stft_cases.fused_reference."""
    rng = np.random.default_rng(seed)
    geo = sc.geom_of(case)
    x = (rng.uniform(-1, 1, (C, case.x.shape[0])) * case.peak).astype(np.float32)
    x[seed % C] = case.x
    mask = rng.uniform(0.2, 0.8, (geo.num_frames(x.shape[1]), 257)).astype(np.float32)
    X = np.transpose(sc.ref_stft(x, geo), (0, 2, 1))
    w = o.mvdr_weight(o.compute_covar(X, mask.astype(np.float64)),
                      o.compute_covar(X, 1 - mask.astype(np.float64))).astype(np.complex64)
    Xm = np.stack([sc.model_stft(c, geo, model=model) for c in x]).astype(np.complex64)
    y = sc.model_istft(np.einsum("fc,ctf->tf", np.conj(w), Xm).astype(np.complex64), geo)
    y = y * np.float32(np.abs(x).max()) / (np.abs(y).max() + np.float32(sc.EPS32))
    ref, yard, inp = sc.fused_reference(x, w, mask, geo, False, case.peak)
    return sc.judge(case.id, sc.blocks(y, 256), sc.blocks(ref, 256), sc.blocks(yard, 256), floor=inp,
                    exact_zero=False)


def test_the_fused_forms_wider_bar_still_catches_a_lost_lo_half():
    """The fused device forms carry an input-referred term in their allowance.  Through that very
    bar the sound model chained forward -> weights -> inverse stays well inside, and the model
    with a lost lo half does not, at two and five channels."""
    names = ("impulses:unit", "zeros:burst", "coloured:tone+floor", "coloured:tilt80dB", "fullscale:square@1/hann",
             "fullscale:bin48@1/hann", "fullscale:bin32@65504/hann")
    cases = [c for c in CASES if c.id in names]
    assert len(cases) == len(names)
    broken = LostLoHalf()
    for C in (2, 5):
        for k, case in enumerate(cases):
            good, bad = chained(case, C, 10 * C + k), chained(case, C, 10 * C + k, model=broken)
            print(f"[chained C={C}] {case.id}: sound {good.worst()[0]:.2f}, lost lo half {bad.worst()[0]:.2f} of the allowance")
            assert good.ok, good.failures[:3]
            assert not bad.ok, case.id
