"""
The TF-mask measure on the CPU (tests/tfmask_cases.py; figures in PARITY_NOTES_TFMASK.md): the
reference tools' own outputs (tests/golden/ref_tfmask.npz) and the reference's float32 arithmetic
on every case stay within every cap and bar the device is held to -- so a cap cannot hide a device
failure -- and a wrong result does not.
"""
import numpy as np
import pytest

import stft_cases as sc
import tfmask_cases as tc


@pytest.fixture(scope="module")
def gold():
    return np.load(tc.GOLDEN)


@pytest.fixture(scope="module")
def mask_pairs():
    return tc.mask_pairs() + tc.other_size_pairs()


def test_the_goldens_are_the_restatement(gold):
    """What the reference's functions returned on the stored pairs, against mask_formula /
    oracle_formula on the same complex64 spectra (make_golden_tfmask.py asserts bit identity on the
    machine that wrote the file; another numpy may round cos / exp differently by an ulp)."""
    for p in tc.noise_pairs()[:2]:
        assert np.array_equal(gold[f"fn_{p.name}_tgt"], p.pcm[0][0]) and np.array_equal(gold[f"fn_{p.name}_mix"], p.pcm[1])
        ts32, m32 = p.spectra(np.complex64)
        for kind in tc.KINDS:
            want, mine = gold[f"fn_{p.name}_{kind}"], tc.mask_formula(kind, ts32[0], m32)
            assert want.shape == mine.shape
            assert np.allclose(want, mine, rtol=4e-6, atol=1e-6, equal_nan=True), (p.name, kind)
    p = tc.oracle_pairs()[2]
    assert np.array_equal(gold["fn_oracle8_mix"], p.pcm[1]) and np.array_equal(gold["fn_oracle8_targets"], np.stack(p.pcm[0]))
    ts32, m32 = p.spectra(np.complex64)
    for kind in tc.ORACLE_KINDS:
        mine = np.stack([np.asarray(x) for x in tc.oracle_formula(kind, m32, ts32)])
        if kind == "ibm":
            assert np.array_equal(gold[f"fn_oracle8_{kind}"], mine)
        else:
            assert np.allclose(gold[f"fn_oracle8_{kind}"], mine, rtol=4e-6, atol=1e-6), kind


@pytest.mark.parametrize("kind", tc.KINDS)
def test_the_reference_arithmetic_stays_within_every_cap_and_bar(mask_pairs, kind):
    """The float32 formulas on the rounded float64 spectra, every case, both cutoffs: inside the
    allowance with C_ROUND, the shares left out under their caps (asserted by judge_mask), the
    rounding constant they need no larger than C_ROUND / m."""
    lines = []
    for p in mask_pairs:
        if not p.judged:
            continue
        for cutoff in tc.CUTOFFS:
            v = tc.judge_mask(f"{p.name}:{kind}@{cutoff}", kind, tc.yardstick_mask(kind, p, cutoff), p, cutoff)
            lines.append(v.line())
            assert v.ok, v.failures
            assert v.need is not None and v.need * tc.M_BITS <= tc.C_ROUND
    print("\n".join(lines))


def test_the_stored_golden_masks_stay_within_the_bars(gold):
    for p in tc.noise_pairs()[:2]:
        for kind in tc.KINDS:
            got = tc.clip_formula(gold[f"fn_{p.name}_{kind}"], -1.0)[0]
            v = tc.judge_mask(f"golden {p.name}:{kind}", kind, got, p)
            assert v.ok, v.failures
    p = tc.oracle_pairs()[2]
    for kind in tc.ORACLE_KINDS:
        for k in range(8):
            v = tc.judge_mask(f"golden oracle8:{kind}[{k}]", kind, gold[f"fn_oracle8_{kind}"][k], p, k=k, oracle=True)
            assert v.ok, v.failures


def test_the_command_line_goldens_stay_within_the_bars(gold):
    for key in [str(k) for k in gold["cli_keys"]]:
        p = tc.Pair(key, [gold[f"cli_clean_{key}"].astype(np.float32) / np.float32(32768)],
                    gold[f"cli_noisy_{key}"].astype(np.float32) / np.float32(32768), sc.Geom())
        for kind, cutoff in (("irm", -1.0), ("psm", 2.0), ("crm", -1.0)):
            v = tc.judge_mask(f"cli golden {key}:{kind}", kind, gold[f"cli_{kind}_{key}"], p, cutoff)
            assert v.ok, v.failures


@pytest.mark.parametrize("kind", tc.ORACLE_KINDS)
def test_the_oracle_arithmetic_stays_within_every_cap_and_bar(kind):
    for p in tc.oracle_pairs():
        assert tc.ibm_band_cells(p) == 0          # the ibm waveform cases have one reference
        for k in range(len(p.targets)):
            v = tc.judge_mask(f"{p.name}:{kind}[{k}]", kind, tc.yardstick_mask(kind, p, k=k, oracle=True), p, k=k,
                              oracle=True)
            assert v.ok, v.failures


def test_special_cells_follow_numpy():
    """Silent operands: np.angle(0) = 0, 0 / 0 = NaN, x / 0 = +-inf, and what the clips make of them."""
    target, mixture, both = tc.zeros_pairs()
    ts, m = both.spectra()
    silent = np.flatnonzero(np.abs(m).max(axis=1) == 0)
    assert silent.size == 5                                  # three leading, two trailing frames
    for kind, want in (("iam", np.nan), ("psm", np.nan), ("irm", 0.0), ("ibm", 0.0), ("psa", 0.0)):
        got = tc.clip_formula(tc.mask_formula(kind, ts[0], m), 2.0)[0][silent]
        assert np.array_equal(got, np.full_like(got, want), equal_nan=True), kind
    ts, m = mixture.spectra()
    raw = tc.mask_formula("psm", ts[0], m)[silent]
    assert np.isinf(raw).all() and (raw > 0).any() and (raw < 0).any()
    clipped = tc.clip_formula(raw, 2.0)[0]
    assert set(np.unique(clipped)) == {0.0, 2.0}             # -inf -> 0, +inf -> the cutoff
    assert np.isposinf(tc.clip_formula(tc.mask_formula("iam", ts[0], m), -1.0)[0][silent]).all()


def test_a_wrong_mask_is_caught():
    """What the caps and bars must not hide: one cell off by 1e-4 of itself, a mask computed from a
    spectrum shifted by one bin, a NaN on a cell of its own, one flipped binary decision."""
    p = tc.noise_pairs()[2]
    ts32, m32 = p.spectra(np.complex64)
    good = tc.clip_formula(tc.mask_formula("irm", ts32[0], m32), -1.0)[0]
    assert tc.judge_mask("good", "irm", good, p).ok
    bad = good.copy()
    bad[7, 100] *= 1 + 1e-4
    assert not tc.judge_mask("one cell", "irm", bad, p).ok
    assert not tc.judge_mask("shifted", "irm", np.roll(good, 1, axis=1), p).ok
    bad = good.copy()
    bad[3, 3] = np.nan
    assert not tc.judge_mask("nan", "irm", bad, p).ok
    ibm = tc.mask_formula("ibm", ts32[0], m32)
    assert tc.judge_mask("ibm", "ibm", ibm, p).ok
    _, _, _, skip = tc.mask_allowance("ibm", p)
    t, f = np.argwhere(~skip)[17]
    ibm[t, f] = 1 - ibm[t, f]
    assert not tc.judge_mask("ibm flipped", "ibm", ibm, p).ok


def test_the_wave_measure_catches_a_lost_frame():
    p = tc.noise_pairs()[2]
    rng = np.random.default_rng(3)
    mk = rng.random((p.T, 257)).astype(np.float32)
    y, y32, inp = tc.wave_reference(p, [mk])[0]
    assert tc.judge_wave("yardstick", y32, y, y32, inp, 256).ok
    bad = y32.copy()
    bad[5 * 256:6 * 256] *= np.float32(1 + 1e-4)
    assert not tc.judge_wave("scaled block", bad, y, y32, inp, 256).ok
