"""
spatial_cases.py on the CPU: the float64 reference reproduces the reference project's recorded
results (tests/golden/ref_spatial.npz) to their own float32 rounding; the float32 model of the
kernels (spatial_model.py, spatial_cases.srp_model) stays within the derived allowance of every cell
on every family, so the allowance is attainable by honest float32 arithmetic; and seeded faults,
each confined to one pair, tile, bin or column, all fail the judge -- the table says which of them
the flat bar of test_gpu_spatial.py (max |device - reference| <= 1e-4 on the whole map) would have
seen.  Figures: PARITY_NOTES_SPATIAL.md.
"""
import numpy as np
import pytest

import spatial_cases as sc
import spatial_model as sm
from conftest import load_golden

IPD_PAIRS = [(0, 1), (3, 1), (2, 2), (0, 1)]        # forward, reversed, (l, l), repeated
T0, F0, D0 = 33, 33, 65


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_spatial.npz")


# ---------------------------------------------------------------- the reference against the recorded results
def test_float64_reference_reproduces_the_recorded_results(gold):
    """The difference is the reference project's own float32 rounding (np.angle of complex64, maps
    stored as float32) plus, for SRP, the table's one rounding to complex64."""
    worst = {}
    for name, (C, T, F, D, topo, samp_doa) in sm.LINEAR.items():
        S = sm.spec_of(gold[name.split("_")[0] + "_S"])
        pairs, w = sm.linear_pairs(C)
        table = sc.pack_table([sm.linear_grid(topo[j] - topo[i], F, D, samp_doa) for i, j in pairs])
        worst[name] = np.abs(sc.ref_srp(S, pairs, table, D).combined(w)[0] - gold[name + "_srp"]).max()
    C, T, F, D, pairs, n, d = sm.CIRCULAR["circ6"]
    table = sc.pack_table([sm.diag_grid(min(i, j) * np.pi * 2 / n, d, F, D) for i, j in pairs])
    ref = sc.ref_srp(sm.spec_of(gold["circ6_S"]), pairs, table, D).combined([1 / 3] * 3)[0]
    worst["circ6"] = np.abs(ref - gold["circ6_srp"]).max()
    C, T, F, D, topo, _ = sm.LINEAR["lin4"]
    pairs, w = sm.linear_pairs(C)
    table = sc.pack_table([sm.linear_grid(topo[j] - topo[i], F, D) for i, j in pairs])
    ref = sc.ref_srp(np.zeros((C, T, F), np.complex64), pairs, table, D).combined(w)[0]
    worst["zero"] = np.abs(ref - gold["zero_srp"]).max()
    S = sm.spec_of(gold["lin4_S"])
    for key, kind in (("ipd_raw", "ipd"), ("ipd_cos", "cos_ipd"), ("ipd_cossin", "cos_sin_ipd")):
        ref = sc.ref_ipd(S, sm.IPD_PAIRS, kind)
        worst[key] = (sm.circle_distance(ref, gold[key]) if kind == "ipd" else np.abs(ref - gold[key])).max()
    for key, (idx, pairs) in sm.DF_CASES.items():
        worst[key] = np.abs(sc.ref_df(S, gold["df_sv"], idx, pairs or sc.all_pairs(4))[0] - gold[key]).max()
    for k, v in worst.items():
        print(f"float64 reference against the recorded {k}: max difference {v:.3e}")
    assert max(worst.values()) <= sc.BAR


# ---------------------------------------------------------------- the float32 model under the judge
def srp_inputs(family, C, T, F, D, samp_doa=True):
    S = sc.spectrogram(family, C, T, F)
    pairs, table, w = sc.linear_tables(C, F, D, samp_doa)
    return S, pairs, table, w


def sm_srp(S, pairs, table, w, D):
    return sm.srp(S, pairs, [table[p][:, :D] for p in range(len(pairs))], w)


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_the_float32_model_passes_the_judge(family):
    tally = sc.Tally(f"model {family}")
    C = 5
    S = sc.spectrogram(family, C, T0, F0)
    for kind, kw in zip(sc.KINDS, ({}, dict(cos=True), dict(cos=True, sin=True))):
        got = sm.ipd(S, IPD_PAIRS, **kw)
        tally.add(kind, sc.judge(f"{family} {kind}", got, sc.ref_ipd(S, IPD_PAIRS, kind), sc.ipd_allowance(kind),
                                 circle=kind == "ipd"))
        if kind == "ipd":
            tally.fail(sc.ipd_range(f"{family} ipd", got, S, IPD_PAIRS))
    sv = sc.steer(7, C, F0)
    for idx, pairs in (([2, 0, 5], sc.all_pairs(C)), ([6, 6], IPD_PAIRS)):
        ref, A = sc.ref_df(S, sv, idx, pairs)
        tally.add("df", sc.judge(f"{family} df {idx}", sm.geometry_df(S, sv, idx, pairs), ref, A))
    for C in (4, 16) if family == "white" else (4,):
        S, pairs, table, w = srp_inputs(family, C, T0, F0, D0)
        if family == "nan":                     # the pairs the NaN does not touch ...
            keep = [p for p, (l, r) in enumerate(pairs) if C - 1 not in (l, r)]
            sub = [pairs[p] for p in keep], table[keep], [1 / len(keep)] * len(keep)
            ref, A = sc.ref_srp(S, sub[0], sub[1], D0).combined(sub[2])
            assert np.isfinite(ref).all()
            tally.add("srp", sc.judge("nan srp, untouched pairs", sm_srp(S, *sub, D0), ref, A))
        r = sc.ref_srp(S, pairs, table, D0)
        ref, A = r.combined(w)
        assert np.isfinite(ref).all() == (family != "nan")       # ... and all of them: every cell a NaN
        tally.add("srp", sc.judge(f"{family} srp C={C}", sm_srp(S, pairs, table, w, D0), ref, A))
        tally.add("srp", sc.judge(f"{family} srp_model C={C}", sc.srp_model(S, pairs, table, w, D0), ref, A))
        p = len(pairs) - 1
        hot = np.eye(len(pairs))[p]
        tally.add("srp one pair", sc.judge(f"{family} g_{p} C={C}", sc.srp_model(S, pairs, table, hot, D0),
                                           *r.combined(hot)))
    tally.finish()


def test_the_float32_model_at_every_modulus_of_complex64():
    """phasor() as the kernels have it, from the smallest subnormal to the largest float32."""
    S = sc.moduli_grid()
    assert np.isfinite(S.view(np.float32)).all()
    tally = sc.Tally("model moduli")
    for kind, kw in zip(sc.KINDS, ({}, dict(cos=True), dict(cos=True, sin=True))):
        got = sm.ipd(S, [(0, 1), (1, 0)], **kw)
        tally.add(kind, sc.judge(kind, got, sc.ref_ipd(S, [(0, 1), (1, 0)], kind), sc.ipd_allowance(kind),
                                 circle=kind == "ipd"))
    tally.finish()


def test_lattice_holds_an_exact_plus_pi():
    S = sc.spectrogram("lattice", 5, T0, F0)
    ref = sc.ref_ipd(S, [(0, 1), (1, 0)], "ipd")
    assert ref[0, 0] == -np.pi and ref[0, F0] == -np.pi and (ref == -np.pi).sum() > 2
    assert (ref >= -np.pi).all() and (ref < np.pi).all()
    assert (S[2] == 0).all() and (S[:, T0 // 2] == 0).all()


# ---------------------------------------------------------------- seeded faults
def fault_table():
    """[(name, verdict failures under the judge, seen by the flat bar)]"""
    rows = []

    def srp_fault(name, family, C, T, F, D, fault, at, dirty=None, hot=False, **kw):
        S, pairs, table, w = srp_inputs(family, C, T, F, D)
        r = sc.ref_srp(S, pairs, table, D)
        if hot:
            w = np.eye(len(pairs))[at]
        ref, A = r.combined(w)
        clean = sc.judge(name, sc.srp_model(S, pairs, table, w, D), ref, A)
        assert not clean.failures, clean.failures        # the same model without the fault passes
        got = sc.srp_model(S, pairs, table if dirty is None else dirty(table), w, D, fault=fault, at=at, **kw)
        rows.append((name, sc.judge(name, got, ref, A).failures, sc.old_bar_sees(got, ref)))

    def unzeroed(table):
        t = table.copy()
        t[:, :, D0:] = np.float32(1.25) * t[:, :, :t.shape[2] - D0]      # (what was left there: louder columns)
        return t

    srp_fault("one bin dropped in pair 77 of 120 (all-pairs sum)", "coherent", 16, 4, 129, D0, "drop_bin", 77)
    srp_fault("one bin dropped in pair 77 of 120 (one-hot weight)", "coherent", 16, 4, 129, D0, "drop_bin", 77,
              hot=True)
    srp_fault("normaliser of pair 2 over one 32-frame tile", "coherent", 4, 65, F0, D0, "tile_norm", 2)
    srp_fault("normaliser of pair 3 over d < Dpad, padding not zeroed", "white", 4, T0, F0, D0, "pad_norm", 3,
              dirty=unzeroed)
    srp_fault("floor after the weighted sum", "white", 4, T0, F0, D0, "late_floor", 0)
    srp_fault("last frame of a partial tile stale in pair 77 of 120", "white", 16, T0, F0, D0, "stale_frame", 77)

    S = sc.spectrogram("white", 5, T0, F0)
    got = sm.ipd(S, IPD_PAIRS, cos=True, sin=True)
    got[:, 1 * 2 * F0 + F0:2 * 2 * F0] *= -1                                   # pair (3, 1): its sine
    ref = sc.ref_ipd(S, IPD_PAIRS, "cos_sin_ipd")
    rows.append(("sinIPD: sign of the reversed pair lost", sc.judge("sin", got, ref, sc.ipd_allowance("cos_sin_ipd"))
                 .failures, sc.old_bar_sees(got, ref)))

    sv = sc.steer(7, 5, F0)
    short = [(0, 1), (3, 1), (2, 4)]
    got = (sm.geometry_df(S, sv, [2], short) * np.float32(len(short)) / np.float32(10)).astype(np.float32)
    ref, A = sc.ref_df(S, sv, [2], short)
    rows.append(("DF divided by C (C - 1) / 2 under a shorter pair list", sc.judge("df", got, ref, A).failures,
                 sc.old_bar_sees(got, ref)))

    S = sc.spectrogram("lattice", 5, T0, F0)
    got = sm.ipd(S, IPD_PAIRS)
    got[got == -sc.PI32] = sc.PI32                                             # the wrap left out
    ref = sc.ref_ipd(S, IPD_PAIRS, "ipd")
    fails = sc.judge("ipd", got, ref, sc.ipd_allowance("ipd"), circle=True).failures + \
        sc.ipd_range("ipd", got, S, IPD_PAIRS)
    rows.append(("raw IPD of +pi left unwrapped", fails, sc.old_bar_sees(got, ref, circle=True)))
    return rows


def test_every_seeded_fault_fails_the_judge():
    rows = fault_table()
    print(f"{'fault':62s} {'judge':8s} flat 1e-4 bar")
    for name, fails, old in rows:
        print(f"{name:62s} {'FAILS' if fails else 'passes':8s} {'sees it' if old else 'blind'}")
    assert len(rows) >= 6
    assert all(fails for _, fails, _ in rows), [name for name, fails, _ in rows if not fails]
    assert any(not old for _, _, old in rows)
