"""
The reference side of the solver conformance tests (no GPU): the generators of
tests/solve_cases.py deliver what they claim, the oracle is scale invariant on them where the
reference's text makes it so, the bars of tests/test_gpu_solve.py are consistent with the
project's existing ones on the well-posed families, and the embedding of 9..15-channel
problems (tests/chol_model.py, the model of chol_lds + run_weights) does not depend on the scale
of the input.
"""
import numpy as np
import pytest

import chol_model
import solve_cases as sc
from oracle import np_oracle as o

ALL_SCALES = sc.SCALES + sc.SCALES_WIDE


# ---- generators ------------------------------------------------------------------------------
def _exactly_hermitian(M):
    return (M.dtype == np.complex64 and not np.diagonal(M, axis1=1, axis2=2).imag.any()
            and np.array_equal(M, np.conj(np.transpose(M, (0, 2, 1)))))


@pytest.mark.parametrize("C", sc.CHANNELS)
def test_gap_families_deliver_their_gap(C):
    for gap in sc.GAPS:
        for floor in sc.FLOORS:
            M = sc.rs_gap(C, gap, floor)
            assert M.shape == (sc.F, C, C) and _exactly_hermitian(M)
            assert np.array_equal(M, sc.rs_gap(C, gap, floor))            # seeded
            if C > 1:
                g = sc.achieved_gap(M)
                assert np.all(np.abs(g / gap - 1) < 0.05), (C, gap, floor, g.min(), g.max())
            for scale in ALL_SCALES:                                      # a power of two: exact
                assert np.array_equal(sc.rs_gap(C, gap, floor, scale), M * np.float32(scale))


@pytest.mark.parametrize("C", sc.CHANNELS)
def test_cond_families_deliver_their_cond(C):
    for cond in sc.CONDS:
        for gen in (sc.rn_cond, sc.ry_cond):
            M = gen(C, cond)
            assert M.shape == (sc.F, C, C) and _exactly_hermitian(M)
            assert np.array_equal(M, gen(C, cond))
            if C > 1:
                k = sc.achieved_cond(M)
                assert np.all(np.abs(k / cond - 1) < 0.05), (C, cond, k.min(), k.max())
        assert not np.array_equal(sc.rn_cond(C, cond), sc.ry_cond(C, cond)) or C == 1


@pytest.mark.parametrize("C", sc.CHANNELS)
def test_special_families(C):
    r1 = sc.rs_rank1(C)
    assert _exactly_hermitian(r1)
    ev = np.linalg.eigvalsh(r1.astype(np.complex128))
    assert np.all(np.abs(ev[:, -1] - 1) < 1e-6) and (C == 1 or np.all(np.abs(ev[:, :-1]) < 4 * sc.EPS32))
    d = sc.rs_diagonal(C)
    assert _exactly_hermitian(d) and not d.imag.any()
    off = d.copy()
    i = np.arange(C)
    off[:, i, i] = 0
    assert not off.any()
    assert np.array_equal(np.argmax(np.diagonal(d, axis1=1, axis2=2).real, axis=1), np.arange(sc.F) % C)
    assert set((np.arange(sc.F) % C).tolist()) == set(range(C))         # every position in turn
    re = sc.rs_real(C)
    assert _exactly_hermitian(re) and not re.imag.any()
    if C > 1:
        assert np.all(np.abs(sc.achieved_gap(re) / 0.5 - 1) < 0.05)
    assert np.array_equal(sc.rs_identity(C)[7], np.eye(C, dtype=np.complex64))
    assert not sc.rs_zero(C).any()


def test_perturbation_is_half_an_ulp_and_hermitian():
    M = sc.rs_gap(5, 0.5, 1e-1)
    P = sc.perturb(np.random.default_rng(1), M)
    assert np.array_equal(P, np.conj(np.transpose(P, (0, 2, 1))))
    L = np.tril(M).astype(np.complex128)
    rel = np.abs(np.tril(P).real - L.real) / np.maximum(np.abs(L.real), 1e-300)
    assert rel.max() <= 0.5 * sc.EPS32 and rel.max() > 0.4 * sc.EPS32


# ---- the oracle and the scale ------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8, 12])
def test_oracle_is_scale_invariant_where_the_reference_is(C):
    Rs, Rn = sc.rs_gap(C, 0.5, 1e-1), sc.rn_cond(C, 1e2)
    base_v = o.solve_pevd(Rs.astype(np.complex128), gauge=True)
    base_w = o.mvdr_weight(Rs.astype(np.complex128), Rn.astype(np.complex128), gauge=True)
    base_g = o.solve_pevd(Rs.astype(np.complex128), Rn.astype(np.complex128), gauge=True)
    for scale in ALL_SCALES:
        A = sc.rs_gap(C, 0.5, 1e-1, scale).astype(np.complex128)
        B = sc.rn_cond(C, 1e2, scale).astype(np.complex128)
        assert sc.rel_rms(o.solve_pevd(A, gauge=True), base_v) < 1e-12
        assert sc.rel_rms(o.mvdr_weight(A, B, gauge=True), base_w) < 1e-12
        # v^H Rn v = 1: the pencil vector goes with scale^-1/2
        assert sc.rel_rms(o.solve_pevd(A, B, gauge=True) * np.sqrt(scale), base_g) < 1e-12


def test_ban_and_the_snr_search_are_not_scale_invariant():
    """do_ban and pmwf_weight's SNR search compare with an absolute EPSILON (np_oracle.py:
    `np.maximum(np.real(den), EPSILON)`): below it the answer changes with the scale, which is why
    the GPU tests compare with the oracle evaluated AT each scale and never with an invariance."""
    C = 4
    Rs, Rn = sc.rs_gap(C, 0.5, 1e-1).astype(np.complex128), sc.rn_cond(C, 1e2).astype(np.complex128)
    w = o.mvdr_weight(Rs, Rn, gauge=True)
    s = 2.0 ** -40
    assert sc.rel_rms(o.do_ban(w, Rn * s), o.do_ban(w, Rn)) > 0.5
    snr1 = sc.pmwf_snr(Rs, Rn)
    snr2 = sc.pmwf_snr(Rs * s, Rn * s)
    assert np.max(np.abs(snr2 / snr1 - 1)) > 0.5


# ---- the bars of the GPU file against the project's existing ones --------------------------------
@pytest.mark.parametrize("C", sc.CHANNELS)
def test_plain_eigenvector_bars(C):
    """s is about 2e-8 / gap; on the well-posed families 8 eps32 + 64 s stays below the existing
    1e-4, and the complex64 oracle is itself within 8 eps32 + 8 s of its complex128 self"""
    for gap in sc.GAPS:
        for floor in sc.FLOORS:
            Rs = sc.rs_gap(C, gap, floor)
            rng = np.random.default_rng(sc.seed_of("probe_pevd", C, gap, floor))
            s, truth = sc.sensitivity(sc.op_pevd, (Rs,), rng)
            if C > 1:
                assert 2e-9 / gap < s < 2e-7 / gap, (C, gap, floor, s)
            if sc.well_posed(gap):
                assert 8 * sc.EPS32 + 64 * s < sc.CAP_VEC, (C, gap, floor, s)
            c64 = sc.rel_rms(o.solve_pevd(Rs, gauge=True), truth)
            assert c64 <= 8 * sc.EPS32 + 8 * s, (C, gap, floor, c64, s)


# Where the reference's own complex64 driver (scipy's chegvd, the only step of the oracle that
# really runs in single precision) is further from its complex128 self than the bar, the comparison
# is with the complex128 oracle only: the pencil kinds at cond >= 1e4 (2e-4 .. 2e-3 there), and
# pmwf_r1gev at every cond -- the rank-1 rebuild makes the TRUTH nearly insensitive to the pencil
# vector (s = 3e-8 at 2 channels) while chegvd still loses eps32 * cond (3e-6 at cond 1e2, 3e-5 at
# 1e3, 2 .. 4 channels).
PENCIL_KINDS = ("gevd", "pmwf_r1gev", "mpdr_whiten")


def c64_oracle_excluded(name, cond):
    return name == "pmwf_r1gev" or (name in PENCIL_KINDS and cond >= 1e4)


@pytest.mark.parametrize("C", sc.CHANNELS)
def test_weight_bars_on_the_well_posed_pairs(C):
    kinds = sc.weight_kinds(C)
    for gap, floor, cond in sc.PAIRS:
        case = sc.Case(C, gap, floor, cond)
        c64 = (case.Rs, case.Rn, case.Ry)
        for name, (_, fn, _, _) in kinds.items():
            truth, s = case.truth_and_s(name, fn)
            if sc.capped(name, gap, cond):
                margin = 8 if name in PENCIL_KINDS else 64
                assert 8 * sc.EPS32 + margin * s < sc.CAP_WEIGHT, (C, gap, cond, name, s)
            if c64_oracle_excluded(name, cond):
                continue
            e64 = sc.rel_rms(fn(*c64), truth)
            assert e64 <= 8 * sc.EPS32 + 64 * s, (C, gap, cond, name, e64, s)


# ---- the embedding of 9..15 channels ---------------------------------------------------------------
@pytest.mark.parametrize("C", range(9, 16))
def test_embedded_mvdr_weight_does_not_depend_on_the_scale(C):
    """chol_lds on blkdiag(Rn, pad I): with pad = max diag(Rn) the MVDR weight is numpy's to 1e-12
    at every scale.  (With the constant pad = 1 the floor eps_f32 * max diag sat above every real
    pivot of a covariance below 1.2e-7: test_constant_pad_depends_on_the_scale.)"""
    for scale in ALL_SCALES:
        Rs, Rn = sc.rs_gap(C, 0.5, 1e-1, scale), sc.rn_cond(C, 1e2, scale)
        for f in range(0, sc.F, 32):
            w, truth, status = chol_model.mvdr(Rs[f], Rn[f])
            assert status == 0
            err = np.linalg.norm(w - truth) / np.linalg.norm(truth)
            assert err < 1e-12, (C, scale, f, err)


def test_constant_pad_depends_on_the_scale():
    """the rule the embedding had before (pad = 1): the demonstration of the finding, kept so that
    the model cannot quietly return to it"""
    C = 12
    for scale, broken in ((1.0, False), (2.0 ** -16, False), (2.0 ** -24, True), (2.0 ** -40, True)):
        Rs, Rn = sc.rs_gap(C, 0.5, 1e-1, scale), sc.rn_cond(C, 1e2, scale)
        w, truth, status = chol_model.mvdr(Rs[0], Rn[0], pad=1.0)
        err = np.linalg.norm(w - truth) / np.linalg.norm(truth)
        assert status == 0 and (err > 1e-3) == broken, (scale, err)
    assert chol_model.chol_lds(chol_model.embed(np.zeros((C, C)), pad=1.0))[1] == 0   # not reported


@pytest.mark.parametrize("C", sc.CHANNELS)
def test_model_reports_an_all_zero_or_negative_matrix(C):
    Z = np.zeros((C, C), complex)
    assert chol_model.chol_lds(chol_model.embed(Z))[1] == 1
    assert chol_model.solve(Z, np.ones(C))[1] == 1
    # SETK_FLAG_STRICT_REFERENCE, GEVD: the pencil (Rs, I) stands in, for every C
    L, status, _ = chol_model.chol_lds(chol_model.embed(Z), zero_is_identity=True)
    assert status == 0 and np.array_equal(L, np.eye(chol_model.lanes(C)))
    N = -sc.rn_cond(C, 1e1)[0]
    assert chol_model.chol_lds(chol_model.embed(N))[1] == 1
    G = sc.rn_cond(C, 1e1)[0]
    assert chol_model.chol_lds(chol_model.embed(G))[1:] == (0, False)
