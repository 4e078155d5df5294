"""
covar_cases.py on the CPU: the float32 models of the device's summation orders stay within the
derived allowance A on every case test_gpu_covar_conformance.py runs (the margins are printed), and
seeded faults confined to the weak bins of a `ladder` spectrogram each fail the judge there while
the suite's older measure, rel_rms over all bins at once, does not move.
"""
import numpy as np
import pytest

import covar_cases as cc
import online_model as om


def _judge_model(tally, family, name, got, ref, A):
    tally.fail(cc.structure(name, got))
    tally.add(family, cc.judge(name, got, ref, A))


@pytest.mark.parametrize("C", range(1, 17))
def test_sequential_fold_within_the_allowance_standalone(C):
    """setk_covar's order: one sequential fold per split, the splits summed in order."""
    tally = cc.Tally(f"model setk_covar C={C}")
    for case in cc.standalone_cases(C):
        x, m = cc.standalone_inputs(case)
        ref = cc.reference(x, m)
        got = cc.fold_model(x, m, cuts=cc.standalone_edges(case.T))
        _judge_model(tally, f"{case.spec}/{case.mask}", case.name, got, ref, cc.allowance(x, m, ref))
    tally.finish()


@pytest.mark.parametrize("C", range(1, 17))
def test_sequential_fold_within_the_allowance_fused(C):
    """The fused cases: the float32 yardstick spectra folded in float32, cut at every tile (C <= 8)
    or at the 128-frame slabs (wide: every eighth bin and bin 256, the whole of it through this
    plain model says little more), against the float64 fold of the float64 spectra."""
    tally = cc.Tally(f"model fused C={C}")
    bins = None if C <= 8 else np.r_[0:256:8, 256]
    for case in cc.fused_cases(C, itf=C <= 8 or C in (11, 16)):
        _, X, X32 = cc.spectra(case.audio, C, case.T)
        _, _, es, en = cc.fused_masks(case)
        cuts = range(128, case.T, 128) if C > 8 else cc.fused_edges(C, case.T)
        if bins is not None:
            X32, es, en = X32[:, :, bins], es[:, bins], en[:, bins]
        for (name, ref, A), m in zip(cc.fused_expectation(case, bins), (es, en)):
            got = cc.fold_model(X32.astype(np.complex64), m.astype(np.float32), cuts=cuts)
            _judge_model(tally, case.label, f"{case.name} {name}", got, ref, A)
    tally.finish()


@pytest.mark.parametrize("C,T", [(9, 5), (10, 9), (11, 129), (13, 7), (14, 8), (15, 3), (16, 129), (12, 1)])
def test_matrix_core_order_within_the_allowance(C, T):
    """wide_model.py as it is: the lane maps, the chunks of 8 frames over two half-waves, the
    128-frame slabs and the tile read-out at run-time C, on a few bins of every family."""
    tally = cc.Tally(f"model wide C={C} T={T}")
    F = 3
    for spec in cc.SPEC_FAMILIES:
        x = cc.spectrogram(spec, C, T, F, seed=C)
        for mk in ("uniform", "onehot", "signed", "tiny"):
            m = cc.mask(mk, T, F, seed=C, edges=cc.fused_edges(C, T))
            ref = cc.reference(x, m)
            got = cc.wide_fold_model(x, m)
            _judge_model(tally, f"{spec}/{mk}", f"{spec}/{mk}", got, ref, cc.allowance(x, m, ref))
    tally.finish()


def test_the_long_case_is_the_first_with_an_empty_split():
    split, per, used = cc.standalone_splits(cc.SA_LONG)
    assert (split, per, used) == (64, 33, 63)
    assert all(cc.standalone_splits(T)[0] == cc.standalone_splits(T)[2] for T in range(1, cc.SA_LONG))


def test_case_tables_cover_what_they_promise():
    for C in range(1, 17):
        cases = cc.standalone_cases(C)
        assert {(c.spec, c.mask) for c in cases} == {(s, k) for s in cc.SPEC_FAMILIES for k in cc.SA_MASKS}
        assert {(c.T, c.F) for c in cases} >= {(T, F) for T in cc.SA_FRAMES for F in cc.SA_BINS} | {(2049, 5)}
        assert all(c.F == 5 for c in cases if c.T == cc.SA_LONG)
        fc = cc.fused_cases(C)
        assert {(c.T, c.label) for c in fc} == {(T, k[0]) for T in cc.fused_frames(C) for k in cc.FUSED_MASKS}
        for label in (k[0] for k in cc.FUSED_MASKS):
            assert {c.audio for c in fc if c.label == label} == {"white", "coherent"}
    assert [cc.tile_frames(C) for C in range(1, 9)] == [8, 8, 8, 8, 6, 5, 4, 4]
    # one frame per bin, on both sides of every edge
    m = cc.mask("onehot", 97, 257, edges=cc.standalone_edges(97))
    assert (m.sum(axis=0) == 1).all() and set(np.argmax(m, axis=0)) == {0, 24, 25, 49, 50, 74, 75, 96}
    assert (cc.mask("tiny", 97, 9).sum(axis=0) < 1e-6).all()
    assert cc.mask("signed", 33, 9).min() < 0 and cc.mask("over", 33, 9).max() > 1.5


def test_online_recursion_is_the_online_model():
    """online_recursion restates online_parts without the weights: the same matrices, bit for bit."""
    C, T, chunk = 3, 65, 33
    _, X, X32 = cc.spectra("white", C, T)
    m = cc.mask("uniform", T, cc.BINS, seed=1).astype(np.float64)
    for alpha in cc.ONLINE_ALPHAS:
        mine = cc.online_recursion((X, X32), m, 1 - m, chunk, alpha)
        ref = om.online_parts(np.transpose(X, (0, 2, 1)), m, chunk, alpha)
        assert np.array_equal(mine["Rs"][0], ref["Rs"]) and np.array_equal(mine["Rn"][0], ref["Rn"])
        assert (mine["Rs"][1] > 0).all()


def test_zero_entries_are_held_to_exact_zero():
    x = cc.spectrogram("sparse", 4, 9, 6)
    m = cc.mask("zero", 9, 6)
    ref = cc.reference(x, m)
    A = cc.allowance(x, m, ref)
    assert (A[0::2] == 0).all() and (A[1::2, 2] == 0).all() and (A[1, 0, 0] > 0)
    got = cc.fold_model(x, m)
    v = cc.judge("clean", got, ref, A)
    assert not v.failures and v.zeros == 3 * 16 + 3 * 7
    got[2, 1, 3] = 1e-30
    v = cc.judge("planted", got, ref, A)
    assert v.failures and v.worst == np.inf and v.where == (2, 1, 3, "re")
    assert cc.structure("planted", got)
    got[2, 1, 3] = np.nan
    assert cc.judge("nan", got, ref, A).worst == np.inf


FAULTS = [("drop", "uniform"), ("twice", "uniform"), ("mask_next_bin", "uniform"), ("swap_planes", "uniform"),
          ("pair_off", "uniform"), ("floor_added", "tiny")]


@pytest.mark.parametrize("fault,mk", FAULTS, ids=[f for f, _ in FAULTS])
@pytest.mark.parametrize("C,T,edge", [(5, 65, 6), (5, 65, 36), (7, 129, 128)], ids=["tile6", "slab36", "slab128"])
def test_seeded_faults_fail_in_a_weak_bin(fault, mk, C, T, edge):
    """Odd channel counts.  The fault lives only in the bins of the last quarter of the ladder (levels below 2^-15,
    powers 2^-90 of the loudest bin's): rel_rms over all bins cannot see it, the judge names it."""
    F = 33
    x = cc.spectrogram("ladder", C, T, F, seed=3)
    m = cc.mask(mk, T, F, seed=3)
    ref = cc.reference(x, m)
    A = cc.allowance(x, m, ref)
    cuts = [k for k in range(edge, T, edge)]
    clean = cc.fold_model(x, m, cuts=cuts)
    assert not cc.judge("clean", clean, ref, A).failures
    weak = np.arange(F) >= 3 * F // 4
    got = clean.copy()
    got[weak] = cc.fold_model(x, m, cuts=cuts, fault=fault, at=edge)[weak]
    v = cc.judge(fault, got, ref, A)
    glob = cc.rel_rms(got, ref)
    print(f"[{fault} at frame {edge}, C={C} T={T}] worst ratio {v.worst:.3g} at {v.where}; rel_rms over all bins {glob:.2e}")
    assert v.failures and v.worst > 1 and weak[v.where[0]]
    assert glob < 1e-5
