"""
The float64 restatement of wav_simulate.py (tests/simu_model.py) and the float32 emulation of the
device's partitioned convolution against the reference's recorded results
(tests/golden/ref_simu*.npz, tools/make_simu_golden.py).  Runs without a GPU.

Bound: 4 x the case's e_ref of the peak, e_ref being the reference's own worst error against the
float64 model (its float32 FFT convolution and float32 coefficients), recorded in the fixture.  A
case without any float32 arithmetic in the reference (one close-talk speaker) has e_ref = 0 and
must be met exactly.
"""
import numpy as np
import pytest

import simu_model as sm


@pytest.fixture(scope="module")
def gold():
    return sm._golden("ref_simu.npz")


def _noise_of(model, ref):
    # a recipe whose only noise is isotropic: the reference returns the first sample (a scalar)
    return model[2][0] if ref["noise"] is not None and np.ndim(ref["noise"]) == 0 else model[2]


@pytest.mark.parametrize("name", list(sm.CASES))
def test_model_and_emulation_meet_the_reference(gold, name):
    case, ref = sm.load_case(gold, name)
    bound = 4.0 * ref["e_ref"]
    for what, conv in (("float64 model", sm.convolve64), ("float32 partitioned emulation", sm.partitioned32)):
        m = sm.run_simu(case, conv=conv)
        err = sm.worst_error((m[0], m[1], _noise_of(m, ref)), ref)
        print(f"{name}: {what} {err:.3e} of the peak (bound {bound:.3e}, e_ref {ref['e_ref']:.3e})")
        assert err <= bound, (name, what, err, bound)
    assert ref["mix"].shape[-1] == sm.mix_nsamps(case)


def test_partitioned_emulation_is_a_convolution():
    """Unit taps at the block boundaries shift the input; a wrong partition or frame would show as
    an error of order one."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(768).astype(np.float32)
    for R, d in ((600, 0), (600, 255), (600, 256), (600, 257), (600, 599), (256, 255)):
        h = np.zeros((1, R), np.float32)
        h[0, d] = 1.0
        want = np.concatenate([np.zeros(d, np.float32), x])[:768]
        assert np.max(np.abs(sm.partitioned32(x, h)[0] - want)) < 1e-6


def test_doc_case_files():
    """The doc-derived case: the float64 model, written as PCM_16, against the reference's files:
    at most 1 LSB anywhere and at most 0.5 % of the samples differ (the reference against a float64
    run of itself: 1 LSB on 0.06 - 0.09 %)."""
    case, files, e_ref = sm.load_doc_case()
    mix, spk, noise = sm.run_simu(case, conv=sm.fftconvolve64)
    for key, got in (("mix", mix.T), ("spk0", spk[0]), ("spk1", spk[1]), ("noise", noise)):
        worst, frac = sm.pcm_diff(sm.to_pcm16(got), files[key])
        print(f"doc {key}: worst {worst} LSB, {100 * frac:.3f} % differ")
        assert worst <= 1 and frac <= 0.005
    assert 1e-7 < e_ref < 3e-7
