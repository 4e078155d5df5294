"""
CPU tests of the RIR path: the float64 model of tests/rir_model.py against the reference's recorded
RIRs (tests/golden/ref_rir.npz, written by tools/make_rir_golden.py) and, where the reference tree
and a compiler are present, against the reference generator rebuilt and run live; the float32
pre-processing of setk_amd.libs.rir and the sampler.

The unit of every bound is the case's recorded e_ref = max |reference - model| / peak: the
reference's own float32 noise (`dist` is a float, the taps are summed in float).
"""
import os
import random
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rir_model as rm  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

FIXTURE = rm.load_fixture()
# another libm moves the model by a few float64 ulps of a tap, some 1e-13 of the peak
LIBM_MARGIN = 1.001
needs_reference = pytest.mark.skipif(
    not (rh.available() and os.path.exists(os.path.join(rh.REF_ROOT, "include", "rir-generator.cc"))
         and shutil.which(os.environ.get("CXX", "g++"))),
    reason="the reference tree or a host compiler is not present")


def test_fixture_holds_every_case_of_the_model():
    assert set(FIXTURE) == set(rm.cases())
    for name, c in rm.cases().items():
        got = FIXTURE[name][0]
        for k in ("room", "src", "mics", "angle"):
            assert np.array_equal(got[k], c[k]), (name, k)
        assert np.array_equal(got["beta"], rm.beta_of(c)), name
        assert (got["num_samples"], got["order"], got["hp"], got["mic_type"]) == \
            (c["num_samples"], c["order"], c["hp"], c["mic_type"]), name


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_model_matches_the_recorded_reference(name):
    c, ref, e_ref, _ = FIXTURE[name]
    bnd = []
    model = rm.generate(c, boundary=bnd)
    assert min(bnd) >= 1e-3, "an image within float32 rounding of the inclusion boundary"
    peak = np.max(np.abs(ref))
    e = np.max(np.abs(ref - model)) / peak
    print(f"[{name}] model against the recorded reference: {e:.3e} of the peak (recorded e_ref {e_ref:.3e})")
    assert 0 < e_ref < 1e-4, "the reference's float32 noise: about 1e-5 of the peak"
    assert e <= e_ref * LIBM_MARGIN


def test_integer_delay_case_has_an_image_at_a_whole_sample():
    """cts = 2^-6 and 0.5 m on one axis: the direct path lies at 32 samples exactly, d = 0; without
    the high-pass filter the model's tap 32 holds the bare gain of that image plus the others' tails."""
    c = dict(FIXTURE["integer_delay"][0], hp=False, order=0)
    direct = rm.generate(c)[0]
    assert direct[32] == pytest.approx(1.0 / (4 * np.pi * 0.5), rel=1e-12)
    assert np.max(np.abs(np.delete(direct, 32))) < 1e-15  # sin(pi m) / (pi m), m != 0


@needs_reference
def test_model_matches_the_live_reference(tmp_path):
    import make_rir_golden as tool
    exe = tool.build_driver(rh.REF_ROOT, str(tmp_path))
    for name, c in rm.cases().items():
        if name == "workload":
            continue  # (0.7 s of the reference; the recorded one covers it)
        ref, _ = tool.run_reference(exe, c, str(tmp_path))
        _, recorded, e_ref, _ = FIXTURE[name]
        e = np.max(np.abs(ref - rm.generate(c))) / np.max(np.abs(ref))
        print(f"[{name}] live reference: {e:.3e} of the peak, recorded bits reproduced: {np.array_equal(ref, recorded)}")
        # (another compiler may round the reference's float32 steps differently: twice its noise)
        assert e <= 2 * e_ref


def test_preprocessing_is_the_reference_float32_arithmetic():
    from setk_amd.libs import rir as lr
    for name, c in rm.cases().items():
        if c["rt60"] is not None:
            got = lr.beta_from_rt60(c["room"], c["rt60"], c["c"])
            assert got.dtype == np.float32 and np.array_equal(got, rm.beta_of(c)), name
    assert np.array_equal(lr.beta_from_rt60((4, 5, 2.5), 0.0), np.zeros(6, np.float32))
    # alfa = 24 V ln 10 / (c S T60) = 0.4776 at T60 = 0.1 s for the 4 x 5 x 2.5 m room; above 1 below 0.0478 s
    with pytest.raises(RuntimeError, match="> 1: The reflection coefficients cannot be calculated"):
        lr.beta_from_rt60((4, 5, 2.5), 0.04)
    assert lr.three_decimals((1.23456, 2.0, 0.1004)) == [1.235, 2.0, 0.1]
    with pytest.raises(ValueError, match="six coefficients"):
        lr.make_spec((4, 5, 2.5), (1, 1, 1), [(2, 2, 1)], (0.5, 0.5))
    sp = lr.make_spec((4, 5, 2.5), (1, 1, 1), [(2, 2, 1), (2, 2.1, 1)], 0.3, rir_nsamps=512, angle=0.5)
    assert (sp.n_mics, sp.n_beta, sp.num_samples, sp.order, sp.hp_filter, sp.mic_type) == (2, 6, 512, -1, 1, 4)
    assert [sp.angle[0], sp.angle[1]] == [0.5, 0.0] and sp.mics[4] == np.float32(2.1)
    with pytest.raises(ValueError, match="--microphone-type"):
        lr.make_spec((4, 5, 2.5), (1, 1, 1), [(2, 2, 1)], 0.3, mic_type="figure8")


def test_uniform_sampler_draws_what_the_reference_draws():
    from setk_amd.libs.sampler import UniformSampler
    random.seed(7)
    want = [random.uniform(0.2, 0.7), random.uniform(3.0, 4.0)]
    random.seed(7)
    assert [UniformSampler("0.2,0.7").sample(), UniformSampler((3, 4)).sample()] == want
    s = UniformSampler([1, 2])
    assert (s.min, s.max) == (1, 2)
