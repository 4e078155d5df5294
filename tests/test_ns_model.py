"""
tests/ns_model.py (the float64 restatement of the reference's libs/ns.py that the GPU tests lean
on) against the reference's own recorded gains in tests/golden/ref_ns.npz, and the host-side
pieces of setk_amd/libs/ns.py that need no GPU.
"""
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ns_model  # noqa: E402
from conftest import load_golden  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_ns.npz")


@pytest.mark.parametrize("name", sorted(ns_model.CASES))
def test_model_reproduces_the_recorded_reference_gains(gold, name):
    kind, T, F, _, conf = ns_model.CASES[name]
    stft = gold[name + "_stft"]
    assert stft.shape == (T, F)
    assert np.array_equal(stft, ns_model.synth_spectrogram(T, F, int(gold[name + "_seed"])))
    info = {}
    model, margin = ns_model.run(kind, stft, **conf) if kind == "mcra" else ns_model.imcra(stft, info=info, **conf)
    want = gold[name + "_gain"]
    err = float(np.max(np.abs(model - want) / np.abs(want)))
    print(f"{name}: model vs reference {err:.3e} (generator: {float(gold[name + '_model_err']):.3e}), "
          f"margin {margin:.3e}")
    # what is left is the reference's numerical integral of exp(-t) / t (scipy.integrate.quad
    # stops at 1.5e-8); the figure the generator recorded, reproduced here
    assert err <= float(gold[name + "_model_err"]) * 1.001 + 1e-13
    assert err <= float(gold["model_err_worst"]) <= 1e-6
    assert margin == float(gold[name + "_margin"]) and margin >= ns_model.MIN_MARGIN
    assert info.get("clamped", 0) == 0


def test_model_on_the_command_line_fixture(gold):
    """The reference's command line computes on a complex64 STFT, partly in float32: the float64
    model on the same STFT stays within the figure the generator recorded."""
    from oracle import np_oracle as o
    x = gold["cli_pcm"].astype(np.float32) / np.float32(32768.0)
    X = o.forward_stft(x, frame_len=512, frame_hop=256, window="hann", center=True, round_power_of_two=True,
                       transpose=True)
    model, margin = ns_model.imcra(X)
    want = gold["cli_gain"]
    err = float(np.max(np.abs(model - want) / np.abs(want)))
    print(f"cli: model vs the command line's gain {err:.3e}, margin {margin:.3e}")
    assert model.shape == want.shape == (76, 257)
    assert err <= float(gold["cli_model_err"]) * 1.001 + 1e-13 and err < 1e-5
    assert gold["cli_wav"].shape == (19200,) and gold["cli_wav"].dtype == np.int16


def test_cases_reach_their_branches(gold):
    # MCRA's second minimum reset (t + 1 = 135) and ten iMCRA blocks of V = 15 frames in (a);
    # F below M // 2 + 1 and just above the 31 taps of w_global in (c); a ring over several blocks in (d)
    assert ns_model.CASES["a_mcra"][1] >= 135 and ns_model.CASES["a_imcra"][1] // 15 == 10
    assert 31 < ns_model.CASES["c_mcra"][2] < 65
    d = ns_model.CASES["d_imcra"]
    assert d[4]["U"] > d[4]["V"] and d[1] // d[4]["V"] >= 4 and d[4]["w_mcra"] == 2
    assert ns_model.CASES["b_mcra"][2] == 257


def test_windows_are_scipys_periodic_ones():
    import scipy.signal
    from setk_amd.libs.ns import smoothing_window
    assert np.allclose(ns_model.window("hann", 1), [0.0, 0.75, 0.75], rtol=0, atol=1e-15)
    for name in ("hann", "hamming", "blackman"):
        for half in (0, 1, 2, 15, 31):
            want = scipy.signal.get_window(name, 2 * half + 1)
            assert np.allclose(ns_model.window(name, half), want, rtol=0, atol=1e-15)
            got = smoothing_window(name, half)
            assert got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-15), (name, half)
    assert np.array_equal(smoothing_window("hann", 1), scipy.signal.get_window("hann", 3))  # the same bits


def test_window_refusals_need_no_gpu():
    from setk_amd import _ffi
    from setk_amd.libs import ns
    with pytest.raises(ValueError, match="unknown window"):
        ns.MCRA(h_local="kaiser")
    with pytest.raises(ValueError, match="unknown window"):
        ns.iMCRA(h_mcra=("tukey", 0.5))
    with pytest.raises(_ffi.SetkUnsupported, match="at most 63"):
        ns.iMCRA(w_mcra=32)
    assert ns.MCRA(w_global=31).opts().n_global == 63


def test_constructors_keep_the_reference_signatures():
    from setk_amd.libs import ns
    for cls, defaults in ((ns.MCRA, ns_model.MCRA_DEFAULTS), (ns.iMCRA, ns_model.IMCRA_DEFAULTS)):
        sig = inspect.signature(cls.__init__)
        got = {k: p.default for k, p in sig.parameters.items() if k != "self"}
        assert list(got) == list(defaults) and got == defaults
        assert list(inspect.signature(cls.run).parameters) == ["self", "stft", "eps"]
        assert inspect.signature(cls.run).parameters["eps"].default == 1e-7
    o = ns.iMCRA(b_min=2.0, gmin_db=-20, xi_min_db=-10, V=5, U=8).opts(eps=1e-6, gain=True, spec=True)
    assert (o.inv_b_min, o.gmin, o.xi_min, o.V, o.U, o.eps, o.flags, o.kind) == (0.5, 0.01, 0.1, 5, 8, 1e-6, 3, 1)
    m = ns.MCRA(zeta_min_db=-20, zeta_p_max_db=20, L=50, M=64).opts()
    assert (m.zeta_min, m.zeta_p_max, m.L, m.M, m.n_mcra, m.n_local, m.n_global, m.kind) == \
        (0.01, 100.0, 50, 64, 3, 3, 31, 0)


def test_model_stays_finite_through_digital_silence():
    stft = ns_model.synth_spectrogram(60, 65, 4)
    stft[20:40] = 0
    info = {}
    g, _ = ns_model.imcra(stft, info=info)
    assert np.isfinite(g).all() and info["clamped"] == 20 * 65
    g, _ = ns_model.mcra(stft)
    assert np.isfinite(g).all()
