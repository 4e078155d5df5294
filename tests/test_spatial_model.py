"""
tests/spatial_model.py (the float32 restatement of what spatial.hip computes) against the
reference's recorded results in tests/golden/ref_spatial.npz (tools/make_spatial_golden.py), at
BASELINE's operator bar of 1e-4 absolute; raw IPD on the circle.  CPU only.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spatial_model as sm  # noqa: E402
from conftest import load_golden  # noqa: E402

BAR = 1e-4


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_spatial.npz")


def test_fixture_is_small_and_data_only(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_spatial.npz")) < 512 * 1024
    assert all(gold[k].dtype != object for k in gold.files)


@pytest.mark.parametrize("name", sorted(sm.LINEAR))
def test_linear_srp(gold, name):
    C, T, F, D, topo, samp_doa = sm.LINEAR[name]
    S = sm.spec_of(gold[name.split("_")[0] + "_S"])
    assert S.shape == (C, T, F)
    got = sm.srp_linear(S, topo, D, samp_doa)
    assert got.shape == (T, D) and got.dtype == np.float32
    dev = np.abs(got.astype(np.float64) - gold[name + "_srp"]).max()
    print(f"{name}: max |model - reference| = {dev:.3e}")
    assert dev <= BAR


def test_circular_srp(gold):
    C, T, F, D, pairs, n, d = sm.CIRCULAR["circ6"]
    got = sm.srp_circular(sm.spec_of(gold["circ6_S"]), pairs, n, d, D)
    assert got.shape == (T, D)
    assert np.abs(got.astype(np.float64) - gold["circ6_srp"]).max() <= BAR


def test_all_zero_spectrogram_gives_the_tables_row_sum(gold):
    got = sm.srp_linear(np.zeros((4, 37, 33), dtype=np.complex64), sm.LINEAR["lin4"][4], 181)
    assert np.isfinite(got).all()
    assert np.abs(got.astype(np.float64) - gold["zero_srp"]).max() <= BAR
    assert np.array_equal(got, np.broadcast_to(got[0], got.shape))  # every frame is the same row


@pytest.mark.parametrize("key,kw", [("ipd_raw", {}), ("ipd_cos", dict(cos=True)),
                                    ("ipd_cossin", dict(cos=True, sin=True))])
def test_ipd(gold, key, kw):
    got = sm.ipd(sm.spec_of(gold["lin4_S"]), sm.IPD_PAIRS, **kw)
    assert got.shape == gold[key].shape
    if key == "ipd_raw":
        assert sm.circle_distance(got, gold[key]).max() <= BAR
        assert got.min() >= -np.pi - 1e-6 and got.max() < np.pi
    else:
        assert np.abs(got.astype(np.float64) - gold[key]).max() <= BAR


@pytest.mark.parametrize("key", sorted(sm.DF_CASES))
def test_geometry_df(gold, key):
    idx, pairs = sm.DF_CASES[key]
    got = sm.geometry_df(sm.spec_of(gold["lin4_S"]), gold["df_sv"], idx, pairs)
    assert got.shape == gold[key].shape == (37, len(idx) * 33)
    assert np.abs(got.astype(np.float64) - gold[key]).max() <= BAR


def test_end_to_end_inputs_keep_the_derived_bound_small(gold):
    """What the generator asserted, on the stored PCM: with E at BASELINE's STFT bar the bound of
    the end-to-end comparison stays below 0.05 on every cell, so no cell is ever skipped."""
    from oracle import np_oracle as o
    for name, (pairs, weights) in {"e2e_lin": sm.linear_pairs(4),
                                   "e2e_circ": ([(0, 3), (1, 4), (2, 5)], [1 / 3] * 3)}.items():
        x = gold[name + "_pcm"].T.astype(np.float32) / np.float32(32768.0)
        X = np.stack([o.forward_stft(c, frame_len=512, frame_hop=256, window="hann", center=True,
                                     round_power_of_two=True, transpose=True) for c in x])
        xmax, xsum = gold[name + "_xabs"]
        assert np.abs(X).max() == xmax and np.isclose(np.abs(X).astype(np.float64).sum(), xsum, rtol=1e-12)
        bound = sm.e2e_bound(X, 1e-4 * xmax, pairs, gold[name + "_norms"], weights)
        assert bound.shape == (X.shape[1],) and bound.max() < 0.05


def test_msc_raises_with_the_reason():
    from setk_amd import _ffi
    from setk_amd.libs import spatial
    with pytest.raises(_ffi.SetkUnsupported, match="MSC is not ported"):
        spatial.msc(np.zeros((4, 5, 3), dtype=np.complex64), context=1)
    assert "N*T*F" in spatial.MSC_REASON
