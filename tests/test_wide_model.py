"""
What the construction of setk_amd/csrc/wide.hip has to give, on its numpy model (tests/wide_model.py;
no GPU): the stacking identity against the oracle's compute_covar, exact Hermitian symmetry in
float32, exact zeros out of the padded rows and out of whatever stands behind the last frame, and
the 9..15-channel embedding the weight solve expects (tests/chol_model.py).
"""
import numpy as np
import pytest

import chol_model
import wide_model as wm
from oracle import np_oracle as o


def _bin(C, T, seed, stale=np.nan):
    """One bin: observations [C][Tp] with `stale` behind the last frame, a mask [T]."""
    rng = np.random.default_rng(seed)
    Tp = (T + 3) & ~3
    x = np.full((C, max(Tp, 8 * -(-T // 8))), complex(stale, stale), np.complex128)
    x[:, :T] = rng.standard_normal((C, T)) + 1j * rng.standard_normal((C, T))
    return x, rng.uniform(0.05, 0.95, T)


@pytest.mark.parametrize("C", [9, 12, 16])
@pytest.mark.parametrize("T", [1, 3, 65, 129, 264])
def test_stacking_identity_against_the_oracle(C, T):
    x, m = _bin(C, T, 100 * C + T)
    ref = o.compute_covar(x[:, None, :T], m[:, None])[0]
    got = wm.matrix_of_planes(wm.covar_planes(x, m, C, T, np.float64), C)
    assert np.max(np.abs(got - ref)) < 1e-12 * np.max(np.abs(ref))
    # the all-ones covariance normalised by the frame count (MPDR's Ry)
    ref = o.compute_covar(x[:, None, :T], np.ones((T, 1)))[0]
    got = wm.matrix_of_planes(wm.covar_planes(x, np.ones(T), C, T, np.float64, den=T), C)
    assert np.max(np.abs(got - ref)) < 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("C", [9, 13, 16])
def test_float32_result_is_hermitian_bit_for_bit(C):
    T = 131
    x, m = _bin(C, T, 7 + C)
    planes = wm.covar_planes(x.astype(np.complex64), m.astype(np.float32), C, T, np.float32)
    assert planes.dtype == np.float32
    R = wm.matrix_of_planes(planes, C)
    assert np.max(np.abs(R - R.conj().T)) == 0 and np.max(np.abs(R.diagonal().imag)) == 0
    # and the tile's own diagonal of B^T - B is an exact zero before anything is mirrored
    assert not planes[wm.NP16 + np.array([wm.pair_index(i, i) for i in range(C)])].any()
    ref = o.compute_covar(x[:, None, :T], m[:, None])[0]
    assert np.max(np.abs(R - ref)) < 1e-5 * np.max(np.abs(ref))


@pytest.mark.parametrize("C", [9, 12, 15])
def test_padded_rows_and_stale_frames_give_exact_zeros(C):
    T = 13  # an odd last frame, three frames of pitch padding, a short last chunk
    x, m = _bin(C, T, 31 + C, stale=np.nan)
    G = wm.slab_tile(x.astype(np.complex64), m.astype(np.float32), C, 0, T, np.float32)
    assert np.isfinite(G).all()
    assert not G[2 * C:].any() and not G[:, 2 * C:].any()
    # through the register image and back: the result map is a bijection onto the tile
    assert np.array_equal(wm.tile_of_regs(wm.result_regs(G)), G)
    planes = wm.pairs_of_tile(G, C)
    inside = np.zeros(wm.NP16, bool)
    inside[[wm.pair_index(j, k) for j in range(C) for k in range(j, C)]] = True
    assert not planes[:wm.NP16][~inside].any() and not planes[wm.NP16:][~inside].any()
    # an infinite stale value must not reach a sum either
    x2, _ = _bin(C, T, 31 + C, stale=np.inf)
    assert np.array_equal(wm.slab_tile(x2.astype(np.complex64), m.astype(np.float32), C, 0, T, np.float32), G)


@pytest.mark.parametrize("C", [9, 11, 15, 16])
def test_embedding_is_the_one_the_solve_expects(C):
    T = 40
    x, m = _bin(C, T, 57 + C)
    for pad_diag in (0.0, 1.0):  # Rs | the matrices that get factored
        planes = wm.covar_planes(x, m, C, T, np.float64, pad_diag=pad_diag)
        R = wm.matrix_of_planes(planes, C)
        assert chol_model.lanes(C) == wm.CP
        want = chol_model.embed(R, pad_diag=pad_diag)
        assert np.array_equal(wm.matrix_of_planes(planes), want)
    # the padded problem has the original's solution in its first C components
    Rn = wm.matrix_of_planes(wm.covar_planes(x, 1 - m, C, T, np.float64, pad_diag=1.0))
    d = np.zeros(wm.CP, complex)
    d[:C] = np.arange(1, C + 1)
    sol, status, _ = chol_model.solve(Rn[:C, :C], d[:C])
    full = np.linalg.solve(Rn, d)
    assert status == 0 and np.allclose(full[:C], sol[:C], rtol=1e-9, atol=0) and not full[C:].any()
