"""
numpy model of chol_lds (setk_amd/csrc/solve.hip) together with the embedding run_weights
(capi_modular.hip) and pack_covar_kernel use for 9..15 channels: the pivot floor at eps_f32 * max diag,
the second attempt with 8 * floor added to the diagonal, the status, and blkdiag(M, pad * I) with
pad = max_i Re M[i][i] of the bin.  The kernel's arithmetic is float64 and so is the model's.
tests/test_solve_cases.py states the property the embedding has to give (no GPU needed); the GPU
tests check the kernel itself.
"""
import numpy as np

EPS32 = 1.1920928955078125e-07


def lanes(C):
    """problem size the kernel solves: 1..8 as they are, 9..16 as 16 x 16"""
    return 16 if C > 8 else C


def embed(M, pad_diag=1.0, pad=None):
    """blkdiag(M, pad * I) of size lanes(C); pad = pad_diag * max diag(M) unless given (the rule
    before this model existed was the constant pad = 1)"""
    C = M.shape[0]
    Cp = lanes(C)
    if Cp == C:
        return M.astype(complex)
    if pad is None:
        pad = pad_diag * float(np.max(M.diagonal().real))
    P = np.zeros((Cp, Cp), complex)
    P[:C, :C] = M
    i = np.arange(C, Cp)
    P[i, i] = pad
    return P


def chol_lds(M, zero_is_identity=False):
    """(L, status, loaded): status 1 = SETK_NUM_SINGULAR (all-zero / negative-diagonal / NaN pivot)"""
    C = M.shape[0]
    scale = float(np.max(M.diagonal().real))
    if zero_is_identity and scale == 0.0:
        return np.eye(C, dtype=complex), 0, False
    bad0 = not scale > 0.0
    floor_piv = EPS32 * scale
    load = 0.0
    for attempt in range(2):
        hit = False
        bad = bad0
        L = np.zeros((C, C), complex)
        A = M.astype(complex).copy()
        A[np.diag_indices(C)] += load
        for k in range(C):
            s = A[k:, k] - L[k:, :k] @ L[k, :k].conj()
            d = s[0].real
            if d != d:
                bad = True
            if not d >= floor_piv:
                hit = True
            d = max(d, floor_piv) if d == d else floor_piv
            rd = 1.0 / np.sqrt(d) if d > 0.0 else 0.0
            L[k, k] = d * rd
            L[k + 1:, k] = s[1:] * rd
        if attempt == 1 or not (hit and not bad0):
            break
        load = 8.0 * floor_piv
    return L, int(bad), load != 0.0


def solve(M, b, pad=None, zero_is_identity=False):
    """M^-1 b through the embedded, floored / loaded factorisation: (x, status, loaded)"""
    C = M.shape[0]
    P = embed(M, pad=pad)
    L, status, loaded = chol_lds(P, zero_is_identity)
    if status:
        return None, status, loaded
    bp = np.zeros(P.shape[0], complex)
    bp[:C] = b
    y = np.linalg.solve(L, bp)
    x = np.linalg.solve(L.conj().T, y)
    return x[:C], status, loaded


def mvdr(Rs, Rn, pad=None):
    """(model weight, numpy weight, status): steering vector from numpy on both sides, so the
    difference is the factorisation's alone"""
    Rs = Rs.astype(complex)
    Rn = Rn.astype(complex)
    _, v = np.linalg.eigh(Rs)
    d = v[:, -1]
    d = d * np.conj(d[0]) / abs(d[0]) if abs(d[0]) > 0 else d
    x, status, _ = solve(Rn, d, pad=pad)
    if status:
        return None, None, status
    truth = np.linalg.solve(Rn, d)
    return x / np.vdot(d, x), truth / np.vdot(d, truth), status
