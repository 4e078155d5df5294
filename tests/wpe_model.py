"""
A float64 numpy model of the arithmetic of wpe_step_kernel (setk_amd/csrc/wpe.hip), one bin at a
time (no GPU).  It is the second yardstick of wpe_cases.py: what a correct fp64 implementation
with the kernel's own algorithm loses against the extended-precision reference.

  correlation   [R | r] = sum_t (yt / lambda) [yt ; x]^H as real products of the stacked parts,
                accumulated in blocks of four frames (one matrix instruction) over chunks of TC
                staged frames; frames past T are staged as zeros with 1 / lambda = 0
  factorisation right-looking Cholesky of the lower triangle with r carried along; a pivot at or
                below eps64 * NK * max diag drops its column (status 4), an all-zero or
                non-finite R is singular (status 1: x comes back unchanged)
  solve         back substitution L^H G = y
  filter        d = x - G^H yt in float64

It follows the kernel's order of operations where that order is defined by the source; inside a
matrix instruction and inside numpy's products the order is whatever the hardware / BLAS does, so
the model is a yardstick, not a bit-exact twin.

`fault` seeds one defect (test_wpe_cases.py shows that the judge catches each):

  f32_tile      one 8 x 8 tile of R accumulated in float32
  drop_frame    the last frame of every chunk dropped for one tile
  tap_off       the last tap of the correlation read one frame off
  imag_sign     the sign of one tile's imaginary part flipped
  skip_rows64   back-substitution rows >= 64 skipped
  filter_group2 channels >= 4 missing from the filter (its second group of four)
  stale_tail    the TC frames past T of the last chunk not zeroed (the previous chunk's stay)

The tile the tile faults hit is (1, 0), or (0, 0) when R is a single tile.
"""
import numpy as np

FAULTS = ("f32_tile", "drop_frame", "tap_off", "imag_sign", "skip_rows64", "filter_group2", "stale_tail")
NUM_SINGULAR, NUM_RANKDEF = 1, 4
EPS64 = 2.220446049250313e-16


def tap_matrix(x, taps, delay, last_tap_shift=0):
    """x [N][T] -> yt [N taps][T], row k N + n = channel n delayed by k + delay frames."""
    N, T = x.shape
    yt = np.zeros((N * taps, T), x.dtype)
    for k in range(taps):
        d = k + delay + (last_tap_shift if k == taps - 1 else 0)
        if d < T:
            yt[k * N:(k + 1) * N, d:] = x[:, :T - d]
    return yt


def _accumulate(A2, B2, acc_dtype=np.float64, keep=None):
    """sum over blocks of four frames of A2[:, blk] @ B2[:, blk]^T; keep: frames that count."""
    acc = np.zeros((A2.shape[0], B2.shape[0]), acc_dtype)
    if keep is not None:
        A2 = A2 * keep
    for s4 in range(0, A2.shape[1], 4):
        acc = (acc + A2[:, s4:s4 + 4] @ B2[:, s4:s4 + 4].T).astype(acc_dtype)
    return acc.astype(np.float64)


def _complex_of(S, na, nb):
    """R[m][n] = (S[m0][n0] + S[m1][n1]) + i (S[m1][n0] - S[m0][n1]); S rows / columns: all real
    parts, then all imaginary parts."""
    return (S[:na, :nb] + S[na:, nb:]) + 1j * (S[na:, :nb] - S[:na, nb:])


def correlate(x, lam, taps, delay, TC, fault=None):
    """R [NK][NK] (Hermitian, filled from the lower triangle the kernel computes), r [NK][N]."""
    N, T = x.shape
    NK = N * taps
    xd = x.astype(np.complex128)
    yt = tap_matrix(xd, taps, delay, 1 if fault == "tap_off" else 0)
    Tp = -(-T // TC) * TC
    ytp = np.zeros((NK, Tp), np.complex128)
    xp = np.zeros((N, Tp), np.complex128)
    il = np.zeros(Tp)
    ytp[:, :T], xp[:, :T], il[:T] = yt, xd, 1.0 / np.asarray(lam, np.float64)
    if fault == "stale_tail" and Tp > T and Tp > TC:
        ytp[:, T:], xp[:, T:], il[T:] = ytp[:, T - TC:Tp - TC], xp[:, T - TC:Tp - TC], il[T - TC:Tp - TC]
    A2 = np.concatenate([ytp.real, ytp.imag]) * il          # rounded before the product, as staged
    B = np.concatenate([ytp, xp])
    B2 = np.concatenate([B.real, B.imag])
    Rr = _complex_of(_accumulate(A2, B2), NK, NK + N)
    R, r = Rr[:, :NK].copy(), Rr[:, NK:].copy()
    if fault in ("f32_tile", "drop_frame", "imag_sign"):
        I = min(1, (NK + 7) // 8 - 1)
        rows = np.arange(8 * I, min(8 * I + 8, NK))
        cols = np.arange(0, min(8, NK))
        a2 = np.concatenate([A2[rows], A2[NK + rows]])
        b2 = np.concatenate([B2[cols], B2[NK + N + cols]])
        keep = None
        if fault == "drop_frame":
            keep = (np.arange(Tp) % TC != TC - 1).astype(np.float64)
        tile = _complex_of(_accumulate(a2, b2, np.float32 if fault == "f32_tile" else np.float64, keep),
                           len(rows), len(cols))
        if fault == "imag_sign":
            tile = tile.conj()
        R[np.ix_(rows, cols)] = tile
    L = np.tril(R)
    return L + np.tril(L, -1).conj().T, r


def factor_and_solve(R, r, fault=None):
    """(G [NK][N], status): the kernel's Cholesky with the column drop, then L^H G = y."""
    NK, N = r.shape
    R = R.copy()
    G = r.copy()
    diag = R.diagonal().real
    dmax = float(np.fmax.reduce(diag, initial=0.0))
    pfloor = dmax * EPS64 * NK
    idiag = np.zeros(NK)
    status = 0
    for k in range(NK):
        dkk = R[k, k].real
        if not dmax > 0.0 or not np.isfinite(dkk) or not np.isfinite(dmax):
            return None, NUM_SINGULAR
        inv = 1.0 / np.sqrt(dkk) if dkk > pfloor else 0.0
        if not dkk > pfloor:
            status = NUM_RANKDEF
        R[k + 1:, k] *= inv
        G[k] *= inv
        idiag[k] = inv
        li = R[k + 1:, k]
        R[k + 1:, k + 1:] -= np.outer(li, li.conj())
        G[k + 1:] -= np.outer(li, G[k])
    top = 64 if fault == "skip_rows64" else NK
    for k in range(min(top, NK) - 1, -1, -1):
        g = G[k] * idiag[k]
        G[:k] -= np.outer(R[k, :k].conj(), g)
        G[k] = g
    return G, status


def wpe_step(x, lam, taps, delay, TC, fault=None):
    """x [N][T] complex64, lam [T] float64 -> (d [N][T] complex128 before the store's rounding,
    status)."""
    x = np.asarray(x)
    N, T = x.shape
    with np.errstate(all="ignore"):
        R, r = correlate(x, lam, taps, delay, TC, fault)
        G, status = factor_and_solve(R, r, fault)
    xd = x.astype(np.complex128)
    if G is None:
        return xd, status
    pred = G.conj().T @ tap_matrix(xd, taps, delay)
    if fault == "filter_group2":
        pred[4:] = 0.0
    return xd - pred, status


def wpe_step_bins(x, lam, taps, delay, TC, fault=None):
    """x [F][N][T], lam [F][T] -> (d [F][N][T] complex128, status [F])."""
    outs = [wpe_step(x[f], lam[f], taps, delay, TC, fault) for f in range(x.shape[0])]
    return np.stack([o for o, _ in outs]), np.array([s for _, s in outs], np.int32)
