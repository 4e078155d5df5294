"""
float64 numpy restatement of AuxIVA as funcwj/setk runs it (scripts/sptk/apply_auxiva.py,
auxiva(), :24-57), vectorised over the frequency bins.  Written from the update rules, none of
the reference's text; the tests check it against recorded outputs of the unmodified reference
(tests/golden/ref_auxiva.npz) and, where the reference tree is present, against the live one.
The GPU tests and tools/bench_auxiva.py use it as the CPU stand-in on the GPU machine.

    W_f = I (complex128),  y_n(f, t) = w_n(f)^H x(f, t)                               (:35-38)
    per epoch:
        r_n(t) = sqrt(sum_f |y_n(f, t)|^2),  g_n(t) = 1 / (r_n(t) + eps_float32)      (:42-44)
        per bin, for n = 0 .. N-1 in order:                                           (:45-52)
            V_n = sum_t g_n(t) x x^H / T
            w = solve(W^H V_n, e_n);   W[:, n] = w / (w^H V_n w)
        y = W^H x                                                                     (:54)
"""
import numpy as np

EPSILON = np.finfo(np.float32).eps  # libs/utils.py:16


def auxiva(X, epochs=20, return_w=False):
    """X: N x T x F complex -> Y: N x T x F complex128 (sources = channels).
    np.linalg.LinAlgError where a bin's W^H V_n is exactly singular, like the reference."""
    X = np.asarray(X)
    N, T, F = X.shape
    x = np.ascontiguousarray(X.transpose(2, 0, 1)).astype(np.complex128)  # F x N x T
    xh = np.ascontiguousarray(x.conj().transpose(0, 2, 1))                 # F x T x N
    W = np.tile(np.eye(N, dtype=np.complex128), (F, 1, 1))                # F x N x N, columns w_n
    eye = np.eye(N, dtype=np.complex128)
    y = np.matmul(W.conj().transpose(0, 2, 1), x)                          # F x N x T
    for _ in range(epochs):
        r = np.sqrt(np.sum(np.abs(y)**2, axis=0))                          # N x T
        g = 1.0 / (r + EPSILON)
        for n in range(N):
            V = np.matmul(x * g[n][None, None, :], xh) / T                 # F x N x N
            A = np.matmul(W.conj().transpose(0, 2, 1), V)
            w = np.linalg.solve(A, np.broadcast_to(eye[:, n:n + 1], (F, N, 1)))[..., 0]  # F x N
            d = np.einsum("fi,fij,fj->f", w.conj(), V, w)
            W[:, :, n] = w / d[:, None]
        y = np.matmul(W.conj().transpose(0, 2, 1), x)
    Y = np.ascontiguousarray(y.transpose(1, 2, 0))                         # N x T x F
    return (Y, W) if return_w else Y


def synth_scene(seed, num_channels, num_samples, fir_len=48, noise=1e-3):
    """num_channels independent speech-like sources (amplitude-modulated coloured noise) mixed
    through short random FIRs, plus a little sensor noise so that no bin is singular.
    Returns float32 C x N, |x| < 1."""
    rng = np.random.default_rng(seed)
    C, N = num_channels, num_samples
    src = np.zeros((C, N))
    for k in range(C):
        e = rng.laplace(size=N)
        # a slow on / off envelope and a one-pole colouring, different per source
        env = np.repeat(rng.uniform(0.05, 1.0, size=N // 800 + 1), 800)[:N]
        a = 0.5 + 0.4 * k / max(C - 1, 1)
        s = np.convolve(e * env, a**np.arange(64))[:N]
        src[k] = s / np.max(np.abs(s))
    mix = np.zeros((C, N))
    for c in range(C):
        for k in range(C):
            h = rng.normal(size=fir_len) * np.exp(-np.arange(fir_len) / 12.0)
            h[0] += 2.0 if c == k else 0.0
            mix[c] += np.convolve(src[k], h)[:N]
    mix += noise * rng.normal(size=mix.shape)
    mix *= 0.5 / np.max(np.abs(mix))
    return mix.astype(np.float32)
