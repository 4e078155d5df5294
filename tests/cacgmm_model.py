"""
A float64 numpy statement of the CACGMM EM (Ito, Araki, Nakatani, EUSIPCO 2016) as
funcwj/setk's CacgmmTrainer runs it, written from the formulas:

    z(f, t)  = x(f, t) / max(||x(f, t)||_2 over the M channels, eps)       eps = float32 eps
    start a  gamma0 [K, F, T], alpha = 1 / K, q = 1
    start b  (K = 2) B_0 = sum_t z z^H / T, B_1 = I, alpha = 1 / 2, gamma and q from one E-step
    M-step   B_k = M sum_t (gamma_k / q_k) z z^H / max(sum_t gamma_k, eps)
             B <- (B + B^H) / 2;  w, V = eigh(B);  w <- max(w / max(w_max, eps), eps)
             alpha_k = mean_t gamma_k   (update_alpha)
    E-step   B_k^-1 = V diag(1 / w) V^H;  q_k = max(|z^H B_k^-1 z|, eps)
             log p_k = -M log q_k - sum log w;  subtract the max over k
             gamma_k = alpha_k exp(log p_k) / max(sum_k alpha_k exp(log p_k), eps)

The normalisation is done in float64 whatever the input's precision (the device does the same);
the reference does it in the input's precision.  cacgmm_em() returns the posteriors after every
iteration, so that a test can compare an implementation iteration by iteration.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)


def normalise(obs):
    """obs M x F x T complex -> z F x M x T complex128."""
    x = np.asarray(obs).astype(np.complex128)
    norm = np.sqrt(np.sum(x.real ** 2 + x.imag ** 2, axis=0, keepdims=True))
    return np.ascontiguousarray(np.transpose(x / np.maximum(norm, EPS), (1, 0, 2)))


def _decompose(B):
    """K x F x M x M -> scaled, floored eigenvalues K x F x M and eigenvectors."""
    B = (B + np.conj(np.swapaxes(B, -1, -2))) / 2
    w, V = np.linalg.eigh(B)
    w = w / np.maximum(np.amax(w, axis=-1, keepdims=True), EPS)
    return np.maximum(w, EPS), V


def _e_step(z, w, V, alpha):
    """z F x M x T -> (gamma, q), both K x F x T."""
    M = z.shape[1]
    B_inv = np.einsum("...xy,...y,...zy->...xz", V, 1 / w, np.conj(V))
    q = np.einsum("fxt,kfxy,fyt->kft", np.conj(z), B_inv, z)
    q = np.maximum(np.abs(q), EPS)
    logp = -M * np.log(q) - np.sum(np.log(w), axis=-1)[..., None]
    logp = logp - np.amax(logp, axis=0, keepdims=True)
    nom = np.exp(logp) * alpha[..., None]
    return nom / np.maximum(np.sum(nom, axis=0, keepdims=True), EPS), q


def cacgmm_em(obs, num_classes, num_iters, gamma0=None, cgmm_init=False, update_alpha=True):
    """obs M x F x T complex; gamma0 K x F x T (start a) or None with cgmm_init and K = 2 (start
    b).  Returns [gamma after 0 iterations, after 1, ..., after num_iters], each K x F x T
    float64."""
    z = normalise(obs)
    F, M, T = z.shape
    K = int(num_classes)
    alpha = np.full((K, F), 1.0 / K)
    if cgmm_init and K == 2:
        if gamma0 is not None:
            raise ValueError("start b takes no gamma0")
        B = np.stack([np.einsum("fxt,fyt->fxy", z, np.conj(z)) / T,
                      np.broadcast_to(np.eye(M, dtype=np.complex128), (F, M, M))])
        w, V = _decompose(B)
        gamma, q = _e_step(z, w, V, alpha)
    else:
        gamma = np.array(gamma0, dtype=np.float64)
        if gamma.shape != (K, F, T):
            raise ValueError(f"gamma0 must be K x F x T, got {gamma.shape}")
        q = np.ones((K, F, T))
    out = [gamma]
    for _ in range(num_iters):
        den = np.maximum(np.sum(gamma, axis=-1), EPS)
        B = M * np.einsum("kft,fxt,fyt->kfxy", gamma / q, z, np.conj(z)) / den[..., None, None]
        w, V = _decompose(B)
        if update_alpha:
            alpha = np.mean(gamma, axis=-1)
        gamma, q = _e_step(z, w, V, alpha)
        out.append(gamma)
    return out


def random_start(K, F, T):
    """The reference's random start, drawn from numpy's legacy global generator."""
    g = np.random.uniform(size=[K, F, T])
    return g / np.sum(g, 0, keepdims=True)


def scene(C, T, F, num_sources, noise, seed):
    """A small synthetic spectrogram M x F x T complex64: `num_sources` point sources with random
    steering vectors, active on random time-frequency points, plus white noise."""
    rng = np.random.RandomState(seed)
    steer = rng.randn(num_sources, F, C) + 1j * rng.randn(num_sources, F, C)
    act = rng.rand(num_sources, F, T) < 0.6
    sig = (rng.randn(num_sources, F, T) + 1j * rng.randn(num_sources, F, T)) * act
    x = np.einsum("sfc,sft->cft", steer, sig)
    x = x + noise * (rng.randn(C, F, T) + 1j * rng.randn(C, F, T))
    return x.astype(np.complex64)


# The cases the tests and tools/make_cacgmm_golden.py share, F = 5 bins each:
# name: (C, T, K, N, sources, noise, scene seed, start seed or None for the CGMM-like start,
#        update_alpha)
CASES = {
    "c1": (1, 37, 2, 4, 1, 0.1, 11, 101, True),
    "c2": (2, 37, 2, 20, 2, 0.1, 12, 102, True),
    "c3_rankdef": (3, 3, 3, 4, 2, 0.1, 13, 103, True),        # T < C: rank-deficient, floor active
    "c7_chunk": (7, 129, 3, 20, 2, 0.1, 14, 104, True),       # crosses a 128-frame chunk by one
    "c8_k4": (8, 300, 4, 50, 3, 0.1, 15, 105, True),
    "c6_near_singular": (6, 129, 3, 20, 2, 1e-4, 16, 106, True),
    "c8_noise_free": (8, 37, 2, 20, 2, 0.0, 17, 107, True),
    "c8_cgmm_init": (8, 5, 2, 4, 2, 0.1, 18, None, True),
    "c4_cgmm_init_fixed_alpha": (4, 64, 2, 20, 2, 0.1, 19, None, False),
}
CASE_BINS = 5
SNAPSHOTS = (0, 1, 2, 5)  # and the last iteration


def case_inputs(name):
    """(spectrogram M x F x T complex64, gamma0 K x F x T or None, K, N, cgmm_init, update_alpha)."""
    C, T, K, N, ns, noise, seed, start, ua = CASES[name]
    x = scene(C, T, CASE_BINS, ns, noise, seed)
    g0 = None
    if start is not None:
        g0 = np.random.RandomState(start).uniform(size=[K, CASE_BINS, T])
        g0 = g0 / np.sum(g0, 0, keepdims=True)
    return x, g0, K, N, start is None, ua


def snapshots(N):
    return sorted(set(s for s in SNAPSHOTS if s <= N) | {N})
