"""
Constructed spectrograms for AuxIVA (numpy only: no audio, no transform, no device), the reference
a device result is held to, and the judge.

MEASURE.  For bin f and source n, with 2-norms over the frames,

    ||got_fn - ref_fn|| <= 2^-24 ||ref_fn|| + m u_fn,     m = 4 (stft_cases.M_BITS)
    u_fn = max(||model - ref||, ||model_reversed - ref||, 2^-40 ||ref_fn||)

  ref      auxiva() restated in np.clongdouble (80-bit): the norms r, g = 1 / (r + eps), the
           weighted covariances, W^H V_n, the solve (an LU of our own with partial pivoting,
           vectorised over the bins; pivot = first largest |re| + |im| of the column), the
           normalisation by w^H V_n w, y = W^H x; the input is the complex64 spectrogram both
           sides receive
  model    auxiva_model.auxiva as it stands (complex128, BLAS sums, LAPACK's solve)
  model_reversed   the same on the frames in reverse order: another summation order
  2^-24    the rounding of a float64 result to complex64: half an ulp per component
  2^-40    a floor: where both yardsticks happen to land closer to the reference, their luck is
           no bar

An element whose reference is exactly zero must come back exactly zero (the frames that are silent
in every bin, for every source), the status must be 0 in every bin and every output finite.

A case has F = 6 bins, one family each, sources = channels:

  0 white   Laplacian sources with slow envelopes (runs of 8 frames) through a random complex
            mixing matrix plus 2 I
  1 levels  channel levels 1, 10, .., 10^(C-1) on strongly coherent channels: the first
            elimination of every bin swaps rows at every step
  2 real    real sources, real mixing matrix: the imaginary part is exactly zero
  3 quiet   as white, at 1e-6 of the other bins' level
  4 ladder  as white, frame levels on a ladder of powers 1e-4 .. 1e2 in runs of 8 frames
  5 tiny    as white at 1e-3; in up to four "tiny" frames the entries have moduli 0.3, 1, 3, 8 x
            float32 eps and every other bin is zero, so that r = |y| of that bin alone is within a
            factor 10 of eps there and g = 1 / (r + eps) differs from 1 / r by a factor up to 4.
            (r is shared by the bins: it cannot be small in a frame unless every bin is.  The
            level 1e-3 of the other frames makes the tiny frames' share of V comparable with the
            others': a^2 / r against eps.)

Three consecutive frames (T // 3 ..) are zero in every bin of every case; the tiny frames precede
them.  The "hard" cases make the last channel of the white bin a near-duplicate of the first
(last = first + 1e-3 x itself): through the shared r its error reaches every other bin, which is
why it has cases of its own.
"""
import os
import sys
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import auxiva_model as am  # noqa: E402

M_BITS = 4.0            # stft_cases.M_BITS: the project's two-bit margin
U32 = 2.0 ** -24
U_FLOOR = 2.0 ** -40
U_CAP = 2.0 ** -28      # the condition on the inputs outside the hard cases
EPS32 = 1.1920928955078125e-07
F = 6
FAMILIES = ("white", "levels", "real", "quiet", "ladder", "tiny")
QUIET, TINY = 3, 5
LD = np.longdouble
CLD = np.clongdouble

CHANNELS = tuple(range(1, 9))
EDGE_T = (31, 32, 33, 127, 128, 129, 257)       # at 1, 2 and 3 epochs, with 4 C + 1
LONG_T = (130, 255, 256, 385)                   # at 2 epochs (130: the T mod 4 = 2 of the table)
HARD_T = (33, 129)                              # every C >= 2
MAX_EPOCHS = 3
# (channels, frames, hard): seed, where the default 100 C + T misses the condition on the inputs
# (test_auxiva_cases.py::test_condition_on_the_inputs) -- none does
SEEDS = {}

LADDER = (1.0, 1e1, 1e2, 1e1, 1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-3, 1e-2, 1e-1)
TINY_LEVEL = 1e-3
TINY_STEPS = (0.3, 1.0, 3.0, 8.0)


@dataclass(frozen=True)
class Case:
    C: int
    T: int
    epochs: int
    hard: bool = False

    @property
    def seed(self):
        return SEEDS.get((self.C, self.T, self.hard), 100 * self.C + self.T)

    @property
    def name(self):
        return f"{'hard ' if self.hard else ''}C={self.C} T={self.T} E={self.epochs}"


def frames_of(C):
    return tuple(sorted({4 * C + 1} | set(EDGE_T)))      # (8 channels: 4 C + 1 is 33)


def cases(C):
    """The table of one channel count (the hard cases apart)."""
    out = [Case(C, T, e) for T in frames_of(C) for e in (1, 2, 3)]
    return out + [Case(C, T, 2) for T in LONG_T]


def hard_cases():
    return [Case(C, T, e, True) for C in CHANNELS[1:] for T in HARD_T for e in (1, 3)]


# ------------------------------------------------------------------ signals
def silent_frames(T):
    return list(range(T // 3, T // 3 + 3))


def tiny_frames(T):
    s0 = T // 3
    return list(range(s0 - min(4, s0), s0))


def _sources(rng, C, T):
    s = rng.laplace(size=(C, T)) + 1j * rng.laplace(size=(C, T))
    env = np.repeat(rng.uniform(0.05, 1.0, size=(C, T // 8 + 1)), 8, axis=1)[:, :T]
    return s * env


def _cn(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _white(rng, C, T):
    return (_cn(rng, C, C) + 2 * np.eye(C)) @ _sources(rng, C, T)


def make_case(C, T, seed, hard=False):
    """X [C][T][F] complex64, the layout setk_auxiva takes."""
    rng = [np.random.default_rng([seed, C, T, f]) for f in range(F)]
    X = np.zeros((F, C, T), np.complex128)
    X[0] = _white(rng[0], C, T)
    if hard:
        X[0, C - 1] = X[0, 0] + 1e-3 * X[0, C - 1]
    A = np.ones((C, C)) * (1 + 0.3j) + 0.2 * _cn(rng[1], C, C)
    X[1] = (10.0 ** np.arange(C))[:, None] * (A @ _sources(rng[1], C, T))
    X[2] = (rng[2].normal(size=(C, C)) + 2 * np.eye(C)) @ _sources(rng[2], C, T).real
    X[3] = 1e-6 * _white(rng[3], C, T)
    lad = np.array([LADDER[(t // 8 + seed) % len(LADDER)] for t in range(T)])
    X[4] = _white(rng[4], C, T) * lad[None]
    X[5] = TINY_LEVEL * _white(rng[5], C, T)
    for k, t in enumerate(tiny_frames(T)):
        X[:5, :, t] = 0.0
        X[5, :, t] *= TINY_STEPS[k] * EPS32 / np.abs(X[5, :, t])
    X[:, :, silent_frames(T)] = 0.0
    return np.ascontiguousarray(X.transpose(1, 2, 0)).astype(np.complex64)


# ------------------------------------------------------------------ the restatement
FAULTS = ("g_f32", "v_f32_quiet", "no_eps", "drop_last_frame_quiet", "unseparated_quiet",
          "sqrt_norm_quiet", "rhs_not_swapped_quiet", "prev_g_last_source_quiet")


def lu_solve(A, b, count=None, keep_rhs=None):
    """A [F][N][N], b [F][N] -> x [F][N]: LU with partial pivoting on every bin at once, the pivot
    the first largest |re| + |im| of the column (LAPACK's ?getf2 / i?amax), substitution.
    count: a list that receives the number of row swaps.  keep_rhs: bins whose right-hand side is
    NOT swapped with the rows (a seeded fault)."""
    A, b = A.copy(), b.copy()
    nb, N, _ = A.shape
    ar = np.arange(nb)
    swap_b = np.ones(nb, bool)
    if keep_rhs is not None:
        swap_b[keep_rhs] = False
    swaps = 0
    for k in range(N):
        mag = np.abs(A[:, k:, k].real) + np.abs(A[:, k:, k].imag)
        p = k + np.argmax(mag, axis=1)                     # argmax: the first of equal maxima
        if not (mag[ar, p - k] > 0).all():
            raise np.linalg.LinAlgError("Singular matrix")
        swaps += int(np.count_nonzero(p != k))
        rk, rp = A[ar, k].copy(), A[ar, p].copy()
        A[ar, k], A[ar, p] = rp, rk
        bk, bp = b[ar, k].copy(), b[ar, p].copy()
        b[ar, k] = np.where(swap_b, bp, bk)
        b[ar, p] = np.where(swap_b | (p == k), bk, bp)
        li = A[:, k + 1:, k] / A[:, k, k][:, None]
        A[:, k + 1:, k:] -= li[:, :, None] * A[:, k, None, k:]
        b[:, k + 1:] -= li * b[:, k, None]
    x = np.zeros_like(b)
    for k in range(N - 1, -1, -1):
        x[:, k] = (b[:, k] - (A[:, k, k + 1:] * x[:, k + 1:]).sum(axis=1)) / A[:, k, k]
    if count is not None:
        count.append(swaps)
    return x


def restated(X, epochs, ctype=CLD, fault=None, count=None):
    """auxiva() of X [N][T][F] in `ctype`, every epoch's y kept: a list of [F][N][T] arrays.
    ctype = np.clongdouble is the reference; np.complex128 with a `fault` of FAULTS is what the
    seeded-fault tests judge.  count: receives the row swaps of every solve."""
    rtype = LD if ctype is CLD else np.float64
    X = np.asarray(X)
    N, T, nb = X.shape
    x = np.ascontiguousarray(X.transpose(2, 0, 1)).astype(ctype)           # F x N x T
    xh = np.ascontiguousarray(x.conj().transpose(0, 2, 1))                  # F x T x N
    W = np.tile(np.eye(N, dtype=ctype), (nb, 1, 1))                        # columns w_n
    eye = np.eye(N, dtype=ctype)
    eps = rtype(EPS32)
    y = x.copy()
    out = []
    for _ in range(epochs):
        r = np.sqrt((y.real ** 2 + y.imag ** 2).sum(axis=0))                # N x T
        g = 1 / (r + eps)
        if fault == "no_eps":        # (a frame that is silent in every bin weighs nothing: its
            g = 1 / np.where(r > 0, r, eps)                                 # weight stays finite)
        if fault == "g_f32":
            g = g.astype(np.float32).astype(rtype)
        for n in range(N):
            V = np.matmul(x * g[n][None, None, :], xh) / T
            q = QUIET
            if fault == "v_f32_quiet":
                V[q] = np.matmul((x[q] * g[n][None]).astype(np.complex64), xh[q].astype(np.complex64)) / T
            if fault == "drop_last_frame_quiet":
                V[q] = np.matmul(x[q, :, :T - 1] * g[n][None, :T - 1], xh[q, :T - 1]) / T
            if fault == "prev_g_last_source_quiet" and n == N - 1 and N > 1:
                V[q] = np.matmul(x[q] * g[n - 1][None], xh[q]) / T
            A = np.matmul(W.conj().transpose(0, 2, 1), V)
            w = lu_solve(A, np.broadcast_to(eye[n], (nb, N)), count,
                         keep_rhs=[q] if fault == "rhs_not_swapped_quiet" else None)
            d = np.einsum("fi,fij,fj->f", w.conj(), V, w)
            if fault == "sqrt_norm_quiet":
                d[q] = np.sqrt(d[q])
            W[:, :, n] = w / d[:, None]
        y = np.matmul(W.conj().transpose(0, 2, 1), x)
        if fault == "unseparated_quiet":
            y[QUIET] = x[QUIET]
        out.append(y)
    return out


def model(X, epochs):
    """auxiva_model.auxiva -> [F][N][T] complex128"""
    return am.auxiva(X, epochs).transpose(2, 0, 1)


def model_reversed(X, epochs):
    """the same with the frames summed in reverse order"""
    Xr = np.ascontiguousarray(np.asarray(X)[:, ::-1])
    return am.auxiva(Xr, epochs)[:, ::-1].transpose(2, 0, 1)


def norm_t(a):
    """2-norm over the frames, in long double -> float64"""
    a = np.asarray(a).astype(CLD)
    return np.sqrt((a.real ** 2 + a.imag ** 2).sum(-1)).astype(np.float64)


class Reference:
    """One case: the input, ref [F][N][T] (clongdouble), its norms, the yardsticks' errors, u."""

    def __init__(self, case, X, ref, swaps):
        self.case, self.X, self.ref, self.swaps = case, X, ref, swaps
        self.norm = norm_t(ref)
        self.err_model = norm_t(model(X, case.epochs) - ref)
        self.err_reversed = norm_t(model_reversed(X, case.epochs) - ref)
        self.u = np.maximum(np.maximum(self.err_model, self.err_reversed), U_FLOOR * self.norm)
        self.allow = U32 * self.norm + M_BITS * self.u
        self.ref128 = ref.astype(np.complex128)
        for a in (self.X, self.ref, self.ref128):
            a.setflags(write=False)


@lru_cache(maxsize=None)
def _data(C, T, hard):
    """The input and the reference after every epoch, computed once per (C, T)."""
    X = make_case(C, T, Case(C, T, 1, hard).seed, hard)
    epochs = 2 if T in LONG_T else MAX_EPOCHS
    count = []
    ys = restated(X, epochs, count=count)
    per_epoch = np.array(count).reshape(epochs, C).sum(axis=1)
    return X, ys, per_epoch


@lru_cache(maxsize=None)
def reference(case):
    """The case's Reference, computed once and shared (read-only)."""
    X, ys, swaps = _data(case.C, case.T, case.hard)
    return Reference(case, X, ys[case.epochs - 1], int(swaps[:case.epochs].sum()))


# ------------------------------------------------------------------ the judge
def judge(name, got, status, R):
    """got [C][T][F] complex64 as the device stored it, status [F] or None, R: a Reference.
    Returns (ratio [F][N] of error to allowance, inf where a rule without a ratio is broken;
    failures: list of strings).  Every (bin, source) is judged."""
    got = np.asarray(got)
    ratio = np.zeros(R.norm.shape)
    if got.shape != R.X.shape:
        return ratio + np.inf, [f"{name}: shape {got.shape} against {R.X.shape}"]
    g = got.transpose(2, 0, 1)
    fails = []
    err = norm_t(g.astype(CLD) - R.ref)
    zero = R.ref == 0
    for f in range(g.shape[0]):
        if status is not None and int(status[f]) != 0:
            fails.append(f"{name}: bin {f} ({FAMILIES[f]}) status {int(status[f])}")
            ratio[f] = np.inf
        for n in range(g.shape[1]):
            where = f"{name}: bin {f} ({FAMILIES[f]}) source {n}"
            if not np.isfinite(g[f, n]).all():
                fails.append(f"{where} holds non-finite values")
                ratio[f, n] = np.inf
                continue
            nz = np.count_nonzero(g[f, n][zero[f, n]])
            if nz:
                fails.append(f"{where}: {nz} elements of an exactly zero reference are not zero")
                ratio[f, n] = np.inf
            if R.norm[f, n] == 0.0:
                continue
            ratio[f, n] = max(ratio[f, n], err[f, n] / R.allow[f, n])
            if not err[f, n] <= R.allow[f, n]:
                fails.append(f"{where} error {err[f, n]:.3e} > allowance {R.allow[f, n]:.3e} "
                             f"(rel {err[f, n] / R.norm[f, n]:.2e}, u rel {R.u[f, n] / R.norm[f, n]:.2e})")
    return ratio, fails


def source_rel_rms(got, R):
    """The older measure: one relative RMS per source over every bin and frame -> [N].
    got [C][T][F]."""
    g = np.asarray(got).transpose(2, 0, 1).astype(np.complex128)
    num = np.sqrt((np.abs(g - R.ref128) ** 2).sum(axis=(0, 2)))
    return num / np.sqrt((np.abs(R.ref128) ** 2).sum(axis=(0, 2)))


def as_stored(y):
    """[F][N][T] of any precision -> [C][T][F] complex64, as the device stores its result"""
    return np.ascontiguousarray(np.asarray(y).transpose(1, 2, 0)).astype(np.complex64)


class Tally:
    """Verdicts of one test: the worst ratio per family and where, and every failure."""

    def __init__(self, form):
        self.form, self.worst, self.failures, self.count = form, {}, [], 0

    def add(self, name, ratio, fails):
        for f, fam in enumerate(FAMILIES):
            w = self.worst.setdefault(fam, [0.0, "", None])
            n = int(np.argmax(ratio[f]))
            if ratio[f, n] >= w[0]:
                w[:] = [float(ratio[f, n]), name, n]
        self.failures += fails
        self.count += ratio.size

    def finish(self):
        for fam in FAMILIES:
            r, name, n = self.worst.get(fam, [0.0, "", None])
            print(f"[{self.form}] {fam:7s} worst ratio {r:.3f} at source {n} ({name})")
        print(f"[{self.form}] {self.count} (bin, source) pairs judged")
        assert not self.failures, f"{len(self.failures)} failures:\n" + "\n".join(self.failures[:25])


def bits(a):
    """the stored bits of a complex64 / float32 array, for bit-for-bit comparisons"""
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ the same bins in a larger F
EMBED_AT = (1, 2, 4, 5, 6, 8)       # where the six bins go among nine


def embedded(X):
    """X [C][T][6] inside nine bins.  The three extra bins are non-zero only in the frames that
    are silent in the six: there the six bins' observations are zero, so whatever r and g come to
    in those frames weighs nothing in their covariances, and in every other frame the extra bins
    add exact zeros to the powers -- r, and with it every result of the six bins, keeps its bits.
    (A copy of `white` in the extra bins would change r in every frame: that cannot be made
    exact.)  The extra bins have three non-zero frames, so at most three channels."""
    C, T, _ = X.shape
    assert C <= 3
    big = np.zeros((C, T, 9), np.complex64)
    big[:, :, EMBED_AT] = X
    rng = np.random.default_rng([C, T, 9])
    for f in sorted(set(range(9)) - set(EMBED_AT)):
        for t in silent_frames(T):
            big[:, t, f] = (_cn(rng, C) + 2 * np.eye(C)[t % C]).astype(np.complex64)
    return big
