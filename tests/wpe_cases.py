"""
Constructed cases for one WPE step (numpy only: no audio, no transform, no device), the reference
a device result is held to, and the judge.

MEASURE.  For bin f and channel c, with norms over the frames,

    ||got - ref||_2 <= 2^-24 ||ref_fc||_2 + m u_fc,     m = 4 (stft_cases.M_BITS)
    u_fc = max(||oracle - ref||_2, ||model - ref||_2, 2^-53 NK ||x_fc - ref_fc||_2)

  ref     wpe_step restated in np.clongdouble (80-bit): tap matrix, R and r with 1 / lambda,
          Cholesky, the two substitutions, x - G^H yt; the input is the complex64 spectrogram both
          sides receive, lambda the float64 array as given
  oracle  oracle.np_oracle.wpe_step in complex128 (einsum + LAPACK's pivoted LU)
  model   wpe_model.wpe_step: the kernel's own arithmetic in float64
  2^-24   the rounding of an fp64 result to complex64: half an ulp per component
  the third term is a floor of one fp64 rounding per tap row on the predicted part: where both
  yardsticks happen to land closer to the reference than that, their luck is no bar

A channel whose reference is exactly zero must come back exactly zero, and the status must be 0
unless the case says otherwise.

SHAPES labels every (channels, taps) with the kernel form it is meant to run -- tiles per wavefront
of the LDS instantiation or "wide", and the staged chunk -- test_wpe_cases.py holds the labels to
the library's own answer (setk_wpe_form).  8 x 9 needs exactly 14 tiles per wavefront; 9 x 7 is there
for the 13 that run <14> with dead tile slots.

A case has F = 4 bins, one signal family each:

  0 white    complex Gaussian, lambda = compute_lambda(x, ctx=1); in the "zeros" variant with 5
             leading and 7 trailing all-zero frames
  1 ladder   AR(1)-coloured in time, mixed across channels, frame levels on a ladder of powers
             1e-8 .. 1e6 in runs of max(5, taps + delay) frames; lambda = compute_lambda(x, ctx=1)
  2 ladder_h the same with a hand-made lambda: the ladder's power times a factor in [1/2, 2],
             floored at float32 eps -- it spans the floor up to 1e6
  3 neardup  white, the last channel a copy of the first plus a perturbation sized so that cond(R)
             is about 1e9 (one channel: the zeros variant of family 0 again)
"""
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as o  # noqa: E402
import wpe_model as wm  # noqa: E402

M_BITS = 4.0            # stft_cases.M_BITS: the project's two-bit margin
U32 = 2.0 ** -24
U64 = 2.0 ** -53
EPS32 = 1.1920928955078125e-07
F = 4
FAMILIES = ("white", "ladder", "ladder_h", "neardup")
LD = np.longdouble
CLD = np.clongdouble

# (channels, taps): (tiles per wavefront of the LDS instantiation, or "wide"; staged chunk)
SHAPES = {
    (1, 1): (1, 64), (2, 4): (1, 64), (1, 10): (2, 64), (2, 12): (3, 64), (6, 5): (4, 64),
    (5, 8): (5, 64), (6, 8): (8, 64), (10, 4): (8, 64), (7, 8): (10, 64), (8, 8): (12, 64),
    (8, 9): (14, 64), (9, 7): (14, 64), (8, 10): (17, 64), (12, 6): (17, 64), (8, 11): (20, 64), (16, 5): (20, 64),
    (9, 9): (23, 64), (4, 24): (23, 32), (5, 19): (23, 32), (11, 8): (23, 32), (6, 16): (23, 16),
    (9, 10): (26, 32), (10, 9): (26, 32), (13, 7): (26, 16), (15, 6): (26, 16),
    (8, 12): ("wide", 64), (1, 97): ("wide", 64), (3, 67): ("wide", 64), (16, 16): ("wide", 64),
}
# every (instantiation, chunk) pair a supported shape can select, and the wide form
REACHABLE = sorted({v for v in SHAPES.values() if v[0] != "wide"}, key=str) + [("wide", 64)]
# shapes that also run the frame counts around a chunk edge, one or more per chunk size
EDGE_SHAPES = ((2, 4), (8, 10), (8, 12), (5, 19), (9, 10), (6, 16), (13, 7))
SMALL_SHAPES = ((1, 1), (2, 4), (1, 10), (2, 12), (6, 5))
LONG_DELAY = (((2, 4), 70), ((5, 19), 70))
# (channels, taps, delay, chunk) of the isolated-impulse cases (three channels and more: the last
# impulses are exactly delay + taps apart)
IMPULSE_SHAPES = ((3, 4, 1, 64), (6, 5, 3, 64), (5, 19, 2, 32), (6, 16, 1, 16), (13, 7, 2, 16), (8, 12, 1, 64))
RAGGED = (((2, 4), (130, 77, 193)), ((6, 16), (145, 129)), ((9, 10), (161, 150)), ((8, 12), (193, 170)))


@dataclass(frozen=True)
class Case:
    ch: int
    taps: int
    T: int
    delay: int = 3
    variant: str = "white"      # family of bin 0: "white" or "zeros"
    seed: int = 0

    @property
    def ntw(self):
        return SHAPES[(self.ch, self.taps)][0]

    @property
    def tc(self):
        return SHAPES[(self.ch, self.taps)][1]

    @property
    def nk(self):
        return self.ch * self.taps

    @property
    def name(self):
        return f"{self.ch}x{self.taps}-T{self.T}-d{self.delay}-{self.variant}"


def edge_frames(ch, taps, delay=3):
    """k TC - 1, k TC, k TC + 1 for the smallest k TC that leaves about 1.5 frames per tap row."""
    tc = SHAPES[(ch, taps)][1]
    need = (3 * ch * taps) // 2 + taps + delay + 8
    k = max(2, -(-need // tc))
    return k * tc - 1, k * tc, k * tc + 1


def all_cases():
    """The table: every shape at k TC + 1 (odd: T mod 4 != 0), the chunk-edge frame counts on
    EDGE_SHAPES, delays 0 and 1 on the small shapes, a delay beyond a chunk on two."""
    cases = []
    for (ch, taps) in SHAPES:
        cases.append(Case(ch, taps, edge_frames(ch, taps)[2]))
    for (ch, taps) in EDGE_SHAPES:
        lo, mid, _ = edge_frames(ch, taps)
        cases.append(Case(ch, taps, lo, variant="zeros"))
        cases.append(Case(ch, taps, mid, variant="zeros"))
        cases.append(Case(ch, taps, mid + 2, variant="zeros"))
    for (ch, taps) in SMALL_SHAPES:
        for delay in (0, 1):
            cases.append(Case(ch, taps, edge_frames(ch, taps, delay)[2] + 1, delay=delay, variant="zeros"))
    for (ch, taps), delay in LONG_DELAY:
        cases.append(Case(ch, taps, edge_frames(ch, taps, delay)[0], delay=delay))
    return cases


# ------------------------------------------------------------------ signals
def _cnormal(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def _rng(case, f):
    return np.random.default_rng([case.seed, case.ch, case.taps, case.T, case.delay, f])


def white(rng, N, T, zeros=False):
    x = _cnormal(rng, N, T)
    if zeros:
        x[:, :5] = 0.0
        x[:, T - 7:] = 0.0
    return x


LADDER = (1.0, 1e2, 1e4, 1e6, 1e4, 1e2, 1.0, 1e-2, 1e-4, 1e-6, 1e-8, 1e-6, 1e-4, 1e-2)


def ladder_power(T, run):
    """the ladder's power per frame: runs of `run` frames, up and down between 1e-8 and 1e6"""
    return np.array([LADDER[(t // run) % len(LADDER)] for t in range(T)])


def ladder_run(taps, delay):
    """Frames per step of the ladder: at least five, and at least the reach of a tap vector, so
    that the rows of one tap vector differ by one step (a factor 100 in power) at the most.  With
    shorter runs a long filter sees the whole 1e14 inside one tap vector, R is a badly scaled
    matrix with cond(R) of 1e13 and more, and whether a pivot passes the kernel's rank floor
    (relative to the largest diagonal entry) is decided by rounding."""
    return max(5, taps + delay)


def coloured(rng, N, T, run):
    """AR(1) in time (pole 0.9 e^{i theta} per channel), mixed across channels, on the ladder."""
    w = _cnormal(rng, N, T)
    pole = 0.9 * np.exp(2j * np.pi * rng.uniform(size=N))
    s = np.zeros((N, T), np.complex128)
    for t in range(T):
        s[:, t] = w[:, t] + (pole * s[:, t - 1] if t else 0.0)
    mix = np.eye(N) + 0.4 * _cnormal(rng, N, N)
    return (mix @ s) * np.sqrt(ladder_power(T, run))


def cond_of(x, lam, taps, delay):
    """cond(R) of one bin from the singular values of yt / sqrt(lambda)."""
    yt = wm.tap_matrix(np.asarray(x, np.complex128), taps, delay) / np.sqrt(lam)
    s = np.linalg.svd(yt, compute_uv=False)
    return float((s[0] / s[-1]) ** 2) if s[-1] > 0 else np.inf


def _lam1(x64):
    return o.compute_lambda(x64[None], ctx=1)[0].astype(np.float64)


def near_duplicate(rng, N, T, taps, delay, target=1e9):
    """white, the last channel = the first + e * noise, e sized (cond scales as e^-2) so that
    cond(R) lands on `target` after the rounding to complex64."""
    base = white(rng, N, T)
    noise = _cnormal(rng, T)
    e = 1e-4
    for _ in range(3):
        x = base.copy()
        x[N - 1] = base[0] + e * noise
        x = x.astype(np.complex64)
        e *= np.sqrt(cond_of(x, _lam1(x), taps, delay) / target)
    return x


def make_case(case):
    """(x [F][N][T] complex64, lam [F][T] float64)"""
    N, T = case.ch, case.T
    x = np.zeros((F, N, T), np.complex64)
    lam = np.zeros((F, T), np.float64)
    zeros = case.variant == "zeros"
    x[0] = white(_rng(case, 0), N, T, zeros).astype(np.complex64)
    lam[0] = _lam1(x[0])
    run = ladder_run(case.taps, case.delay)
    x[1] = coloured(_rng(case, 1), N, T, run).astype(np.complex64)
    lam[1] = _lam1(x[1])
    rng = _rng(case, 2)
    x[2] = coloured(rng, N, T, run).astype(np.complex64)
    lam[2] = np.maximum(ladder_power(T, run) * 2.0 ** rng.uniform(-1, 1, size=T), EPS32)
    if N >= 2:
        x[3] = near_duplicate(_rng(case, 3), N, T, case.taps, case.delay)
    else:
        x[3] = white(_rng(case, 3), N, T, True).astype(np.complex64)
    lam[3] = _lam1(x[3])
    return x, lam


def family_of_bin(case, f):
    if f == 0:
        return case.variant
    return "zeros" if (f == 3 and case.ch < 2) else FAMILIES[f]


# ------------------------------------------------------------------ the extended reference
def ref_step(x, lam, taps, delay, rows=None):
    """wpe_step of one bin in np.clongdouble: x [N][T] (complex64 values), lam [T] float64 ->
    d [N][T] clongdouble.  rows: the tap rows the filter may use (a rank-deficient case passes the
    independent ones: the least-squares residual is unique though G is not); default all."""
    xl = np.asarray(x).astype(CLD)
    N, T = xl.shape
    yt = wm.tap_matrix(xl, taps, delay)
    if rows is not None:
        yt = yt[np.asarray(rows)]
    NK = yt.shape[0]
    yn = yt / np.asarray(lam).astype(LD)
    R = yn @ yt.conj().T
    G = yn @ xl.conj().T
    for k in range(NK):                                   # Cholesky, r carried along
        d = np.sqrt(R[k, k].real)
        R[k + 1:, k] /= d
        G[k] /= d
        R[k, k] = d
        li = R[k + 1:, k]
        R[k + 1:, k + 1:] -= np.outer(li, li.conj())
        G[k + 1:] -= np.outer(li, G[k])
    for k in range(NK - 1, -1, -1):                       # L^H G = y
        G[k] /= R[k, k].real
        G[:k] -= np.outer(R[k, :k].conj(), G[k])
    return xl - G.conj().T @ yt


def ref_bins(x, lam, taps, delay, rows=None):
    return np.stack([ref_step(x[f], lam[f], taps, delay, rows) for f in range(x.shape[0])])


def oracle_bins(x, lam, taps, delay):
    x128 = np.asarray(x).astype(np.complex128)
    return o.wpe_step(x128, o.compute_tap_mat(x128, taps, delay), np.asarray(lam, np.float64))


def _norm_t(a):
    """2-norm over the frames, in long double -> float64 [F][N]"""
    a = np.asarray(a).astype(CLD)
    return np.sqrt((a.real ** 2 + a.imag ** 2).sum(-1)).astype(np.float64)


class Reference:
    """ref (clongdouble), the two yardsticks' errors and u [F][N] of given data."""

    def __init__(self, x, lam, taps, delay, tc, rows=None, yardsticks=True):
        self.x, self.lam = x, lam
        self.ref = ref_bins(x, lam, taps, delay, rows)
        self.norm = _norm_t(self.ref)
        nk = x.shape[1] * taps
        self.floor = U64 * nk * _norm_t(x.astype(CLD) - self.ref)
        self.u = self.floor.copy()
        self.err_oracle = self.err_model = None
        if yardsticks:
            self.model, self.model_status = wm.wpe_step_bins(x, lam, taps, delay, tc)
            self.err_oracle = _norm_t(oracle_bins(x, lam, taps, delay) - self.ref)
            self.err_model = _norm_t(self.model - self.ref)
            self.u = np.maximum(self.u, np.maximum(self.err_oracle, self.err_model))


_refs = {}


def reference(case):
    """The case's data and Reference, computed once and shared (treat as read-only)."""
    if case not in _refs:
        x, lam = make_case(case)
        _refs[case] = Reference(x, lam, case.taps, case.delay, case.tc)
    return _refs[case]


# ------------------------------------------------------------------ the judge
def judge(name, got, status, R, m=M_BITS, expect_status=0, bins=None, extra=0.0):
    """got [F][N][T] (what the device stored, complex64), status [F] or None, R: a Reference.
    Returns (worst ratio of error to allowance, failures: list of strings).  bins: the bins
    judged (default all).  extra [F][N]: added to the allowance by a caller whose device result
    rests on variances the device estimated itself (lambda_sensitivity)."""
    got = np.asarray(got)
    fails = []
    worst = 0.0
    if got.shape != R.ref.shape:
        return np.inf, [f"{name}: shape {got.shape} against {R.ref.shape}"]
    bins = range(got.shape[0]) if bins is None else bins
    err = _norm_t(got.astype(CLD) - R.ref)
    allow = U32 * R.norm + m * R.u + extra
    for f in bins:
        if status is not None and int(status[f]) != expect_status:
            fails.append(f"{name}: bin {f} status {int(status[f])}, expected {expect_status}")
        for c in range(got.shape[1]):
            if not np.isfinite(got[f, c]).all():
                fails.append(f"{name}: bin {f} channel {c} holds non-finite values")
                worst = np.inf
            elif R.norm[f, c] == 0.0:
                if err[f, c] != 0.0:
                    fails.append(f"{name}: bin {f} channel {c} of an all-zero reference holds {err[f, c]:.3e}")
                    worst = np.inf
            else:
                ratio = err[f, c] / allow[f, c]
                worst = max(worst, ratio)
                if not err[f, c] <= allow[f, c]:
                    fails.append(f"{name}: bin {f} channel {c} error {err[f, c]:.3e} > allowance "
                                 f"{allow[f, c]:.3e} (rel {err[f, c] / R.norm[f, c]:.2e}, u rel "
                                 f"{R.u[f, c] / R.norm[f, c]:.2e})")
    return worst, fails


def rel_rms(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------ exact cases
def impulse_frames(ch, taps, delay, tc, first):
    """`ch` frames: `first`, the next chunk boundary at least delay + taps further (2 TC while the
    filter's reach is shorter than a chunk), then exactly delay + taps apart"""
    gap = delay + taps
    frames = [first]
    if ch > 1:
        frames.append(-(-(first + gap) // tc) * tc)
    while len(frames) < ch:
        frames.append(frames[-1] + gap)
    return frames[:ch]


def impulses(ch, taps, delay, tc, seed=0):
    """(x [2][N][T] complex64, lam [2][T]): per bin N linearly independent single-frame vectors
    spaced at least delay + taps apart -- the last ones exactly that, the closest the filter's
    reach allows -- on and beside chunk boundaries: bin 0 starts at frame TC - 1, bin 1 at TC,
    both go on at the next chunk boundary the spacing allows.  No frame of the tap matrix then meets a non-zero frame of x, r = 0 and
    G = 0 exactly, and the step returns its input bit for bit; a tap or a delay that reaches one
    frame further does meet one."""
    assert delay >= 1
    gap = delay + taps
    fr = [impulse_frames(ch, taps, delay, tc, tc - 1 + b) for b in range(2)]
    T = max(f[-1] for f in fr) + gap + 2
    rng = np.random.default_rng([seed, ch, taps, delay, 5])
    x = np.zeros((2, ch, T), np.complex64)
    for b in range(2):
        vecs = np.eye(ch) * 2.0 + 0.5 * _cnormal(rng, ch, ch)  # diagonally dominant: independent
        for i, t in enumerate(fr[b]):
            x[b, :, t] = vecs[:, i]
    lam = rng.uniform(0.5, 2.0, size=(2, T))
    return x, lam


def bits(a):
    """the stored bits of a complex64 / float array, for bit-for-bit comparisons (NaN included)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype in (np.complex64, np.float32) else np.uint64)


# ------------------------------------------------------------------ degenerate cases
def duplicated_channel(case, f=1):
    """(x [1][N + 1][T], lam [1][T], want [1][N + 1][T] complex128): bin f of the case with a
    bitwise copy of channel 0 appended.  R is exactly rank deficient (status SETK_NUM_RANKDEF);
    G is not unique but the fitted values are: every channel's result is the one of the utterance
    without the twin, the twin's that of channel 0."""
    R = reference(case)
    x = np.concatenate([R.x[f], R.x[f][:1]])[None]
    lam = R.lam[f][None].copy()
    base = ref_bins(R.x[f][None], lam, case.taps, case.delay)
    want = np.concatenate([base[0], base[0][:1]])[None].astype(np.complex128)
    return np.ascontiguousarray(x), lam, want


def silent_channel(case, f=0):
    """(x [1][N + 1][T], lam, want): bin f with an all-zero channel appended.  Its tap rows are
    zero (status SETK_NUM_RANKDEF), its result is exactly zero, the others' are those of the
    utterance without it."""
    R = reference(case)
    x = np.concatenate([R.x[f], np.zeros_like(R.x[f][:1])])[None]
    lam = R.lam[f][None].copy()
    base = ref_bins(R.x[f][None], lam, case.taps, case.delay)
    want = np.concatenate([base[0], np.zeros_like(base[0][:1])])[None].astype(np.complex128)
    return np.ascontiguousarray(x), lam, want


def with_nan_bin(case, f=1):
    """(x, lam) of the case with one NaN in bin f (channel N - 1, frame T // 2)."""
    R = reference(case)
    x = R.x.copy()
    x[f, -1, case.T // 2] = np.complex64(complex(np.nan, 0.0))
    return x, R.lam


# ------------------------------------------------------------------ device-estimated variances
def lambda_rel_bound(C, ctx):
    """float32 summation of non-negative terms as wpe_lambda_kernel does it: two roundings in
    |v|^2, C - 1 in the channel sum, one in the division by C, 2 ctx in the context sum, one in
    the final rounding of 1 / lambda to float32 -- (C + 2 ctx + 3) 2^-24."""
    return (C + 2 * ctx + 3) * U32


def compute_lambda64(x, ctx):
    """compute_lambda of complex64 data in float64 throughout -> [F][T]: the channel-mean power
    averaged over the frames of t - ctx .. t + ctx that exist, floored at float32 eps.  Equal to
    oracle.np_oracle.compute_lambda on float64 input wherever that is defined (its slices need
    T > ctx; the device takes any T)."""
    x = np.asarray(x).astype(np.complex128)
    L = np.mean(x.real ** 2 + x.imag ** 2, axis=1)
    T = L.shape[1]
    lam = np.empty_like(L)
    for t in range(T):
        lo, hi = max(t - ctx, 0), min(t + ctx + 1, T)
        lam[:, t] = L[:, lo:hi].sum(axis=1) / (hi - lo)
    return np.maximum(lam, EPS32)


def _signs(shape, seed):
    return np.random.default_rng([seed, 4711]).choice([-1.0, 1.0], size=shape)


def lambda_sensitivity(x, lam, taps, delay, rel, seed=0):
    """[F][N]: how far the extended result moves (norm over frames) when every lambda_t moves by
    a relative +-rel -- a property of the reference alone (cf. solve_cases.sensitivity)."""
    moved = ref_bins(x, lam * (1.0 + rel * _signs(lam.shape, seed)), taps, delay)
    return _norm_t(moved - ref_bins(x, lam, taps, delay))


def chain(x, taps, delay, ctx, iters, rel=0.0, seed=0):
    """wpe() in extended precision, rounded to complex64 between steps as the device stores it;
    every lambda_t moved by +-rel.  Returns (result of the last step in clongdouble, the lambda of
    the last step)."""
    d = np.asarray(x)
    for it in range(iters):
        lam = compute_lambda64(d, ctx)
        if rel:
            lam = lam * (1.0 + rel * _signs(lam.shape, seed + it))
        last = ref_bins(x, lam, taps, delay)
        d = last.astype(np.complex64)
    return last, lam
