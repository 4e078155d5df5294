"""
Constructed cases for mask-based sound source localisation (numpy only: no device): the inputs, the
float64 reference a device score is held to, the allowance per (window, direction) cell, the judge,
and float32 models of the ML and SRP kernels that can carry the seeded faults of test_ssl_cases.py.

REFERENCE.  ssl_model.ml_ssl / srp_ssl / music_ssl per window of frames (float64, the reference
project's own operations) on complex128 / float64 copies of exactly what the device receives: the
complex64 spectrogram, the complex64 steer vectors, the float32 mask.  The functions *_frames() and
music_terms() below restate the same formulas with their per-cell terms kept (ML: power, proj, delta;
SRP: the pair terms; MUSIC: lambda_1, lambda_2, |v^H s|), which the allowances need;
test_ssl_cases.py holds the two to each other.

UNITS.  A cell is one (window, direction) score.  A single-frame window (t, t + 1) is the frame
score S[t][a]; a one-hot mask in (t, f) (ML, SRP) or a steer vector that is zero outside one bin
(MUSIC) leaves one term of the sum.

ALLOWANCES, per cell, derived and not measured (PARITY_NOTES_SSL.md), u32 = 2^-24:

    SRP frame   [(2 F K + 2) u32 sum_fp |m| c_fp + (2 K_U + 1) u32 sum_fp |m|] / K + u32 |S|
                c_fp = |Re d Re u| + |Im d Im u| <= 1, K_U = 11 (spatial_cases: a pair coherence)
    SRP fold    [(2 F K + 3) u32 sum_fp c(d, U_pf) + (2 K_U + 2) u32 sum_fpt |m|] / K + u32 |S|
                U_pf = sum_t m u_p: the float64 fold keeps the cancellation of the sum over frames
    ML          |d delta| <= K_D(C) u32 power + (4 C + 4) 2^-126,  K_D = 9 C + 14 (+ 16 under norm)
                |d ll| <= the image of [delta - |d delta|, delta + |d delta|] under ll() + E_FN
                log form   E_FN = E_LOG = 4 u32 |ll| + u32
                power form E_FN = |ll| (6 u32 |c ln delta| + 3 u32)
                frame: sum_f |m| |d ll| + (F + 1) u32 sum_f |m ll|;  a window: the sum over its frames
    MUSIC       sum_f [2 |v^H s| ||s|| e_v(f) + (2 C + 4) u32 ||s||^2],
                e_v(f) = 2 (sqrt 2 ||A_cov(f)||_F + 16 u32 lambda_1) / (lambda_1 - lambda_2),
                A_cov the covariance allowance of covar_cases.py

The bar of a cell is min(allowance, 1e-4 x spread of that window's reference spectrum): nothing is
judged more loosely than test_gpu_ssl.py does.  (A reference spectrum that is constant over the
directions has no spread and no flat bar: ML and MUSIC at one channel.  There the allowance alone
is the bar.)  Where the reference is not finite the device must be non-finite in exactly the same
cells.  The `aligned` family and ML at one channel are pure cancellation (delta is the rounding of
power - power): they are held to the range the formula allows, ml_range().

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***
"""
from dataclasses import dataclass

import numpy as np

import spatial_cases as spc
import spatial_model as sm
import ssl_model

U32 = 2.0 ** -24
EPS32 = float(np.finfo(np.float32).eps)
K_U = spc.K_U
BAR = 1e-4
TINY = 2.0 ** -126
TILE, CHUNK = 32, 64
FAMILIES = ("white", "plane", "aligned", "lattice", "ladder", "extreme", "nan", "spiked", "close")
LEVEL = 0.1                       # the noise level of `plane`
DELTA_FLOOR = 2.0 ** -10          # delta >= DELTA_FLOOR x power where the allowance needs it
SR, SPEED = 16000, 343.0
f32 = np.float32
topo, all_pairs = spc.topo, spc.all_pairs


# ------------------------------------------------------------------ inputs
def _cnormal(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def pair_lists(pairs):
    """[(l, r), ...] -> the reference's (left indices, right indices)"""
    return [p[0] for p in pairs], [p[1] for p in pairs]


def pairs_of(C):
    """all pairs; one channel: the pair (0, 0)"""
    return all_pairs(C) if C >= 2 else [(0, 0)]


def unit_steer(A, C, F):
    """complex64 [A][C][F]: plane waves over the unequal linear topology topo(C), unit modulus."""
    omega = np.linspace(0, SR / 2, F) * 2 * np.pi
    theta = np.linspace(0, np.pi, A) if A > 1 else np.array([np.pi / 3])
    tau = np.cos(theta)[:, None] * np.asarray(topo(C))[None, :] / SPEED
    return np.exp(-1j * tau[:, :, None] * omega[None, None, :]).astype(np.complex64)


def random_steer(A, C, F):
    """complex64 [A][C][F]: random phases, moduli in (0.2, 3)."""
    rng = np.random.default_rng([98, A, C, F])
    return (np.exp(1j * rng.uniform(-np.pi, np.pi, size=(A, C, F))) * rng.uniform(0.2, 3.0, size=(A, C, F))).astype(
        np.complex64)


def duplicate_steer(sv, best, positions):
    """copies of direction `best` at `positions` (for exact ties)"""
    out = np.array(sv)
    for p in positions:
        out[p] = sv[best]
    return out


def source_direction(A):
    return A // 3


def spectrogram(family, C, T, F, A=65, spike=False):
    """complex64 [C][T][F], seeded by (family, C, T, F).  plane / aligned: a plane wave from direction
    source_direction(A) of unit_steer(A, C, F).  spike (MUSIC's ladder): the ladder of `spiked`."""
    rng = np.random.default_rng([FAMILIES.index(family), C, T, F])
    x = _cnormal(rng, C, T, F)
    if spike:
        x = spectrogram("spiked", C, T, F).astype(np.complex128)
    if family in ("plane", "aligned"):
        d = unit_steer(A, C, F)[source_direction(A)].astype(np.complex128)               # [C][F]
        s = rng.uniform(0.5, 1.5, size=(1, T, F)) * np.exp(1j * rng.uniform(-np.pi, np.pi, size=(1, T, F)))
        y = d[:, None, :] * s
        if family == "plane":
            # noise as a gain and a phase per microphone: the moduli then differ between the microphones
            # with a variance of at least 0.3 LEVEL^2 |s|^2, and for ANY unit-modulus steer vector
            # delta >= sum |x_m|^2 - (sum |x_m|)^2 / C = C var_m |x_m|   (Cauchy-Schwarz)
            g = rng.uniform(0.7, 1.0, size=(C, T, F)) * np.where(np.arange(C) % 2, -1.0, 1.0)[:, None, None]
            y = y * (1 + LEVEL * g) * np.exp(1j * LEVEL * rng.uniform(-1, 1, size=(C, T, F)))
        x = y
    elif family == "lattice":
        kind = rng.integers(0, 4, size=(C, T, F))               # 0: zero, 1: real, 2: imaginary, 3: both
        re = rng.integers(-3, 4, size=(C, T, F)) * ((kind == 1) | (kind == 3))
        im = rng.integers(-3, 4, size=(C, T, F)) * ((kind == 2) | (kind == 3))
        x = re + 1j * im
        x[:, rng.uniform(size=T) < 0.2] = 0.0
        x[:, T // 2] = 0.0
        if C >= 3:
            x[C // 2] = 0.0
    elif family == "ladder":
        x = x * 2.0 ** np.linspace(30, -30, F)
    elif family == "extreme":
        x = x * 2.0 ** np.linspace(100, -100, F)
    elif family == "spiked":
        # white plus a rank-one component of three times its level: MUSIC needs a principal direction
        u = _cnormal(rng, C, 1, F)
        x = x + 3.0 * u / np.sqrt(np.sum(np.abs(u) ** 2, axis=0, keepdims=True)) * np.sqrt(C) * _cnormal(rng, 1, T, F)
    elif family == "close":
        # per bin: eigenvalues 1, 1 - 1e-3, then a geometric tail, over the whole utterance (T >= C)
        assert T >= C >= 2
        lam = np.concatenate([[1.0, 1.0 - 1e-3], np.geomspace(0.5, 0.05, C)[:C - 2]])
        for f in range(F):
            q, _ = np.linalg.qr(_cnormal(rng, C, C))
            v, _ = np.linalg.qr(_cnormal(rng, T, C))
            x[:, :, f] = (q * np.sqrt(T * lam)) @ v.conj().T
    x = x.astype(np.complex64)
    if family == "nan":
        c, t, f = nan_cell(C, T, F)
        x[c, t, f] = complex(np.nan, x[c, t, f].imag)
    return x


def nan_cell(C, T, F):
    return C - 1, T // 2, F // 3


def mask(T, F, seed=0):
    """float32 [T][F] in (0.05, 0.95)"""
    return np.random.default_rng([77, T, F, seed]).uniform(0.05, 0.95, size=(T, F)).astype(f32)


def onehot_mask(T, F, cells):
    m = np.zeros((T, F), f32)
    for t, f in cells:
        m[t, f] = 1.0
    return m


def single_frames(T):
    return [(t, t + 1) for t in range(T)]


# ------------------------------------------------------------------ the reference, per window
def reference(backend, x, sv, windows, mask=None, pairs=None, **ml_kw):
    """ssl_model per window -> (indices [W], scores [W][A]); pairs [(l, r), ...]."""
    T = x.shape[1]
    idx, sc = [], []
    for t0, t1 in (windows or [(0, T)]):
        m = None if mask is None else mask[t0:t1]
        with np.errstate(all="ignore"):
            if backend == "ml":
                i, s = ssl_model.ml_ssl(x[:, t0:t1], sv, mask=m, **ml_kw)
            elif backend == "srp":
                i, s = ssl_model.srp_ssl(x[:, t0:t1], sv, pair_lists(pairs), mask=m)
            else:
                i, s = ssl_model.music_ssl(x[:, t0:t1], sv, mask=m)
        idx.append(int(i))
        sc.append(s)
    return np.array(idx), np.stack(sc)


def window_sums(frames, windows):
    """[T][A] per frame -> [W][A]"""
    return np.stack([frames[t0:t1].sum(axis=0) for t0, t1 in windows])


# ------------------------------------------------------------------ ML: terms and allowance
def k_delta(C, norm=False):
    """|d delta| <= K_D u32 power.  The steer vector is normalised with C + 3 roundings; the 2 C
    multiply-adds of sv conj(x) leave each component within 2 C u32 ||sv|| ||x||, the vector within
    sqrt 2 of that: |dz| <= (4 C + 3) u32 sqrt(power).  |z|^2 adds 3, 1 / (1 + eps) as a float and its
    product 2: proj within (8 C + 11) u32 power.  The power is a sum of 2 C squares, (C + 2) u32 power;
    the subtraction rounds once.  Under norm every sample carries 4 more roundings (the modulus, the
    maximum with a rounded eps, the reciprocal, the product), twice in proj and twice in power."""
    return 9 * C + 14 + (16 if norm else 0)


def _ll(delta, eps, compression):
    with np.errstate(all="ignore"):
        if compression <= 0:
            return -np.log(np.maximum(delta, eps))
        return -np.power(delta, compression)


def ml_frames(x, sv, mask=None, compression=0, eps=1e-8, norm=False):
    """(S [T][A] the frame scores, A [T][A] their allowance, terms) in float64."""
    x, sv = np.asarray(x).astype(np.complex128), np.asarray(sv).astype(np.complex128)
    C, T, F = x.shape
    m = np.ones((T, F)) if mask is None else np.asarray(mask, np.float64)
    with np.errstate(all="ignore"):
        svn = sv / np.sqrt(np.sum(np.abs(sv) ** 2, axis=1, keepdims=True))
        if norm:
            x = x / np.maximum(np.abs(x), eps)
        power = np.sum(np.abs(x) ** 2, axis=0)                              # [T][F]
        proj = np.abs(np.einsum("amf,mtf->atf", svn, x.conj())) ** 2        # [A][T][F]
        delta = power[None] - proj / (1 + eps)
        dd = k_delta(C, norm) * U32 * power[None] + (4 * C + 4) * TINY
        ll = _ll(delta, eps, compression)
        lo = _ll(np.maximum(delta - dd, 0.0) if compression > 0 else delta - dd, eps, compression)
        hi = _ll(delta + dd, eps, compression)
        if compression <= 0:
            e_fn = 4 * U32 * np.abs(ll) + U32
        else:
            e_fn = np.abs(ll) * (6 * U32 * np.abs(compression * np.log(np.maximum(delta, TINY))) + 3 * U32)
        dll = np.maximum(np.abs(lo - ll), np.abs(hi - ll)) + e_fn
        S = np.einsum("tf,atf->ta", m, ll)
        A = np.einsum("tf,atf->ta", np.abs(m), dll) + (F + 1) * U32 * np.einsum("tf,atf->ta", np.abs(m), np.abs(ll))
    return S, A, dict(power=power, proj=proj, delta=delta)


def ml_range(x, mask, windows, eps, A):
    """(lo, hi) [W][A]: what the log form allows of a cell whose delta is pure cancellation -- every
    ll in [-log(power (1 + 2 C u32)), -log(eps)], widened by E_LOG and the float32 accumulation."""
    x = np.asarray(x).astype(np.complex128)
    C, T, F = x.shape
    m = np.ones((T, F)) if mask is None else np.asarray(mask, np.float64)
    assert (m >= 0).all()
    power = np.sum(np.abs(x) ** 2, axis=0)
    top = -np.log(eps)
    bot = -np.log(np.maximum(power * (1 + 2 * C * U32), eps))
    slack = lambda v: 4 * U32 * np.abs(v) + U32 + (F + 1) * U32 * np.abs(v)
    lo = (m * (bot - slack(bot))).sum(axis=1)                                # [T]
    hi = (m * (top + slack(top))).sum(axis=1)
    lo, hi = window_sums(lo[:, None], windows), window_sums(hi[:, None], windows)
    return np.repeat(lo, A, axis=1), np.repeat(hi, A, axis=1)


# ------------------------------------------------------------------ SRP: terms and allowances
def _srp_phasors(x, sv, pairs):
    with np.errstate(all="ignore"):
        phi, psi = spc.phase(x), spc.phase(sv)
        l, r = pair_lists(pairs)
        return np.exp(1j * (phi[l] - phi[r])), np.exp(1j * (psi[:, l] - psi[:, r]))    # [P][T][F], [A][P][F]


def _contract(d, U):
    """sum_pf Re(conj(d) U) and sum_pf (|Re d Re U| + |Im d Im U|): d [A][P][F], U [P][N][F] -> [N][A]"""
    with np.errstate(all="ignore"):
        val = np.einsum("apf,pnf->na", d.real, U.real) + np.einsum("apf,pnf->na", d.imag, U.imag)
        mag = np.einsum("apf,pnf->na", np.abs(d.real), np.abs(U.real)) + \
            np.einsum("apf,pnf->na", np.abs(d.imag), np.abs(U.imag))
    return val, mag


def srp_frames(x, sv, pairs, mask=None):
    """(S [T][A], A [T][A], terms) of the frame-score path."""
    C, T, F = x.shape
    K = len(pairs)
    m = np.ones((T, F)) if mask is None else np.asarray(mask, np.float64)
    u, d = _srp_phasors(x, sv, pairs)
    with np.errstate(all="ignore"):
        val, mag = _contract(d, u * m[None])
        S = val / K
        A = ((2 * F * K + 2) * U32 * mag + (2 * K_U + 1) * U32 * K * np.abs(m).sum(axis=1)[:, None]) / K + U32 * np.abs(S)
    return S, A, dict(u=u, d=d)


def srp_fold(x, sv, pairs, mask, windows):
    """(S [W][A], A [W][A]) of the offline path: the frames folded first."""
    C, T, F = x.shape
    K = len(pairs)
    m = np.ones((T, F)) if mask is None else np.asarray(mask, np.float64)
    u, d = _srp_phasors(x, sv, pairs)
    with np.errstate(all="ignore"):
        U = np.stack([(u[:, t0:t1] * m[None, t0:t1]).sum(axis=1) for t0, t1 in windows], axis=1)     # [P][W][F]
        val, mag = _contract(d, U)
        S = val / K
        msum = np.array([np.abs(m[t0:t1]).sum() for t0, t1 in windows])
        A = ((2 * F * K + 3) * U32 * mag + (2 * K_U + 2) * U32 * K * msum[:, None]) / K + U32 * np.abs(S)
    return S, A


# ------------------------------------------------------------------ MUSIC: terms and allowance
def music_terms(x, sv, mask=None, window=None):
    """One window -> dict(score [A], A [A], lam1 [F], lam2 [F], gap [F], vs [F][A], dead [F]).
    dead: bins whose covariance is zero or not finite (the device reports a status there and they are
    not judged: the caller gives them a zero steer vector)."""
    import covar_cases
    t0, t1 = window or (0, x.shape[1])
    xw = np.asarray(x)[:, t0:t1]
    C, T, F = xw.shape
    m = np.ones((T, F), f32) if mask is None else np.asarray(mask, f32)[t0:t1]
    m2 = (m * m).astype(np.float64)
    s = np.asarray(sv).astype(np.complex128).transpose(2, 0, 1)             # [F][A][C]
    with np.errstate(all="ignore"):
        R = covar_cases.reference(xw, m2)                                   # [F][C][C]
        Acov = covar_cases.allowance(xw, m2, R)
        dead = ~np.isfinite(R).all(axis=(1, 2)) | ~(np.abs(R).sum(axis=(1, 2)) > 0)
        lam, vec = np.linalg.eigh(np.where(dead[:, None, None], np.eye(C)[None], R))
        lam1 = lam[:, -1]
        lam2 = lam[:, -2] if C >= 2 else np.zeros(F)
        v = vec[:, :, -1]                                                   # [F][C]
        e_v = 2 * (np.sqrt(2.0) * np.linalg.norm(Acov, axis=(1, 2)) + 16 * U32 * lam1) / (lam1 - lam2)
        if C == 1:
            e_v = np.zeros(F)                                               # a 1 x 1 eigenvector is 1
        vs = np.abs(np.einsum("fc,fac->fa", v.conj(), s))
        ns2 = np.sum(np.abs(s) ** 2, axis=2)
        term = np.abs(ns2 - vs ** 2)
        a_f = 2 * vs * np.sqrt(ns2) * e_v[:, None] + (2 * C + 4) * U32 * ns2
        live = ~dead[:, None]
        score = np.where(live, term, 0.0).sum(axis=0)
        A = np.where(live, a_f, 0.0).sum(axis=0)
    return dict(score=score, A=A, lam1=lam1, lam2=lam2, gap=(lam1 - lam2) / lam1, vs=vs, dead=dead)


# ------------------------------------------------------------------ the judge
@dataclass
class Verdict:
    name: str
    worst: float                # the largest error / bar over the cells (inf: a non-finite mismatch)
    where: tuple                # (window, direction) of the worst
    cells: int
    failures: list
    unjudged: int = 0


def spreads(ref):
    """[W]: max - min of every window's finite reference scores; 0 where the spectrum is constant to
    the reference's own float64 rounding (1e-9 of its size)."""
    out = np.zeros(len(ref))
    for w, r in enumerate(np.asarray(ref, np.float64)):
        r = r[np.isfinite(r)]
        if r.size:
            s = r.max() - r.min()
            out[w] = s if s > 1e-9 * np.abs(r).max() else 0.0
    return out


def flat_bar(ref):
    """[W][1]: 1e-4 x spread, inf where there is no spread"""
    s = spreads(ref)
    return np.where(s > 0, BAR * s, np.inf)[:, None]


def judge(name, got, ref, A, report=4):
    """got [W][A] float64 as the device returned it, ref [W][A], A the allowance [W][A]: every cell
    non-finite exactly where the reference is, else |got - ref| <= min(A, 1e-4 x spread of its window)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return Verdict(name, np.inf, (-1, -1), 0, [f"{name}: shape {got.shape} against {ref.shape}"])
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        bar = np.minimum(np.broadcast_to(np.asarray(A, np.float64), ref.shape), flat_bar(ref))
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(fin, ratio, np.where(np.isfinite(got), np.inf, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    v = _verdict(name, ratio, got, ref, err, bar, report)
    v.unjudged = int((fin & ~np.isfinite(bar)).sum())          # a finite reference without a finite bar
    return v


def judge_range(name, got, lo, hi, report=4):
    """every cell finite and inside [lo, hi]; the ratio is the distance from the middle over the half width"""
    got = np.asarray(got, np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    with np.errstate(all="ignore"):
        err = np.abs(got - mid)
        ratio = np.where(half > 0, err / np.where(half > 0, half, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return _verdict(name, ratio, got, mid, err, half, report)


def _verdict(name, ratio, got, ref, err, bar, report):
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else (-1, -1)
    bad = np.argwhere(~(ratio <= 1.0))
    fails = [f"{name}: cell (window, direction) = ({w}, {a}): got {got[w, a]:.12e}, reference {ref[w, a]:.12e}, "
             f"error {err[w, a]:.3e} > bar {bar[w, a]:.3e} (ratio {ratio[w, a]:.3g}); {len(bad)} of {ratio.size} cells fail"
             for w, a in bad[:report]]
    return Verdict(name, float(ratio[k]) if ratio.size else 0.0, tuple(int(v) for v in k), ratio.size, fails)


def flat_bar_sees(got, ref):
    """Whether the bar of test_gpu_ssl.py, max_a |got - ref| <= 1e-4 x spread per window, fails."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        return bool((np.nan_to_num(np.abs(got - ref), nan=np.inf) > flat_bar(ref)).any())


def index_failures(name, idx, got, ref, take_min=False):
    """The index of every window: the lowest direction attaining the extremum of the DEVICE's own
    scores, a non-finite score counting as the extremum (np.argmax / np.argmin, exactly); the lowest
    non-finite direction of the reference where it has one; and the reference's index wherever its
    gap to the runner-up exceeds 2e-4 of the spread (the gap rule of test_gpu_ssl.py)."""
    fails = []
    pick = np.argmin if take_min else np.argmax
    for w in range(len(ref)):
        own = int(pick(got[w]))
        if int(idx[w]) != own:
            fails.append(f"{name}: window {w}: index {int(idx[w])}, but the first extremum of its own scores is {own}")
        bad = np.flatnonzero(~np.isfinite(ref[w]))
        if bad.size:
            if int(idx[w]) != int(bad[0]):
                fails.append(f"{name}: window {w}: index {int(idx[w])}, the lowest non-finite direction is {int(bad[0])}")
        elif spreads(ref[w:w + 1])[0] > 0 and ssl_model.gap(ref[w], take_min) > 2 * BAR:
            if int(idx[w]) != int(pick(ref[w])):
                fails.append(f"{name}: window {w}: index {int(idx[w])}, the reference's is {int(pick(ref[w]))}")
    return fails


class Tally(spc.Tally):
    def report(self):
        for fam, (r, name, where) in sorted(self.worst.items()):
            print(f"[{self.form}] {fam:18s} worst error/allowance {r:.3f} at (window, direction) = {where} ({name})")
        r, name, where = self.overall()
        print(f"[{self.form}] {self.count} spectra sets, {self.cells} cells judged; worst error/allowance {r:.3f} "
              f"at {where} ({name})")


# ------------------------------------------------------------------ float32 models of the kernels
def _fma(a, b, c):
    """round32(a b + c): the product of two float32 is exact in float64"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _sv_ml(sv):
    """ssl_sv_prep_kernel, ML: sv / ||sv||_2 in float32 -> (re, im) [A][C][F]"""
    sv = np.asarray(sv, np.complex64)
    re, im = sv.real.astype(f32), sv.imag.astype(f32)
    n2 = np.zeros(re[:, 0].shape, f32)
    with np.errstate(all="ignore"):
        for c in range(sv.shape[1]):
            n2 = (n2 + (re[:, c] * re[:, c] + im[:, c] * im[:, c]).astype(f32)).astype(f32)
        scale = (f32(1) / np.sqrt(n2, dtype=f32)).astype(f32)[:, None, :]
        return (re * scale).astype(f32), (im * scale).astype(f32)


def _tile_fault_frames(T):
    """the frames of the second tile (the first, when there is one tile)"""
    t0 = TILE if T > TILE else 0
    return slice(t0, min(T, t0 + TILE))


def model_ml(x, sv, mask=None, compression=0, eps=1e-8, norm=False, fault=None, naive_modulus=False):
    """ssl_obs_prep_kernel<ML> and ssl_frame_score_kernel<ML> in float32, bins in order, the
    microphones in order, multiply-adds fused -> S [T][A] float32.

    fault: "drop_bin" (bin F // 2 left out in one frame tile), "stale_frame" (frame 32 reads frame
    31's observation), "mask_neighbour" (bin 32 takes bin 31's mask), "no_inv1pe", "no_clamp",
    "nan_clamp" (the clamp as fmaxf: a NaN becomes eps); naive_modulus: |x| as sqrtf(re^2 + im^2)
    without the rescaling (the kernel before it was made range-safe)."""
    x = np.array(x, np.complex64)
    C, T, F = x.shape
    A = sv.shape[0]
    if fault == "stale_frame" and T > TILE:
        x[:, TILE] = x[:, TILE - 1]
    m = np.ones((T, F), f32) if mask is None else np.array(mask, f32)
    if fault == "stale_frame" and T > TILE and mask is not None:
        m[TILE] = m[TILE - 1]
    sr, si = _sv_ml(sv)
    e32, c32 = f32(eps), f32(compression)
    inv1pe = f32(1.0) if fault == "no_inv1pe" else f32(1.0 / (1.0 + eps))
    xr, xi = x.real.astype(f32), x.imag.astype(f32)
    with np.errstate(all="ignore"):
        if norm:
            if naive_modulus:
                mod = np.sqrt((xr * xr + xi * xi).astype(f32), dtype=f32)
                r = (f32(1) / np.maximum(mod, e32)).astype(f32)
                r = np.where(np.isnan(mod), f32(1) / e32, r)                  # fmaxf(NaN, eps) = eps
                xr, xi = (xr * r).astype(f32), (xi * r).astype(f32)
            else:
                n2 = (xr * xr + xi * xi).astype(f32)
                big = n2 > f32(2.0 ** 124)
                pr, pi = sm.phasor(x)
                r = (f32(1) / np.maximum(np.sqrt(n2, dtype=f32), e32)).astype(f32)
                r = np.where(np.isnan(n2), f32(1) / e32, r)
                xr, xi = np.where(big, pr, (xr * r).astype(f32)), np.where(big, pi, (xi * r).astype(f32))
        q = np.zeros((T, F), f32)
        for c in range(C):
            q = (q + (xr[c] * xr[c] + xi[c] * xi[c]).astype(f32)).astype(f32)
        S = np.zeros((A, T), f32)
        tf = _tile_fault_frames(T)
        for f in range(F):
            ar, ai = np.zeros((A, T), f32), np.zeros((A, T), f32)
            for c in range(C):
                s_r, s_i = sr[:, c, f][:, None], si[:, c, f][:, None]
                ar = _fma(s_r, xr[c, :, f][None], _fma(s_i, xi[c, :, f][None], ar))
                ai = _fma(s_i, xr[c, :, f][None], _fma(-s_r, xi[c, :, f][None], ai))
            delta = (q[:, f][None] - ((ar * ar + ai * ai).astype(f32) * inv1pe).astype(f32)).astype(f32)
            if compression <= 0:
                if fault == "no_clamp":
                    cl = delta
                elif fault == "nan_clamp":
                    cl = np.fmax(delta, e32)
                else:
                    cl = np.where(delta < e32, e32, delta)
                ll = -np.log(cl.astype(np.float64)).astype(f32)
            else:
                ll = -np.exp((c32 * np.log(delta.astype(np.float64)).astype(f32)).astype(np.float64)).astype(f32)
            mf = m[:, 31] if (fault == "mask_neighbour" and f == 32) else m[:, f]
            new = _fma(mf[None], ll, S)
            if fault == "drop_bin" and f == F // 2:
                new[:, tf] = S[:, tf]
            S = new
    return np.ascontiguousarray(S.T)


def _srp_operands(x, sv, pairs, fault=None):
    l, r = pair_lists(pairs)
    ur, ui = sm.coherence(np.asarray(x)[l], np.asarray(x)[r])               # [P][T][F]
    dr, di = sm.coherence(np.asarray(sv)[:, l], np.asarray(sv)[:, r])       # [A][P][F]
    if fault == "imag_sign":
        di = di.copy()
        di[:, len(pairs) // 2, di.shape[2] // 2] *= f32(-1)
    return ur, ui, dr, di


def model_srp(x, sv, pairs, mask=None, fault=None):
    """ssl_obs_prep_kernel<SRP> and ssl_frame_score_kernel<SRP> in float32 -> S [T][A] float32.

    fault: "drop_bin", "stale_frame", "mask_neighbour" as model_ml; "last_pair" (the last pair
    skipped), "imag_sign" (the imaginary sign of one pair's steer-vector phasor flipped in one bin)."""
    x = np.array(x, np.complex64)
    C, T, F = x.shape
    A, K = sv.shape[0], len(pairs)
    m = np.ones((T, F), f32) if mask is None else np.array(mask, f32)
    if fault == "stale_frame" and T > TILE:
        x[:, TILE] = x[:, TILE - 1]
        m[TILE] = m[TILE - 1]
    ur, ui, dr, di = _srp_operands(x, sv, pairs, fault)
    S = np.zeros((A, T), f32)
    tf = _tile_fault_frames(T)
    with np.errstate(all="ignore"):
        for f in range(F):
            mf = m[:, 31] if (fault == "mask_neighbour" and f == 32) else m[:, f]
            new = S
            for p in range(K - 1 if fault == "last_pair" else K):
                vr, vi = (mf * ur[p, :, f]).astype(f32), (mf * ui[p, :, f]).astype(f32)
                new = _fma(dr[:, p, f][:, None], vr[None], _fma(di[:, p, f][:, None], vi[None], new))
            if fault == "drop_bin" and f == F // 2:
                new = new.copy()
                new[:, tf] = S[:, tf]
            S = new
        S = (S * (f32(1) / f32(K))).astype(f32)
    return np.ascontiguousarray(S.T)


def model_srp_fold(x, sv, pairs, mask, window, fault=None):
    """ssl_srp_fold_kernel, ssl_srp_fold_sum_kernel and the frame-score kernel on the one folded
    pseudo-frame -> S [A] float32.  fault: "fold_boundary" (the first frame of the second 64-frame
    chunk left out), "last_pair", "imag_sign"."""
    x = np.asarray(x, np.complex64)
    C, T, F = x.shape
    A, K = sv.shape[0], len(pairs)
    m = np.ones((T, F), f32) if mask is None else np.asarray(mask, f32)
    ur, ui, dr, di = _srp_operands(x, sv, pairs, fault)
    t0, t1 = window
    Ur, Ui = np.zeros((K, F)), np.zeros((K, F))
    with np.errstate(all="ignore"):
        for ta in range(t0, t1, CHUNK):
            tb = min(t1, ta + CHUNK)
            pr, pi = np.zeros((K, F)), np.zeros((K, F))
            for t in range(ta, tb):
                if fault == "fold_boundary" and t == t0 + CHUNK:
                    continue
                pr += (m[t][None] * ur[:, t]).astype(f32)
                pi += (m[t][None] * ui[:, t]).astype(f32)
            Ur, Ui = Ur + pr, Ui + pi
        Ur, Ui = Ur.astype(f32), Ui.astype(f32)
        S = np.zeros(A, f32)
        for f in range(F):
            for p in range(K - 1 if fault == "last_pair" else K):
                S = _fma(dr[:, p, f], Ur[p, f], _fma(di[:, p, f], Ui[p, f], S))
        return (S * (f32(1) / f32(K))).astype(f32)


def model_pad_overwrite(S, pad_value):
    """the padding lane a = A of frame 0 stored: it lands on direction 0 of frame 1"""
    S = np.array(S)
    if S.shape[0] > 1 and S.shape[1] % 64:
        S[1, 0] = pad_value
    return S


def model_windows(S, windows, take_min=False, fault=None):
    """ssl_window_kernel: (index [W], score [W][A] float64) out of frame scores S [T][A] float32.
    fault: "t1_inclusive" (the first window only), "tie_highest"."""
    S = np.asarray(S, f32).astype(np.float64)
    T = S.shape[0]
    sc = []
    for w, (t0, t1) in enumerate(windows):
        if fault == "t1_inclusive" and w == 0:
            t1 = min(t1 + 1, T)
        sc.append(S[t0:t1].sum(axis=0))
    sc = np.stack(sc)
    return model_index(sc, take_min, fault), sc


def model_index(sc, take_min=False, fault=None):
    idx = []
    for row in np.asarray(sc, np.float64):
        nan = np.flatnonzero(np.isnan(row))
        hit = nan if nan.size else np.flatnonzero(row == (row.min() if take_min else row.max()))
        idx.append(int(hit[-1] if fault == "tie_highest" else hit[0]))
    return np.array(idx)


# ------------------------------------------------------------------ the cases, shared by the CPU and the GPU file
@dataclass
class Case:
    name: str
    backend: str                    # "ml" | "srp" | "music"
    family: str
    x: np.ndarray                   # complex64 [C][T][F]
    sv: np.ndarray                  # complex64 [A][C][F]
    mask: object = None             # float32 [T][F] or None
    windows: object = None          # [(t0, t1), ...]
    pairs: object = None            # SRP: [(l, r), ...]
    kw: object = None               # ML: compression, eps, norm
    rule: str = "ref"               # "ref": the reference and the allowance; "range": ml_range()
    needs_delta: bool = False       # the condition delta >= 2^-10 power is part of the case
    min_gap: float = 0.1            # MUSIC: (lambda_1 - lambda_2) / lambda_1 of every judged bin
    dead_bins: tuple = ()           # MUSIC: bins of zero covariance (status non-OK, zero steer vector)

    @property
    def fold(self):
        """SRP with one window goes through the offline fold"""
        return self.backend == "srp" and len(self.windows) == 1

    @property
    def take_min(self):
        return self.backend == "music"


ML_CLI = dict(compression=-1, eps=EPS32)


def make(name, backend, family, C, T, F, A, windows=None, masked=True, steer="unit", pairs=None, kw=None, **extra):
    if backend == "music" and family == "white":
        family = "spiked"
    x = spectrogram(family, C, T, F, A, spike=backend == "music" and family == "ladder")
    sv = unit_steer(A, C, F) if steer == "unit" else random_steer(A, C, F)
    if backend == "ml":
        kw = dict(ML_CLI if kw is None else kw)
        if C == 1 or family == "aligned":
            extra.setdefault("rule", "range")
    if backend == "srp" and pairs is None:
        pairs = pairs_of(C)
    if backend == "ml" and extra.get("rule", "ref") == "ref":
        extra["needs_delta"] = True
        x = condition_ml(x, sv, kw)
    return Case(f"{name} {backend} {family} C={C} T={T} F={F} A={A}", backend, family, x, sv,
                mask(T, F) if masked else None, windows or [(0, T)], pairs, kw, **extra)


def condition_ml(x, sv, kw, floor=2 * DELTA_FLOOR, rounds=12):
    """ML is a cancellation: a cell (t, f) whose observation lies within sin^2 < 2^-9 of a candidate
    direction is out of reach of any float32 evaluation at the flat bar, in every family.  Such cells
    are moved: one microphone's sample is doubled (an exact operation: lattices stay lattices) or,
    every other round, turned by the angle of 0.6 + 0.8i (under norm the moduli do not count)."""
    x = np.array(x)
    for k in range(rounds):
        _, _, terms = ml_frames(x, sv, None, **kw)
        with np.errstate(all="ignore"):
            low = (terms["delta"] < floor * terms["power"][None]).any(axis=0) & (terms["power"] > 0)    # [T][F]
        if not low.any():
            return x
        if k % 2 == 0:
            x[(k // 2) % x.shape[0]][low] *= np.complex64(2.0)
        else:
            x[0][low] *= np.complex64(0.6 + 0.8j)
    raise AssertionError("condition_ml: cells below the floor remain")


def frames_and_whole(T, limit=None):
    """every single frame and the whole utterance; limit: the tile edges among the single frames only"""
    singles = single_frames(T)
    if limit:
        keep = sorted({t for t in (0, 1, 30, 31, 32, 33, 62, 63, 64, T - 2, T - 1) if 0 <= t < T})[:limit]
        singles = [(t, t + 1) for t in keep]
    return singles + [(0, T)]


def expected(case):
    """dict(idx [W], ref [W][A], A [W][A] | lo, hi, own [W][A], ...): what a result of the case is held to."""
    c, W = case, case.windows
    out = {}
    if c.backend == "ml":
        out["idx"], out["ref"] = reference("ml", c.x, c.sv, W, c.mask, **c.kw)
        S, A, terms = ml_frames(c.x, c.sv, c.mask, **c.kw)
        out["own"], out["A"] = window_sums(S, W), window_sums(A, W)
        with np.errstate(all="ignore"):
            fin = np.isfinite(terms["delta"]) & (terms["power"][None] > 0)
            out["delta_ratio"] = float(np.min(np.where(fin, terms["delta"] / np.where(fin, terms["power"][None], 1), np.inf)))
        if c.rule == "range":
            out["lo"], out["hi"] = ml_range(c.x, c.mask, W, c.kw["eps"], c.sv.shape[0])
    elif c.backend == "srp":
        out["idx"], out["ref"] = reference("srp", c.x, c.sv, W, c.mask, c.pairs)
        if c.fold:
            out["own"], out["A"] = srp_fold(c.x, c.sv, c.pairs, c.mask, W)
        else:
            S, A, _ = srp_frames(c.x, c.sv, c.pairs, c.mask)
            out["own"], out["A"] = window_sums(S, W), window_sums(A, W)
    else:
        sv = c.sv
        out["idx"], out["ref"] = reference("music", c.x, sv, W, c.mask)
        terms = [music_terms(c.x, sv, c.mask, w) for w in W]
        out["own"], out["A"] = np.stack([t["score"] for t in terms]), np.stack([t["A"] for t in terms])
        live = [~t["dead"] for t in terms]
        out["gap"] = float(min(t["gap"][l].min() for t, l in zip(terms, live) if l.any()))
        out["dead"] = sorted({int(f) for t in terms for f in np.flatnonzero(t["dead"])})
        if out["dead"]:
            # the reference's eigh picks an arbitrary basis in a zero bin: with a zero steer vector there
            # the bin contributes 0 in any basis, and the rest of the sum is the score
            assert not np.asarray(sv)[:, :, out["dead"]].any()
    return out


def evaluate(case, exp, idx, got, tally, status=0):
    """Judge one result (device or model) of a case into the tally."""
    c = case
    if c.rule == "range":
        v = judge_range(c.name, got, exp["lo"], exp["hi"])
    else:
        v = judge(c.name, got, exp["ref"], exp["A"])
    tally.add(f"{c.backend} {c.family}" + (" (range)" if c.rule == "range" else ""), v)
    if v.unjudged:
        tally.fail([f"{c.name}: {v.unjudged} cells have no finite bar"])
    if c.rule == "range":
        own = [int((np.argmin if c.take_min else np.argmax)(g)) for g in got]
        tally.fail([f"{c.name}: window {w}: index {int(i)}, the first extremum of its own scores is {o}"
                    for w, (i, o) in enumerate(zip(idx, own)) if int(i) != o])
    else:
        tally.fail(index_failures(c.name, idx, got, exp["ref"], c.take_min))
    if c.backend == "music" and bool(c.dead_bins) != (status != 0):
        tally.fail([f"{c.name}: status {status} with zero-covariance bins {c.dead_bins}"])
    elif c.backend != "music" and status != 0:
        tally.fail([f"{c.name}: status {status}"])
    return v


def run_model(case, fault=None, **kw):
    """The float32 models on a case -> (index [W], score [W][A] float64); ML and SRP."""
    c = case
    if c.backend == "ml":
        S = model_ml(c.x, c.sv, c.mask, fault=fault, **c.kw, **kw)
    elif c.fold:
        S = model_srp_fold(c.x, c.sv, c.pairs, c.mask, c.windows[0], fault=fault)[None]
        return model_windows(S, [(0, 1)], fault=fault)
    else:
        S = model_srp(c.x, c.sv, c.pairs, c.mask, fault=fault)
    return model_windows(S, c.windows, fault=fault)


BACKENDS = ("ml", "srp", "music")
EDGES = [("T", v) for v in (1, 31, 32, 33, 64, 65)] + [("F", v) for v in (1, 2, 31, 32, 33, 65)] + \
        [("A", v) for v in (1, 63, 64, 65, 255, 256, 257, 513)]
EDGE_BASE = dict(T=3, F=5, A=7)
HOT_BINS = (0, 31, 32, 64)          # F = 65
FOLD_WHOLE = (63, 64, 65, 128, 129)
FOLD_WINDOWS = ((5, 70), (64, 65), (63, 129))
TIE_SETS = ((0, 255, 256, 300, 512), (255, 256), (300, 512), (256, 512), (44, 300), (512,))
NAN_DIRECTIONS = ((0,), (255,), (256,), (300,), (512,), (300, 44), (512, 257), (511, 256, 300))
MUSIC_TABLE = [(0, 65), (0, 1), (64, 65), (5, 20), (31, 34), (32, 65), (7, 8), (0, 32)]


def channel_cases(C, backend):
    """every channel count: T = 33, F = 33, A = 65, every single frame and the whole, all pairs"""
    W = frames_and_whole(33) if backend != "music" else frames_and_whole(33, limit=6)
    return [make("channels", backend, fam, C, 33, 33, 65, W, masked=fam == "plane") for fam in ("white", "plane")]


def edge_cases(axis, value, backend):
    shape = dict(EDGE_BASE)
    shape[axis] = value
    T, F, A = shape["T"], shape["F"], shape["A"]
    W = frames_and_whole(T, limit=6 if backend == "music" else None)
    return [make(f"edge {axis}", backend, fam, C, T, F, A, W, steer="unit" if fam == "plane" else "random")
            for C in (3, 8) for fam in ("white", "plane")]


def onehot_cases(backend):
    """one term of the sum over the bins: a one-hot mask (ML, SRP), a one-hot steer vector (MUSIC)"""
    out = []
    T, F, A, C = 34, 65, 65, 4
    for f in HOT_BINS:
        c = make(f"one-hot bin {f}", backend, "white", C, T, F, A, frames_and_whole(T, limit=6), masked=False,
                 steer="random")
        if backend == "music":
            sv = np.zeros_like(c.sv)
            sv[:, :, f] = c.sv[:, :, f]
            c.sv = sv
        else:
            c.mask = onehot_mask(T, F, [(32, f), (0, f)])
        out.append(c)
    return out


def fold_cases():
    """[(the single-window case, the same window first in a two-window table)]"""
    out = []
    for T, w in [(T, (0, T)) for T in FOLD_WHOLE] + [(129, w) for w in FOLD_WINDOWS]:
        one = make(f"fold {w}", "srp", "white", 4, T, 33, 65, [w])
        two = make(f"frames {w}", "srp", "white", 4, T, 33, 65, [w, (0, 1)])
        out.append((one, two))
    return out


def ml_option_cases():
    out = []
    W = frames_and_whole(33, limit=4)
    for family, norms in (("ladder", (False, True)), ("extreme", (True,))):
        for norm in norms:
            for eps in (EPS32, 1e-8, 1e-3):
                out.append(make(f"log eps={eps:.1e} norm={norm}", "ml", family, 6, 33, 33, 65, W, steer="random",
                                kw=dict(compression=0, eps=eps, norm=norm)))
            for comp in (0.3, 0.5, 1.0):
                out.append(make(f"power c={comp} norm={norm}", "ml", family, 6, 33, 33, 65, W, steer="random",
                                kw=dict(compression=comp, eps=1e-3, norm=norm)))
    for eps in (EPS32, 1e-8, 1e-3):
        out.append(make(f"aligned eps={eps:.1e}", "ml", "aligned", 6, 33, 33, 65, W, kw=dict(compression=0, eps=eps)))
    return out


FAMILIES_OF = dict(ml=("white", "plane", "aligned", "lattice", "ladder", "extreme", "nan"),
                   srp=("white", "plane", "lattice", "ladder", "extreme", "nan"),
                   music=("spiked", "plane", "ladder", "close"))


def family_cases(backend, C):
    out = []
    for fam in FAMILIES_OF[backend]:
        if fam == "close" and C < 2:
            continue
        W = [(0, 33)] if fam == "close" else frames_and_whole(33, limit=5)
        F = 9           # (the ladder's |ll| reach 40: over more bins the float32 sum of a frame nears the flat bar)
        kw = dict(compression=0, eps=1e-3, norm=True) if (backend == "ml" and fam == "extreme") else None
        out.append(make("family", backend, fam, C, 33, F, 65, W, masked=fam != "close", steer="unit" if fam in ("plane", "aligned") else "random",
                        kw=kw, **(dict(min_gap=5e-4) if fam == "close" else {})))
    return out


def tie_cases(backend):
    """A = 513: exact copies of the best direction at chosen positions"""
    out = []
    base = make("tie", backend, "plane", 4, 3, 5, 513, [(0, 3), (1, 2)])
    best = int(reference(backend, base.x, base.sv, [(0, 3)], base.mask, base.pairs, **(base.kw or {}))[0][0])
    for pos in TIE_SETS:
        c = make(f"tie {pos}", backend, "plane", 4, 3, 5, 513, [(0, 3), (1, 2)])
        c.sv = duplicate_steer(base.sv, best, pos)
        out.append((c, best, pos))
    return out


def nan_cases(backend):
    """A = 513.  A NaN in the spectrogram, in the mask (ML, SRP: every direction of the frames it
    touches), in the steer vectors of chosen directions (every backend: exactly those directions)."""
    out = []
    W = [(0, 5), (2, 3), (0, 2)]
    if backend != "music":
        for cell in ((3, 2, 1), (0, 0, 4)):
            c = make(f"nan in x{cell}", backend, "white", 4, 5, 5, 513, W)
            c.x = c.x.copy()
            c.x[cell] = complex(c.x[cell].real, np.nan)
            out.append(c)
        c = make("nan in mask", backend, "white", 4, 5, 5, 513, W)
        c.mask = c.mask.copy()
        c.mask[2, 3] = np.nan
        out.append(c)
    for dirs in NAN_DIRECTIONS:
        c = make(f"nan in sv{dirs}", backend, "white", 4, 5, 5, 513, W)
        c.sv = c.sv.copy()
        for k, a in enumerate(dirs):
            c.sv[a, k % 4, (2 * k + 1) % 5] = complex(np.nan, 0.0)
        out.append(c)
    return out


def music_window_cases():
    out = [make("music windows", "music", "spiked", 4, 65, 33, 65, MUSIC_TABLE),
           make("music windows", "music", "plane", 5, 65, 33, 65, MUSIC_TABLE, masked=False),
           make("music close", "music", "close", 4, 65, 33, 65, [(0, 65)], masked=False, min_gap=5e-4)]
    c = make("music zero bin", "music", "spiked", 4, 65, 33, 65, MUSIC_TABLE[:4])
    c.x, c.sv = c.x.copy(), c.sv.copy()
    for f in (8, 32):
        c.x[:, :, f] = 0
        c.sv[:, :, f] = 0
    c.dead_bins = (8, 32)
    out.append(c)
    return out
