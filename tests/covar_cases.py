"""
Constructed cases for the masked spatial covariance (numpy only: no device), the reference a device
result is held to, the allowance, the judge, and float32 models of the device's summation orders.

    Phi_f[i][j] = sum_t m_t,f x_i,t,f conj(x_j,t,f) / max(sum_t m_t,f, 1e-6)

REFERENCE.  oracle.np_oracle.compute_covar on complex128 / float64 copies of what the device gets.

ALLOWANCE, per bin f, entry (i, j) and part (re, im) -- derived, not measured:

    A = (T + 8) u32 (S_ij + |Phi_ij| Sm) / den
    S_ij = sum_t |m_t| |x_i,t| |x_j,t|,  Sm = sum_t |m_t|,  den = max(sum_t m_t, 1e-6),  u32 = 2^-24

the gamma_n bound of an n-term float32 multiply-add fold in ANY order, for the numerator (S) and
for the denominator (|Phi| Sm); the 8 pays for the roundings outside the fold: the product
x_i conj(x_j) (two), m times it, 1 - m of a noise mask, the slab sums' extra level, the division.
A sequential register fold (covar_fold.h), the k-ordered chain of v_mfma_f32_32x32x2_f32 (wide.hip)
and a sum of slab partials are all such folds.  No entry is left out: where A == 0 (a bin whose
mask is identically zero, an entry of an all-zero channel) the device must return exactly 0.
PARITY_NOTES_COVAR.md has the derivation and the float32 range limit of the `ladder` family.

FORWARD TERM.  The fused forms fold the device's own float32 spectra; the reference folds float64
spectra of the same samples.  The forward transform promises, per channel and frame, an error
vector of norm at most a_c,t = M_BITS max(||X32_c,t - X_c,t||, u32 ||X_c,t||) (stft_cases: X32 the
float32 yardstick transform), so an entry may move by

    A_fwd = sum_t |m_t| (a_i,t |X_j,t| + |X_i,t| a_j,t + a_i,t a_j,t) / den

SPECTROGRAM FAMILIES, complex64 [C][T][F]: white, coherent (x_c = a_c s + 1e-3 n_c with real gains:
the off-diagonal imaginary parts are nearly pure cancellation), ladder (white scaled per bin by
2^linspace(30, -30, F)), sparse (whole frames and one whole channel exactly zero).
MASK FAMILIES, float32 [T][F]: uniform (0.05, 0.95); onehot (one frame per bin at 1, placed at 0,
T - 1 and on both sides of every edge handed in); zero (even bins identically 0); ones (bins
identically 1: the odd ones, bin 0 when there is one bin); tiny (uniform x 1e-9: the 1e-6 floor is
active); over (values up to 1.7); itf (an independent second mask, for the noise side); signed
(1 - over: the noise mask an unclamped `over` produces, negative in places).

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***
"""
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as o  # noqa: E402
import stft_cases as sc  # noqa: E402
import wide_model  # noqa: E402

M_BITS = sc.M_BITS
U32 = 2.0 ** -24
BINS, HOP = 257, 256
SPEC_FAMILIES = ("white", "coherent", "ladder", "sparse")
MASK_FAMILIES = ("uniform", "onehot", "zero", "ones", "tiny", "over", "itf", "signed")
PARTS = ("re", "im")


# ------------------------------------------------------------------ spectrograms and masks
def _cnormal(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def spectrogram(family, C, T, F, seed=0):
    """complex64 [C][T][F]"""
    rng = np.random.default_rng([seed, C, T, F, SPEC_FAMILIES.index(family)])
    x = _cnormal(rng, C, T, F)
    if family == "coherent":
        gains = rng.uniform(0.5, 1.5, size=(C, 1, 1))
        x = gains * _cnormal(rng, 1, T, F) + 1e-3 * x
    elif family == "ladder":
        x = x * 2.0 ** np.linspace(30, -30, F)
    elif family == "sparse":
        x[:, rng.uniform(size=T) < 0.3] = 0.0
        x[:, T // 2] = 0.0
        if C >= 2:
            x[C // 2] = 0.0
    return x.astype(np.complex64)


def onehot_frames(T, edges=()):
    """0, T - 1 and both sides of every edge inside (0, T), in order, without repeats."""
    want = [0, T - 1]
    for e in sorted(set(edges)):
        if 0 < e < T:
            want += [e - 1, e]
    return sorted(set(want))


def mask(family, T, F, seed=0, edges=()):
    """float32 [T][F]"""
    rng = np.random.default_rng([seed, T, F, MASK_FAMILIES.index(family), 77])
    m = rng.uniform(0.05, 0.95, size=(T, F))
    if family == "onehot":
        frames = onehot_frames(T, edges)
        m[:] = 0.0
        for f in range(F):
            m[frames[(f + seed) % len(frames)], f] = 1.0
    elif family == "zero":
        m[:, 0::2] = 0.0
    elif family == "ones":
        m[:, (1 if F > 1 else 0)::2] = 1.0
    elif family == "tiny":
        m *= 1e-9
    elif family in ("over", "signed"):
        m = rng.uniform(0.05, 1.7, size=(T, F))
    elif family == "itf":
        m = rng.uniform(0.02, 1.5, size=(T, F))
    m = m.astype(np.float32)
    return np.float32(1) - m if family == "signed" else m


# ------------------------------------------------------------------ reference and allowance
def reference(x, m):
    """x [C][T][F] complex, m [T][F] -> compute_covar in complex128, [F][C][C]"""
    X = np.transpose(np.asarray(x).astype(np.complex128), (0, 2, 1))
    return o.compute_covar(X, np.asarray(m, np.float64))


def _fct(a):
    return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))       # [C][T][F] -> [F][C][T]


def allowance(x, m, ref, terms=None):
    """A [F][C][C] (the same for the real and the imaginary part).  terms: n of gamma_n (T + 8)."""
    ax = _fct(np.abs(np.asarray(x).astype(np.complex128)))
    m = np.asarray(m, np.float64)
    am = np.abs(m).T                                                # [F][T]
    S = (ax * am[:, None, :]) @ np.transpose(ax, (0, 2, 1))
    den = np.maximum(m.sum(axis=0), 1e-6)
    n = (m.shape[0] + 8) if terms is None else terms
    return n * U32 * (S + np.abs(ref) * am.sum(axis=1)[:, None, None]) / den[:, None, None]


def forward_promise(X, X32, floor=0.0, axis=-1):
    """What the forward transform promises of one frame's spectrum, as a norm over `axis` (the
    bins): max(||X32 - X||, u32 ||X||) + floor, X the float64 spectra and X32 the float32
    yardstick's (stft_cases.f32_stft).  Without M_BITS."""
    return np.maximum(np.linalg.norm(X32 - X, axis=axis), U32 * np.linalg.norm(X, axis=axis)) + floor


def bin_forward_term(mask_ft, xf, at):
    """Per bin [F]: sum_t m_t 2 ||X_f,t|| a_t / max(sum_t m_t, 1e-6) -- how far the norm of a bin's
    covariance may move when every frame's spectrum moves by a_t (dR = X dX^H + dX X^H).
    mask_ft [F][T] float64, xf [F][T] the norm over the channels, at [T]."""
    return (mask_ft * 2 * xf * at[None, :]).sum(axis=1) / np.maximum(mask_ft.sum(axis=1), 1e-6)


def forward_allowance(X, X32, m, a=None):
    """A_fwd [F][C][C] of the module docstring.  X, X32 [C][T][F]; a [C][T]: the promise, when the
    caller hands in a subset of the bins."""
    X = np.asarray(X, np.complex128)
    if a is None:
        a = M_BITS * forward_promise(X, np.asarray(X32).astype(np.complex128))  # [C][T]
    aX = _fct(np.abs(X))                                                          # [F][C][T]
    m = np.asarray(m, np.float64)
    W = np.abs(m).T[:, None, :] * a[None]                                         # [F][C][T]
    t1 = W @ np.transpose(aX, (0, 2, 1))                                          # a_i |X_j|
    den = np.maximum(m.sum(axis=0), 1e-6)
    return (t1 + np.transpose(t1, (0, 2, 1)) + W @ a.T[None]) / den[:, None, None]


# ------------------------------------------------------------------ the judge
@dataclass
class Verdict:
    name: str
    worst: float            # the largest error / allowance (inf: a non-zero where A == 0, a non-finite)
    where: tuple            # (f, i, j, part) of the worst
    zeros: int              # entries with A == 0, each held to exactly 0
    failures: list


def judge(name, got, ref, A, report=4):
    """got [F][C][C] complex64 as the device stored it, ref complex128, A [F][C][C].  Every entry
    and part is judged: |got - ref| <= A, and got == 0 exactly where A == 0."""
    got = np.asarray(got)
    if got.shape != ref.shape:
        return Verdict(name, np.inf, (-1, -1, -1, "shape"), 0, [f"{name}: shape {got.shape} against {ref.shape}"])
    g = got.astype(np.complex128)
    err = np.stack([np.abs(g.real - ref.real), np.abs(g.imag - ref.imag)], axis=-1)
    err[~np.isfinite(err)] = np.inf
    A2 = np.broadcast_to(np.asarray(A, np.float64)[..., None], err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(A2 > 0, err / A2, np.where(err == 0, 0.0, np.inf))
    ratio = np.nan_to_num(ratio, nan=np.inf, posinf=np.inf)
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    fails = []
    bad = np.argwhere(~(ratio <= 1.0))
    for f, i, j, p in bad[:report]:
        gv = (g.real, g.imag)[p][f, i, j]
        rv = (ref.real, ref.imag)[p][f, i, j]
        fails.append(f"{name}: bin {f} entry ({i}, {j}) {PARTS[p]}: got {gv:.9e}, reference {rv:.9e}, error "
                     f"{err[f, i, j, p]:.3e} > allowance {A2[f, i, j, p]:.3e} (ratio {ratio[f, i, j, p]:.3g}, "
                     f"|Phi| {abs(ref[f, i, j]):.3e}); {len(bad)} of {ratio.size} parts fail")
    return Verdict(name, float(ratio[k]), (int(k[0]), int(k[1]), int(k[2]), PARTS[k[3]]), int((A2 == 0).sum()) // 2, fails)


def structure(name, got):
    """Failure lines for: a non-finite value, a diagonal that is not real, an entry (j, i) that
    is not bit for bit the conjugate of (i, j)."""
    got = np.asarray(got)
    fails = []
    if not np.isfinite(got.view(np.float32)).all():
        fails.append(f"{name}: {int((~np.isfinite(got)).sum())} non-finite entries")
    gt = np.transpose(got, (0, 2, 1))
    herm = (got.real == gt.real) & (got.imag == -gt.imag)
    if not herm.all():
        f, i, j = np.argwhere(~herm)[0]
        fails.append(f"{name}: not Hermitian at bin {f} ({i}, {j}): {got[f, i, j]} against {got[f, j, i]}")
    d = np.einsum("fii->fi", got.imag)
    if d.any():
        f, i = np.argwhere(d != 0)[0]
        fails.append(f"{name}: diagonal ({i}, {i}) of bin {f} has imaginary part {d[f, i]}")
    return fails


def rel_rms(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Tally:
    """Verdicts of one test: the worst ratio per family and where it occurred, and every failure."""

    def __init__(self, form):
        self.form, self.worst, self.failures, self.count, self.zeros = form, {}, [], 0, 0

    def add(self, family, v):
        w = self.worst.setdefault(family, [0.0, "", None])
        if v.worst >= w[0]:
            w[:] = [v.worst, v.name, v.where]
        self.failures += v.failures
        self.count += 1
        self.zeros += v.zeros

    def fail(self, lines):
        self.failures += list(lines)

    def overall(self):
        return max(self.worst.values(), key=lambda w: w[0]) if self.worst else [0.0, "", None]

    def finish(self):
        for fam, (r, name, where) in sorted(self.worst.items()):
            print(f"[{self.form}] {fam:12s} worst ratio {r:.3f} at (f, i, j, part) = {where} ({name})")
        r, name, where = self.overall()
        print(f"[{self.form}] {self.count} matrices judged, {self.zeros} entries held to exactly 0; "
              f"worst ratio {r:.3f} at {where} ({name})")
        assert not self.failures, f"{len(self.failures)} failures:\n" + "\n".join(self.failures[:25])


# ------------------------------------------------------------------ float32 models of the device orders
def upper_pairs(C):
    return [(i, j) for i in range(C) for j in range(i, C)]


def fold_model(x, m, cuts=(), fault=None, at=None):
    """The sequential float32 fold: per slab (cut at the frames `cuts`) frame after frame
    acc += m (x_i conj x_j), den += m, every operation rounded to float32; the slabs summed in slab
    order; one division.  x [C][T][F] complex64, m [T][F] float32 -> [F][C][C] complex64.

    fault: one of the seeded faults of test_covar_cases.py --
      "drop" / "twice"  frame `at` (a tile or slab edge) left out / counted twice
      "mask_next_bin"   the mask read from bin f + 1
      "swap_planes"     the real and imaginary planes of pair (0, 1) exchanged
      "pair_off"        the pair after (0, C - 1) read in its place (an index off by one)
      "floor_added"     the normaliser taken as 1e-6 + den"""
    x = np.asarray(x, np.complex64)
    m = np.asarray(m, np.float32)
    C, T, F = x.shape
    if fault == "mask_next_bin":
        m = np.roll(m, -1, axis=1)
    xr = np.ascontiguousarray(np.transpose(x.real, (1, 2, 0)))      # [T][F][C]
    xi = np.ascontiguousarray(np.transpose(x.imag, (1, 2, 0)))
    bounds = [0] + [c for c in sorted(set(cuts)) if 0 < c < T] + [T]
    num_re = np.zeros((F, C, C), np.float32)
    num_im = np.zeros((F, C, C), np.float32)
    den = np.zeros(F, np.float32)
    for t0, t1 in zip(bounds[:-1], bounds[1:]):
        a_re = np.zeros((F, C, C), np.float32)
        a_im = np.zeros((F, C, C), np.float32)
        d = np.zeros(F, np.float32)
        frames = list(range(t0, t1))
        if fault == "drop" and at in frames:
            frames.remove(at)
        if fault == "twice" and at in frames:
            frames.insert(frames.index(at), at)
        for t in frames:
            r, i, w = xr[t], xi[t], m[t][:, None, None]
            p_re = r[:, :, None] * r[:, None, :] + i[:, :, None] * i[:, None, :]
            p_im = i[:, :, None] * r[:, None, :] - r[:, :, None] * i[:, None, :]
            a_re = a_re + w * p_re
            a_im = a_im + w * p_im
            d = d + m[t]
        num_re, num_im, den = num_re + a_re, num_im + a_im, den + d
    assert num_re.dtype == np.float32 and den.dtype == np.float32
    dd = (np.float32(1e-6) + den) if fault == "floor_added" else np.maximum(den, np.float32(1e-6))
    re, im = num_re / dd[:, None, None], num_im / dd[:, None, None]
    # the device stores the upper triangle and mirrors it: Hermitian bit for bit, a real diagonal
    iu = np.triu_indices(C, 1)
    re[:, iu[1], iu[0]] = re[:, iu[0], iu[1]]
    im[:, iu[1], iu[0]] = -im[:, iu[0], iu[1]]
    im[:, np.arange(C), np.arange(C)] = 0.0
    if fault == "swap_planes" and C >= 2:
        re[:, 0, 1], im[:, 0, 1] = im[:, 0, 1].copy(), re[:, 0, 1].copy()
        re[:, 1, 0], im[:, 1, 0] = re[:, 0, 1], -im[:, 0, 1]
    if fault == "pair_off" and C >= 2:
        pairs = upper_pairs(C)
        i2, j2 = pairs[pairs.index((0, C - 1)) + 1]                 # (1, 1)
        re[:, 0, C - 1], im[:, 0, C - 1] = re[:, i2, j2].copy(), im[:, i2, j2].copy()
        re[:, C - 1, 0], im[:, C - 1, 0] = re[:, 0, C - 1], -im[:, 0, C - 1]
    return (re + 1j * im).astype(np.complex64)


def wide_fold_model(x, m, bins=None):
    """The 9-to-16-channel matrix-core fold through tests/wide_model.py as it is (chunks of 8 frames
    over the two half-waves, 128-frame slabs, the pairs read out of the 32 x 32 tile), float32.
    Returns [len(bins)][C][C] complex64 for the bins asked for (default all)."""
    x = np.asarray(x, np.complex64)
    C, T, F = x.shape
    bins = range(F) if bins is None else bins
    Tp = (T + 3) & ~3
    out = np.zeros((len(bins), C, C), np.complex64)
    for k, f in enumerate(bins):
        xb = np.zeros((C, Tp), np.complex64)
        xb[:, :T] = x[:, :, f]
        planes = wide_model.covar_planes(xb, np.asarray(m[:, f], np.float32), C, T, dtype=np.float32)
        out[k] = wide_model.matrix_of_planes(planes, C)
    return out


# ------------------------------------------------------------------ the stand-alone operator's cases
SA_BINS = (1, 5, 9, 255, 256, 257, 258)         # the 256-thread block edge; pitch ceil8(F)
SA_FRAMES = (1, 2, 31, 32, 33, 65, 97)
SA_MASKS = ("uniform", "onehot", "zero", "tiny", "over", "signed")
SA_LONG = 2049                                  # the smallest T whose last split is empty


@dataclass(frozen=True)
class Case:
    spec: str
    mask: str
    C: int
    T: int
    F: int

    @property
    def name(self):
        return f"{self.spec}/{self.mask} C={self.C} T={self.T} F={self.F}"


def standalone_splits(T):
    """(splits launched, frames per split, splits that hold frames) of setk_covar"""
    split = max(1, min(64, -(-T // 32)))
    per = -(-T // split)
    return split, per, -(-T // per)


def standalone_edges(T):
    _, per, _ = standalone_splits(T)
    return list(range(per, T, per))


def standalone_cases(C):
    """Every (frames, bins) pair with the (spectrogram, mask) pairs dealt round (49 = 2 x 24 + 1:
    each pair at least twice, shifted by C), every pair at (97, 257) -- three split edges, the whole
    width -- and T = 2049 at F = 5."""
    pairs = [(s, k) for s in SPEC_FAMILIES for k in SA_MASKS]
    cases, n = [], C
    for T in SA_FRAMES:
        for F in SA_BINS:
            s, k = pairs[n % len(pairs)]
            cases.append(Case(s, k, C, T, F))
            n += 1
    cases += [Case(s, k, C, 97, 257) for s, k in pairs]
    cases += [Case(s, k, C, SA_LONG, 5) for s, k in
              (("ladder", "onehot"), ("white", "uniform"), ("coherent", "signed"), ("sparse", "tiny"))]
    return cases


def standalone_inputs(case):
    """(x [C][T][F] complex64, m [T][F] float32) of a case"""
    return (spectrogram(case.spec, case.C, case.T, case.F, seed=case.C),
            mask(case.mask, case.T, case.F, seed=case.C, edges=standalone_edges(case.T)))


# ------------------------------------------------------------------ the fused forms' cases
def tile_frames(C):
    """pass1_tile_frames (csrc/common.h)"""
    return min(32 // C, 8)


def fused_frames(C):
    """Frame counts of the fused fold (C <= 8: tiles of TB frames) and of the wide fold (chunks of
    8 frames in two halves of 4, slabs of 128).  T = 1 runs under center = False."""
    if C > 8:
        return (1, 3, 4, 5, 7, 8, 9, 127, 128, 129, 257)
    TB = tile_frames(C)
    return tuple(sorted({1, 2, TB - 1, TB, TB + 1, 8 * TB - 1, 8 * TB, 8 * TB + 1, 16 * TB + 1}))


def fused_edges(C, T):
    """Every frame at which a tile, a chunk half or a slab of the form may begin (the slabs are
    cut at multiples of the tile)."""
    return list(range(4, T, 4)) if C > 8 else list(range(tile_frames(C), T, tile_frames(C)))


# (label, speech mask family, clamp flag, noise mask family or None)
FUSED_MASKS = (("uniform", "uniform", True, None), ("onehot", "onehot", True, None), ("zero", "zero", True, None),
               ("ones", "ones", True, None), ("tiny", "tiny", True, None), ("over-raw", "over", False, None),
               ("over-clamped", "over", True, None), ("itf", "uniform", True, "itf"))


@dataclass(frozen=True)
class FusedCase:
    C: int
    T: int
    audio: str          # "white" / "coherent"
    label: str
    ms: str
    clamp: bool
    mn: object

    @property
    def center(self):
        return self.T > 1

    @property
    def name(self):
        return f"{self.audio}/{self.label} C={self.C} T={self.T}"

    @property
    def well_posed(self):
        """No bin has an all-zero or indefinite Rs or Rn, and there are frames enough for a
        positive definite Rn: the solve's status must be 0."""
        return (self.audio == "white" and self.label in ("uniform", "tiny", "over-clamped", "itf")
                and self.T >= 2 * self.C)


def fused_cases(C, itf=True):
    """Every frame count x every mask entry; the audio family alternates, so that each frame count
    and each mask meets both."""
    cases, n = [], 0
    for T in fused_frames(C):
        for label, ms, clamp, mn in FUSED_MASKS:
            n += 1
            if mn is not None and not itf:
                continue
            cases.append(FusedCase(C, T, ("white", "coherent")[(n + T) % 2], label, ms, clamp, mn))
    return cases


def samples_for(T, center=True):
    """A length with exactly T frames that is no multiple of the hop."""
    return HOP * (T - 1) + 100 + (0 if center else 512)


def audio(family, C, T, center=True, seed=0):
    """int16 [C][N] with peak about 0.1 of full scale: the float form is pcm / 32768 exactly."""
    N = samples_for(T, center)
    rng = np.random.default_rng([seed, C, T, int(center), SPEC_FAMILIES.index(family)])
    x = 0.03 * rng.standard_normal((C, N))
    if family == "coherent":
        x = rng.uniform(0.5, 1.0, size=(C, 1)) * (0.03 * rng.standard_normal(N))[None] + 1e-3 * x
    return np.round(np.clip(x, -0.1, 0.1) * 32768).astype(np.int16)


def as_float(pcm):
    return pcm.astype(np.float32) / np.float32(32768)


_spectra = {}


def spectra(family, C, T):
    """(pcm, X [C][T][F] complex128, X32 the float32 yardstick's) -- computed once, read-only."""
    key = (family, C, T)
    if key not in _spectra:
        pcm = audio(family, C, T, T > 1, seed=C)
        geo = sc.Geom(center=T > 1)
        x = as_float(pcm)
        X, X32 = sc.ref_stft(x, geo), sc.f32_stft(x, geo)
        assert X.shape == (C, T, BINS) and X32.shape == X.shape
        for a in (pcm, X, X32):
            a.setflags(write=False)
        _spectra[key] = (pcm, X, X32)
    return _spectra[key]


def fused_masks(case):
    """(speech mask as handed to the device, noise mask handed to it or None,
    the speech and noise masks the fold applies, float64)"""
    edges = fused_edges(case.C, case.T)
    ms = mask(case.ms, case.T, BINS, seed=case.C, edges=edges)
    mn = None if case.mn is None else mask(case.mn, case.T, BINS, seed=case.C + 100, edges=edges)
    es = np.minimum(ms, np.float32(1)) if case.clamp else ms
    en = (1.0 - es.astype(np.float64)) if mn is None else mn.astype(np.float64)
    return ms, mn, es.astype(np.float64), en


def fused_expectation(case, bins=None):
    """[(name, reference, allowance)] for Rs and Rn of a fused case: the float64 fold of the
    float64 spectra, A + A_fwd.  bins: the bins wanted (default all)."""
    _, X, X32 = spectra(case.audio, case.C, case.T)
    _, _, es, en = fused_masks(case)
    a = M_BITS * forward_promise(X, X32)           # (the promise is a norm over ALL bins of a frame)
    if bins is not None:
        X, X32, es, en = X[:, :, bins], X32[:, :, bins], es[:, bins], en[:, bins]
    out = []
    for name, m in (("Rs", es), ("Rn", en)):
        ref = reference(X, m)
        out.append((name, ref, allowance(X, m, ref) + forward_allowance(X, X32, m, a)))
    return out


# ------------------------------------------------------------------ the online recursion
ONLINE_CHANNELS = (1, 3, 5, 8)
ONLINE_T = 65
ONLINE_ALPHAS = (0.0, float(np.float32(0.8)))        # the C ABI takes a float: the value it receives
ONLINE_MASKS = ("uniform", "onehot", "over-clamped", "itf")


def online_chunks(C):
    TB = tile_frames(C)
    return tuple(sorted({1, TB - 1, TB + 1, 32, 33}))


def online_edges(C, T, chunk):
    """chunk boundaries, and the tiles inside each chunk"""
    TB = tile_frames(C)
    return sorted({t for c0 in range(0, T, chunk) for t in range(c0, min(c0 + chunk, T), TB)} - {0})


def online_recursion(X, ms, mn, chunk, alpha):
    """What online_model.online_parts computes for Rs and Rn, without its weights (np.linalg.solve
    refuses the exactly singular chunks of a one-frame chunk or a one-hot mask), and the allowance
    carried along: A_c = alpha A_{c-1} + phi_c a_c + 2 u32 |R_c| per entry, a_c the chunk's own
    A + A_fwd.  X [C][T][F] complex128 with its yardstick X32 in X = (X, X32).
    Returns {"Rs": (R [K][F][C][C], A [K][F][C][C]), "Rn": ...}."""
    X, X32 = X
    T = X.shape[1]
    out = {}
    for name, m in (("Rs", ms), ("Rn", mn)):
        R = A = 0.0
        Rs, As = [], []
        for c, t0 in enumerate(range(0, T, chunk)):
            sl = slice(t0, min(t0 + chunk, T))
            r = reference(X[:, sl], m[sl])
            a = allowance(X[:, sl], m[sl], r) + forward_allowance(X[:, sl], X32[:, sl], m[sl])
            phi = 1.0 if c == 0 else 1.0 - alpha
            R = alpha * R + phi * r
            A = alpha * A + phi * a + 2 * U32 * np.abs(R)
            Rs.append(R)
            As.append(A)
        out[name] = (np.stack(Rs), np.stack(As))
    return out
