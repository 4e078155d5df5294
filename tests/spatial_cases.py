"""
Constructed cases for the geometry-driven spatial features (numpy only: no device): the inputs, the
float64 reference a device result is held to, the allowance per cell, the judge, and a float32 model
of the SRP kernels that can carry the seeded faults of test_spatial_cases.py.

REFERENCE.  scripts/sptk/libs/spatial.py of the reference project, in its own operations, on
complex128 copies of exactly what the device receives (the complex64 spectrogram, the complex64
steer vectors, the SRP table as packed and rounded once to complex64, the float32 pair weights):

    phi = np.angle(x)                                       (np.angle(0) = 0; exact at any modulus)
    IPD      np.mod(phi_l - phi_r + pi, 2 pi) - pi          [T][p F + f]
    cosIPD   cos(phi_l - phi_r)                             [T][p F + f]
    cos/sin  [cos, sin](phi_l - phi_r)                      [T][p 2F + f], [T][p 2F + F + f]
    DF       mean_p cos((phi_l - phi_r) - (psi_l - psi_r))  [T][k F + f], psi the phases of steer vector idx[k]
    SRP      sum_p w_p g_p,  g_p = max(s_p / m_p, 0),  m_p = max(max_{t,d} |s_p|, eps32),
             s_p[t][d] = sum_f Re(u_p[t][f] W_p[f][d]),  u_p = exp(i (phi_l - phi_r))

ALLOWANCES, per cell, derived and not measured (PARITY_NOTES_SPATIAL.md), u32 = 2^-24:

    e_u  = K_U u32, K_U = 11            a component of the pair coherence, and its error as a vector
    cosIPD, sinIPD                      e_u
    raw IPD (on the circle)             e_u + ATAN2_ULPS ulp32(pi); and every value in [-pi, pi)
    DF                                  (2 K_U + 2) u32 + (P + 1) u32 mean_p |term_p| + u32 |DF|
    SRP  A_s[p][d] = (2F + 2 + K_U) u32 sum_f (|Re W_fd| + |Im W_fd|)
         A_g       = (A_s[d] + |g| max_d A_s) / m_p + 2 u32 |g|
         A         = sum_p |w_p| A_g,p + (P + 1) u32 sum_p |w_p g_p|

The bar of a cell is min(A, 1e-4): 1e-4 is the flat operator bar of test_gpu_spatial.py, so nothing
is judged more loosely than before.  No cell is left out; where the reference is not finite the
device must be non-finite in exactly the same cells.

SPECTROGRAM FAMILIES, complex64 [C][T][F], seeded by (family, C, T, F): white; coherent (a plane wave
over the linear topology topo(C) from the direction THETA0 plus 1e-3 noise: m_p is close to F);
lattice (small integers with exact zeros, zero frames, one all-zero channel when C >= 3: the phases
0, +-pi/2 and pi exactly, and at cell (0, 0) channels 0 and 1 are -2 and 3: a raw IPD of exactly
+pi, which must come out as -pi); ladder (white scaled per bin by 2^linspace(30, -30, F)); extreme
(the same with 2^linspace(100, -100, F)); nan (white, the real part of one cell of the last channel
a NaN: nan_cell()).  moduli_grid() is a two-channel spectrogram of every float32 magnitude at which
phasor() could change its path, subnormals and the largest float32 included.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***
"""
from dataclasses import dataclass

import numpy as np

import spatial_model as sm

U32 = 2.0 ** -24
EPS32 = float(np.finfo(np.float32).eps)
K_U = 11
ATAN2_ULPS = 6                  # OpenCL C's bound for atan2, which the device math library is built to
ULP_PI = 2.0 ** -22             # the float32 spacing in [2, 4)
BAR = 1e-4                      # the operator bar of test_gpu_spatial.py
PI32 = np.float32(np.pi)
FAMILIES = ("white", "coherent", "lattice", "ladder", "extreme", "nan")
THETA0 = np.pi / 3
SR, SPEED = 16000, 343
KINDS = ("ipd", "cos_ipd", "cos_sin_ipd")


# ------------------------------------------------------------------ inputs
def _cnormal(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def topo(C):
    """A linear topology with unequal spacings (metres)."""
    return tuple(float(v) for v in np.cumsum([0.0] + [0.03 + 0.01 * (k % 3) for k in range(C - 1)]))


def all_pairs(C):
    return [(i, j) for i in range(C) for j in range(i + 1, C)]


def nan_cell(C, T, F):
    """(channel, frame, bin) of the NaN of the `nan` family."""
    return C - 1, T // 2, F // 3


def spectrogram(family, C, T, F):
    """complex64 [C][T][F]"""
    rng = np.random.default_rng([FAMILIES.index(family), C, T, F])
    x = _cnormal(rng, C, T, F)
    if family == "coherent":
        omega = np.linspace(0, SR / 2, F) * 2 * np.pi
        delay = np.cos(THETA0) * np.asarray(topo(C)) / SPEED
        x = np.exp(-1j * delay[:, None, None] * omega[None, None, :]) * _cnormal(rng, 1, T, F) + 1e-3 * x
    elif family == "lattice":
        kind = rng.integers(0, 4, size=(C, T, F))               # 0: zero, 1: real, 2: imaginary, 3: both
        re = rng.integers(-3, 4, size=(C, T, F)) * ((kind == 1) | (kind == 3))
        im = rng.integers(-3, 4, size=(C, T, F)) * ((kind == 2) | (kind == 3))
        x = re + 1j * im
        x[:, rng.uniform(size=T) < 0.2] = 0.0
        x[:, T // 2] = 0.0
        if C >= 3:
            x[C // 2] = 0.0
        x[0, 0, 0], x[1, 0, 0] = -2.0, 3.0
    elif family == "ladder":
        x = x * 2.0 ** np.linspace(30, -30, F)
    elif family == "extreme":
        x = x * 2.0 ** np.linspace(100, -100, F)
    x = x.astype(np.complex64)
    if family == "nan":
        c, t, f = nan_cell(C, T, F)
        x[c, t, f] = complex(np.nan, x[c, t, f].imag)
    return x


def moduli_grid():
    """complex64 [2][N][N]: every combination of real and imaginary parts drawn from zero, the
    smallest and a larger subnormal, the smallest normal, both sides of the moduli at which the
    squares leave float32's normal range (2^-63, 2^64) and of phasor()'s rescaling thresholds
    (2^-62, 2^62), and the largest float32 -- in both signs."""
    pos = [2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -126, 2.0 ** -64, 2.0 ** -63, 1.5 * 2.0 ** -62, 2.0 ** -61, 1.0,
           2.0 ** 61, 1.5 * 2.0 ** 62, 2.0 ** 63, 2.0 ** 64, 2.0 ** 127, float(np.finfo(np.float32).max)]
    v = np.array([0.0] + pos + [-p for p in pos], np.float32)
    x = np.empty((2, len(v), len(v)), np.complex64)
    x[0].real, x[0].imag = v[:, None], v[None, :]
    x[1].real, x[1].imag = np.roll(v, 7)[None, :], v[::-1][:, None]
    return x


def steer(A, C, F):
    """Steer vectors complex64 [A][C][F]: random non-unit moduli, about one in twenty exactly zero."""
    rng = np.random.default_rng([99, A, C, F])
    v = _cnormal(rng, A, C, F) * rng.uniform(0.2, 3.0, size=(A, C, F))
    v[rng.uniform(size=(A, C, F)) < 0.05] = 0.0
    return v.astype(np.complex64)


def dpad(D):
    return (int(D) + 63) & ~63


def pack_table(grids):
    """P grids [F][D] complex128 -> [P][F][dpad(D)] complex64, zero beyond D (libs.spatial.pack_srp_table)."""
    F, D = np.asarray(grids[0]).shape
    table = np.zeros((len(grids), F, dpad(D)), np.complex64)
    for p, g in enumerate(grids):
        table[p, :, :D] = g
    return table


def linear_tables(C, F, D, samp_doa=True):
    """(pairs, table, weights) of srp_phat_linear over topo(C) (libs.spatial.linear_srp_tables)."""
    t = topo(C)
    pairs, w = sm.linear_pairs(C)
    return pairs, pack_table([sm.linear_grid(t[j] - t[i], F, D, samp_doa) for i, j in pairs]), w


# ------------------------------------------------------------------ the reference
def phase(x):
    return np.angle(np.asarray(x).astype(np.complex128))


def _dphi(S, pairs):
    """[P][T][F] phi_l - phi_r"""
    phi = phase(S)
    return np.stack([phi[l] - phi[r] for l, r in pairs])


def ref_ipd(S, pairs, kind):
    """float64 [T][width] in the device's layout; kind one of KINDS."""
    d = _dphi(S, pairs)
    if kind == "ipd":
        return np.hstack(list(np.mod(d + np.pi, 2 * np.pi) - np.pi))
    if kind == "cos_ipd":
        return np.hstack(list(np.cos(d)))
    return np.hstack([np.concatenate((np.cos(v), np.sin(v)), axis=1) for v in d])


def ipd_allowance(kind):
    return K_U * U32 + (ATAN2_ULPS * ULP_PI if kind == "ipd" else 0.0)


def ref_df(S, sv, idx, pairs):
    """(DF [T][len(idx) F], its allowance): S [C][T][F], sv [A][C][F], idx the directions."""
    S = np.asarray(S)
    T, F = S.shape[1:]
    ds = _dphi(S, pairs)                                        # [P][T][F]
    psi = phase(sv)
    out, A = np.empty((T, len(idx), F)), np.empty((T, len(idx), F))
    for k, a in enumerate(idx):
        dt = np.stack([psi[a, l] - psi[a, r] for l, r in pairs])  # [P][F]
        terms = np.cos(ds - dt[:, None, :])
        out[:, k] = np.average(terms, axis=0)
        A[:, k] = ((2 * K_U + 2) + (len(pairs) + 1) * np.abs(terms).mean(axis=0) + np.abs(out[:, k])) * U32
    return out.reshape(T, -1), A.reshape(T, -1)


@dataclass
class SrpRef:
    s: np.ndarray               # [P][T][D] the pair spectra
    m: np.ndarray               # [P] max(max |s_p|, eps32)
    g: np.ndarray               # [P][T][D] normalised and floored
    A_g: np.ndarray             # [P][T][D] allowance of g_p

    def combined(self, weights):
        """(sum_p w_p g_p [T][D], its allowance) for float32 weights as the device receives them."""
        w = np.asarray(weights, np.float32).astype(np.float64)
        P = len(w)
        with np.errstate(invalid="ignore"):
            out = np.tensordot(w, self.g, axes=1)
            A = np.tensordot(np.abs(w), self.A_g, axes=1) + \
                (P + 1) * U32 * np.tensordot(np.abs(w), np.abs(self.g), axes=1)
        return out, A


def ref_srp(S, pairs, table, D):
    """S [C][T][F] complex64, table [P][F][dpad(D)] complex64 as the device receives it."""
    W = np.asarray(table).astype(np.complex128)[:, :, :D]       # [P][F][D]
    F = W.shape[1]
    with np.errstate(invalid="ignore"):
        u = np.exp(1j * _dphi(S, pairs))                        # [P][T][F]
        s = np.real(u @ W)                                      # [P][T][D]
        m = np.max(np.maximum(np.abs(s), EPS32), axis=(1, 2))
        g = np.maximum(s / m[:, None, None], 0)
        A_s = (2 * F + 2 + K_U) * U32 * (np.abs(W.real) + np.abs(W.imag)).sum(axis=1)       # [P][D]
        A_g = (A_s[:, None, :] + np.abs(g) * A_s.max(axis=1)[:, None, None]) / m[:, None, None] + 2 * U32 * np.abs(g)
    return SrpRef(s, m, g, A_g)


# ------------------------------------------------------------------ the judge
@dataclass
class Verdict:
    name: str
    worst: float                # the largest error / bar over the cells (inf: a non-finite mismatch)
    where: tuple                # (t, column) of the worst
    cells: int
    failures: list


def judge(name, got, ref, A, circle=False, report=4):
    """got [T][W] float32 as the device stored it, ref float64, A a scalar or [T][W].  Every cell:
    non-finite exactly where the reference is, else |got - ref| (circle: on the circle) <= min(A, BAR)."""
    got = np.asarray(got)
    ref = np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return Verdict(name, np.inf, (-1, -1), 0, [f"{name}: shape {got.shape} against {ref.shape}"])
    g = got.astype(np.float64)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        err = sm.circle_distance(g, ref) if circle else np.abs(g - ref)
        bar = np.minimum(np.broadcast_to(np.asarray(A, np.float64), ref.shape), BAR)
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(fin, ratio, np.where(np.isfinite(g), np.inf, 0.0))  # the non-finite pattern
    ratio = np.where(np.isnan(ratio), np.inf, ratio)                     # a non-finite device cell, a NaN bar
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else (-1, -1)
    bad = np.argwhere(~(ratio <= 1.0))
    fails = [f"{name}: cell (t, col) = ({t}, {c}): got {g[t, c]:.9e}, reference {ref[t, c]:.9e}, error {err[t, c]:.3e}"
             f" > bar {bar[t, c]:.3e} (ratio {ratio[t, c]:.3g}); {len(bad)} of {ratio.size} cells fail"
             for t, c in bad[:report]]
    return Verdict(name, float(ratio[k]) if ratio.size else 0.0, tuple(int(v) for v in k), ratio.size, fails)


def ipd_range(name, got, S=None, pairs=None):
    """Failure lines for a raw IPD outside [-pi, pi) (the circle distance cannot see a missing
    wrap); with S and pairs also for a cell whose exact phase difference is +-pi and which did not
    come out negative."""
    got = np.asarray(got)
    v = got[np.isfinite(got)]
    fails = []
    if v.size and not (v.min() >= -PI32 and v.max() < PI32):
        fails.append(f"{name}: raw IPD outside [-pi, pi): min {v.min()!r}, max {v.max()!r}")
    if S is not None:
        at = ref_ipd(S, pairs, "ipd") == -np.pi
        if at.any() and not (got[at] < 0).all():
            fails.append(f"{name}: {int((got[at] >= 0).sum())} cells of phase difference +-pi did not come out as -pi")
    return fails


def old_bar_sees(got, ref, circle=False):
    """Whether the flat bar of test_gpu_spatial.py, max |got - ref| <= 1e-4 over the whole map, fails."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = sm.circle_distance(g, r) if circle else np.abs(g - r)
    return bool(np.nanmax(err) > BAR)


class Tally:
    """Verdicts of one test: the worst ratio per family and where it occurred, and every failure."""

    def __init__(self, form):
        self.form, self.worst, self.failures, self.count, self.cells = form, {}, [], 0, 0

    def add(self, family, v):
        w = self.worst.setdefault(family, [0.0, "", None])
        if v.worst >= w[0]:
            w[:] = [v.worst, v.name, v.where]
        self.failures += v.failures
        self.count += 1
        self.cells += v.cells
        return v

    def fail(self, lines):
        self.failures += list(lines)

    def overall(self):
        return max(self.worst.values(), key=lambda w: w[0]) if self.worst else [0.0, "", None]

    def report(self):
        for fam, (r, name, where) in sorted(self.worst.items()):
            print(f"[{self.form}] {fam:12s} worst error/allowance {r:.3f} at (t, col) = {where} ({name})")
        r, name, where = self.overall()
        print(f"[{self.form}] {self.count} maps, {self.cells} cells judged; worst error/allowance {r:.3f} "
              f"at {where} ({name})")

    def finish(self):
        self.report()
        assert not self.failures, f"{len(self.failures)} failures:\n" + "\n".join(self.failures[:25])


# ------------------------------------------------------------------ a float32 model of the SRP kernels
def srp_model(S, pairs, table, weights, D, fault=None, at=0, stale=0.0):
    """spatial_srp_pair_kernel and spatial_srp_combine_kernel in float32 on the packed table
    [P][F][dpad(D)] (the bin sums not in the kernel's fused order: a model of the arithmetic, not a
    bit-exact twin).  Returns [T][D] float32.

    fault: one of the seeded faults of test_spatial_cases.py, each confined to pair `at` --
      "drop_bin"     bin F // 2 left out of the contraction
      "tile_norm"    the normaliser taken over the last 32-frame tile instead of the utterance
      "pad_norm"     the normaliser taken over all dpad(D) columns (of a table whose padding is not zero)
      "stale_frame"  the last frame of a partial tile not stored: s_p[T - 1] keeps the value `stale`
      "late_floor"   (every pair) the floor applied after the weighted sum instead of per pair"""
    f32 = np.float32
    table = np.asarray(table, np.complex64)
    T = S.shape[1]
    out = np.zeros((T, D), f32)
    for p, ((l, r), w) in enumerate(zip(pairs, weights)):
        c, s = sm.coherence(S[l], S[r])
        hit = fault is not None and p == at
        if hit and fault == "drop_bin":
            c, s = c.copy(), s.copy()
            c[:, c.shape[1] // 2] = 0
            s[:, s.shape[1] // 2] = 0
        sp = (c @ table[p].real.astype(f32) - s @ table[p].imag.astype(f32)).astype(f32)     # [T][Dpad]
        if hit and fault == "stale_frame":
            sp[T - 1] = f32(stale)
        scope = sp[:, :D]
        if hit and fault == "pad_norm":
            scope = sp
        if hit and fault == "tile_norm":
            scope = sp[32 * ((T - 1) // 32):, :D]
        m = np.maximum(np.max(np.abs(scope)), f32(EPS32)).astype(f32)
        g = (sp[:, :D] / m).astype(f32)
        if fault != "late_floor":
            g = np.maximum(g, f32(0))
        out = (out + f32(w) * g).astype(f32)
    return np.maximum(out, f32(0)) if fault == "late_floor" else out
