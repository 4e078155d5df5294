"""
Constructed covariance families for the per-bin solver (setk_amd/csrc/solve.hip), reference side
only: seeded stacks of F = 256 Hermitian matrices `Q diag(eigs) Q^H` with Haar-random unitary Q,
multiplied by a power-of-two scale, rounded to complex64 and then made exactly Hermitian with an
exactly real diagonal by copying the lower triangle (the triangle pack_covar_kernel reads).  Both
sides of every comparison receive these complex64 arrays; "truth" is always oracle/np_oracle.py
called on them cast to complex128.

`sensitivity` measures how far that truth moves when every stored float32 of the inputs moves by
a uniform [-1/2, +1/2] ulp: a property of the problem and of the reference, never of the kernel.
The GPU tests (tests/test_gpu_solve.py) build their bars from it.
"""
import zlib

import numpy as np
import scipy.linalg

from oracle import np_oracle as o

F = 256
EPS32 = float(np.finfo(np.float32).eps)

GAPS = (0.9, 0.5, 1e-1, 1e-2, 1e-3)
FLOORS = (1e-1, 1e-4)
CONDS = (1e1, 1e2, 1e3, 1e4, 1e5)
CHANNELS = tuple(range(1, 17))
# powers of two, applied to Rs, Rn and Ry together
SCALES = (2.0 ** -40, 2.0 ** -24, 1.0, 2.0 ** 30)
# 2^+-80: only for the plain eigenvector, the pencil vector, MVDR and GEVD without BAN.  Left out
# for BAN (w^H Rn Rn w is of order scale^2 = 2^+-160, which the reference's own complex64 einsum
# cannot hold: float32 ends at 2^128 / 2^-149) and for PMWF and MPDR-whiten with the rank-1
# rebuild or the SNR search, whose |Rn v|^2 and w^H Rn w are products of the same order.
SCALES_WIDE = (2.0 ** -80, 2.0 ** 80)
SCALE_CHANNELS = (3, 4, 7, 8, 9, 12, 15, 16)


def rel_rms(a, ref):
    a = np.asarray(a, dtype=np.complex128)
    ref = np.asarray(ref, dtype=np.complex128)
    return float(np.sqrt(np.mean(np.abs(a - ref) ** 2)) / max(np.sqrt(np.mean(np.abs(ref) ** 2)), 1e-300))


def seed_of(*key):
    """A reproducible 32-bit seed from the family's name and parameters."""
    return zlib.crc32(repr(key).encode())


def haar_unitary(rng, n, C):
    """n Haar-distributed C x C unitaries (QR of a complex Ginibre matrix, phases of R's diagonal
    moved into Q)."""
    A = rng.standard_normal((n, C, C)) + 1j * rng.standard_normal((n, C, C))
    Q, R = np.linalg.qr(A)
    d = np.diagonal(R, axis1=1, axis2=2)
    return Q * (d / np.abs(d))[:, None, :]


def make_hermitian(M):
    """complex64, the lower triangle mirrored, the diagonal exactly real"""
    M = np.asarray(M).astype(np.complex64)
    L = np.tril(M)
    M = L + np.conj(np.transpose(np.tril(M, -1), (0, 2, 1)))
    i = np.arange(M.shape[-1])
    M[:, i, i] = M[:, i, i].real
    return np.ascontiguousarray(M)


def from_spectrum(rng, C, eigs, scale=1.0, real=False, n=F):
    eigs = np.asarray(eigs, dtype=np.float64)
    if real:
        Q, R = np.linalg.qr(rng.standard_normal((n, C, C)))
        Q = Q * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]
    else:
        Q = haar_unitary(rng, n, C)
    M = (Q * eigs[None, None, :]) @ np.conj(np.transpose(Q, (0, 2, 1)))
    return make_hermitian(M * scale)


def spectrum_gap(C, gap, floor):
    """1, 1 - gap, then a geometric tail down to `floor` (never above 1 - gap)"""
    if C == 1:
        return np.array([1.0])
    if C == 2:
        return np.array([1.0, 1.0 - gap])
    return np.concatenate([[1.0], np.geomspace(1.0 - gap, min(floor, 1.0 - gap), C - 1)])


def spectrum_cond(C, cond):
    return np.geomspace(1.0, 1.0 / cond, C) if C > 1 else np.array([1.0])


# ---- the families --------------------------------------------------------------------------
def rs_gap(C, gap, floor, scale=1.0):
    rng = np.random.default_rng(seed_of("rs_gap", C, gap, floor))
    return from_spectrum(rng, C, spectrum_gap(C, gap, floor), scale)


def rs_rank1(C, scale=1.0):
    """exactly rank 1 before rounding: a a^H with |a| = 1"""
    rng = np.random.default_rng(seed_of("rs_rank1", C))
    return from_spectrum(rng, C, np.concatenate([[1.0], np.zeros(C - 1)]), scale)


def rs_diagonal(C, scale=1.0):
    """exactly diagonal; the largest entry sits at position f % C of matrix f, the others are
    distinct values in [0.05, 0.5]"""
    rng = np.random.default_rng(seed_of("rs_diagonal", C))
    d = rng.uniform(0.05, 0.5, size=(F, C))
    d[np.arange(F), np.arange(F) % C] = 1.0
    M = np.zeros((F, C, C), np.complex64)
    i = np.arange(C)
    M[:, i, i] = (d * scale).astype(np.float32)
    return M


def rs_real(C, scale=1.0):
    """real symmetric (imaginary parts exactly 0), gap 0.5, floor 1e-1"""
    rng = np.random.default_rng(seed_of("rs_real", C))
    M = from_spectrum(rng, C, spectrum_gap(C, 0.5, 1e-1), scale, real=True)
    assert not M.imag.any()
    return M


def rs_identity(C, scale=1.0):
    M = np.zeros((F, C, C), np.complex64)
    i = np.arange(C)
    M[:, i, i] = np.float32(scale)
    return M


def rs_zero(C):
    return np.zeros((F, C, C), np.complex64)


def rn_cond(C, cond, scale=1.0, tag="rn"):
    rng = np.random.default_rng(seed_of(tag, C, cond))
    return from_spectrum(rng, C, spectrum_cond(C, cond), scale)


def ry_cond(C, cond, scale=1.0):
    return rn_cond(C, cond, scale, tag="ry")


def achieved_gap(M):
    """relative gap (lambda_1 - lambda_2) / lambda_1 of every matrix, in float64"""
    ev = np.linalg.eigvalsh(M.astype(np.complex128))
    return (ev[:, -1] - ev[:, -2]) / ev[:, -1]


def achieved_cond(M):
    ev = np.linalg.eigvalsh(M.astype(np.complex128))
    return ev[:, -1] / ev[:, 0]


# ---- the probe -----------------------------------------------------------------------------
def perturb(rng, M):
    """every stored float32 moved by a uniform [-1/2, +1/2] ulp relative amount, kept Hermitian
    (lower triangle mirrored); complex128 out"""
    d = 1 + EPS32 * rng.uniform(-0.5, 0.5, size=M.shape)
    e = 1 + EPS32 * rng.uniform(-0.5, 0.5, size=M.shape)
    P = (M.real.astype(np.float64) * d + 1j * M.imag.astype(np.float64) * e)
    P = np.tril(P) + np.conj(np.transpose(np.tril(P, -1), (0, 2, 1)))
    return P


def sensitivity(fn, mats, rng, draws=2):
    """Relative RMS (over the family, in the gauge fn declares) by which fn's complex128 answer
    moves under `perturb` of every input; mean over `draws`.  mats: tuple of complex64 stacks
    (None entries pass through)."""
    c128 = [None if m is None else m.astype(np.complex128) for m in mats]
    truth = fn(*c128)
    moved = []
    for _ in range(draws):
        moved.append(rel_rms(fn(*[None if m is None else perturb(rng, m) for m in mats]), truth))
    return float(np.mean(moved)), truth


# ---- the operations, as the oracle states them (declared gauge) ------------------------------
def op_pevd(Rs):
    return o.solve_pevd(Rs, gauge=True)


def op_pencil(Rs, Rn):
    return o.solve_pevd(Rs, Rn, gauge=True)


def pmwf_snr(Rs, Rn, beta=0, rank1_appro=""):
    """The per-channel SNR estimates of pmwf_weight's reference-channel search (np_oracle.py,
    libs/beamformer.py:620-630), which the oracle does not return."""
    if rank1_appro == "eig":
        Rs = o.rank1_constraint(Rs, gauge=False)
    if rank1_appro == "gev":
        Rs = o.rank1_constraint(Rs, Rn=Rn, gauge=False)
    num = np.linalg.solve(Rn, Rs)
    den = beta + np.trace(num, axis1=1, axis2=2)
    wmat = num / den[..., None, None]
    snr = []
    for c in range(Rs.shape[1]):
        w = wmat[..., c]
        ps = np.einsum("...fa,...fab,...fb->...", np.conj(w), Rs, w)
        pn = np.einsum("...fa,...fab,...fb->...", np.conj(w), Rn, w)
        snr.append(np.real(ps) / np.maximum(o.EPSILON, np.real(pn)))
    return np.asarray(snr)


# name -> (needs, oracle function of (Rs, Rn, Ry) in complex128, C ABI options, inherits the plain
# eigenvector of Rs).  `needs` names the inputs the sensitivity probe perturbs.
def weight_kinds(C):
    last = C - 1
    return {
        "mvdr": ("sn", lambda Rs, Rn, Ry: o.mvdr_weight(Rs, Rn, gauge=True), dict(kind="MVDR"), True),
        "gevd": ("sn", lambda Rs, Rn, Ry: o.gevd_weight(Rs, Rn, gauge=True), dict(kind="GEVD"), False),
        "pmwf_search": ("sn", lambda Rs, Rn, Ry: o.pmwf_weight(Rs, Rn, beta=0),
                        dict(kind="PMWF", pmwf_ref=-1), False),
        "pmwf_last_beta1": ("sn", lambda Rs, Rn, Ry: o.pmwf_weight(Rs, Rn, beta=1, ref_channel=last),
                            dict(kind="PMWF", pmwf_ref=last, pmwf_beta=1.0), False),
        "pmwf_r1eig": ("sn", lambda Rs, Rn, Ry: o.pmwf_weight(Rs, Rn, beta=0, ref_channel=0, rank1_appro="eig"),
                       dict(kind="PMWF", pmwf_ref=0, rank1="EIG"), True),
        "pmwf_r1gev": ("sn", lambda Rs, Rn, Ry: o.pmwf_weight(Rs, Rn, beta=0, ref_channel=0, rank1_appro="gev"),
                       dict(kind="PMWF", pmwf_ref=0, rank1="GEV"), False),
        "mpdr": ("sy", lambda Rs, Rn, Ry: o.mpdr_weight(Rs, Ry, gauge=True), dict(kind="MPDR"), True),
        "mpdr_whiten": ("sny", lambda Rs, Rn, Ry: o.mpdr_weight(Rs, Ry, Rn=Rn, gauge=True),
                        dict(kind="MPDR_WHITEN"), False),
    }


def with_ban(fn):
    return lambda Rs, Rn, Ry: o.do_ban(fn(Rs, Rn, Ry), Rn)


def pencil_rho(Rs, Rn):
    """largest eigenvalue of every pencil (Rs, Rn), complex128, from scipy"""
    Rs = Rs.astype(np.complex128)
    Rn = Rn.astype(np.complex128)
    return np.array([scipy.linalg.eigh(Rs[f], Rn[f], eigvals_only=True)[-1] for f in range(Rs.shape[0])])


# ---- the pairs of families the pencil and the weights are tested on ---------------------------
# (Rs gap, Rs floor, cond of Rn and Ry): every cond at a clear gap, every gap at a moderate cond
# (3e2 is there for PMWF with the rank-1 eigenvector rebuild, see `capped`)
PAIRS = tuple([(0.5, 1e-1, c) for c in sorted(CONDS + (3e2,))] + [(g, 1e-4, 1e2) for g in GAPS])
CAP_VEC, CAP_WEIGHT = 1e-4, 2e-4   # the bars of test_covar_pevd_weights, never exceeded where well posed


def well_posed(gap, cond=1.0):
    return gap >= 1e-1 and cond <= 1e3


def capped(name, gap, cond=1.0):
    """Is this family's bar capped at the project's existing one?  The well-posed families; for
    pmwf_r1eig the cond 1e3 family is replaced by cond 3e2 (its sensitivity at 1e3 is 3.3e-6 at
    6 and 7 channels and 8 eps32 + 64 s = 2.1e-4 passes the cap of 2e-4:
    tests/test_solve_cases.py checks the condition for every family that stays)."""
    return well_posed(gap, cond) and not (name == "pmwf_r1eig" and cond > 3e2)


def bar(s, margin, name, gap, cond=1.0, cap=CAP_WEIGHT):
    """8 eps32 + margin * s, capped at the project's existing bar on the well-posed families"""
    b = 8 * EPS32 + margin * s
    return min(b, cap) if capped(name, gap, cond) else b


class Case:
    """One (C, pair, scale): the complex64 inputs, and the oracle's complex128 answers on them
    and on `draws` perturbed copies.  The pencil's eigenvectors (the scipy loop, the slow part)
    are computed once per set of inputs and shared by every kind that asks the oracle for them."""

    def __init__(self, C, gap, floor, cond, scale=1.0, draws=2):
        self.C, self.gap, self.floor, self.cond, self.scale = C, gap, floor, cond, scale
        self.Rs = rs_gap(C, gap, floor, scale)
        self.Rn = rn_cond(C, cond, scale)
        self.Ry = ry_cond(C, cond, scale)
        rng = np.random.default_rng(seed_of("probe", C, gap, floor, cond, scale))
        self.inputs = [tuple(m.astype(np.complex128) for m in (self.Rs, self.Rn, self.Ry))]
        for _ in range(draws):
            self.inputs.append(tuple(perturb(rng, m) for m in (self.Rs, self.Rn, self.Ry)))
        self._pencil = {}
        self._out = {}

    def _solve_pevd(self, orig):
        def wrapped(Rs, Rn=None, gauge=False):
            if Rn is None:
                return orig(Rs, gauge=gauge)
            key = (id(Rs), id(Rn))
            if key not in self._pencil:
                self._pencil[key] = (orig(Rs, Rn, gauge=False), Rs, Rn)
            raw = self._pencil[key][0]
            return o.fix_gauge_gev(raw, Rn) if gauge else raw
        return wrapped

    def outputs(self, name, fn):
        """fn(Rs, Rn, Ry) on the unperturbed inputs and on every perturbed copy"""
        if name not in self._out:
            orig = o.solve_pevd
            o.solve_pevd = self._solve_pevd(orig)
            try:
                self._out[name] = [fn(*m) for m in self.inputs]
            finally:
                o.solve_pevd = orig
        return self._out[name]

    def truth_and_s(self, name, fn, ban=False):
        """(complex128 oracle answer, its sensitivity); with ban, do_ban applied with each copy's
        own Rn"""
        outs = self.outputs(name, fn)
        if ban:
            key = name + "+ban"
            if key not in self._out:
                self._out[key] = [o.do_ban(w, m[1]) for w, m in zip(outs, self.inputs)]
            outs = self._out[key]
        return outs[0], float(np.mean([rel_rms(x, outs[0]) for x in outs[1:]]))
