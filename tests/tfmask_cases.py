"""Cases, float64 reference and the one judging helper for the TF-mask suites
(test_tfmask_cases.py on the CPU, test_gpu_tfmask.py on the device, tools/make_golden_tfmask.py).

Reference: the formulas of compute_mask.py:59-107 / :136-152 and oracle_separate.py:19-45 restated
dtype-generically (mask_formula, oracle_formula).  On complex128 spectra of stft_cases.ref_stft they
are the float64 reference; on those spectra rounded to complex64 they are the reference's own
float32 arithmetic -- the yardstick.  tools/make_golden_tfmask.py holds the restatement to the
unmodified reference functions bit for bit and stores the reference's outputs in
tests/golden/ref_tfmask.npz.

Measure (judge_mask): per cell.  The forward transform promises a frame ||dX_t||_2 <= a_t, a_t =
m max(||X32_t - X_t||, 2^-24 ||X_t||), m = 4, floor 0 (PARITY_NOTES_STFT.md); a bin answers to its
frame, so |dX[t, k]| <= a_t too.  A mask cell n / d gets (a_n + g a_d) / d + c 2^-24 |out|, g the
magnitude the denominator's error is scaled by:
    irm    n = |tgt|, d = sqrt(|tgt|^2 + |inf|^2 + eps): a_n = a_tgt, a_d = a_tgt + a_inf (both partial
           derivatives of d are at most 1), a_inf = a_mix + a_tgt, g = |mask|
    iam    n = |tgt|, d = |mix|: a_n = a_tgt, a_d = a_mix, g = |mask|
    psm    = Re(tgt / mix): (a_tgt + g a_mix) / |mix| with g = |tgt| / |mix| (>= |mask|: the whole
           quotient moves with the denominator, not its real part alone)
    psa    = max(0, Re(tgt conj(mix / |mix|))): a_tgt + |tgt| a_mix / |mix|  (a scaled by the other factor)
    crm    q = tgt / (mix + eps): (a_tgt + |q| a_mix) / |mix + eps| through the tangent's slope (at most
           K C / 2 = 1 / 2), and the rounding term on |out| + slope(x) |q| + K / 2 (a part of q is a
           difference of products as large as |q|; the reference forms 1 - e^{-C x} by subtraction
           from 1, an ABSOLUTE error of 2^-24 that K / (1 + e) carries into a small output whole)
    oracle irm: d = sum_j |tgt_j| + eps, a_d = sum_j a_j; iam / psm: d = |mix| + eps as above
c (C_ROUND) is not typed in advance: make_golden_tfmask.py --check prints the smallest integer that
covers the yardstick on every case, and C_ROUND is that times m = 4 for another operation order
(tests/PARITY_NOTES_TFMASK.md).

Cells left out are conditions on the REFERENCE, not measurements of the result: a ratio cell with
d < 10^-2 S_t (S_t the frame RMS of the mixture spectrum) has no first-order bound -- at most 1 % of
a case, asserted; an ibm cell with | |tgt| - |inf| | <= 10^-4 S_t (the gap of the two largest
targets for the argmax) may fall either way -- at most 0.5 %, asserted, and outside the band not
one cell may differ.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import stft_cases as sc  # noqa: E402

KINDS = ("ibm", "irm", "iam", "psm", "psa", "crm")
ORACLE_KINDS = ("ibm", "irm", "iam", "psm")
CUTOFFS = (-1.0, 2.0)
EPS32 = float(np.finfo(np.float32).eps)
M_BITS = sc.M_BITS
U32 = sc.U32
C_ROUND = 8                 # = M_BITS x 2, the yardstick's 2 (make_golden_tfmask.py --check; PARITY_NOTES_TFMASK.md)
D_MIN = 1e-2                # ratio cells below D_MIN S_t are left out ...
D_CAP = 0.01                # ... at most this share of a case
IBM_BAND = 1e-4             # ibm cells inside the band may fall either way ...
IBM_CAP = 0.005             # ... at most this share of a case
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_tfmask.npz")


# ------------------------------------------------------------------ the formulas, dtype-generic
def _abs(z):
    return np.sqrt(z.real ** 2 + z.imag ** 2)


def _squash(x, K=10, C=0.1):
    out = np.empty_like(x)
    pos = x >= 0
    e = np.exp(-C * x[pos])
    out[pos] = K * (1 - e) / (1 + e)
    e = np.exp(C * x[~pos])
    out[~pos] = K * (e - 1) / (e + 1)
    return out


def mask_formula(kind, tgt, mix):
    """compute_mask.py:77-107 in the dtype of the spectra (complex64: the reference's arithmetic)."""
    real = np.float32 if tgt.dtype == np.complex64 else np.float64
    eps = real(EPS32)
    with np.errstate(all="ignore"):
        ta, ma, ia = _abs(tgt), _abs(mix), _abs(mix - tgt)
        if kind == "ibm":
            return (ta > ia).astype(np.float32)
        if kind == "irm":
            return ta / np.sqrt(ta ** 2 + ia ** 2 + eps)
        if kind == "iam":
            return ta / ma
        if kind == "crm":
            q = tgt / (mix + eps)
            return np.hstack([_squash(np.real(q)), _squash(np.imag(q))])
        c = np.cos(np.angle(mix) - np.angle(tgt))
        if kind == "psm":
            return ta * c / ma
        assert kind == "psa"
        return ta * np.maximum(0, c)


def clip_formula(mask, cutoff):
    """run() :136-152: the mask written and the three numbers logged."""
    with np.errstate(all="ignore"):
        over = 0
        if cutoff > 0:
            over = int(np.sum(mask > cutoff))
            mask = np.minimum(mask, mask.dtype.type(cutoff))
        neg = mask < 0
        below = int(np.sum(neg))
        below_sum = float(mask[neg].astype(np.float64).sum())
        return np.maximum(mask, 0), (over, below, below_sum)


def oracle_formula(kind, mix, targets):
    """oracle_separate.py:19-45."""
    real = np.float32 if mix.dtype == np.complex64 else np.float64
    eps = real(EPS32)
    with np.errstate(all="ignore"):
        tas = [_abs(t) for t in targets]
        if kind == "ibm":
            idx = np.argmax(np.stack(tas), 0)
            return [(idx == k) for k in range(len(targets))]
        den = (sum(tas) if kind == "irm" else _abs(mix)) + eps
        if kind != "psm":
            return [ta / den for ta in tas]
        ph = np.angle(mix)
        return [ta * np.cos(ph - np.angle(t)) / den for ta, t in zip(tas, targets)]


# ------------------------------------------------------------------ signals
def coloured(rng, n):
    """Envelope-modulated coloured noise, peak about 0.5."""
    w = rng.standard_normal(n + 64)
    k = np.array([1.0, 0.9, 0.55, 0.2, -0.1, -0.15, 0.05])
    x = np.convolve(w, k, mode="full")[32:32 + n]
    env = 0.55 + 0.45 * np.sin(2 * np.pi * (np.arange(n) / (900.0 + 400.0 * rng.random()) + rng.random()))
    x = x * env
    return 0.5 * x / np.abs(x).max()


class Pair:
    """A target (or K targets) and the mixture, float32 samples (int16 twins where given)."""

    def __init__(self, name, targets, mix, geo, pcm=None):
        self.name, self.geo = name, geo
        self.targets = [np.ascontiguousarray(t, np.float32) for t in targets]
        self.mix = np.ascontiguousarray(mix, np.float32)
        self.pcm = pcm              # (targets int16, mix int16) with x == pcm / 32768 exactly, or None
        self.judged = True
        self._cache = {}

    @property
    def tgt(self):
        return self.targets[0]

    @property
    def T(self):
        return self.geo.num_frames(self.mix.shape[0])

    def spectra(self, dtype=np.complex128):
        """(targets, mix): float64 reference spectra of the float32 samples, or their rounding."""
        if "X" not in self._cache:
            self._cache["X"] = ([sc.ref_stft(t, self.geo) for t in self.targets], sc.ref_stft(self.mix, self.geo))
        ts, m = self._cache["X"]
        if dtype == np.complex128:
            return ts, m
        return [t.astype(dtype) for t in ts], m.astype(dtype)

    def promises(self):
        """a_t of every target and of the mixture: m max(||X32_t - X_t||, 2^-24 ||X_t||), [T] each."""
        if "a" not in self._cache:
            ts, m = self.spectra()

            def a_of(x, X):
                y = sc.f32_stft(x, self.geo)
                return M_BITS * np.maximum(np.linalg.norm(y - X, axis=1), U32 * np.linalg.norm(X, axis=1))
            self._cache["a"] = ([a_of(x, X) for x, X in zip(self.targets, ts)], a_of(self.mix, m))
        return self._cache["a"]


def _mixture(parts):
    return (parts[0] + 0.7 * sum(parts[1:])).astype(np.float32)


NOISE_SIZES = ((512, False), (1000, True), (4133, False), (16000, True))


def noise_pairs(K=2, sizes=NOISE_SIZES, seed=20250117):
    """A target plus 0.7 x the interferer (K > 2: 0.7 shared among the K - 1 interferers): with
    K = 2 the pair (target, mixture) of the mask tests; the K parts are the oracle targets and sum to
    the mixture."""
    out = []
    for n, center in sizes:
        rng = np.random.default_rng(seed + n)
        parts = [coloured(rng, n) for _ in range(K)]
        # on the 16-bit grid, so that every pair has its int16 twin (peaks 0.5 and 0.35 / (K - 1))
        pcm = [np.rint(32768 * g * p).astype(np.int16)
               for g, p in zip([1.0] + [0.7 / max(1, K - 1)] * (K - 1), parts)]
        mix = np.sum(np.stack(pcm).astype(np.int64), axis=0)
        assert np.abs(mix).max() < 32768
        mix = mix.astype(np.int16)
        out.append(Pair(f"noise{n}{'c' if center else 'u'}/K{K}", [p.astype(np.float32) / np.float32(32768) for p in pcm],
                        mix.astype(np.float32) / np.float32(32768), sc.Geom(center=center), pcm=(pcm, mix)))
    return out


ORACLE_SEED = 20250118      # the first seed from 20250117 whose argmax band is empty on all three pairs


def oracle_pairs():
    """K = 2 and 3 on the 4133-sample case, K = 8 on the 1000-sample case.  The seed is one for
    which no cell lies in the argmax band, so that the ibm WAVES have one reference
    (tools/make_golden_tfmask.py asserts it)."""
    return [noise_pairs(2, ((4133, False),), ORACLE_SEED)[0], noise_pairs(3, ((4133, False),), ORACLE_SEED)[0],
            noise_pairs(8, ((1000, True),), ORACLE_SEED)[0]]


def ibm_band_cells(pair):
    """Cells whose two largest targets lie within the band."""
    ts, m = pair.spectra()
    top = np.sort(np.stack([_abs(t) for t in ts]), axis=0)
    return int(((top[-1] - top[-2]) <= IBM_BAND * _frame_rms(m)).sum())


def oracle_wave_extra(kind, pair, k, mask):
    """The 2-norm bound per frame of |mix| x (the error of mask k) behind the forward's promises:
    |mix| / d <= 1 for every kind (irm: the triangle inequality), so it is a_n + max_f g a_d of
    mask_allowance; an ibm mask outside the band is exact."""
    a_ts, a_m = pair.promises()
    if kind == "ibm":
        return np.zeros_like(a_m)
    g = np.abs(mask).max(axis=1)
    if kind == "irm":
        return a_ts[k] + g * sum(a_ts)
    if kind == "psm":
        ts, m = pair.spectra()
        g = (_abs(ts[k]) / (_abs(m) + EPS32)).max(axis=1)
    return a_ts[k] + g * a_m


def _stft_case(family, name):
    return [c for c in sc.signal_cases(families=(family,)) if c.name == name][0]


def zeros_pairs():
    """Silent stretches (three leading, two trailing frames of stft_cases' `zeros`) in the target
    only, in the mixture only and in both; 16-bit twins."""
    burst = _stft_case("zeros", "burst").pcm.astype(np.int64)
    n = burst.shape[0]
    rng = np.random.default_rng(4711)
    noise = rng.integers(-9000, 9001, n)
    lo = np.flatnonzero(burst)[0]
    hi = np.flatnonzero(burst)[-1]
    gated = np.zeros(n, np.int64)
    gated[lo:hi + 1] = rng.integers(-9000, 9001, hi + 1 - lo)
    out = []
    for name, t, m in (("target", burst, burst + noise), ("mixture", noise, burst), ("both", burst, burst + gated)):
        t = np.clip(t, -32768, 32767).astype(np.int16)
        m = np.clip(m, -32768, 32767).astype(np.int16)
        out.append(Pair(f"zeros:{name}", [t.astype(np.float32) / np.float32(32768)],
                        m.astype(np.float32) / np.float32(32768), sc.Geom(), pcm=([t], m)))
    return out


def pcm_pairs():
    """stft_cases' 16-bit extremes as targets, the mixture a few LSB of dither away."""
    rng = np.random.default_rng(515)
    out = []
    for c in sc.signal_cases(families=("pcm",)):
        t = c.pcm.astype(np.int64)
        m = np.clip(t + rng.integers(-3, 4, t.shape[0]), -32768, 32767).astype(np.int16)
        p = Pair(f"pcm:{c.name}", [c.x], m.astype(np.float32) / np.float32(32768), sc.Geom(), pcm=([c.pcm], m))
        # the alternation is ONE spectral line: 99 % of its cells lie below the floor D_MIN S_t, no
        # cap holds there.  It stays for what the family is about -- 16-bit input against its float32
        # twin, bit for bit -- and is not judged per cell.
        p.judged = not c.name.startswith("alt")
        out.append(p)
    return out


def quiet_pairs():
    c = _stft_case("quiet", "2^-16")
    rng = np.random.default_rng(616)
    other = sc._at_peak(sc._noise(rng, c.x.shape[0]), 2.0 ** -16)
    return [Pair("quiet:2^-16", [c.x], (c.x.astype(np.float64) + 0.7 * other).astype(np.float32), sc.Geom())]


def other_size_pairs():
    """The operator path: frame_len 400 in n_fft 512, and n_fft 256."""
    out = []
    for geo in (sc.Geom(n_fft=512, hop=160, frame_len=400, center=True), sc.Geom(n_fft=256, hop=128, center=True)):
        rng = np.random.default_rng(99 + geo.n_fft)
        parts = [coloured(rng, 3000).astype(np.float32), (0.7 * coloured(rng, 3000)).astype(np.float32)]
        mix = (parts[0].astype(np.float64) + parts[1]).astype(np.float32)
        out.append(Pair(f"other:{geo!r}", parts, mix, geo))
    return out


def mask_pairs():
    return noise_pairs() + zeros_pairs() + pcm_pairs() + quiet_pairs()


# ------------------------------------------------------------------ the helper
class MaskVerdict:
    def __init__(self, name):
        self.name, self.failures = name, []
        self.worst, self.left_out, self.cells = 0.0, 0.0, 0

    @property
    def ok(self):
        return not self.failures

    def line(self):
        return (f"{self.name}: worst cell {self.worst:.3f} of its allowance, {100 * self.left_out:.3f} % of "
                f"{self.cells} cells left out")


def _frame_rms(X):
    return np.linalg.norm(X, axis=1)[:, None] / np.sqrt(X.shape[1])


def mask_allowance(kind, pair, k=0, oracle=False):
    """(ref, base, unit, skip) per cell: the float64 reference mask (unclipped), the first-order
    part of the allowance, what the rounding term c 2^-24 multiplies, and the cells left out.  A
    frame whose mixture is exactly silent has S_t = 0 and no cell left out: there the operands are
    exact and so is the result."""
    ts, m = pair.spectra()
    a_ts, a_m = pair.promises()
    a_m = a_m[:, None]
    S = _frame_rms(m)
    with np.errstate(all="ignore"):
        ta, ma = _abs(ts[k]), _abs(m)
        a_t = a_ts[k][:, None]

        def over(x, d):                      # x / d where d > 0, else 0 (x is 0 there: a silent frame)
            return np.where(d > 0, x / np.where(d > 0, d, 1), 0.0)
        if oracle:
            ref = np.asarray(oracle_formula(kind, m, ts)[k], np.float64)
            tas = np.stack([_abs(t) for t in ts])
            if kind == "ibm":
                top = np.sort(tas, axis=0)
                return ref, np.zeros_like(ref), np.zeros_like(ref), ((top[-1] - top[-2]) <= IBM_BAND * S) & (S > 0)
            if kind == "irm":
                d = tas.sum(0) + EPS32
                a_d = sum(a[:, None] for a in a_ts)
                base = (a_t + np.abs(ref) * a_d) / d
            else:
                d = ma + EPS32
                g = np.abs(ref) if kind == "iam" else ta / d
                base = (a_t + g * a_m) / d
            return ref, base, np.abs(ref), d < D_MIN * S
        ref = np.asarray(mask_formula(kind, ts[k], m), np.float64)
        ia = _abs(m - ts[k])
        a_i = a_m + a_t
        if kind == "ibm":
            return ref, np.zeros_like(ref), np.zeros_like(ref), (np.abs(ta - ia) <= IBM_BAND * S) & (S > 0)
        if kind == "irm":
            d = np.sqrt(ta ** 2 + ia ** 2 + EPS32)
            return ref, (a_t + np.abs(ref) * (a_t + a_i)) / d, np.abs(ref), d < D_MIN * S
        if kind == "iam":
            return ref, over(a_t + over(ta, ma) * a_m, ma), np.abs(ref), ma < D_MIN * S
        if kind == "psm":
            return ref, over(a_t + over(ta, ma) * a_m, ma), np.abs(ref), ma < D_MIN * S
        if kind == "psa":
            return ref, a_t + over(ta * a_m, ma), np.abs(ref), ma < D_MIN * S
        assert kind == "crm"
        den = m + EPS32
        q = ts[k] / den
        dq = (a_t + np.abs(q) * a_m) / np.abs(den)

        def slope(x):
            return 0.5 / np.cosh(np.minimum(np.abs(0.05 * x), 300.0)) ** 2
        skip = np.abs(den) < D_MIN * S
        return (ref, np.hstack([slope(q.real) * dq, slope(q.imag) * dq]),
                np.hstack([np.abs(_squash(q.real)) + slope(q.real) * np.abs(q) + 5.0,
                           np.abs(_squash(q.imag)) + slope(q.imag) * np.abs(q) + 5.0]), np.hstack([skip, skip]))


def judge_mask(name, kind, got, pair, cutoff=-1.0, c_round=C_ROUND, k=0, oracle=False):
    """One clipped mask (the device's, or the clipped yardstick) against the float64 reference, per
    cell.  The clips are applied to the reference as the tool applies them; they only shrink an
    error.  v.need is the smallest c that would have covered the result."""
    v = MaskVerdict(name)
    ref, base, unit, skip = mask_allowance(kind, pair, k=k, oracle=oracle)
    if not oracle:
        ref = clip_formula(ref, cutoff)[0]
    got = np.asarray(got, np.float64)
    v.need = 0
    if got.shape != ref.shape:
        v.failures.append(f"{name}: shape {got.shape} against {ref.shape}")
        return v
    v.cells = ref.size
    special = ~np.isfinite(ref)
    # NaN / +-inf sit on exactly the reference's cells
    if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)) and
            np.array_equal(np.isneginf(got), np.isneginf(ref))):
        v.failures.append(f"{name}: NaN / inf on other cells than the reference's "
                          f"({int(np.isnan(got).sum())} / {int(np.isnan(ref).sum())} NaN, "
                          f"{int(np.isinf(got).sum())} / {int(np.isinf(ref).sum())} inf)")
        return v
    skip = skip & ~special
    v.left_out = float(skip.mean())
    cap = IBM_CAP if kind == "ibm" else D_CAP
    if v.left_out > cap:
        v.failures.append(f"{name}: {100 * v.left_out:.3f} % of the cells left out, the cap is {100 * cap} %")
    live = ~skip & ~special
    with np.errstate(all="ignore"):
        err = np.where(live, np.abs(got - ref), 0.0)
        base = np.where(live, np.nan_to_num(base, nan=0.0, posinf=0.0), 0.0)
        unit = np.where(live, np.nan_to_num(unit, nan=0.0, posinf=0.0), 0.0)
        allow = base + c_round * U32 * unit
        excess = err - base
        need = np.where((excess > 0) & (unit > 0), excess / np.where(unit > 0, U32 * unit, 1), 0.0)
        hopeless = (excess > 0) & (unit == 0)
    v.need = int(np.ceil(need.max())) if need.size else 0
    if hopeless.any():
        v.need = None
    bad = live & ~(err <= allow)
    ratio = np.where(allow > 0, err / np.where(allow > 0, allow, 1), 0.0)
    v.worst = float(ratio.max()) if ratio.size else 0.0
    if bad.any():
        t, f = np.argwhere(bad)[0]
        v.failures.append(f"{name}: {int(bad.sum())} cells outside their allowance, first ({t}, {f}): "
                          f"{got[t, f]!r} against {ref[t, f]!r}, allowance {allow[t, f]:.3e}")
    return v


def yardstick_mask(kind, pair, cutoff=-1.0, k=0, oracle=False):
    """The reference's own float32 arithmetic on the float64 spectra rounded to complex64."""
    ts32, m32 = pair.spectra(np.complex64)
    if oracle:
        return np.asarray(oracle_formula(kind, m32, ts32)[k])
    return clip_formula(mask_formula(kind, ts32[k], m32), cutoff)[0]


def smallest_c(kind, pair, oracle=False):
    """The smallest integer c whose rounding term covers the float32 yardstick on this pair (None:
    no c does, or a cap is exceeded)."""
    worst = 0
    for k in range(len(pair.targets) if oracle else 1):
        for cutoff in ((-1.0,) if oracle else CUTOFFS):
            v = judge_mask("yardstick", kind, yardstick_mask(kind, pair, cutoff, k, oracle), pair, cutoff,
                           c_round=1 << 30, k=k, oracle=oracle)
            if not v.ok or v.need is None:
                return None
            worst = max(worst, v.need)
    return worst


# ------------------------------------------------------------------ waves
def wave_reference(pair, masks, geo=None, phase_ref=None, nsamps=None, norm=None, a_mask=None):
    """inverse_stft(mix x mask) (or |mix| x mask x exp(i angle(ref))) in float64, the same in
    float32, and the input-referred allowance per block of hop samples: the forward's promise
    through max_f |mask| of the frame (plus a_mask, the 2-norm bound of |mix| x the mask's own
    error, where the mask is computed and not given), carried to samples as
    stft_cases.fused_reference does: sqrt(2 / n_fft), the root mean square of w / sum w^2, the
    frames over a block as squares, the renorm's gain."""
    geo = geo or pair.geo
    _, X = pair.spectra()
    a_ts, a_m = pair.promises()
    X32 = sc.f32_stft(pair.mix, geo)
    out = []
    # w / sum w^2 in the steady state, any frame_len and hop: the padded window's squares folded
    # modulo the hop
    win = sc._padded_window(geo, np.float64)
    fold = np.zeros(-(-geo.n_fft // geo.hop) * geo.hop)
    fold[:geo.n_fft] = win ** 2
    wss = np.tile(fold.reshape(-1, geo.hop).sum(axis=0), fold.shape[0] // geo.hop)[:geo.n_fft]
    syn = np.sqrt(np.mean((win[win > 0] / wss[win > 0]) ** 2)) * np.sqrt(2.0 / geo.n_fft)
    for i, mk in enumerate(masks):
        mk = np.asarray(mk, np.float64)
        if phase_ref is not None:
            R = sc.ref_stft(phase_ref, geo)
            with np.errstate(all="ignore"):
                ph = np.where(np.abs(R) > 0, R / np.where(np.abs(R) > 0, np.abs(R), 1), 1.0)
            R32 = sc.f32_stft(phase_ref, geo)
            Y = np.abs(X) * mk * ph
            Y32 = (np.abs(X32) * mk.astype(np.float32) * np.exp(1j * np.angle(R32))).astype(np.complex64)
        else:
            Y = X * mk
            Y32 = (X32 * mk.astype(np.float32)).astype(np.complex64)
        y = sc.ref_istft(Y, geo, nsamps)
        y32 = sc.f32_istft(Y32, geo, nsamps)
        gain = 1.0
        if norm is not None and norm > 0:
            gain = norm / (np.abs(y).max() + EPS32)
            y32 = y32 * np.float32(norm) / (np.abs(y32).max() + np.float32(EPS32))
        aY = np.abs(mk).max(axis=1) * a_m + (0.0 if a_mask is None else a_mask[i])
        aY = aY * syn * gain
        nb = -(-y.shape[0] // geo.hop)
        start = geo.n_fft // 2 if geo.center else 0           # the wave's sample 0 in frame coordinates
        inp = np.zeros(nb)
        for b in range(nb):
            lo, hi = start + b * geo.hop, start + (b + 1) * geo.hop   # frame t covers [t hop, t hop + n_fft)
            t0 = max(0, -(-(lo - geo.n_fft + 1) // geo.hop))
            t1 = min(aY.shape[0], (hi - 1) // geo.hop + 1)
            inp[b] = np.sqrt((aY[t0:t1] ** 2).sum())
        out.append((y * gain, y32, inp))
    return out


def judge_wave(name, got, y, y32, inp, hop):
    return sc.judge(name, sc.blocks(np.asarray(got, np.float64), hop), sc.blocks(y, hop), sc.blocks(y32, hop),
                    floor=np.asarray(inp) / M_BITS, exact_zero=False)   # (inp carries m already)
