"""Constructed signals and spectrograms for the transform conformance suites
(test_stft_cases.py on the CPU, test_gpu_stft_conformance.py on the device), the float64
reference, the plain float32 yardstick and the one helper that judges a result.

Reference: oracle/np_oracle.py's librosa_stft / librosa_istft.  Given float64 samples (complex128
spectra) they compute in float64 end to end -- only float32 input is rounded to complex64 on the
way out -- so they are called with float64 input, not restated.

Yardstick: the same operation in plain single precision (scipy's pocketfft on float32 frames,
float32 window and overlap-add; a float32 chirp-z where n_fft is no power of two).  Its error on
a frame (a block of hop output samples) is u_t; it is floored at the unit roundoff of float32,
2^-24: pocketfft cancels exactly on a few symmetric signals (DC under a rectangular window), which
no float32 pipeline with rounded twiddles promises, while rounding one result to float32 costs
up to 2^-24 of it in any of them.

Measure (judge): for every frame t, ||got_t - X_t||_2 and max_k |got - X|[t, k] are both held to
m (u_t ||X_t||_2 + floor), m = 4: two bits, the 22 significant bits of an fp16-split product
against float32's 24, and the room of one summation order (radix 16, radix 2) against another
(pocketfft's radix 4 / 2).  A bin answers to its frame's norm -- what an FFT promises -- not to
its own magnitude; since max_k |d_k| <= ||d||_2 the bin check is implied by the frame check and
is kept as the statement of what is promised (the report prints both ratios).  Frames whose
reference is exactly zero must be exactly zero.

floor (matrix-core forms only; mc_floor): mcdft.h's forward takes window x sample x 2^10 / peak
into fp16 pairs (hi, lo).  fp16's subnormal spacing is 2^-24, so below it the lo half keeps no
bits: every operand carries an ABSOLUTE error of up to one quantum 2^-24 / 2^10 = 2^-34 of full
scale, however small the sample.  A bin is a sum of n_fft such operands times unit-modulus
factors, a random walk of 2^-34 sqrt(n_fft) fullscale; a frame's norm over its F bins is that
times sqrt(F).  fullscale = max(1, 2^ceil(log2 peak)) is the power of two the kernel divides by.
"""
import os
import sys

import numpy as np
import scipy.fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as o  # noqa: E402

M_BITS = 4.0
U32 = 2.0 ** -24
POS512 = (0, 1, 15, 16, 17, 31, 32, 100, 255, 256, 257, 300, 383, 496, 510, 511)
PEAKS = (1.0, float(np.nextafter(np.float32(1), np.float32(2))), 2.0, 65504.0, 2.0 ** 40, 2.0 ** 60)
QUIET_PEAKS = (2.0 ** -12, 2.0 ** -16, 2.0 ** -24, 2.0 ** -32)
INV_BINS = (0, 1, 15, 16, 17, 31, 32, 48, 255, 256)


# ------------------------------------------------------------------ windows and geometry
def window_of(name, frame_len):
    """float64 analysis / synthesis window of frame_len samples."""
    if name == "rect":
        return np.ones(frame_len)
    return o.make_window(name, frame_len).astype(np.float64)


def plan_window(name, frame_len):
    """What stft_plan takes: None (the periodic Hann default) or float32 samples."""
    return None if name == "hann" else window_of(name, frame_len).astype(np.float32)


class Geom:
    def __init__(self, n_fft=512, hop=256, frame_len=None, center=True, window="hann"):
        self.n_fft, self.hop, self.center, self.window = n_fft, hop, center, window
        self.frame_len = n_fft if frame_len is None else frame_len
        self.F = n_fft // 2 + 1

    def with_(self, **kw):
        d = dict(n_fft=self.n_fft, hop=self.hop, frame_len=self.frame_len, center=self.center,
                 window=self.window)
        d.update(kw)
        return Geom(**d)

    def num_frames(self, n):
        return 1 + (n + (self.n_fft if self.center else 0) - self.n_fft) // self.hop

    def plan_args(self):
        return (self.frame_len, self.hop, self.n_fft, self.center, plan_window(self.window, self.frame_len))

    def __repr__(self):
        return f"n{self.n_fft}/l{self.frame_len}/h{self.hop}/{'c' if self.center else 'nc'}/{self.window}"


# ------------------------------------------------------------------ reference (float64)
def ref_stft(x, g):
    """x [N] or [C][N] -> [.., T][F] complex128."""
    x = np.asarray(x, np.float64)
    if x.ndim == 2:
        return np.stack([ref_stft(c, g) for c in x])
    S = o.librosa_stft(x, g.n_fft, g.hop, win_length=g.frame_len, window=window_of(g.window, g.frame_len),
                       center=g.center)
    assert S.dtype == np.complex128
    return np.ascontiguousarray(S.T)


def ref_istft(S, g, nsamps=None):
    """S [T][F] -> float64 samples."""
    S = np.asarray(S).astype(np.complex128)
    y = o.librosa_istft(S.T, g.hop, win_length=g.frame_len, window=window_of(g.window, g.frame_len),
                        center=g.center, length=nsamps)
    assert y.dtype == np.float64
    return y


# ------------------------------------------------------------------ yardstick (float32)
def _pow2(n):
    return n & (n - 1) == 0


def _czt32(a, n, inverse=False):
    """Bluestein's chirp-z DFT of length n along the last axis in complex64:
    X[k] = c[k] sum_j (a[j] c[j]) conj(c)[k - j], c[j] = exp(-i pi j^2 / n)."""
    M = 1 << int(np.ceil(np.log2(2 * n - 1)))
    j = np.arange(n)
    c = np.exp((1j if inverse else -1j) * np.pi * ((j * j) % (2 * n)) / n).astype(np.complex64)
    b = np.zeros(M, np.complex64)
    b[:n] = np.conj(c)
    b[M - n + 1:] = np.conj(c[1:][::-1])
    u = np.zeros(a.shape[:-1] + (M,), np.complex64)
    u[..., :n] = a.astype(np.complex64) * c
    v = scipy.fft.ifft(scipy.fft.fft(u, axis=-1) * scipy.fft.fft(b), axis=-1)
    assert v.dtype == np.complex64
    return v[..., :n] * c


def _rfft32(frames, n):
    if _pow2(n):
        X = scipy.fft.rfft(frames, axis=-1)
    else:
        X = _czt32(frames, n)[..., :n // 2 + 1]
    assert X.dtype == np.complex64
    return X


def _irfft32(S, n):
    S = S.astype(np.complex64)
    if _pow2(n):
        y = scipy.fft.irfft(S, n=n, axis=-1)
    else:
        full = np.concatenate([S, np.conj(S[..., -2:0:-1])], axis=-1)
        full[..., 0] = full[..., 0].real
        full[..., n // 2] = full[..., n // 2].real
        y = (_czt32(full, n, inverse=True).real / np.float32(n)).astype(np.float32)
    assert y.dtype == np.float32
    return y


def _padded_window(g, dtype):
    return o._pad_center(window_of(g.window, g.frame_len), g.n_fft).astype(dtype)


def f32_stft(x, g):
    x = np.asarray(x, np.float32)
    if x.ndim == 2:
        return np.stack([f32_stft(c, g) for c in x])
    if g.center:
        x = np.pad(x, g.n_fft // 2, mode="reflect")
    T = 1 + (x.shape[0] - g.n_fft) // g.hop
    idx = g.hop * np.arange(T)[:, None] + np.arange(g.n_fft)[None, :]
    return _rfft32(x[idx] * _padded_window(g, np.float32), g.n_fft)


def f32_istft(S, g, nsamps=None):
    """The float32 twin of librosa_istft (same frame count, trim and padding rules)."""
    S = np.asarray(S, np.complex64)
    n, hop = g.n_fft, g.hop
    T = S.shape[0]
    if nsamps is not None:
        T = min(T, int(np.ceil((nsamps + (n if g.center else 0)) / hop)))
    w = _padded_window(g, np.float32)
    fr = _irfft32(S[:T], n) * w
    L = n + hop * (T - 1)
    y = np.zeros(L, np.float32)
    wss = np.zeros(L, np.float32)
    w2 = w * w
    for t in range(T):
        y[t * hop:t * hop + n] += fr[t]
        wss[t * hop:t * hop + n] += w2
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    start = n // 2 if g.center else 0
    if nsamps is None:
        return y[start:L - start] if g.center else y
    y = y[start:start + nsamps]
    return np.pad(y, (0, nsamps - y.shape[0]))


# ------------------------------------------------------------------ the helper
def fullscale_of(peak):
    return max(1.0, 2.0 ** np.ceil(np.log2(peak))) if peak > 0 else 1.0


def mc_floor(peak, n_fft=512):
    """Frame-norm floor of the matrix-core forward (module docstring)."""
    return 2.0 ** -34 * fullscale_of(peak) * np.sqrt(n_fft * (n_fft // 2 + 1))


class Verdict:
    def __init__(self, name):
        self.name, self.rows, self.failures = name, [], []

    @property
    def ok(self):
        return not self.failures

    def worst(self):
        """(frame error / allowance, bin error / allowance, worst frame's relative error)."""
        if not self.rows:
            return 0.0, 0.0, 0.0
        r = np.asarray(self.rows)
        return float(r[:, 0].max()), float(r[:, 1].max()), float(r[:, 2].max())

    def line(self):
        f, b, rel = self.worst()
        return f"{self.name}: frame {f:.3f} bin {b:.3f} of the allowance; worst relative frame error {rel:.2e}"


def judge(name, got, ref, yard, floor=0.0, m=M_BITS, exact_zero=True, u_min=U32):
    """got, ref (float64 / complex128), yard: [..., T][K] -- every leading index and every frame
    (block) t is judged: ||got_t - ref_t||_2 and max_k |got - ref|[t, k] against
    m (u_t ||ref_t||_2 + floor), u_t = max(||yard_t - ref_t|| / ||ref_t||, u_min), u_min = 2^-24: one float32 rounding of the
    result (a caller whose result is a product of float32 operands says how many roundings)."""
    v = Verdict(name)
    got = np.asarray(got)
    ref = np.asarray(ref)
    if got.shape != ref.shape or np.asarray(yard).shape != ref.shape:
        v.failures.append(f"{name}: shapes {got.shape} {np.asarray(yard).shape} against {ref.shape}")
        return v
    K = ref.shape[-1]
    got2 = got.reshape(-1, K).astype(np.complex128)
    ref2 = ref.reshape(-1, K).astype(np.complex128)
    yard2 = np.asarray(yard).reshape(-1, K).astype(np.complex128)
    if not np.isfinite(got2).all():
        v.failures.append(f"{name}: non-finite values in {int((~np.isfinite(got2)).any(1).sum())} frames")
        return v
    norm = np.linalg.norm(ref2, axis=1)
    d = np.abs(got2 - ref2)
    err = np.linalg.norm(d, axis=1)
    bin_err = d.max(axis=1)
    uy = np.linalg.norm(yard2 - ref2, axis=1)
    allow = m * (np.maximum(uy, u_min * norm) + floor) * np.ones_like(norm)     # floor: one number, or one per frame
    for t in range(ref2.shape[0]):
        if norm[t] == 0:
            if exact_zero and err[t] != 0:
                v.failures.append(f"{name}: frame {t} of an all-zero reference holds {err[t]:.3e}")
            elif not exact_zero and err[t] > allow[t]:
                v.failures.append(f"{name}: frame {t} (zero reference) {err[t]:.3e} > {allow[t]:.3e}")
            continue
        # (the relative figure is for the report only: a frame 180 dB below the loudest one is
        #  float64 rounding of its neighbours, its ratio means nothing)
        v.rows.append((err[t] / allow[t], bin_err[t] / allow[t],
                       err[t] / norm[t] if norm[t] > 1e-9 * norm.max() else 0.0))
        if not err[t] <= allow[t]:
            v.failures.append(f"{name}: frame {t} error {err[t]:.3e} > allowance {allow[t]:.3e} "
                              f"(rel {err[t] / norm[t]:.2e}, yardstick {uy[t] / norm[t]:.2e})")
        elif not bin_err[t] <= allow[t]:
            v.failures.append(f"{name}: frame {t} bin {int(d[t].argmax())} error {bin_err[t]:.3e} > "
                              f"allowance {allow[t]:.3e}")
    return v


def blocks(y, hop):
    """A wave as [ceil(L / hop)][hop] blocks (the tail padded with zeros) for judge()."""
    y = np.asarray(y)
    nb = -(-y.shape[-1] // hop)
    out = np.zeros(y.shape[:-1] + (nb * hop,), y.dtype)
    out[..., :y.shape[-1]] = y
    return out.reshape(y.shape[:-1] + (nb, hop))


def yardstick_health(ref, yard):
    """Worst per-frame relative error of the yardstick (frames with a non-zero reference)."""
    K = ref.shape[-1]
    r = ref.reshape(-1, K)
    n = np.linalg.norm(r, axis=1)
    e = np.linalg.norm(np.asarray(yard).reshape(-1, K) - r, axis=1)
    return float((e[n > 0] / n[n > 0]).max()) if (n > 0).any() else 0.0


EPS32 = float(np.finfo(np.float32).eps)


def fused_reference(x, w, mask, geo, post, mc_peak=None):
    """The tapped weights applied to float64 spectra, float64 iSTFT, the max-abs renorm
    (inverse_stft(norm = max |x|)); the same in float32; and the input-referred allowance per
    block of hop samples.

    The forward transform of channel c promises ||dX_c,t|| <= u_c,t ||X_c,t|| (+ floor) per
    frame -- a bin answers to its frame's norm.  Behind the weights that is ||dY_t|| <= sum_c
    max_f |w_fc| (u_c,t ||X_c,t|| + floor), whatever is left of Y_t itself: a channel whose
    energy sits in one bin leaves the solver free in all the others, a post mask of 2^-20 takes
    the output 120 dB below the input.  irfft turns a half-spectrum error e into sqrt(2 / n_fft)
    ||e|| of samples, the synthesis window over the summed squared window scales it by w / sum w^2
    (its root mean square over the frame: the error is spread over the frame), the renorm applies
    its gain; channels and the frames that overlap a block are independent roundings and add as
    squares, the way the floor itself is accumulated.
    u_c,t is the float32 yardstick's on that channel and frame (at least 2^-24); floor is
    mc_floor(mc_peak) where stage 3 runs on the matrix cores."""
    norm = float(np.abs(x).max())
    X = ref_stft(x, geo)
    Y = np.einsum("fc,ctf->tf", np.conj(w.astype(np.complex128)), X)
    if post:
        Y = Y * np.minimum(mask, 1).astype(np.float64)
    y = ref_istft(Y, geo)
    gain = norm / (np.abs(y).max() + EPS32)
    X32 = f32_stft(x, geo)
    Y32 = np.einsum("fc,ctf->tf", np.conj(w), X32).astype(np.complex64)
    if post:
        Y32 = Y32 * np.minimum(mask, 1)
    y32 = f32_istft(Y32, geo)
    y32 = y32 * np.float32(norm) / (np.abs(y32).max() + np.float32(EPS32))
    nrm = np.linalg.norm(X, axis=2)                                           # [C][T]
    a = np.maximum(np.linalg.norm(X32 - X, axis=2), U32 * nrm) + (0.0 if mc_peak is None else mc_floor(mc_peak))
    aY = np.sqrt(((np.abs(w).max(axis=0)[:, None] * a) ** 2).sum(axis=0)) * np.sqrt(2.0 / geo.n_fft)   # [T], samples
    win = window_of(geo.window, geo.frame_len)
    wss = np.tile((win ** 2).reshape(-1, geo.hop).sum(axis=0), geo.n_fft // geo.hop)
    aY = aY * np.sqrt(np.mean((win / wss) ** 2)) * gain
    r = geo.n_fft // geo.hop                                                 # frames over a block
    nb = -(-y.shape[0] // geo.hop)
    inp = np.array([np.sqrt((aY[b:b + r] ** 2).sum()) for b in range(nb)])
    return y * gain, y32, inp


# ------------------------------------------------------------------ signals
class Case:
    def __init__(self, family, name, x, window="hann", pcm=None):
        self.family, self.name, self.window = family, name, window
        self.x = np.ascontiguousarray(x, np.float32)
        self.pcm = pcm              # int16 twin: x == pcm / 32768 exactly, or None
        self.peak = float(np.abs(self.x).max())

    @property
    def id(self):
        return f"{self.family}:{self.name}"


def channels(x, C):
    """C channels out of one signal: channel c is the signal rotated by 37 c samples, every other
    one negated -- the same peak and level structure in every channel."""
    x = np.asarray(x)
    return np.ascontiguousarray(np.stack([np.roll(x, 37 * c) * (-1 if c % 2 else 1) for c in range(C)]))


def _noise(rng, n):
    return rng.uniform(-1.0, 1.0, n)


def _at_peak(x, peak):
    x = np.asarray(x, np.float64)
    y = (x / np.abs(x).max() * peak).astype(np.float32)
    assert float(np.abs(y).max()) == float(np.float32(peak))
    return y


def signal_cases(n_fft=512, hop=256, families=None, peaks=PEAKS):
    """Every family at the geometry (n_fft, hop); the frame counts run from 10 to 19 of hop
    (odd and even), `ladder` alone is longer: eleven levels of one frame pair each."""
    rng = np.random.default_rng(20240611)
    s = n_fft / 512.0
    out = []

    def add(family, name, x, window="hann", pcm=None):
        if families is None or family in families:
            out.append(Case(family, name, x, window, pcm))

    # impulses: one unit sample per frame at the listed in-frame positions, one at each edge
    pos = sorted({min(n_fft - 1, int(round(p * s))) for p in POS512} | {0, 1, n_fft - 2, n_fft - 1})
    N = hop * (len(pos) + 2) + hop // 2 + 3
    x = np.zeros(N)
    for t, p in enumerate(pos):
        i = hop * t + p - (n_fft // 2 - hop)          # position p of centred frame t + 1 (hop = n / 2)
        x[min(max(i, 0), N - 1)] = 1.0
    x[1] = 1.0
    x[N - 2] = 1.0
    add("impulses", "unit", x)
    # full scale: tones on the bin grid, DC, alternation, square wave; Hann and rectangular
    N = 10 * hop + (hop // 2)
    n = np.arange(N)
    bins = {"bin16": 16, "bin48": 48, "bin240": 240, "bin1": 1, "bin32": 32, "bin255": 255}
    shapes = {"dc": np.ones(N), "alt": (-1.0) ** n,
              "square": np.where((n // max(1, int(round(8 * s)))) % 2 == 0, 1.0, -1.0)}
    for k, b in bins.items():
        shapes[k] = np.cos(2 * np.pi * max(1, int(round(b * s))) * n / n_fft)
    for peak in peaks:
        for k, v in shapes.items():
            for win in ("hann", "rect"):
                add("fullscale", f"{k}@{peak:.9g}/{win}", _at_peak(v, peak), win)
    # ladder: bursts one frame pair long at 2^0, 2^-4 .. 2^-40 inside one utterance of peak 1
    levels = [2.0 ** -e for e in range(0, 41, 4)]
    x = np.concatenate([_at_peak(_noise(rng, 2 * hop), lv) for lv in levels])
    add("ladder", "2^0..2^-40", x)
    # quiet: whole utterances far below full scale (float only)
    for i, peak in enumerate(QUIET_PEAKS):
        add("quiet", f"2^{int(np.log2(peak))}", _at_peak(_noise(rng, hop * (11 + i) + 17 * i), peak))
    # coloured: a loud tone off the bin grid over a 1e-6 floor; noise under an 80 dB tilt
    N = 15 * hop + 100
    n = np.arange(N)
    add("coloured", "tone+floor", 0.9 * np.cos(2 * np.pi * 37.3 * s * n / n_fft + 0.3) + 1e-6 * _noise(rng, N))
    N = 18 * hop + 192
    spec = np.fft.rfft(_noise(rng, N))
    spec *= 10.0 ** (-4.0 * np.arange(spec.shape[0]) / (spec.shape[0] - 1))
    add("coloured", "tilt80dB", _at_peak(np.fft.irfft(spec, n=N), 0.9))
    # pcm: 16-bit extremes (float twin = pcm / 32768, exact)
    def add_pcm(family, name, p):
        p = np.ascontiguousarray(p, np.int16)
        add(family, name, p.astype(np.float32) / np.float32(32768), "hann", p)
    N = 12 * hop + 5
    add_pcm("pcm", "alt+32767/-32768", np.where(np.arange(N) % 2 == 0, 32767, -32768))
    add_pcm("pcm", "dither1lsb", rng.integers(-1, 2, N))
    p = np.zeros(11 * hop, np.int64)
    p[5 * hop + 3] = -7
    add_pcm("pcm", "one-sample", p)
    # zeros: three leading and two trailing frames exactly zero around a burst (centred frames)
    T = 13
    p = np.zeros(hop * (T - 1), np.int64)
    lo, hi = 2 * hop + n_fft // 2, hop * (T - 2) - n_fft // 2
    p[lo:hi] = rng.integers(-20000, 20001, hi - lo)
    add_pcm("zeros", "burst", p)
    # the shortest legal utterances
    add("shortest", "centred", _at_peak(_noise(rng, n_fft // 2 + 1), 0.7))
    add("shortest", "uncentred", _at_peak(_noise(rng, n_fft), 0.7))
    return out


def geom_of(case, n_fft=512, hop=256, **kw):
    center = kw.pop("center", case.name != "uncentred")
    return Geom(n_fft=n_fft, hop=hop, window=case.window, center=center, **kw)


# ------------------------------------------------------------------ spectrograms for the inverse
class InvCase:
    def __init__(self, name, S, window="hann"):
        self.name, self.window = name, window
        self.S = np.ascontiguousarray(S, np.complex64)     # [T][F]


def inverse_cases(n_fft=512):
    rng = np.random.default_rng(977)
    F = n_fft // 2 + 1
    out = []
    for k in sorted({min(F - 1, int(round(k * n_fft / 512))) for k in INV_BINS}):
        for t in (4, 7):
            S = np.zeros((10 + t % 2, F), np.complex64)
            S[t, k] = 0.75 if k in (0, F - 1) else 0.6 - 0.8j
            out.append(InvCase(f"cell(t={t},k={k})", S))
    S = np.full((11, F), 1 + 1j, np.complex64)
    S[:, 0] = 1
    S[:, F - 1] = 1
    # irfft(1 + 1j) is a unit impulse at sample 0 of the frame plus an odd cotangent tail: the Hann
    # window has a zero on the impulse and at hop = n_fft / 2 the tails of neighbouring frames
    # cancel, so under Hann the wave is zero to rounding -- ill posed.  It is judged under the
    # rectangular window; (-1)^k moves the impulse to the window's centre for Hann.
    out.append(InvCase("flat-aligned", S, "rect"))
    out.append(InvCase("flat-centred", S * ((-1.0) ** np.arange(F)).astype(np.float32)))
    T = 14
    S = (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))).astype(np.complex64)
    lev = 10.0 ** np.linspace(-6, 3, T)
    S *= lev[:, None].astype(np.float32)
    S[9] *= np.float32(1e30) / np.float32(lev[9])
    S[:, 0] = S[:, 0].real
    S[:, F - 1] = S[:, F - 1].real
    out.append(InvCase("levels1e-6..1e3+1e30", S))
    S = (rng.standard_normal((12, F)) + 1j * rng.standard_normal((12, F))).astype(np.complex64)
    out.append(InvCase("imag-at-dc-nyquist", S))                    # irfft ignores those parts
    return out


# ------------------------------------------------------------------ the CPU lane model as a transform
def mc_exponent(peak, negative=True):
    """The power of two of pass2_mc.hip: 2^e > max |x| when max |x| > 1, e = 0 down to 2^-15,
    and (negative) again 2^e > max |x| below that -- no non-zero 16-bit utterance peaks there."""
    if peak > 1.0 or (negative and 0 < peak < 2.0 ** -15):
        e = int(np.floor(np.log2(peak))) + 1
        return max(-100, min(100, e))
    return 0


def model_stft(x, g, negative=True, model=None):
    """One channel through mcdft_model.forward with the kernel's window rows (float32 window x
    2^-e) and operand scale 2^10: [T][257] complex128."""
    import mcdft_model
    model = model or mcdft_model
    assert g.n_fft == 512 and g.frame_len == 512
    x = np.asarray(x, np.float32)
    e = mc_exponent(float(np.abs(x).max()), negative)
    if g.center:
        x = np.pad(x, 256, mode="reflect")
    T = 1 + (x.shape[0] - 512) // g.hop
    idx = g.hop * np.arange(T)[:, None] + np.arange(512)[None, :]
    w = (_padded_window(g, np.float32) * np.float32(2.0 ** -e)).astype(np.float32)
    X = model.forward((x[idx] * w).astype(np.float32)).astype(np.complex128)
    return X * 2.0 ** e


def model_istft(S, g, model=None):
    """mcdft_model.inverse + float32 window, overlap-add and normalisation (length: natural)."""
    import mcdft_model
    model = model or mcdft_model
    S = np.asarray(S, np.complex64)
    T = S.shape[0]
    w = _padded_window(g, np.float32)
    fr = (model.inverse(S) / np.float32(512)) * w
    L = 512 + g.hop * (T - 1)
    y = np.zeros(L, np.float32)
    wss = np.zeros(L, np.float32)
    for t in range(T):
        y[t * g.hop:t * g.hop + 512] += fr[t]
        wss[t * g.hop:t * g.hop + 512] += w * w
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[256:L - 256] if g.center else y
