"""
Constructed cases for the sample I/O of every pipeline (numpy only: no device): the float -> PCM_16
quantiser, the max-abs renorm in front of it, and the 16-bit ingest.  PARITY_NOTES_SAMPLES.md has
the figures measured with them.

THE RULE.  The project declares one float -> PCM_16 rule (libs/wavio.float_to_pcm16): rint(x * 32767)
of the float32 sample, the product taken in float64 (exact there: 24 + 15 significand bits), ties to
even, no clipping -- a value out of range wraps modulo 2^16.

REFERENCE.  exact_pcm16: integer arithmetic on the sample's significand and exponent, no floating
point of any width.  x = m 2^e with integers m, e; m 32767 is a Python int, divided by 2^-e with
round-half-to-even, reduced modulo 2^16 into int16.

THE OTHER RULE.  f32_product_pcm16: rintf(x * 32767.f), the product rounded to float32 first.  It
differs from the rule by one step wherever that rounding lands on or across a half; it is here so
that a test can show that the family below tells the two apart.

QUANTISER FAMILY (float32, quantiser_family()).  For every k in [-32768, 32767) the float32 nearest
(k + 0.5) / 32767 and its two float32 neighbours: the values whose product lies within a few ulp of a
rounding boundary.  The two exact ties +-0.5 (+-16383.5 in double; 32767 is odd, so no other
float32 in (-1, 1) is one) are among them, and named again explicitly.  Then 0, -0.0, the smallest
normal, a subnormal, +-1 and the first floats past +-1, a few values out to +-4.0 where the result
wraps (none of +-1.5, +-2.5, +-3.5: those would be further ties), and 1000 seeded uniform values.
Duplicates are dropped (by bit pattern), so every member counts once.
Non-finite samples are left out: the conversion of a NaN or an infinity to an integer is defined
neither in C nor in numpy, and the library reports non-finite data through its status words
(SETK_NUM_NONFINITE) before any sample is written.

INGEST PATTERNS (ingest_pattern()).  int16 frames pcm[n][c] = 40503 (n C + c) mod 2^16 - 32768 (40503
is odd: the map is a bijection of the 16-bit range, consecutive samples differ by about 25000), with
-32768 and 32767 then placed in every channel (rows 3c and 3c + 1 modulo n; a one-frame pattern
alternates them over the channels).  A sample that lands in the wrong place is an error of order one.

RENORM STATEMENT (renorm_f32()).  What scale_kernel (pass2.hip) computes, in numpy float32:
sc = float32(norm) / (float32(omax) + float32(2^-23)), or 1 when norm <= 0; out = float32(src * sc).

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***
"""
import functools

import numpy as np

EPS = np.float32(2.0 ** -23)
WRAP_VALUES = (1.25, 2.0, 2.75, 3.0, 3.999, 4.0)


def exact_pcm16_one(bits):
    """One float32, given as its 32 bits: the rule in integers."""
    sign = -1 if bits >> 31 else 1
    expo = (bits >> 23) & 0xFF
    frac = bits & 0x7FFFFF
    if expo == 0xFF:
        raise ValueError("non-finite sample")
    m, e = (frac, -149) if expo == 0 else (frac | 0x800000, expo - 150)
    p = m * 32767
    if e >= 0:
        q = p << e
    else:
        s = -e
        q, r = p >> s, p & ((1 << s) - 1)
        half = 1 << (s - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
    return (sign * q + 32768) % 65536 - 32768


def exact_pcm16(x):
    """The rule on an array of float32, element by element in Python integers."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.fromiter((exact_pcm16_one(b) for b in x.view(np.uint32).ravel().tolist()), dtype=np.int64,
                      count=x.size)
    return out.astype(np.int16).reshape(x.shape)


def f32_product_pcm16(x):
    """rintf(x * 32767.f): the product rounded to float32 before the rounding to an integer."""
    p = np.asarray(x, dtype=np.float32) * np.float32(32767.0)
    assert p.dtype == np.float32
    return np.rint(p).astype(np.int64).astype(np.int16)


def exact_ties(x):
    """Members whose product x * 32767 (exact in float64) lies exactly on a half."""
    p = np.asarray(x, dtype=np.float32).astype(np.float64) * 32767.0
    return np.abs(p - np.trunc(p)) == 0.5


@functools.lru_cache(maxsize=None)
def quantiser_family():
    """(values float32 [M], exact reference int16 [M]); both read-only."""
    k = np.arange(-32768, 32767, dtype=np.float64)
    mid = ((k + 0.5) / 32767.0).astype(np.float32)
    near = np.stack([np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))], axis=1)
    one = np.float32(1.0)
    tiny = np.finfo(np.float32).tiny
    edge = [0.5, -0.5, 0.0, -0.0, tiny, -tiny, np.float32(3e-45), -np.float32(3e-45), one, -one,
            np.nextafter(one, np.float32(2)), -np.nextafter(one, np.float32(2))]
    edge += [s * v for v in WRAP_VALUES for s in (1, -1)]
    rnd = np.random.default_rng(20240607).uniform(-1.0, 1.0, 1000)
    x = np.concatenate([near.ravel(), np.asarray(edge, dtype=np.float32), rnd.astype(np.float32)]).astype(np.float32)
    _, first = np.unique(x.view(np.uint32), return_index=True)      # (by bits: 0 and -0.0 both stay)
    x = np.ascontiguousarray(x[np.sort(first)])
    assert np.isfinite(x).all()
    ref = exact_pcm16(x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def family_rows(C, N):
    """The family laid out as C x N for setk_float_to_pcm16: channel c is the family rotated by
    c * 7919 members and cut (or wrapped round) to N.  Returns (audio float32 [C][N], the exact
    reference in the operator's interleaved order int16 [N][C])."""
    x, ref = quantiser_family()
    idx = (np.arange(N)[None, :] + 7919 * np.arange(C)[:, None]) % x.size
    return np.ascontiguousarray(x[idx]), np.ascontiguousarray(ref[idx].T)


def ingest_pattern(n, C, seed=0):
    """int16 frames [n][C] (a wave file's layout) whose value identifies (n, c)."""
    i = np.arange(n, dtype=np.int64)[:, None] * C + np.arange(C, dtype=np.int64)[None, :] + 977 * seed
    pcm = ((40503 * i) % 65536 - 32768).astype(np.int16)
    for c in range(C):
        if n >= 2:
            pcm[(3 * c) % n, c] = -32768
            pcm[(3 * c + 1) % n, c] = 32767
        else:
            pcm[0, c] = 32767 if c % 2 else -32768
    return np.ascontiguousarray(pcm)


def ingest_float(pcm):
    """read_wav's dtype='float32' decode, channel major: exact (a 16-bit integer times 2^-15)."""
    return np.ascontiguousarray(pcm.T.astype(np.float32) / np.float32(32768.0))


def ingest_power0(pcm):
    """sum (pcm[:, 0] / 32768)^2 in float64."""
    return float(np.sum((pcm[:, 0].astype(np.float64) / 32768.0) ** 2))


def renorm_scale(norm, omax):
    """sc of scale_kernel as a float32."""
    norm = np.float32(norm)
    if not norm > 0:
        return np.float32(1.0)
    sc = norm / (np.float32(omax) + EPS)
    assert sc.dtype == np.float32
    return sc


def renorm_f32(src, norm, omax, sc=None):
    """float32(src * sc): the float output of the renorm, and what its 16-bit branch quantises."""
    sc = renorm_scale(norm, omax) if sc is None else np.float32(sc)
    out = np.asarray(src, dtype=np.float32) * sc
    assert out.dtype == np.float32
    return out


def renorm_scale_neighbours(norm, omax):
    """sc and its two float32 neighbours: what a device division that is not correctly rounded
    could hand the kernel (one choice per utterance)."""
    sc = renorm_scale(norm, omax)
    return [sc, np.nextafter(sc, np.float32(-np.inf)), np.nextafter(sc, np.float32(np.inf))]


def gaussian_disagreement(peak, n=400000, seed=5):
    """Samples (of n) on which the two rules differ for a Gaussian waveform renormed to `peak` as the
    kernel does it."""
    w = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    y = renorm_f32(w, peak, np.abs(w).max())
    rule = np.rint(y.astype(np.float64) * 32767.0).astype(np.int64).astype(np.int16)   # (= exact_pcm16, faster)
    return int(np.count_nonzero(f32_product_pcm16(y) != rule))
