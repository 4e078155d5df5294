"""
Constructed spectrograms for the two-class CGMM (numpy only: no audio, no transform, no device).

A case is a seeded complex64 [C][F][T] array.  Every bin has a KIND, fixed by its index
(kind_of_bin: f % 6), so a failing bin names its cause:

  0 zero_frame  an ordinary bin with one exactly-zero frame (frame T // 3)
  1 half_zero   an ordinary bin whose first T // 2 frames are exactly zero
  2 tiny        an ordinary bin scaled by 2^-14: |x|^2 is below float32 eps in most frames (phi is
                floored there) and above it in the loudest
  3 big         an ordinary bin scaled by 2^12
  4 rank1       every channel an exact (power of two times a power of i) multiple of channel 0:
                the covariance is exactly rank 1, the eigenvalue floor is active
  5 ordinary    a rank-1 gated source (about 40 % of the frames active) in full-rank
                correlated noise

The helpers the CPU and the GPU tests share are here too: the initial mask, the frame counts on
the edges of a dispatcher (t_edges), and the per-bin error report.
"""
import numpy as np

KINDS = ("zero_frame", "half_zero", "tiny", "big", "rank1", "ordinary")
FIXED_T = (1, 2, 3, 31, 32, 33, 63, 65)


def kind_of_bin(f):
    return KINDS[f % len(KINDS)]


def _cnormal(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def _ordinary_bin(rng, C, T):
    """[C][T] complex128: gated rank-1 source (amplitude 3) + full-rank correlated noise."""
    steer = np.exp(2j * np.pi * rng.uniform(size=C)) * rng.uniform(0.7, 1.3, size=C)
    gate = rng.uniform(size=T) < 0.4
    src = 3.0 * _cnormal(rng, T) * gate
    mix = np.eye(C) + 0.3 * _cnormal(rng, C, C)      # noise covariance mix mix^H: full rank
    return steer[:, None] * src[None, :] + mix @ _cnormal(rng, C, T)


def _well_posed(x):
    """Every eigenvalue of x x^H is either far above float32 resolution relative to the largest
    (> 1e-4) or an exact rank deficiency (< 1e-12).  In between, rounding the input to complex64
    alone moves the eigenvalue across the reference's floor at eps (cluster.py:107-113) -- a
    question float32 data cannot answer, for the oracle as little as for a kernel.  It happens to
    about one random bin in a hundred when the frame count is close to the channel count."""
    w = np.linalg.eigvalsh(x @ x.conj().T)
    r = w / max(w[-1], 1e-300)
    return not np.any((r > 1e-12) & (r < 1e-4))


def make_case(C, T, F=6, seed=0):
    """complex64 [C][F][T]; bin f is of kind_of_bin(f)."""
    rng = np.random.default_rng([int(seed), int(C), int(T), int(F)])
    obs = np.empty((C, F, T), np.complex64)
    for f in range(F):
        kind = kind_of_bin(f)
        x = _ordinary_bin(rng, C, T)
        while not (_well_posed(x) and _well_posed(x[:, T // 2:]) and _well_posed(np.delete(x, T // 3, 1))):
            x = _ordinary_bin(rng, C, T)             # (the same stream: still seeded)
        if kind == "zero_frame":
            x[:, T // 3] = 0.0
        elif kind == "half_zero":
            x[:, :T // 2] = 0.0
        elif kind == "tiny":
            x *= 2.0 ** -14
        elif kind == "big":
            x *= 2.0 ** 12
        elif kind == "rank1":
            ch0 = x[0].astype(np.complex64)          # rounded first: the multiples stay exact
            x = np.stack([ch0 * ((1j) ** c * 2.0 ** ((c % 3) - 1)) for c in range(C)])
        obs[:, f, :] = x
    return obs


def init_mask(F, T, seed=0):
    """uniform(0.05, 0.95) speech mask, float32 [F][T] (the oracle's axis order)."""
    rng = np.random.default_rng([int(seed), 77, int(F), int(T)])
    return rng.uniform(0.05, 0.95, size=(F, T)).astype(np.float32)


def perturbed(obs, seed=0, rel=6e-8):
    """The case with a float32-rounding-sized relative perturbation, re-rounded to complex64."""
    rng = np.random.default_rng([int(seed), 99])
    return (obs.astype(np.complex128) * (1.0 + rel * rng.standard_normal(obs.shape))).astype(np.complex64)


STARTS = ("identity", "mask", "alpha")      # deterministic start, initial mask, update_alpha
SENSITIVITY_BAR = 5e-5
SHORT_T = 70


def start_args(start, F, T, seed=0):
    """(init_mask F x T float32 or None, update_alpha) of one of STARTS."""
    return (init_mask(F, T, seed) if start == "mask" else None), start == "alpha"


def oracle_gamma(obs, iters, init=None, update_alpha=False):
    """The float64 reference: posteriors [2][F][T] of obs [C][F][T] (init: F x T or None)."""
    from oracle import np_oracle as o
    return o.cgmm_gamma(obs, iters, init_mask=None if init is None else init.astype(np.float64),
                        update_alpha=update_alpha)


def sensitivity(obs, seed=0, iters=(1, 2), oracle=oracle_gamma):
    """Worst per-cell move of the oracle's posteriors under perturbed(obs), over the three starts
    and `iters`; and the report rows of the worst run."""
    F, T = obs.shape[1:]
    pert = perturbed(obs, seed)
    worst, rows = 0.0, []
    for start in STARTS:
        init, ua = start_args(start, F, T, seed)
        for n in iters:
            r = bin_report(oracle(pert, n, init, ua)[0], oracle(obs, n, init, ua)[0])
            m = max(x["max"] for x in r)
            if m >= worst:
                worst, rows = m, r
    return worst, rows


_sound = {}


def sound_case(C, T, F=6):
    """(obs, seed): make_case(C, T, F, seed) for the first seed = C, C + 100, ... at which the
    float64 `oracle` itself answers input rounding with less than SENSITIVITY_BAR per cell (all
    starts, 0 to 2 iterations).  When the non-zero frames of a bin are about as many as the
    channels, a class's weighted covariance can have an eigenvalue near eps times the largest
    without the input's having one (_well_posed does not see the weights); the reference's
    floor then makes the posterior a discontinuous function of float32 data, and no reference
    exists to hold a kernel to.  About one short construction in twenty is like that, none of
    those seen had more than 33 frames; only T <= SHORT_T is searched, a longer case is
    make_case(C, T, F, C) as it comes (test_cgmm_cases.py checks every one the GPU file uses)."""
    key = (C, T, F)
    if key not in _sound:
        seed = C
        obs = make_case(C, T, F, seed)
        while T <= SHORT_T and not sensitivity(obs, seed, iters=(0, 1, 2))[0] < SENSITIVITY_BAR:
            seed += 100
            if seed > C + 2000:
                raise RuntimeError(f"no sound construction for C={C} T={T} F={F}")
            obs = make_case(C, T, F, seed)
        _sound[key] = (obs, seed)
    return _sound[key]


def scan_configs(C, config, t_max=4400):
    """[(first T, (idx, nt, u, rf)), ...]: where config(C, T) changes over T = 1 .. t_max."""
    out, prev = [], None
    for T in range(1, t_max + 1):
        cur = tuple(config(C, T))
        if cur != prev:
            out.append((T, cur))
            prev = cur
    return out


def t_edges(C, config, t_max=4400):
    """Frame counts on the edges of the dispatcher config(C, T) -> (idx, nt, u, rf) (idx < 0: not
    bin-resident): every T at which the configuration changes and every nt * rf (all of a
    thread's frames in registers, the LDS tile empty), each with T - 1 and T + 1; the short
    and tile-edge counts 1, 2, 3, C - 1, C, C + 1, 31, 32, 33, 63, 65."""
    ts = set(FIXED_T) | {C - 1, C, C + 1}
    for first, (idx, nt, u, rf) in scan_configs(C, config, t_max):
        ts |= {first - 1, first, first + 1}
        if idx >= 0:
            ts |= {nt * rf - 1, nt * rf, nt * rf + 1}
    return sorted(t for t in ts if 1 <= t <= t_max)


def bin_report(got, ref, nt=0):
    """got, ref: class-0 posteriors [F][T].  One dict per bin: kind, max |d|, mean |d|, the worst
    frame and its frame % nt (the thread that owns it; nt = 0: not bin-resident)."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    rows = []
    for f in range(d.shape[0]):
        t = int(np.argmax(d[f]))
        rows.append(dict(bin=f, kind=kind_of_bin(f), max=float(d[f, t]), mean=float(d[f].mean()),
                         frame=t, lane=(t % nt) if nt else -1))
    return rows


def describe(rows, bad=lambda r: True):
    return "; ".join(f"bin {r['bin']} ({r['kind']}): max {r['max']:.2e} mean {r['mean']:.2e} at frame "
                     f"{r['frame']} (frame % nt = {r['lane']})" for r in rows if bad(r))
