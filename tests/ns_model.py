"""
numpy restatement of funcwj/setk scripts/sptk/libs/ns.py (MCRA.run :56-209, iMCRA.run :247-387)
for the tests: the same operations in the same order on float64, with the exponential integral
from scipy.special.exp1 where the reference integrates exp(-t) / t numerically per cell.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***

Every run also returns its DECISION MARGIN: the smallest relative distance |q - threshold| /
|threshold| of any quantity the recursion compares against a threshold
  iMCRA  gamma_min / zeta against gamma0 / zeta0; gamma_min_hat against 1 and gamma1; zeta_hat
         against zeta0
  MCRA   var_sr against delta; zeta_g / zeta_l against zeta_min / zeta_max; the frame-level tests
         (zeta_frame against zeta_min, against the previous frame's, against zeta_min x peak and
         zeta_max x peak where those are evaluated)
A fixture whose margin is above the rounding level of two float64 implementations takes the same
decisions in both: tools/make_ns_golden.py keeps only cases with a margin of at least 1e-9.

One deliberate difference (tests/PARITY_NOTES_NS.md): iMCRA evaluates E1 with its a-posteriori SNR
floored at eps, as the device does; `clamped` counts the cells where that floor acted (0 in every
golden case, so the recorded reference gains are unaffected).

The module also owns the inputs of the golden cases (CASES, synth_spectrogram, synth_samples).
"""
import numpy as np
from scipy.special import exp1

WINDOWS = {"hann": (0.5, 0.5), "hamming": (0.54, 0.46), "blackman": (0.42, 0.50, 0.08)}


def window(name, half):
    """scipy.signal.get_window(name, 2 half + 1), fftbins=True, for the cosine windows."""
    n = 2 * half + 1
    if n == 1:
        return np.ones(1)
    fac = np.linspace(-np.pi, np.pi, n + 1)
    w = np.zeros(n + 1)
    for k, a in enumerate(WINDOWS[name]):
        w += a * np.cos(k * fac)
    return w[:-1]


class _Margin(object):
    def __init__(self):
        self.value = np.inf

    def __call__(self, q, thr, where=None):
        q = np.asarray(q, dtype=np.float64)
        d = np.abs(q - thr) / np.abs(thr)
        if where is not None:
            d = d[where]
        if np.size(d):
            self.value = min(self.value, float(np.min(d)))


MCRA_DEFAULTS = dict(alpha=0.92, delta=5, beta=0.7, alpha_s=0.9, alpha_d=0.85, alpha_p=0.2, gmin_db=-10,
                     xi_min_db=-18, w_mcra=1, w_local=1, w_global=15, h_mcra="hann", h_local="hann",
                     h_global="hann", q_max=0.95, zeta_min_db=-10, zeta_max_db=-5, zeta_p_max_db=10,
                     zeta_p_min_db=0, L=125, M=128)
IMCRA_DEFAULTS = dict(alpha=0.92, alpha_s=0.9, alpha_d=0.85, b_min=1.66, gamma0=4.6, gamma1=3, zeta0=1.67,
                      xi_min_db=-18, gmin_db=-10, w_mcra=1, h_mcra="hann", beta=1.47, V=15, U=8)


def mcra(stft, eps=1e-7, **conf):
    """-> (gain T x F, margin)"""
    c = dict(MCRA_DEFAULTS, **conf)
    a_t, a_s, a_d, a_p = c["alpha"], c["alpha_s"], c["alpha_d"], c["alpha_p"]
    gmin, xi_min = 10**(c["gmin_db"] / 10), 10**(c["xi_min_db"] / 10)
    w_m, w_g, w_l = (window(c["h_mcra"], c["w_mcra"]), window(c["h_global"], c["w_global"]),
                     window(c["h_local"], c["w_local"]))
    zmin, zmax = 10**(c["zeta_min_db"] / 10), 10**(c["zeta_max_db"] / 10)
    zpmin, zpmax = 10**(c["zeta_p_min_db"] / 10), 10**(c["zeta_p_max_db"] / 10)
    stft = np.asarray(stft).astype(np.complex128)
    T, F = stft.shape
    power = stft.real**2 + stft.imag**2
    margin = _Margin()
    gh1, p_hat, zeta, zeta_peak = 1, np.ones(F), np.ones(F), 0
    lam = power[0]
    G = []

    def prob(z):
        margin(z, zmin)
        margin(z, zmax)
        p = np.zeros(F)
        mid = np.logical_and(z > zmin, z < zmax)
        p[mid] = np.log10(z[mid] / zmin) / np.log10(zmax / zmin)
        p[z >= zmax] = 1
        return p

    for t in range(T):
        gamma = np.maximum(power[t] / np.maximum(lam, eps), eps)
        xi = np.maximum(a_t * gh1**2 * gamma + (1 - a_t) * np.maximum(gamma - 1, 0), xi_min)
        v = gamma * xi / (1 + xi)
        gh1 = xi * np.exp(0.5 * exp1(v)) / (1 + xi)
        var_sf = np.convolve(power[t], w_m, mode="same")
        if t == 0:
            var_s = power[t]
            var_s_min = var_s
            var_s_tmp = var_s
        else:
            var_s = a_s * var_s + (1 - a_s) * var_sf
        if (t + 1) % c["L"] == 10:
            var_s_min = np.minimum(var_s_tmp, var_s)
            var_s_tmp = var_s
        else:
            var_s_min = np.minimum(var_s_min, var_s)
            var_s_tmp = np.minimum(var_s_tmp, var_s)
        var_sr = var_s / np.maximum(eps, var_s_min)
        margin(var_sr, c["delta"])
        p_hat = a_p * p_hat + (1 - a_p) * (var_sr > c["delta"])
        a_d_hat = a_d + (1 - a_d) * p_hat
        lam = a_d_hat * lam + (1 - a_d_hat) * power[t]
        zeta = c["beta"] * zeta + (1 - c["beta"]) * xi
        p_g = prob(np.convolve(zeta, w_g, mode="same"))
        p_l = prob(np.convolve(zeta, w_l, mode="same"))
        zf = np.mean(zeta[:c["M"] // 2 + 1])
        if t == 0:
            zf_pre = zf
        margin(zf, zmin)
        if zf > zmin:
            if t > 0:
                margin(zf, zf_pre)
            if zf > zf_pre:
                zeta_peak = min(max(zf, zpmin), zpmax)
                p_frame = 1
            else:
                if zeta_peak > 0:
                    margin(zf, zmin * zeta_peak)
                if zf <= zmin * zeta_peak:
                    p_frame = 0
                else:
                    if zeta_peak > 0:
                        margin(zf, zmax * zeta_peak)
                    if zf >= zmax * zeta_peak:
                        p_frame = 1
                    else:
                        p_frame = np.log10(zf / (zmin * zeta_peak)) / np.log10(zmax / zmin)
        else:
            p_frame = 0
        zf_pre = zf
        q = np.minimum(c["q_max"], 1 - p_l * p_frame * p_g)
        p = 1 / (1 + q * (1 + xi) * np.exp(-v) / (1 - q))
        G.append(gh1**p * gmin**(1 - p))
    return np.stack(G), margin.value


def imcra(stft, eps=1e-7, info=None, **conf):
    """-> (gain T x F, margin); info (a dict) receives `clamped`."""
    c = dict(IMCRA_DEFAULTS, **conf)
    a_t, a_s, a_d = c["alpha"], c["alpha_s"], c["alpha_d"]
    gmin, xi_min = 10**(c["gmin_db"] / 10), 10**(c["xi_min_db"] / 10)
    b_min = 1 / c["b_min"]
    gamma0, gamma1, zeta0, V, U = c["gamma0"], c["gamma1"], c["zeta0"], c["V"], c["U"]
    w_m = window(c["h_mcra"], c["w_mcra"])
    stft = np.asarray(stft).astype(np.complex128)
    T, F = stft.shape
    power = stft.real**2 + stft.imag**2
    margin = _Margin()
    lam, gh1 = power[0], 1
    sw, sw_hat, G, clamped = [], [], [], 0
    for t in range(T):
        gamma = power[t] / np.maximum(lam * c["beta"], eps)
        xi = np.maximum(a_t * (gh1**2 * gamma) + (1 - a_t) * np.maximum(gamma - 1, 0), xi_min)
        v = gamma * xi / (1 + xi)
        clamped += int(np.sum(gamma < eps))
        gh1 = xi / (1 + xi) * np.exp(0.5 * exp1(np.maximum(gamma, eps) * xi / (1 + xi)))
        var_sf = np.convolve(power[t], w_m, mode="same")
        if t == 0:
            var_s = var_sf
            var_s_hat = var_sf
            var_s_min = var_sf
            var_s_min_sw = var_sf
        else:
            var_s = a_s * var_s + (1 - a_s) * var_sf
            var_s_min = np.minimum(var_s_min, var_s)
            var_s_min_sw = np.minimum(var_s_min_sw, var_s)
        gamma_min = power[t] * b_min / np.maximum(var_s_min, eps)
        zeta = var_sf * b_min / np.maximum(var_s_min, eps)
        margin(gamma_min, gamma0)
        margin(zeta, zeta0)
        indicator = np.logical_and(gamma_min < gamma0, zeta < zeta0)
        ind_conv = np.convolve(indicator, w_m, mode="same")
        nz = ind_conv > 0
        obs_conv = np.convolve(power[t] * indicator, w_m, mode="same")
        var_sf_hat = var_s_hat.copy()
        var_sf_hat[nz] = obs_conv[nz] / ind_conv[nz]
        if t == 0:
            var_s_min_hat = var_s
            var_s_min_sw_hat = var_sf
        else:
            var_s_hat = a_s * var_s_hat + (1 - a_s) * var_sf_hat
            var_s_min_hat = np.minimum(var_s_min_hat, var_s_hat)
            var_s_min_sw_hat = np.minimum(var_s_min_sw_hat, var_s_hat)
        gmh = power[t] * b_min / np.maximum(var_s_min_hat, eps)
        zh = var_s * b_min / np.maximum(var_s_min_hat, eps)
        margin(gmh, 1.0)
        margin(gmh, gamma1)
        margin(zh, zeta0)
        q_idx = np.logical_and(np.logical_and(gmh > 1, gmh < gamma1), zh < zeta0)
        q = np.zeros(F)
        q[q_idx] = (gamma1 - gmh[q_idx]) / (gamma1 - 1)
        p = np.zeros(F)
        p[q_idx] = 1 / (1 + q[q_idx] * (1 + xi[q_idx]) / (1 - q[q_idx]) * np.exp(-v[q_idx]))
        p[np.logical_and(gmh >= gamma1, zh >= zeta0)] = 1
        a_d_hat = a_d + (1 - a_d) * p
        lam = a_d_hat * lam + (1 - a_d_hat) * power[t]
        sw.append(var_s_min_sw)
        sw_hat.append(var_s_min_sw_hat)
        if (t + 1) % V == 0:
            # the last U FRAMES' running sub-window minima, as the reference's lists hold them
            var_s_min = np.min(np.stack(sw[-U:]), 0)
            var_s_min_hat = np.min(np.stack(sw_hat[-U:]), 0)
            var_s_min_sw = var_s
            var_s_min_sw_hat = var_s_hat
        G.append(gh1**p * gmin**(1 - p))
    if info is not None:
        info["clamped"] = clamped
    return np.stack(G), margin.value


def run(kind, stft, eps=1e-7, **conf):
    return mcra(stft, eps, **conf) if kind == "mcra" else imcra(stft, eps, **conf)


# ---- the golden cases: name -> (kind, T, F, seed, conf) ----
CONF_D = dict(V=5, U=8, w_mcra=2)
CASES = {
    "a_mcra": ("mcra", 150, 129, 11, {}),
    "a_imcra": ("imcra", 150, 129, 11, {}),
    "b_mcra": ("mcra", 40, 257, 12, {}),
    "b_imcra": ("imcra", 40, 257, 12, {}),
    "c_mcra": ("mcra", 40, 33, 13, {}),
    "d_imcra": ("imcra", 40, 129, 14, CONF_D),
}
MIN_MARGIN = 1e-9


def synth_spectrogram(T, F, seed):
    """Speech-like bursts over a tilted noise floor: complex64 T x F."""
    rng = np.random.default_rng(seed)
    tilt = 0.05 * (1.0 + 4.0 * np.exp(-np.arange(F) / (0.15 * F)))
    drift = 1.0 + 0.3 * np.sin(2 * np.pi * np.arange(T) / 97.0)[:, None]
    x = tilt * drift * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F)))
    t = 6
    while t < T:
        dur = int(rng.integers(5, 18))
        f0 = int(rng.integers(3, max(4, F // 12)))
        amp = float(rng.uniform(0.5, 2.0))
        for h in range(1, 1 + (F - 2) // f0):
            b = h * f0
            env = amp / h**0.7 * np.hanning(dur + 2)[1:-1]
            seg = slice(t, min(T, t + dur))
            n = seg.stop - seg.start
            ph = np.exp(1j * rng.uniform(0, 2 * np.pi, n))
            x[seg, b] += env[:n] * ph
            if b + 1 < F:
                x[seg, b + 1] += 0.4 * env[:n] * ph
        t += dur + int(rng.integers(4, 14))
    return x.astype(np.complex64)


def synth_samples(num_samples, seed):
    """The time-domain counterpart for the waveform cases: float64 in (-1, 1)."""
    rng = np.random.default_rng(seed)
    n = np.arange(num_samples)
    x = 0.02 * rng.standard_normal(num_samples)
    t = 1500
    while t < num_samples:
        dur = int(rng.integers(1500, 4000))
        f0 = float(rng.uniform(110, 260))
        seg = slice(t, min(num_samples, t + dur))
        m = seg.stop - seg.start
        env = np.hanning(dur)[:m]
        for h in range(1, 12):
            x[seg] += 0.25 / h * env * np.sin(2 * np.pi * h * f0 * n[seg] / 16000.0 + rng.uniform(0, 6.28))
        t += dur + int(rng.integers(800, 2500))
    return np.clip(x, -0.99, 0.99)
