"""
Device-backed mirror of funcwj/setk ``scripts/sptk/libs/ns.py``: single-channel OM-LSA noise
suppression with MCRA (:10-209) and iMCRA (:212-387) noise tracking.

Same class names, constructor signatures and defaults; ``run(stft, eps=1e-7)`` returns the
float64 T x F gain.  The recursion runs in setk_ns_gain (libsetk_hip.so): float64 like the
reference, with the exponential integral in closed form where the reference integrates
numerically per cell.  The observations go to the device as complex64, the library's spectrogram
type (what forward_stft returns).

The smoothing windows are scipy.signal.get_window(name, 2 w + 1) with its default fftbins=True,
i.e. PERIODIC: "hann" with w = 1 is [0, 0.75, 0.75], not symmetric.  That is what the reference
convolves with, so it is kept.  They are computed here in float64 for the names libs/utils.py
evaluates itself (hann, hamming, blackman); other names are refused.

See tests/PARITY_NOTES_NS.md for what differs on purpose (digital silence under iMCRA).
"""
import numpy as np

from .. import _ffi
from .utils import _COSINE_WINDOWS, _cosine_window

MAX_HALF_WIDTH = (_ffi.NS_MAX_TAPS - 1) // 2


def smoothing_window(name, half_width):
    """scipy.signal.get_window(name, 2 * half_width + 1) (fftbins=True), float64."""
    if not isinstance(name, str) or name not in _COSINE_WINDOWS:
        raise ValueError(f"unknown window {name!r} for noise suppression: one of {sorted(_COSINE_WINDOWS)}")
    half_width = int(half_width)
    if half_width < 0:
        raise ValueError("window half width must not be negative")
    if half_width > MAX_HALF_WIDTH:
        raise _ffi.SetkUnsupported(f"smoothing window of {2 * half_width + 1} taps: at most "
                                   f"{_ffi.NS_MAX_TAPS} (w <= {MAX_HALF_WIDTH})")
    taps = 2 * half_width + 1
    return np.ones(1) if taps == 1 else _cosine_window(name, taps)


class _Suppressor(object):
    kind = None

    def opts(self, eps=1e-7, gain=True, spec=False):
        """The setk_ns_opts of this suppressor."""
        return _ffi.ns_opts(self.kind, eps=eps, gain=gain, spec=spec, **self._fields)

    def run(self, stft, eps=1e-7):
        """
        Arguments:
            stft: complex STFT, T x F
        Return:
            gain: real array, T x F (float64)
        """
        stft = np.asarray(stft)
        if stft.ndim != 2 or 0 in stft.shape or not np.iscomplexobj(stft):
            raise ValueError("run expects a complex array of shape T x F")
        T, F = stft.shape
        spec = np.ascontiguousarray(stft, dtype=np.complex64)
        gain = np.empty((T, F), dtype=np.float64)
        _ffi.default_context().ns_gain(self.opts(eps), spec, T, F, gain=gain)
        return gain


class MCRA(_Suppressor):
    """
    OM-LSA (Optimally Modified Log-Spectral Amplitude Estimator) with MCRA
    Reference:
        1) Cohen I, Berdugo B. Speech enhancement for non-stationary noise environments[J].
           Signal processing, 2001, 81(11): 2403-2418.
    """
    kind = "mcra"

    def __init__(self,
                 alpha=0.92,
                 delta=5,
                 beta=0.7,
                 alpha_s=0.9,
                 alpha_d=0.85,
                 alpha_p=0.2,
                 gmin_db=-10,
                 xi_min_db=-18,
                 w_mcra=1,
                 w_local=1,
                 w_global=15,
                 h_mcra="hann",
                 h_local="hann",
                 h_global="hann",
                 q_max=0.95,
                 zeta_min_db=-10,
                 zeta_max_db=-5,
                 zeta_p_max_db=10,
                 zeta_p_min_db=0,
                 L=125,
                 M=128):
        self._fields = dict(
            alpha=alpha, delta=delta, beta=beta, alpha_s=alpha_s, alpha_d=alpha_d, alpha_p=alpha_p,
            gmin=10**(gmin_db / 10), xi_min=10**(xi_min_db / 10),
            w_mcra=smoothing_window(h_mcra, w_mcra), w_local=smoothing_window(h_local, w_local),
            w_global=smoothing_window(h_global, w_global), q_max=q_max,
            zeta_min=10**(zeta_min_db / 10), zeta_max=10**(zeta_max_db / 10),
            zeta_p_min=10**(zeta_p_min_db / 10), zeta_p_max=10**(zeta_p_max_db / 10), L=int(L), M=int(M))


class iMCRA(_Suppressor):
    """
    OM-LSA (Optimally Modified Log-Spectral Amplitude Estimator) with iMCRA
    Reference:
        1) Cohen I. Noise spectrum estimation in adverse environments: Improved minima controlled
           recursive averaging[J]. IEEE Transactions on speech and audio processing, 2003, 11(5):
           466-475.
    """
    kind = "imcra"

    def __init__(self,
                 alpha=0.92,
                 alpha_s=0.9,
                 alpha_d=0.85,
                 b_min=1.66,
                 gamma0=4.6,
                 gamma1=3,
                 zeta0=1.67,
                 xi_min_db=-18,
                 gmin_db=-10,
                 w_mcra=1,
                 h_mcra="hann",
                 beta=1.47,
                 V=15,
                 U=8):
        self._fields = dict(
            alpha=alpha, alpha_s=alpha_s, alpha_d=alpha_d, inv_b_min=1 / b_min, gamma0=gamma0, gamma1=gamma1,
            zeta0=zeta0, xi_min=10**(xi_min_db / 10), gmin=10**(gmin_db / 10),
            w_mcra=smoothing_window(h_mcra, w_mcra), beta=beta, V=int(V), U=int(U))
