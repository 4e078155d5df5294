"""
Device-backed mirror of funcwj/setk ``scripts/sptk/libs/spatial.py``:

    linear_tdoa_grid(dist, ...)                                    (:11-34, host, float64)
    gcc_phat_linear(si, sj, dij, ...)                              (:37-57)
    gcc_phat_diag(si, sj, angle_delta, d, ...)                     (:60-92)
    srp_phat_linear(S, d, ...)                                     (:95-123)
    ipd(si, sj, cos=False, sin=False)                              (:163-181)
    directional_feats(spectrogram, steer_vector, df_pair=None)     (:184-208)

Same signatures, defaults, error messages and shapes as the reference; results are float32.  The
kernels are setk_spatial_feats and setk_directional_feats in libsetk_hip.so.  The SRP tables
exp(-i omega tau) are computed here in float64 exactly as the reference does and rounded once to
complex64 (omega tau reaches about 117 rad: not a float32 computation).  ``msc`` raises: see
MSC_REASON.  ``ipd_feats``, ``srp_feats``, ``geometry_df`` and the ``*_srp_tables`` helpers are what
the three command lines and engine.BatchSpatialFeatures share: several pairs / directions in one call.
"""
import numpy as np

from .. import _ffi


def directional_feats(spectrogram, steer_vector, df_pair=None):
    """mean over microphone pairs of cos((arg X_i - arg X_j) - (arg v_i - arg v_j));
    spectrogram M x F x T, steer_vector M x F  ->  T x F float32."""
    spectrogram = np.asarray(spectrogram)
    steer_vector = np.asarray(steer_vector)
    M, F, T = spectrogram.shape
    if steer_vector.shape != (M, F):
        raise ValueError(f"steer_vector {steer_vector.shape} does not match spectrogram "
                         f"{spectrogram.shape}")
    if df_pair is None:
        df_pair = [(i, j) for i in range(M) for j in range(i + 1, M)]
    if not len(df_pair):
        raise ValueError("no microphone pair given")
    spec = np.ascontiguousarray(np.transpose(spectrogram, (0, 2, 1)), dtype=np.complex64)
    sv = np.ascontiguousarray(np.transpose(steer_vector), dtype=np.complex64)  # F x M
    out = np.empty((T, F), dtype=np.float32)
    _ffi.default_context().directional_feats(spec, sv, [tuple(p) for p in df_pair], M, T, F, out)
    return out


MSC_REASON = ("MSC is not ported: the reference's msc() adds the scalar N*T*F to every cell before it "
              "normalises (np.sum without an axis, libs/spatial.py:154), so its output is constant to "
              "float32 precision and NaN as soon as one bin is silent")


def msc(spectrogram, context=1, normalize=True):
    raise _ffi.SetkUnsupported(MSC_REASON)


def linear_tdoa_grid(dist, speed=343, num_bins=513, samp_doa=True, sample_frequency=16000, num_doa=181,
                     max_doa=np.pi):
    """T_{ij} = exp(-i omega_i tau_j), F x D complex128 (host)."""
    dist = np.abs(dist)  # make sure >= 0
    if samp_doa:
        tau = np.cos(np.linspace(0, max_doa, num_doa)) * dist / speed
    else:
        max_tdoa = dist / speed
        tau = np.linspace(max_tdoa, -max_tdoa, num_doa)
    omega = np.linspace(0, sample_frequency / 2, num_bins) * 2 * np.pi
    return np.exp(-1j * np.outer(omega, tau))


def diag_tdoa_grid(angle_delta, d, speed=343, num_doas=121, sr=16000, num_bins=513):
    """The transform of gcc_phat_diag (:78-83), F x D complex128 (host)."""
    tau = np.cos(angle_delta - np.linspace(0, np.pi * 2, num_doas)) * d / speed
    omega = np.linspace(0, sr / 2, num_bins) * 2 * np.pi
    return np.exp(-1j * np.outer(omega, tau))


def pack_srp_table(grids):
    """P grids F x D (complex128) -> [P][F][Dpad] complex64, zero beyond D: setk_spatial_opts.table."""
    grids = [np.asarray(g) for g in grids]
    F, D = grids[0].shape
    table = np.zeros((len(grids), F, _ffi.spatial_dpad(D)), dtype=np.complex64)
    for p, g in enumerate(grids):
        if g.shape != (F, D):
            raise ValueError("SRP grids of different shapes")
        table[p, :, :D] = g
    return table


def linear_srp_tables(topo, num_bins, **kwargs):
    """srp_phat_linear's pairs, table and pair weights for a linear topology (:115-123)."""
    N = len(topo)
    if N == 2:
        pairs, weight = [(0, 1)], [1.0]
    else:
        pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
        weight = [2.0 / (N * (N - 1))] * len(pairs)
    grids = [linear_tdoa_grid(topo[j] - topo[i], num_bins=num_bins, **kwargs) for i, j in pairs]
    return pairs, pack_srp_table(grids), weight


def circular_srp_tables(diag_pair, n, d, num_bins, sr=16000, num_doas=121):
    """compute_circular_srp.py:42-51: the diagonal pairs, their table and the weights of the mean."""
    pairs = [(int(i), int(j)) for i, j in diag_pair]
    grids = [diag_tdoa_grid(min(i, j) * np.pi * 2 / n, d, num_bins=num_bins, sr=sr, num_doas=num_doas)
             for i, j in pairs]
    return pairs, pack_srp_table(grids), [1.0 / len(pairs)] * len(pairs)


def _spec(S):
    S = np.ascontiguousarray(S, dtype=np.complex64)
    if S.ndim != 3:
        raise ValueError(f"expected a C x T x F spectrogram, got {S.shape}")
    return S


def _feats(opts, S):
    C, T, F = S.shape
    out = np.empty((T, _ffi.spatial_width(opts, F)), dtype=np.float32)
    _ffi.default_context().spatial_feats(opts, S, C, T, F, out)
    return out


def srp_feats(S, pairs, table, weight, num_doas):
    """S C x T x F -> T x D: sum_p weight_p floor(normalise(Re u_p W_p))."""
    S = _spec(S)
    if table.shape[1] != S.shape[2]:
        raise ValueError(f"SRP table of {table.shape[1]} bins against a spectrogram of {S.shape[2]}")
    return _feats(_ffi.spatial_opts("srp", pairs, table=table, num_doas=num_doas, pair_weight=weight), S)


def ipd_feats(S, pairs, cos=False, sin=False):
    """S C x T x F -> ipd() of every pair side by side (compute_ipd_and_linear_srp.py:36-47)."""
    kind = "ipd" if not cos else ("cos_sin_ipd" if sin else "cos_ipd")
    return _feats(_ffi.spatial_opts(kind, pairs), _spec(S))


def geometry_df(S, steer_vector, idx, df_pair):
    """S M x T x F, steer_vector A x M x F, idx a list of directions -> T x (len(idx) F), laid out
    as compute_df_on_geometry.py:49-60 does."""
    S = _spec(S)
    sv = np.ascontiguousarray(steer_vector, dtype=np.complex64)
    if sv.ndim != 3 or sv.shape[1:] != (S.shape[0], S.shape[2]):
        raise ValueError(f"steer_vector {sv.shape} does not match spectrogram {S.shape}")
    return _feats(_ffi.spatial_opts("df", df_pair, steer_vector=sv, num_sv=sv.shape[0], doa_index=[list(idx)]), S)


def _unsupported_switch(normalize, apply_floor):
    if not normalize or not apply_floor:
        raise _ffi.SetkUnsupported("the device SRP spectrum is normalised and floored (the reference's "
                                   "defaults, which its command lines never change)")


def gcc_phat_linear(si, sj, dij, normalize=True, apply_floor=True, **kwargs):
    """GCC-PHAT for a linear array: si, sj T x F, dij the distance -> T x D."""
    _unsupported_switch(normalize, apply_floor)
    grid = linear_tdoa_grid(dij, **kwargs)
    return srp_feats(np.stack([si, sj]), [(0, 1)], pack_srp_table([grid]), [1.0], grid.shape[1])


def gcc_phat_diag(si, sj, angle_delta, d, speed=343, num_doas=121, sr=16000, normalize=True, num_bins=513,
                  apply_floor=True):
    """GCC-PHAT between diagonal microphones of a circular array of diameter d -> T x D."""
    _unsupported_switch(normalize, apply_floor)
    grid = diag_tdoa_grid(angle_delta, d, speed=speed, num_doas=num_doas, sr=sr, num_bins=num_bins)
    return srp_feats(np.stack([si, sj]), [(0, 1)], pack_srp_table([grid]), [1.0], num_doas)


def srp_phat_linear(S, d, normalize=True, apply_floor=True, **kwargs):
    """SRP-PHAT for a linear array: S N x T x F, d the topology (list / tuple) -> T x D."""
    if type(d) is not list and type(d) is not tuple:
        raise ValueError("Now only support linear arrays(in python list/tuple type)")
    S = np.asarray(S)
    N = S.shape[0]
    if N != len(d):
        raise ValueError("{:d} microphones available, while get {:d}-channel STFT".format(len(d), N))
    if S.ndim == 2:
        raise ValueError("Only one-channel STFT available")
    if N > 2:  # (the two-microphone return takes gcc_phat_linear's own defaults, :115-117)
        _unsupported_switch(normalize, apply_floor)
    kwargs.setdefault("num_bins", 513)
    pairs, table, weight = linear_srp_tables(d, **kwargs)
    return srp_feats(S, pairs, table, weight, kwargs.get("num_doa", 181))


def ipd(si, sj, cos=False, sin=False):
    """IPD (wrapped into [-pi, pi)), cosIPD (cos=True) or [cosIPD, sinIPD] (sin=True): si, sj T x F."""
    return ipd_feats(np.stack([si, sj]), [(0, 1)], cos=cos, sin=sin)
