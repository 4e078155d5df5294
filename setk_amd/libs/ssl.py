#!/usr/bin/env python
"""
Sound Source Localization (SSL) on the MI355X: the call surface of funcwj/setk
``scripts/sptk/libs/ssl.py`` (ml_ssl / srp_ssl / music_ssl, same signatures and return values) on
top of ``setk_ssl_scores``.  ``ssl_spectrum`` is the general form: the score spectrum of every
window of frames as well as the index, which the command line's online mode and
``engine.BatchLocalizer`` use.
"""
import warnings

import numpy as np

from .. import _ffi
from .._ffi import SetkUnsupported

MAX_CHANNELS = 16


def ssl_spectrum(backend, stft, sv, mask=None, srp_pair=None, windows=None, compression=0, eps=1e-8,
                 norm=False, ctx=None):
    """
    Arguments:
        backend: "ml" | "srp" | "music"
        stft: M x T x F (complex), sv: A x M x F (complex), mask: T x F or None
        windows: list of frame ranges (t0, t1), None: the whole utterance
    Return:
        index (W, int64), score (W x A, float64), status (SETK_NUM_*: MUSIC's eigen-solves)
    """
    stft, sv = np.asarray(stft), np.asarray(sv)
    if stft.ndim != 3 or sv.ndim != 3 or 0 in stft.shape or 0 in sv.shape:
        raise ValueError("expect stft in M x T x F and sv in A x M x F")
    M, T, F = stft.shape
    A = sv.shape[0]
    if sv.shape[1:] != (M, F):
        raise ValueError(f"steer vector {sv.shape} does not match the spectrogram {stft.shape}")
    if M > MAX_CHANNELS:
        raise SetkUnsupported(f"SSL on the device needs 1 <= channels <= {MAX_CHANNELS} (got {M} channels)")
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.float32)
        if mask.shape != (T, F):
            raise ValueError(f"mask {mask.shape} does not match the spectrogram {stft.shape}")
    opts = _ffi.ssl_opts(backend, srp_pair=srp_pair, compression=compression, eps=eps, norm=norm)
    W = 1 if windows is None else len(windows)
    score = np.empty((W, A), dtype=np.float64)
    index = np.empty(W, dtype=np.int32)
    status = np.zeros(1, dtype=np.int32)
    ctx = ctx or _ffi.default_context()
    ctx.ssl_scores(opts, np.ascontiguousarray(stft, dtype=np.complex64), mask,
                   np.ascontiguousarray(sv, dtype=np.complex64), A, M, T, F, windows, score, index, status=status)
    return index.astype(np.int64), score, int(status[0])


def ml_ssl(stft, sv, compression=0, eps=1e-8, norm=False, mask=None):
    """
    Maximum likelihood SSL
    Arguments:
        stft: STFT transform result, M x T x F
        sv: steer vector in each directions, A x M x F
        norm: normalze STFT or not
        mask: TF-mask for source, T x F, or N x T x F (then N indices come back)
    Return:
        index: DoA index
    """
    kw = dict(compression=compression, eps=eps, norm=norm)
    if mask is not None and np.ndim(mask) == 3:
        return np.array([ssl_spectrum("ml", stft, sv, mask=m, **kw)[0][0] for m in mask])
    return ssl_spectrum("ml", stft, sv, mask=mask, **kw)[0][0]


def srp_ssl(stft, sv, srp_pair=None, mask=None):
    """
    Do SRP-PHAT based SSL
    Arguments:
        stft: STFT transform result, M x T x F
        sv: steer vector in each directions, A x M x F
        srp_pair: index pair to compute srp response
        mask: TF-mask for source, T x F
    Return:
        index: DoA index
    """
    if srp_pair is None:
        raise ValueError("srp_pair cannot be None, (list, list)")
    return ssl_spectrum("srp", stft, sv, mask=mask, srp_pair=srp_pair)[0][0]


def music_ssl(stft, sv, mask=None):
    """
    Do MUSIC based SSL
    Arguments:
        stft: STFT transform result, M x T x F
        sv: steer vector in each directions, A x M x F
        mask: TF-mask for source, T x F
    Return:
        index: DoA index
    """
    index, _, status = ssl_spectrum("music", stft, sv, mask=mask)
    if status != _ffi.NUM_OK:
        # (numpy's eigh goes through on such a bin with an arbitrary basis)
        warnings.warn(f"music_ssl: eigen-solve status {status} in some bin (zero or non-finite covariance)")
    return index[0]
