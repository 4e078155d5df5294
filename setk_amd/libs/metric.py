"""
Device-backed mirror of funcwj/setk ``scripts/sptk/libs/metric.py``:

    si_snr(x, s, eps=1e-8, remove_dc=True)             (:13-33)
    permute_si_snr(xlist, slist, align=False)          (:36-60)

Same signatures and defaults; they return Python floats and, with align, the order as a tuple.
The sums run in float64 on the float32 samples (the reference computes in float32), in
setk_si_snr / setk_si_snr_batch of libsetk_hip.so; the K! orders are walked on the device in
``itertools.permutations``' order with the reference's own additions, so the order returned is what
``np.argmax`` picks from the same table, ties included.  ``permute_ed`` raises: see
PERMUTE_ED_REASON.
"""
import numpy as np

from .. import _ffi

PERMUTE_ED_REASON = ("permute_ed is not ported: it is editdistance.eval over token lists, and the "
                     "editdistance package is not available to this project")

_engines = {}


def _vector(v, name):
    v = np.ascontiguousarray(v, dtype=np.float32)
    if v.ndim != 1:
        raise ValueError(f"{name}: a vector of samples, got shape {v.shape}")
    return v


def si_snr(x, s, eps=1e-8, remove_dc=True):
    """Si-SNR of the enhanced / separated vector x against the reference vector s."""
    x, s = _vector(x, "x"), _vector(s, "s")
    if x.size != s.size:
        raise ValueError(f"x and s differ in length: {x.size} vs {s.size}")
    return _ffi.default_context().si_snr(x, s, eps=eps, flags=0 if remove_dc else _ffi.FLAG_KEEP_DC)


def permute_si_snr(xlist, slist, align=False):
    """The best average Si-SNR over the assignments of the N estimates to the N references; with
    align also the order: estimate n belongs to reference order[n]."""
    N = len(xlist)
    if N != len(slist):
        raise RuntimeError("size do not match between xlist " + f"and slist: {N} vs {len(slist)}")
    from ..engine.metric import BatchSiSnr
    ctx = _ffi.default_context()
    if ctx.device not in _engines:
        _engines[ctx.device] = BatchSiSnr(device=ctx.device)
    best, order, _, _ = _engines[ctx.device].score([([_vector(x, "x") for x in xlist],
                                                     [_vector(s, "s") for s in slist])])[0]
    return (best, order) if align else best


def permute_ed(hlist, rlist):
    raise _ffi.SetkUnsupported(PERMUTE_ED_REASON)
