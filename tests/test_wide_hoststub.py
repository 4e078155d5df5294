"""
setk_enhance_batch(_taps) for 9 to 16 channels on the plain HIP stand-in (tools/hoststub, PLAIN=1):
kernels do nothing there, so what is checked is the front end of the wide path -- validation, the
refusals, the scratch it takes from the arena and that its launches were reached without a copy
leaving its allocation (hoststub_report).  The library is loaded in a child process because
SETK_LIB is read at import.
"""
from hoststub_case import report, run_child

HOP, F = 256, 257


def test_wide_enhance_batch_on_the_plain_stand_in():
    run_child(__file__, "wide enhance_batch on the stand-in: ok")


def _child():
    import numpy as np
    import pytest
    from setk_amd import _ffi

    ctx = _ffi.default_context()
    ctx.stft_plan(512, HOP, 512, True)
    blocks = []

    def dev(nbytes):
        blocks.append(ctx.device_alloc(max(int(nbytes), 256)))
        return blocks[-1]

    def batch(C, lengths, itf=False):
        frames = [1 + n // HOP for n in lengths]
        audio = [dev(4 * C * n) for n in lengths]
        masks = [dev(4 * t * F) for t in frames]
        itfs = [dev(4 * t * F) for t in frames] if itf else None
        waves = [dev(4 * HOP * (t - 1)) for t in frames]
        return audio, list(lengths), masks, itfs, waves

    kinds = [dict(kind=_ffi.BF_MVDR), dict(kind=_ffi.BF_GEVD, flags=_ffi.FLAG_BAN | _ffi.FLAG_POST_MASK),
             dict(kind=_ffi.BF_PMWF, pmwf_ref=-1, rank1=_ffi.RANK1_GEV), dict(kind=_ffi.BF_PMWF, pmwf_ref=3, pmwf_beta=1.0),
             dict(kind=_ffi.BF_MPDR), dict(kind=_ffi.BF_MPDR_WHITEN, flags=_ffi.FLAG_OUT_PCM16)]
    for C in (9, 12, 16):
        for k, kw in enumerate(kinds):
            a, ns, m, itf, w = batch(C, [9000, 300, 16384 + 255 * k], itf=(k in (1, 2)))
            before = report()[0]
            n = len(a)
            taps = dict(Rs=np.empty((n, F, C, C), np.complex64), Rn=np.empty((n, F, C, C), np.complex64),
                        weight=np.empty((n, F, C), np.complex64), maxabs=np.empty(n, np.float32)) if k % 2 else None
            st = ctx.enhance_batch(_ffi.BfOpts(**kw), C, a, ns, m, itf, w, want_status=True, taps=taps)
            assert st == [0] * n
            # STFT, max |audio|, covariance, its reduction, solve, beamform, iSTFT, renorm (+ taps, + select)
            assert report()[0] - before >= 8 + (3 if taps else 0), (C, k, report()[0] - before)
    # the limits of the two entry points
    a, ns, m, _, w = batch(17, [9000])
    with pytest.raises(_ffi.SetkUnsupported, match="1 <= num_channels <= 16"):
        ctx.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR), 17, a, ns, m, None, w)
    a, ns, m, itf, w = batch(12, [9000, 9100], itf=True)
    with pytest.raises(_ffi.SetkUnsupported, match="setk_pcm16_to_float_batch"):
        ctx.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_IN_PCM16), 12, a, ns, m, None, w)
    with pytest.raises(_ffi.SetkUnsupported, match="fused MPDR derives Ry"):
        ctx.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MPDR), 12, a, ns, m, itf, w)
    for which in range(4):
        lists = [list(a), list(m), list(itf), list(w)]
        lists[which][1] = 0
        # SETK_ERR_INVALID is the binding's ValueError
        with pytest.raises(ValueError, match="null utterance pointer"):
            ctx.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR), 12, lists[0], ns, lists[1], lists[2], lists[3])
    # up to 8 channels: as before
    a, ns, m, _, w = batch(8, [9000, 12000])
    assert ctx.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR), 8, a, ns, m, None, w) == [0, 0]
    for b in blocks:
        ctx.device_free(b)
    launches, violations, copies, _, first = report()
    assert violations == 0, first
    print(f"wide enhance_batch on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child()
