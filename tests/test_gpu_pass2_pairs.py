"""
Stage 3 walks the frames of a wave in pairs (pass2_mc.hip: one paired transform per channel
and group, one paired tail per group).  What must not depend on how frames fall into pairs:
the waveform against the oracle on shapes whose waves get odd and even frame counts, lead-in
frames, trailing half groups and no frames at all; the waveform's bits under a different cut
of the work list (SETK_MC_P2_ITEMS); and the 16-bit PCM input form against the float32 one.
All at hop 256 (the only hop the matrix-core pass 2 serves).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rms
from oracle import np_oracle as o

pytestmark = pytest.mark.gpu

# (C, N) -> T = 274, 274, 274, 75, 36, 12 frames with centre on.  274: the eight (sixteen) waves of
# a workgroup get odd and even counts, a lead-in frame and a trailing half group; 12: waves
# without a frame; C = 3, 1: the masked columns of the odd-family tile of two frames.
SHAPES = [(8, 70000), (3, 70000), (1, 70000), (8, 19000), (8, 9001), (8, 2900)]
BATCH = [70000, 19000, 2900]


@functools.lru_cache(maxsize=None)
def case(C, N):
    """(mix C x N, mask T x F) of one synthetic utterance, computed once per module run."""
    mix, sp, nz = o.synth_utterance(900 + 7 * C + N % 13, C, N, return_parts=True)
    return np.ascontiguousarray(mix, dtype=np.float32), o.irm_mask(sp, nz)


@functools.lru_cache(maxsize=None)
def oracle_wave(C, N, post_mask=False):
    mix, mask = case(C, N)
    return o.enhance_utterance(mix, mask, kind="mvdr", gauge=True, post_mask=post_mask)


def new_ctx(center=True):
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, 256, 512, center)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    c.close()


def enhance_f32(c, utts, masks, flags=None):
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    C = utts[0].shape[0]
    a = [torch.from_numpy(np.ascontiguousarray(u)).to(dev) for u in utts]
    m = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in masks]
    ns = [u.shape[1] for u in utts]
    outs = [torch.empty(c.istft_num_samples(c.num_frames(n)), dtype=torch.float32, device=dev) for n in ns]
    opts = _ffi.BfOpts(kind=0, flags=_ffi.FLAG_CLAMP_MASK if flags is None else flags)
    st = c.enhance_batch(opts, C, [t.data_ptr() for t in a], ns, [t.data_ptr() for t in m], None,
                         [t.data_ptr() for t in outs])
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], st


def enhance_pcm(c, frames, masks):
    """frames: int16 [N][C] arrays, de-interleaved on the device and enhanced with FLAG_IN_PCM16."""
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    C = frames[0].shape[1]
    ns = [f.shape[0] for f in frames]
    src = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    planar = [torch.zeros((C, c.pcm16_channel_stride(n)), dtype=torch.int16, device=dev) for n in ns]
    c.pcm16_deinterleave_batch(C, [t.data_ptr() for t in src], ns, [t.data_ptr() for t in planar])
    m = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in masks]
    outs = [torch.empty(c.istft_num_samples(c.num_frames(n)), dtype=torch.float32, device=dev) for n in ns]
    opts = _ffi.BfOpts(kind=0, flags=_ffi.FLAG_CLAMP_MASK | _ffi.FLAG_IN_PCM16)
    st = c.enhance_batch(opts, C, [t.data_ptr() for t in planar], ns, [t.data_ptr() for t in m], None,
                         [t.data_ptr() for t in outs])
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], st


def batch(C, center):
    """The ragged batch of BATCH lengths: (utterances, masks).  Centre on: the oracle's IRM masks;
    centre off: seeded uniform masks of the plan's frame count."""
    if center:
        pairs = [case(C, n) for n in BATCH]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    utts, masks = [], []
    for i, n in enumerate(BATCH):
        utts.append(case(C, n)[0])
        T = (n - 512) // 256 + 1
        masks.append((0.1 + 0.8 * np.random.default_rng(40 + i).random((T, 257))).astype(np.float32))
    return utts, masks


@pytest.mark.parametrize("C,N", SHAPES)
def test_paired_frames_match_oracle(ctx, C, N):
    """MVDR, gauge fixed, centre on, the project's bar rms(wav - ref) / rms(ref) < 1e-3."""
    mix, mask = case(C, N)
    assert ctx.num_frames(N) == {70000: 274, 19000: 75, 9001: 36, 2900: 12}[N]
    (wav,), st = enhance_f32(ctx, [mix], [mask])
    ref = oracle_wave(C, N)
    assert st == [0] and wav.shape == ref.shape
    err = rms(wav, ref) / rms(ref)
    print(f"C={C} N={N}: rel rms {err:.3e}")
    assert err < 1e-3, err


@pytest.mark.parametrize("C,N", [(8, 19000), (3, 2900)])
def test_paired_frames_match_oracle_with_post_mask(ctx, C, N):
    """The post-mask multiplies both frames' spectra (and the odd family of each frame in its
    half of the tile's columns) by their own mask rows: the same bar."""
    from setk_amd import _ffi
    mix, mask = case(C, N)
    (wav,), st = enhance_f32(ctx, [mix], [mask], flags=_ffi.FLAG_CLAMP_MASK | _ffi.FLAG_POST_MASK)
    ref = oracle_wave(C, N, True)
    assert st == [0] and wav.shape == ref.shape
    err = rms(wav, ref) / rms(ref)
    print(f"post-mask C={C} N={N}: rel rms {err:.3e}")
    assert err < 1e-3, err


@pytest.mark.parametrize("C,center", [(8, True), (3, False)])
def test_work_list_cut_does_not_change_a_bit(monkeypatch, C, center):
    """SETK_MC_P2_ITEMS (read when the handle is created) moves the frame ranges of pass 2's
    work items, and with them which frames share a pair, which are lead-ins and which groups
    are half empty.  Pass 1's cut does not depend on it, so the weights are the same and the
    waveforms must be bit-identical.  Centre off: finiteness and bit-identity only."""
    utts, masks = batch(C, center)
    got = {}
    for items in ("1", "3", None):
        if items is None:
            monkeypatch.delenv("SETK_MC_P2_ITEMS", raising=False)
        else:
            monkeypatch.setenv("SETK_MC_P2_ITEMS", items)
        c = new_ctx(center)
        try:
            got[items], st = enhance_f32(c, utts, masks)
        finally:
            c.close()
        assert st == [0] * len(utts), (items, st)
        assert all(np.isfinite(w).all() for w in got[items])
    for items in ("1", "3"):
        for i, n in enumerate(BATCH):
            assert np.array_equal(got[items][i], got[None][i]), (items, n, rms(got[items][i], got[None][i]))
    if center:
        ref = oracle_wave(C, BATCH[0])
        assert rms(got[None][0], ref) / rms(ref) < 1e-3


@pytest.mark.parametrize("C,center", [(8, True), (3, False)])
def test_pcm16_pairs_are_the_float_pairs_bit_for_bit(C, center):
    """16-bit PCM input (the group's last half frame carried through LDS) against the float32
    call on pcm / 32768: the scale is a power of two folded into the window rows, so the
    waveforms are equal bit for bit -- on the same ragged batches."""
    utts, masks = batch(C, center)
    frames = [np.ascontiguousarray(np.clip(np.rint(u.T * 32767.0 * 4.0), -32768, 32767).astype(np.int16)) for u in utts]
    floats = [np.ascontiguousarray(f.T.astype(np.float32) / 32768.0) for f in frames]
    c = new_ctx(center)
    try:
        ys, st = enhance_pcm(c, frames, masks)
        yf, stf = enhance_f32(c, floats, masks)
    finally:
        c.close()
    assert st == [0] * len(utts) and stf == st
    for i, n in enumerate(BATCH):
        assert np.isfinite(yf[i]).all()
        assert np.array_equal(ys[i], yf[i]), (C, n, rms(ys[i], yf[i]) / rms(yf[i]))
