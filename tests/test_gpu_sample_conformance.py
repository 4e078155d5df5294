"""
Sample I/O conformance on the device, sample by sample (cases and references: sample_cases.py;
figures: PARITY_NOTES_SAMPLES.md).  Everything goes through _ffi.Context and the engines on device
tensors; every test prints its figures before it asserts.

  a. setk_float_to_pcm16 on the quantiser family against the exact integer reference
  b. the renorm's float output (setk_istft with norm) against the numpy float32 statement, bit for bit
  c. the renorm's 16-bit output in every consumer of scale_kernel: pcm == wavio.float_to_pcm16 of the
     same call's float output
  d. a public path past full scale: the 16-bit output wraps as the rule says
  e. the ingest operators: every channel count, ragged lengths, three pointer alignments, sentinels
     around every destination, power0 against its derived bound
  f. 16-bit frames through BatchEnhancer against the same samples as float32, 1 to 16 channels
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import auxiva_model  # noqa: E402
import sample_cases as sm  # noqa: E402
from oracle import np_oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu
F = 257
STFT_KW = dict(frame_len=512, frame_hop=256, window="hann", center=True)


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, 256, 512, True)
    yield c
    c.close()


def dev():
    import torch
    return torch.device("cuda:0")


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def sync():
    import torch
    torch.cuda.synchronize()


class Guarded:
    """A destination of `size` elements inside a larger tensor filled with a sentinel.  The view
    starts 16 bytes in (so it is as aligned as an allocation) plus `offset` elements."""

    def __init__(self, size, dtype, sentinel, offset=0):
        import torch
        self.lead = 16 // torch.empty(0, dtype=dtype).element_size() + offset
        self.size, self.sentinel = size, sentinel
        self.whole = torch.full((self.lead + size + 16,), sentinel, dtype=dtype, device=dev())
        self.view = self.whole[self.lead:self.lead + size]

    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        """The destination as numpy, after checking that nothing around it changed."""
        w = self.whole.cpu().numpy()
        assert (w[:self.lead] == self.sentinel).all() and (w[self.lead + self.size:] == self.sentinel).all(), \
            "written outside the destination"
        return w[self.lead:self.lead + self.size].copy()


# ---------------------------------------------------------------- a. the stand-alone quantiser
@pytest.mark.parametrize("C", [1, 3, 8])
def test_float_to_pcm16_is_the_exact_rule(ctx, C):
    import torch
    N = sm.quantiser_family()[0].size
    assert N % 256 != 0
    audio, want = sm.family_rows(C, N)
    out = Guarded(N * C, torch.int16, 12345)
    ctx.float_to_pcm16(to_dev(audio), C, N, out.view)
    sync()
    got = out.result().reshape(N, C)
    bad = np.argwhere(got != want)
    print(f"setk_float_to_pcm16 C={C} N={N}: {len(bad)} of {got.size} samples differ from the exact rule")
    for n, c in bad[:10]:
        print(f"  frame {n} channel {c}: x = {float(audio[c, n])!r} -> {got[n, c]}, exact {want[n, c]}")
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- b. renorm, float output
NORMS = np.array([0.9, 0.25, 0.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def small_spectrograms():
    rng = np.random.default_rng(77)
    spec = (rng.standard_normal((3, 9, F)) + 1j * rng.standard_normal((3, 9, F))).astype(np.complex64)
    spec[..., 0].imag = 0
    spec[..., -1].imag = 0
    spec *= np.array([1.0, 40.0, 1e-3], dtype=np.float32)[:, None, None]   # (three different maxima)
    return spec


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-one-float"])
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_renorm_float_output_is_the_float32_statement(ctx, tail, offset):
    """setk_istft: norm=None gives the raw wave and its maximum; norm = [0.9, 0.25, 0] must give
    float32(raw * sc) bit for bit, sc = float32(norm) / (float32(max) + 2^-23), and the raw wave
    where norm = 0.  L % 4 = tail runs the scalar tail of the 16-byte path (and leaves items 1 and
    2 of the batch unaligned); the offset tensor runs the scalar path for every item."""
    import torch
    B, T = 3, 9
    nsamps = next(n for n in range(2048, 2040, -1) if ctx.istft_num_samples(T, n) % 4 == tail)
    L = ctx.istft_num_samples(T, nsamps)
    assert L % 4 == tail and L > 1024
    spec = to_dev(small_spectrograms())
    waves = {}
    for name, norm in (("raw", None), ("scaled", NORMS)):
        out = Guarded(B * L, torch.float32, -777.25, offset)
        assert out.ptr() % 16 == 4 * offset
        ctx.istft(spec, B, T, nsamps, norm, out.view)
        sync()
        waves[name] = out.result().reshape(B, L)
    raw, got = waves["raw"], waves["scaled"]
    assert np.isfinite(raw).all()
    for b in range(B):
        omax = np.abs(raw[b]).max()
        choices = sm.renorm_scale_neighbours(NORMS[b], omax) if NORMS[b] > 0 else [np.float32(1)]
        hits = [i for i, sc in enumerate(choices)
                if np.array_equal(sm.renorm_f32(raw[b], NORMS[b], omax, sc).view(np.uint32), got[b].view(np.uint32))]
        differ = np.count_nonzero(sm.renorm_f32(raw[b], NORMS[b], omax).view(np.uint32) != got[b].view(np.uint32))
        print(f"renorm float L={L} (L % 4 = {tail}) offset={offset} item {b} norm={NORMS[b]} max={omax!r}: "
              f"{differ} of {L} samples differ in bits from the statement; sc candidates that match "
              f"(0 = the correctly rounded quotient, 1 / 2 = its lower / upper neighbour): {hits}")
        # the device's float32 division is correctly rounded under this build's flags: the
        # statement's own sc, no neighbour (PARITY_NOTES_SAMPLES.md, "the division")
        assert hits and hits[0] == 0, (b, hits, differ)
    assert np.array_equal(got[2].view(np.uint32), raw[2].view(np.uint32))


# ---------------------------------------------------------------- c. renorm, 16-bit output
PEAK = 0.95
LENS = (16384, 9003)     # a ragged batch of two; 9003: odd, L % 4 != 0 after the transform


def white(seed, C, n, peak=PEAK):
    """Independent uniform noise per channel (a full-rank covariance in every bin), max |x| = peak."""
    x = (np.random.default_rng(seed).uniform(-1, 1, (C, n)) * peak).astype(np.float32)
    x[C // 2, n // 3] = np.float32(peak)
    return x


def mask_for(ctx, seed, n):
    return np.random.default_rng(seed).uniform(0.2, 0.8, (ctx.num_frames(n), F)).astype(np.float32)


def out_len(ctx, n):
    return ctx.istft_num_samples(ctx.num_frames(n))


class Consumer:
    """One caller of scale_kernel: call(flags, wave pointers) on inputs that stay on the device;
    rows: how many waves of out_len(n) samples an utterance's output holds."""
    rows = 1

    def __init__(self, ctx, lens):
        self.ctx, self.lens = ctx, list(lens)


class Fused(Consumer):
    def __init__(self, ctx, lens, C):
        super().__init__(ctx, lens)
        self.C = C
        self.audio = [to_dev(white(100 * C + i, C, n)) for i, n in enumerate(lens)]
        self.masks = [to_dev(mask_for(ctx, 200 * C + i, n)) for i, n in enumerate(lens)]

    def call(self, flags, waves):
        from setk_amd import _ffi
        st = self.ctx.enhance_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK | flags), self.C,
                                    [t.data_ptr() for t in self.audio], self.lens,
                                    [t.data_ptr() for t in self.masks], None, waves)
        assert st == [0] * len(self.lens), st


class Fixed(Consumer):
    """setk_apply_weights_batch; audio (C x n arrays), the weight table [sets][257][C] and the set of
    every utterance may be given, otherwise white noise under two random sets."""

    def __init__(self, ctx, lens, C=4, audio=None, w=None, pick=None):
        super().__init__(ctx, lens)
        self.C = C
        if w is None:
            rng = np.random.default_rng(31)
            w = (rng.standard_normal((2, F, C)) + 1j * rng.standard_normal((2, F, C))).astype(np.complex64)
        self.w = np.ascontiguousarray(w, dtype=np.complex64)
        self.pick = [i % self.w.shape[0] for i in range(len(lens))] if pick is None else list(pick)
        audio = [white(300 + i, C, n) for i, n in enumerate(lens)] if audio is None else audio
        self.audio = [to_dev(x) for x in audio]

    def call(self, flags, waves):
        self.ctx.apply_weights_batch(self.C, [t.data_ptr() for t in self.audio], self.lens, self.w, self.w.shape[0],
                                     self.pick, waves, flags=flags)


class Online(Fused):
    def call(self, flags, waves):
        from setk_amd import _ffi
        st = np.full(len(self.lens), -1, dtype=np.int32)
        self.ctx.enhance_online_batch(_ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK | flags, pmwf_ref=-1),
                                      32, 0.8, self.C, [t.data_ptr() for t in self.audio], self.lens,
                                      [t.data_ptr() for t in self.masks], None, waves, status=st)
        assert not st.any(), st


class Auxiva(Consumer):
    rows = 2

    def __init__(self, ctx, lens):
        super().__init__(ctx, lens)
        scenes = [auxiva_model.synth_scene(400 + i, 2, n) for i, n in enumerate(lens)]
        self.audio = [to_dev((s * (PEAK / np.abs(s).max())).astype(np.float32)) for s in scenes]

    def call(self, flags, waves):
        st = np.full(len(self.lens), -1, dtype=np.int32)
        self.ctx.auxiva_batch(2, [t.data_ptr() for t in self.audio], self.lens, 3, waves, status=st, flags=flags)
        assert not st.any(), st


class TfSeparate(Consumer):
    def __init__(self, ctx, lens):
        super().__init__(ctx, lens)
        self.audio = [to_dev(white(500 + i, 1, n)[0]) for i, n in enumerate(lens)]
        self.masks = [to_dev(np.random.default_rng(600 + i).uniform(0, 1, (ctx.num_frames(n), F)).astype(np.float32))
                      for i, n in enumerate(lens)]

    def call(self, flags, waves):
        st = np.full(len(self.lens), -1, dtype=np.int32)
        self.ctx.tf_separate_batch([t.data_ptr() for t in self.audio], self.lens, [t.data_ptr() for t in self.masks],
                                   waves, norm=[PEAK] * len(self.lens), status=st, flags=flags)
        assert not st.any(), st


CONSUMERS = {
    "fused-4ch": lambda c, lens: Fused(c, lens, 4),
    "fused-12ch": lambda c, lens: Fused(c, lens, 12),
    "fixed": Fixed,
    "online": lambda c, lens: Online(c, lens, 4),
    "auxiva-2src": Auxiva,
    "tf-separate": TfSeparate,
}


def float_and_pcm(consumer, offset, extra_flags=0):
    """The consumer's float output and its 16-bit output on the same inputs: two calls.  offset: the
    16-bit destinations start one sample past a 16-byte boundary (2-byte aligned only)."""
    import torch
    from setk_amd import _ffi
    sizes = [consumer.rows * out_len(consumer.ctx, n) for n in consumer.lens]
    f32 = [Guarded(s, torch.float32, -777.25) for s in sizes]
    consumer.call(extra_flags, [g.ptr() for g in f32])
    sync()
    i16 = [Guarded(s, torch.int16, 12345, offset) for s in sizes]
    assert all(g.ptr() % 16 == 2 * offset for g in i16)
    consumer.call(extra_flags | _ffi.FLAG_OUT_PCM16, [g.ptr() for g in i16])
    sync()
    return [g.result() for g in f32], [g.result() for g in i16]


def differing(pcm, flt):
    from setk_amd.libs.wavio import float_to_pcm16
    want = float_to_pcm16(flt)
    d = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
    return int(np.count_nonzero(d)), int(d.max()), want


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-one-sample"])
@pytest.mark.parametrize("name", list(CONSUMERS))
def test_pcm16_output_is_the_host_writers_rule(ctx, name, offset):
    """Every SETK_FLAG_OUT_PCM16 output equals wavio.float_to_pcm16 of the same call's float output,
    sample for sample; input peak 0.95 (the renorm restores it), 16 384 samples and a shorter
    second utterance, the 16-bit destinations once 16-byte and once 2-byte aligned."""
    flt, pcm = float_and_pcm(CONSUMERS[name](ctx, LENS), offset)
    total = 0
    for u, (f, q) in enumerate(zip(flt, pcm)):
        assert np.isfinite(f).all() and abs(float(np.abs(f).max()) - PEAK) < 1e-3, float(np.abs(f).max())
        n, worst, want = differing(q, f)
        total += n
        print(f"{name} offset={offset} utterance {u} ({f.size} samples, peak {np.abs(f).max():.4f}): "
              f"{n} samples differ from float_to_pcm16(float output), largest step {worst}")
    assert total == 0
    for f, q in zip(flt, pcm):
        assert np.array_equal(q, differing(q, f)[2])


def test_pcm16_output_long_enough_to_tell_the_rules_apart(ctx):
    """The 4-channel fused call at 480 000 samples: quantising the float32 product instead
    (rintf(src * sc * 32767.f)) differs on about 2e-4 of the samples -- about a hundred here.
    Seen failing on the kernel before it took this rule: 104 samples (PARITY_NOTES_SAMPLES.md)."""
    flt, pcm = float_and_pcm(Fused(ctx, [480000], 4), 0)
    n, worst, want = differing(pcm[0], flt[0])
    print(f"fused 4ch, {flt[0].size} samples, peak {np.abs(flt[0]).max():.4f}: {n} samples differ from "
          f"float_to_pcm16(float output), largest step {worst}; the float32-product rule on the same float "
          f"output would differ on {np.count_nonzero(sm.f32_product_pcm16(flt[0]) != want)}")
    assert np.array_equal(pcm[0], want)


# ---------------------------------------------------------------- d. past full scale
def test_pcm16_output_wraps_past_full_scale(ctx):
    """setk_apply_weights_batch with one-hot weights and SETK_FLAG_NO_RENORM hands a channel through
    (forward and inverse transform, no scaling).  Input uniform in (-2, 2): the float64 model of the
    round trip has thousands of samples past +-1, the float output must have them too, and the
    16-bit output must be the rule's wrap of it (exact integer reference and host writer alike)."""
    from setk_amd import _ffi
    from setk_amd.libs.wavio import float_to_pcm16
    n = 16384
    x = white(900, 2, n, peak=2.0)
    model = o.inverse_stft(o.forward_stft(x[1].astype(np.float64), **STFT_KW), **STFT_KW)
    over_model = int(np.count_nonzero(np.abs(model) > 1))
    assert over_model >= 100
    one_hot = np.zeros((2, F, 2), np.complex64)
    one_hot[0, :, 0] = 1
    one_hot[1, :, 1] = 1
    con = Fixed(ctx, [n], C=2, audio=[x], w=one_hot, pick=[1])
    (f,), (q,) = float_and_pcm(con, 0, _ffi.FLAG_NO_RENORM)
    over = int(np.count_nonzero(np.abs(f) > 1))
    wrapped = int(np.count_nonzero((np.abs(f) > 1.001) & (np.sign(q) != np.sign(f))))
    print(f"past full scale: {over_model} samples of the float64 model beyond +-1, {over} of the float output "
          f"(max |y| = {np.abs(f).max():.4f}), {wrapped} change sign in 16 bits; "
          f"{np.count_nonzero(q != sm.exact_pcm16(f))} differ from the exact wrapped reference")
    assert f.shape == model.shape and np.abs(f - model).max() < 1e-4
    assert over >= 100 and np.abs(f).max() > 1.5 and wrapped > 0
    assert np.array_equal(q, sm.exact_pcm16(f))
    assert np.array_equal(q, float_to_pcm16(f))


# ---------------------------------------------------------------- e. ingest
@pytest.mark.parametrize("C", range(1, 17))
def test_pcm16_to_float_every_channel_count(ctx, C):
    import torch
    for N in (1, 255, 256, 257):
        pcm = sm.ingest_pattern(N, C, seed=N)
        out = Guarded(C * N, torch.float32, -777.25)
        ctx.pcm16_to_float(to_dev(pcm), C, N, out.view)
        sync()
        got = out.result().reshape(C, N)
        want = sm.ingest_float(pcm)
        print(f"setk_pcm16_to_float C={C} N={N}: {np.count_nonzero(got != want)} samples differ")
        assert np.array_equal(got, want), (C, N)


# (the issue's lengths, and 3080: with 3 x 256 threads per item it is the one multiple of four whose 770
#  groups give a thread of the four-frames-per-thread path a second turn of its grid-stride loop)
RAGGED = (1, 2, 3, 4, 5, 2047, 2048, 2052, 3080, 4099)
CT_FORMS = (2, 4, 6, 8)      # channel counts with a compile-time form (modular.hip)
VARIANTS = {"aligned": (0, 0), "source-offset-one-sample": (1, 0), "destination-offset-one-element": (0, 1)}


def staged_sources(C, src_off):
    """The interleaved frames of the ragged batch on the device, each in a tensor of its own,
    `src_off` samples past its start."""
    import torch
    pcms = [sm.ingest_pattern(n, C, seed=i) for i, n in enumerate(RAGGED)]
    holds = []
    for p in pcms:
        t = torch.zeros(p.size + 8, dtype=torch.int16, device=dev())
        t[src_off:src_off + p.size] = to_dev(p.reshape(-1))
        holds.append(t)
    ptrs = [t.data_ptr() + 2 * src_off for t in holds]
    assert all(p % 16 == 2 * src_off for p in ptrs)
    return pcms, holds, ptrs


def power_bound(n, fast, tail):
    """The relative bound on power0 for an item of n frames in this batch, derived from the kernel
    (modular.hip): all terms are positive; the launch has bx = ceil(max_n / 2048) blocks of 256
    threads per item.  On the frame-by-frame path the grid-stride loop hands a thread at most
    ceil(n / (256 bx)) frames; on the four-frames-per-thread path (`fast`) at most
    ceil((n // 4) / (256 bx)) groups of four, plus one frame of the n % 4 tail where the kernel
    has one (`tail`: the planar kernel; the float kernel takes such an item frame by frame).  Every
    frame is one fused multiply-add into the thread's float32 sum, i.e. one rounding; then six
    shuffle adds and the widening to double (the float64 atomics add 2^-53 each: nothing at this
    scale).  (frames + 7) 2^-24, about 1e-6."""
    threads = 256 * -(-max(RAGGED) // 2048)
    if fast:
        frames = 4 * -(-(n // 4) // threads) + (1 if tail and n % 4 else 0)
    else:
        frames = -(-n // threads)
    return (frames + 7) * 2.0 ** -24, frames


def check_power(name, C, variant, power, pcms, fast_path, tail):
    """fast_path(n): whether the kernel takes the four-frames-per-thread path for an item of n frames."""
    worst = 0.0
    for i, p in enumerate(pcms):
        want = sm.ingest_power0(p)
        bound, frames = power_bound(p.shape[0], fast_path(p.shape[0]), tail)
        err = abs(float(power[i]) - want) / want
        worst = max(worst, err / bound)
        print(f"{name} C={C} {variant} n={p.shape[0]}: power0 relative error {err:.3e}, bound {bound:.3e} "
              f"({frames} frames per thread at most)")
        assert err <= bound, (C, variant, p.shape[0], err, bound)
    return worst


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("C", range(1, 17))
def test_pcm16_to_float_batch(ctx, C, variant):
    """float out[c][n] = pcm[n][c] / 32768 exactly (a 16-bit integer times 2^-15), nothing written
    outside [C][n], power0 within its derived bound."""
    import torch
    src_off, dst_off = VARIANTS[variant]
    pcms, holds, ptrs = staged_sources(C, src_off)
    outs = [Guarded(C * n, torch.float32, -777.25, dst_off) for n in RAGGED]
    assert all(g.ptr() % 16 == 4 * dst_off for g in outs)
    power = torch.zeros(len(RAGGED), dtype=torch.float64, device=dev())
    ctx.pcm16_to_float_batch(C, ptrs, list(RAGGED), [g.ptr() for g in outs], power0=power.data_ptr())
    sync()
    for p, g in zip(pcms, outs):
        n = p.shape[0]
        got = g.result().reshape(C, n)
        want = sm.ingest_float(p)
        assert np.array_equal(got, want), (C, variant, n, int(np.count_nonzero(got != want)))
    # four frames per thread: a compile-time form, both pointers aligned, n a multiple of four
    check_power("setk_pcm16_to_float_batch", C, variant, power.cpu().numpy(), pcms,
                lambda n: C in CT_FORMS and variant == "aligned" and n % 4 == 0, tail=False)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("C", range(1, 17))
def test_pcm16_deinterleave_batch(ctx, C, variant):
    """planar int16 out[c][stride], stride = setk_pcm16_channel_stride(n): the file's samples in
    [0, n), zero in [n, stride) of every channel, nothing written outside [C][stride], power0 within
    its derived bound."""
    import torch
    src_off, dst_off = VARIANTS[variant]
    pcms, holds, ptrs = staged_sources(C, src_off)
    strides = [ctx.pcm16_channel_stride(n) for n in RAGGED]
    assert all(s >= n and s % 8 == 0 and s - n < 8 for s, n in zip(strides, RAGGED))
    outs = [Guarded(C * s, torch.int16, 12345, dst_off) for s in strides]
    assert all(g.ptr() % 16 == 2 * dst_off for g in outs)
    power = torch.zeros(len(RAGGED), dtype=torch.float64, device=dev())
    ctx.pcm16_deinterleave_batch(C, ptrs, list(RAGGED), [g.ptr() for g in outs], power0=power.data_ptr())
    sync()
    for p, g, s in zip(pcms, outs, strides):
        n = p.shape[0]
        got = g.result().reshape(C, s)
        assert np.array_equal(got[:, :n], p.T), (C, variant, n, int(np.count_nonzero(got[:, :n] != p.T)))
        assert not got[:, n:].any(), (C, variant, n, "padding is not silence")
    # four frames per thread: a compile-time form and both pointers aligned (the stride is a multiple
    # of eight); the n % 4 frames left go frame by frame
    check_power("setk_pcm16_deinterleave_batch", C, variant, power.cpu().numpy(), pcms,
                lambda n: C in CT_FORMS and variant == "aligned", tail=True)


# ---------------------------------------------------------------- f. 16-bit frames through the engine
@pytest.mark.parametrize("C", range(1, 17))
def test_engine_pcm16_frames_equal_float_samples(C):
    """BatchEnhancer on Pcm16Frames against the same samples handed in as float32 (pcm / 32768): the
    waves must be equal bit for bit at every channel count (1 to 8: the 16-bit samples go into the
    fused kernels as stored; 9 to 16: converted on the device).  Four utterances, N % 4 = 1, 2, 3, 0,
    two of them odd."""
    from setk_amd.engine import BatchEnhancer, Pcm16Frames
    eng = BatchEnhancer(beamformer="mvdr")
    rng = np.random.default_rng(7000 + C)
    lens = [5001, 5002, 5003, 5004]
    frames = [rng.integers(-30000, 30001, (n, C)).astype(np.int16) for n in lens]
    masks = [rng.uniform(0.2, 0.8, (1 + n // 256, F)).astype(np.float32) for n in lens]
    got = eng.enhance([(Pcm16Frames(f), m, None) for f, m in zip(frames, masks)])
    want = eng.enhance([(sm.ingest_float(f), m, None) for f, m in zip(frames, masks)])
    for n, (g, sg), (w, sw) in zip(lens, got, want):
        assert sg == 0 and sw == 0, (C, n, sg, sw)
        differ = int(np.count_nonzero(g.view(np.uint32) != w.view(np.uint32)))
        print(f"BatchEnhancer C={C} N={n}: {differ} of {g.size} samples differ between 16-bit frames and float32 in")
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w), (C, n, differ)


# ---------------------------------------------------------------- g. the engines' stand-alone operator tail
UNFUSED_N = 96000     # long enough to be sensitive: the float32-product rule differs on about 2e-4 of the samples


def unfused_fixed(C, pcm16, renorm=True, peak=PEAK, **geometry):
    from setk_amd.engine import FixedBatchBeamformer
    bins = geometry.get("frame_len", 512) // 2 + 1
    rng = np.random.default_rng(800 + C)
    w = (rng.standard_normal((2, bins, C)) + 1j * rng.standard_normal((2, bins, C))).astype(np.complex64)
    if not renorm:                      # one-hot: the channel itself goes through, scale and all
        w[:] = 0
        w[0, :, 0] = w[1, :, 1] = 1
    eng = FixedBatchBeamformer(w, pcm16=pcm16, renorm=renorm, **geometry)
    try:
        return eng.run([(white(810 + C, C, UNFUSED_N, peak), 1), (white(820 + C, C, 9003, peak), 0)])
    finally:
        eng.close()


def unfused_enhancer(C, pcm16, **geometry):
    from setk_amd.engine import BatchEnhancer
    bins, hop = geometry["frame_len"] // 2 + 1, geometry["frame_hop"]
    eng = BatchEnhancer(beamformer="mvdr", pcm16=pcm16, **geometry)
    utts = []
    for i, n in enumerate((UNFUSED_N, 9003)):
        mask = np.random.default_rng(830 + i).uniform(0.2, 0.8, (1 + n // hop, bins)).astype(np.float32)
        utts.append((white(840 + C + i, C, n), mask, None))
    try:
        out = eng.enhance(utts)
    finally:
        eng.close()
    assert [st for _, st in out] == [0, 0]
    return [w for w, _ in out]


UNFUSED = {
    "fixed-12ch": lambda pcm16: unfused_fixed(12, pcm16),
    "fixed-12ch-no-renorm-past-full-scale": lambda pcm16: unfused_fixed(12, pcm16, renorm=False, peak=2.0),
    "fixed-4ch-nfft256": lambda pcm16: unfused_fixed(4, pcm16, frame_len=256, frame_hop=128),
    "enhancer-4ch-nfft256": lambda pcm16: unfused_enhancer(4, pcm16, frame_len=256, frame_hop=128),
}


@pytest.mark.parametrize("name", list(UNFUSED))
def test_engine_unfused_pcm16_output_is_the_host_writers_rule(name):
    """More than 8 channels in FixedBatchBeamformer, or any n_fft != 512, go through the stand-alone
    operators (setk_stft -> ... -> setk_istft) and the engines' own tail (_Engine._unfused_tail).
    Its pcm16=True output must be wavio.float_to_pcm16 of the pcm16=False output of the same engine
    on the same inputs, sample for sample -- wrapped past full scale when there is no renorm.
    Seen failing on the tail as it was (torch.round(out * 32767.0).to(int16), the float32 product):
    PARITY_NOTES_SAMPLES.md has the counts."""
    flt, pcm = UNFUSED[name](False), UNFUSED[name](True)
    total = 0
    for u, (f, q) in enumerate(zip(flt, pcm)):
        assert f.dtype == np.float32 and q.dtype == np.int16 and q.shape == f.shape and np.isfinite(f).all()
        n, worst, want = differing(q, f)
        total += n
        print(f"{name} utterance {u} ({f.size} samples, max |y| = {np.abs(f).max():.4f}): {n} samples differ from "
              f"float_to_pcm16(float output), largest step {worst}; the float32-product rule on the same float "
              f"output would differ on {np.count_nonzero(sm.f32_product_pcm16(f) != want)}")
        if "past-full-scale" in name:
            assert np.count_nonzero(np.abs(f) > 1) >= 100
            assert np.array_equal(want, sm.exact_pcm16(f))
    assert total == 0
    for f, q in zip(flt, pcm):
        assert np.array_equal(q, differing(q, f)[2])
