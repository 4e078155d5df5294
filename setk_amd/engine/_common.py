"""
What every batch engine needs around its library calls: the utterance types, the STFT geometry,
the lazy torch import, grouping and batching of utterances, the grow-only buffers and the slabs
of the torch-free paths, and the two inverse-transform tails.
"""
import numpy as np

from .. import _ffi
from ..libs.utils import nextpow2, stft_window, cmat_abs

BEAMFORMER_KINDS = {
    # name -> (kind, pmwf_beta)
    "mvdr": (_ffi.BF_MVDR, 0.0),
    "mpdr": (_ffi.BF_MPDR, 0.0),
    "mpdr-whiten": (_ffi.BF_MPDR_WHITEN, 0.0),
    "gevd": (_ffi.BF_GEVD, 0.0),
    "pmwf-0": (_ffi.BF_PMWF, 0.0),
    "pmwf-1": (_ffi.BF_PMWF, 1.0),
}
RANK1 = {"": _ffi.RANK1_NONE, "none": _ffi.RANK1_NONE, "eig": _ffi.RANK1_EIG,
         "gev": _ffi.RANK1_GEV}


class Pcm16Frames(object):
    """Interleaved 16-bit PCM frames [N, C] of one utterance, exactly as stored in
    its wav (WaveReader.read_pcm16).  BatchEnhancer uploads the 2-byte samples and
    converts / transposes them on the device (setk_pcm16_to_float)."""

    def __init__(self, frames):
        frames = np.asarray(frames)
        if frames.dtype != np.int16 or frames.ndim != 2:
            raise ValueError("Pcm16Frames expects an int16 array of shape N x C")
        # (a private, writable copy: np.frombuffer views of file bytes are read-only
        # and torch.from_numpy wants to own writable memory)
        self.frames = np.array(frames, dtype=np.int16, order="C", copy=True)

    @property
    def num_channels(self):
        return self.frames.shape[1]

    @property
    def size(self):
        return self.frames.size

    def to_float(self):
        """The reference's host view: C x N float32 (soundfile scaling)."""
        return np.ascontiguousarray(self.frames.T.astype(np.float32) / np.float32(32768.0))


def channels_and_size(samps):
    if isinstance(samps, Pcm16Frames):
        return samps.num_channels, samps.size
    samps = np.asarray(samps)
    return (1 if samps.ndim == 1 else samps.shape[0]), samps.size


def host_samples(samps):
    """An utterance (Pcm16Frames, C x N or N samples of any float type) as C x N float32 on the host."""
    if isinstance(samps, Pcm16Frames):
        samps = samps.to_float()
    samps = np.ascontiguousarray(samps, dtype=np.float32)
    return samps[None] if samps.ndim == 1 else samps


def compute_vad_masks(spectrogram, proportion):
    """Energy based VAD mask of apply_adaptive_beamformer.py:50-71: keep
    proportion*100 % of the energy.  spectrogram F x T -> (T x F bool, index).
    The cumulative sum replaces the reference's python while-loop."""
    energy = cmat_abs(spectrogram)
    vec = np.sort(energy.flatten())
    filter_energy = np.sum(vec) * (1 - proportion)
    csum = np.cumsum(vec)
    index = int(np.searchsorted(csum, filter_energy, side="right"))
    threshold = vec[min(index, vec.shape[0] - 1)] if vec.shape[0] else 0
    return (energy < threshold).transpose(), index


def align256(v):
    return (v + 255) & ~255


class _Layout(object):
    """Offsets carved out of one block, each a multiple of 256 bytes; `size` is the block's."""

    def __init__(self):
        self.size = 0

    def take(self, nbytes):
        o = self.size
        self.size = align256(o + nbytes)
        return o


class _Twin(object):
    """A grow-only page-locked host buffer with a device twin (one memcpy up or down per batch);
    host=False: the device block alone (scratch).  It grows to 1.25 x the request plus `slack`."""

    def __init__(self, ctx, slack=256, host=True):
        self.ctx, self.slack, self.host = ctx, slack, host
        self.cap, self.h, self.d, self.view = 0, 0, 0, None

    def reserve(self, nbytes, stream=None):
        """stream: what may still use the old block, waited for before it is freed (None: the
        caller has waited already)."""
        if nbytes > self.cap:
            if stream is not None:
                self.ctx.stream_synchronize(stream)
            self.close()
            self.cap = int(nbytes * 1.25) + self.slack
            if self.host:
                self.h, self.view = self.ctx.host_alloc(self.cap)
            self.d = self.ctx.device_alloc(self.cap)

    def close(self):
        if self.d:
            self.view = None
            if self.h:
                self.ctx.host_free(self.h)
            self.ctx.device_free(self.d)
        self.cap, self.h, self.d = 0, 0, 0


class _Slabs(object):
    """Grow-only working set of the engines' torch-free batch paths: a page-locked input slab
    and its device twin, a device scratch for converted samples, a device output slab and its
    page-locked twin, one stream -- all from the library (setk_host_alloc / setk_device_alloc
    / setk_stream_create)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.inp, self.f32, self.out = _Twin(ctx, 0), _Twin(ctx, 0, host=False), _Twin(ctx, 0)
        self.stream = ctx.stream_create()

    def reserve(self, n_in, n_f32, n_out):
        self.ctx.stream_synchronize(self.stream)  # the previous call's work has left the slabs
        self.inp.reserve(n_in)
        self.f32.reserve(n_f32)
        self.out.reserve(n_out)

    def stage_audio(self, utts, C, extra_out):
        """Lay the utterances (C x N float32 arrays or Pcm16Frames) out in the input slab,
        copy it up in one piece and convert the 16-bit ones on the device.  extra_out(N) ->
        output bytes of an utterance.  Returns (device sample pointers, lengths, output
        offsets, output bytes)."""
        ctx = self.ctx
        lay, l_in, l_f32, l_out = [], _Layout(), _Layout(), _Layout()
        for s in utts:
            pcm = isinstance(s, Pcm16Frames)
            N = s.frames.shape[0] if pcm else channels_and_size(s)[1] // C
            lay.append((pcm, N, l_in.take((2 if pcm else 4) * C * N),
                        l_f32.take(4 * C * N) if pcm else l_f32.size, l_out.take(extra_out(N))))
        self.reserve(max(l_in.size, 256), max(l_f32.size, 256), max(l_out.size, 256))
        np_in, d_in, d_f32 = self.inp.view, self.inp.d, self.f32.d
        aptr, ns, pcm_jobs = [], [], []
        for s, (pcm, N, o_in, o_f32, _) in zip(utts, lay):
            if pcm:
                np_in[o_in:o_in + 2 * C * N] = np.frombuffer(s.frames, dtype=np.uint8)
                pcm_jobs.append((d_in + o_in, N, d_f32 + o_f32))
                aptr.append(d_f32 + o_f32)
            else:
                a = np.ascontiguousarray(s, dtype=np.float32)
                np_in[o_in:o_in + a.nbytes] = np.frombuffer(a, dtype=np.uint8)
                aptr.append(d_in + o_in)
            ns.append(N)
        ctx.memcpy_h2d_async(d_in, self.inp.h, l_in.size, self.stream)
        if pcm_jobs:
            ctx.pcm16_to_float_batch(C, [p for p, _, _ in pcm_jobs], [n for _, n, _ in pcm_jobs],
                                     [o for _, _, o in pcm_jobs], stream=self.stream)
        return aptr, ns, [l[4] for l in lay], l_out.size

    def fetch(self, n_out):
        """One copy down into the page-locked output slab (valid until the next reserve())."""
        self.ctx.memcpy_d2h_async(self.out.h, self.out.d, n_out, self.stream)
        self.ctx.stream_synchronize(self.stream)

    def read(self, offset, count, dtype, shape=-1):
        """A private copy of `count` items of `dtype` at `offset` of the fetched output slab."""
        nbytes = count * np.dtype(dtype).itemsize
        return np.frombuffer(self.out.view[offset:offset + nbytes], dtype=dtype).reshape(shape).copy()

    def close(self):
        ctx = self.ctx
        if not self.stream:
            return
        ctx.stream_synchronize(self.stream)
        twins = (self.inp, self.f32, self.out)
        # (the page-locked blocks first, then the device's: not twin by twin)
        for t in twins:
            t.view = None
            if t.h:
                ctx.host_free(t.h)
        for t in twins:
            if t.d:
                ctx.device_free(t.d)
            t.cap, t.h, t.d = 0, 0, 0
        ctx.stream_destroy(self.stream)
        self.stream = 0


class _Engine(object):
    """What the batch engines share: the library handle, the STFT geometry and its plan, torch on
    first use, the slabs of the torch-free path on first use, and one close() for what they own."""

    _no_gpu = "setk_amd needs an MI355X GPU (no CPU fallback)"

    def __init__(self, ctx, frame_len, frame_hop, center, round_power_of_two, window):
        self.ctx = ctx
        self._torch = None
        self._slabs = None
        self._owned = []  # grow-only blocks besides the slabs; close() empties them, in this order
        n_fft = nextpow2(frame_len) if round_power_of_two else frame_len
        self.stft = dict(frame_len=frame_len, frame_hop=frame_hop, n_fft=n_fft, center=center,
                         window=stft_window(window, frame_len))
        self.n_fft, self.window_name, self.round_power_of_two = n_fft, window, round_power_of_two
        self.num_bins = n_fft // 2 + 1

    @property
    def torch(self):
        if self._torch is None:
            torch = _ffi.import_torch(type(self).__name__ + ': this input (more than 8 channels / an unfused geometry)')
            if not torch.cuda.is_available():
                raise _ffi.SetkError(self._no_gpu)
            self._torch = torch
        return self._torch

    @property
    def dev(self):
        return self.torch.device("cuda", self.ctx.device)

    def _plan(self, ctx=None):
        s = self.stft
        (ctx or self.ctx).stft_plan(s["frame_len"], s["frame_hop"], s["n_fft"], s["center"], s["window"])

    def _get_slabs(self):
        if self._slabs is None:
            self._slabs = _Slabs(self.ctx)
        return self._slabs

    def close(self):
        """Give the slabs, their stream and the device blocks back (also done when the engine is
        collected); the next call allocates afresh."""
        b, self._slabs = self._slabs, None
        for r in [b] + self._owned:
            if r:
                r.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _by_channels(samps, also=None):
        """{channel count (or (channel count, also[i])): indices}, in order of first appearance."""
        groups = {}
        for i, s in enumerate(samps):
            C = channels_and_size(s)[0]
            groups.setdefault(C if also is None else (C, also[i]), []).append(i)
        return groups

    @staticmethod
    def _batches(idx, samps, max_samples, max_utts=None):
        """Cut idx into runs of at most max_samples samples (and max_utts utterances); a single
        utterance above the limit is a run of its own."""
        batch, load = [], 0
        for i in idx:
            n = channels_and_size(samps[i])[1]
            if batch and (load + n > max_samples or (max_utts and len(batch) >= max_utts)):
                yield batch
                batch, load = [], 0
            batch.append(i)
            load += n
        if batch:
            yield batch

    def _same_channels(self, utts):
        C = channels_and_size(utts[0])[0]
        if any(channels_and_size(u)[0] != C for u in utts):
            raise ValueError(f"{type(self).__name__}.run needs the same channel count in every utterance")
        return C

    def _upload(self, samps, C):
        """An utterance as a C x N float32 torch tensor on the device, and N; 16-bit frames go up
        as stored and are scaled and transposed there."""
        torch, dev = self.torch, self.dev
        if isinstance(samps, Pcm16Frames):
            pcm = torch.from_numpy(samps.frames).to(dev)
            N = samps.frames.shape[0]
            a = torch.empty((C, N), dtype=torch.float32, device=dev)
            self.ctx.pcm16_to_float(pcm, C, N, a)
            return a, N
        samps = host_samples(samps)
        return torch.from_numpy(samps).to(dev), samps.shape[1]

    def _istft_out(self, spec, C, T, L, norm, wav32, dst, stream):
        """The tail of the resident paths: the inverse transform of C spectra straight into the
        output slab, or (PCM16 out) into the float scratch `wav32` and quantised from there."""
        ctx = self.ctx
        if self.pcm16:
            ctx.istft(spec, C, T, None, norm, wav32, stream=stream)
            ctx.float_to_pcm16(wav32, C, L, dst, stream=stream)
        else:
            ctx.istft(spec, C, T, None, norm, dst, stream=stream)

    def _unfused_tail(self, enh, T, a, renorm=True):
        """The tail of the stand-alone operator paths: inverse transform of the T x F tensor `enh`,
        renorm to max |a|, quantised by the writer's rule when PCM16 goes out (setk_float_to_pcm16:
        rint(x * 32767) in float64, wrapping); returns the host waveform."""
        torch, ctx = self.torch, self.ctx
        L = ctx.istft_num_samples(T)
        wave = torch.empty((1, L), dtype=torch.float32, device=self.dev)
        norm = a.abs().max().reshape(1).contiguous() if renorm else None
        ctx.istft(enh.reshape(1, T, self.num_bins), 1, T, None, norm, wave)
        out = wave[0]
        if self.pcm16:
            out = torch.empty(L, dtype=torch.int16, device=self.dev)
            if L > 0:
                ctx.float_to_pcm16(wave, 1, L, out)
        return out.cpu().numpy()
