"""Block-online MVDR / GEV beamforming for a batch: setk_enhance_online_batch."""
import numpy as np

from .. import _ffi
from ._common import _Engine, _Layout, _Twin, BEAMFORMER_KINDS, RANK1, Pcm16Frames, channels_and_size
from .enhance import BatchEnhancer


class BatchOnlineEnhancer(_Engine):
    """The loop of apply_adaptive_beamformer.py --online.chunk-size (do_online_beamform over
    OnlineMvdrBeamformer / OnlineGevdBeamformer.run, post-mask, inverse_stft) for a batch, resident
    on the device: one upload of the samples and masks per batch, the chunk covariances, the
    smoothing R_c = alpha R_{c-1} + phi_c r_c (phi_0 = 1, phi_c = 1 - alpha), the weights of every
    chunk in one solve, beamforming with the weight set of each frame's chunk, one download of the
    waves.  No state survives an utterance.  enhance() takes a list of (C x N float32 | Pcm16Frames,
    speech mask, interferer mask | None) -- any mix of channel counts up to 8 -- and returns
    [(wave | None, status)] in input order; a status other than 0 is the reference's LinAlgError
    case.  Torch-free; the buffers only grow.  A batch is cut where its device working set (samples,
    masks, the slabs and planes of every chunk) would pass max_batch_bytes."""

    _no_gpu = "BatchOnlineEnhancer needs an MI355X (no CPU fallback)"

    def __init__(self, beamformer="mvdr", chunk_size=64, alpha=0.8, ban=False, post_mask=False, pcm16=False,
                 frame_len=512, frame_hop=256, center=True, round_power_of_two=True, window="hann",
                 device=None, ctx=None, max_batch_bytes=3 << 30):
        if beamformer not in BEAMFORMER_KINDS:
            raise ValueError(f"unknown beamformer {beamformer}")
        if int(chunk_size) < 1:
            raise ValueError("chunk_size must be at least 1")
        super().__init__(ctx or _ffi.default_context(device), frame_len, frame_hop, center,
                         round_power_of_two, window)
        kind, beta = BEAMFORMER_KINDS[beamformer]
        self.opts_kw = dict(kind=kind, pmwf_beta=beta, pmwf_ref=-1, rank1=RANK1[""])
        self.base_flags = (_ffi.FLAG_BAN if ban else 0) | (_ffi.FLAG_POST_MASK if post_mask else 0) | \
            (_ffi.FLAG_OUT_PCM16 if pcm16 else 0)
        self.chunk_size, self.alpha, self.ban, self.pcm16 = int(chunk_size), float(alpha), bool(ban), pcm16
        self.max_batch_bytes = max_batch_bytes
        self._inp, self._dev, self._out = _Twin(self.ctx), _Twin(self.ctx, host=False), _Twin(self.ctx)
        self._owned += [self._inp, self._dev, self._out]
        self._stream = 0

    frames_and_length = BatchEnhancer.frames_and_length
    condition_mask = BatchEnhancer.condition_mask

    def close(self):
        if self._stream:
            self.ctx.stream_synchronize(self._stream)
        super().close()
        if self._stream:
            self.ctx.stream_destroy(self._stream)
            self._stream = 0

    def num_chunks(self, num_frames):
        return -(-num_frames // self.chunk_size)

    def _device_bytes(self, samps, C):
        """What an utterance takes on the device: samples, two masks, the wave, and per chunk the
        partial slabs (one per 64 frames), the smoothed planes, the chunk's rn (BAN), the weights."""
        n = channels_and_size(samps)[1]
        T, L = self.frames_and_length(n // C)
        NP = C * (C + 1) // 2
        slabs = -(-min(self.chunk_size, T) // 64)
        per_chunk = 264 * 4 * (slabs * (4 * NP + 2) + 4 * NP + (2 * NP if self.ban else 0) + 2 * C)
        return 6 * n + 8 * T * self.num_bins + 8 * L + self.num_chunks(T) * per_chunk

    def enhance(self, utts):
        results = [None] * len(utts)
        if not len(utts):
            return results
        self._plan()
        samps = [u[0] for u in utts]
        groups = self._by_channels(samps, also=[u[2] is not None for u in utts])
        for (C, has_itf), idx in groups.items():
            batch, load = [], 0
            for i in idx:
                n = self._device_bytes(samps[i], C)
                if batch and load + n > self.max_batch_bytes:
                    self._run(utts, batch, C, has_itf, results)
                    batch, load = [], 0
                batch.append(i)
                load += n
            self._run(utts, batch, C, has_itf, results)
        return results

    def _run(self, utts, batch, C, has_itf, results):
        ctx, F = self.ctx, self.num_bins
        if not self._stream:
            self._stream = ctx.stream_create()
        stream = self._stream
        # 16-bit samples go into the kernels as stored (SETK_FLAG_IN_PCM16) when the whole batch
        # has them; a mixed batch is widened to float32 on the device
        all_pcm = all(isinstance(utts[i][0], Pcm16Frames) for i in batch)
        direct = all_pcm and self.stft["frame_hop"] % 2 == 0
        l_in, l_dev, l_out = _Layout(), _Layout(), _Layout()
        plan = []
        for i in batch:
            s, mask, itf = utts[i]
            pcm = isinstance(s, Pcm16Frames)
            N = s.frames.shape[0] if pcm else channels_and_size(s)[1] // C
            T, L = self.frames_and_length(N)
            mask = np.ascontiguousarray(self.condition_mask(mask, T), dtype=np.float32)
            itf = np.ascontiguousarray(self.condition_mask(itf, T), dtype=np.float32) if has_itf else None
            o_a = l_in.take((2 if pcm else 4) * C * N)
            o_m = l_in.take(4 * T * F)
            o_i = l_in.take(4 * T * F) if has_itf else None
            o_c = None
            if pcm:  # planar int16 [C][stride], or float32 [C][N]
                o_c = l_dev.take(2 * C * ctx.pcm16_channel_stride(N) if direct else 4 * C * N)
            o_w = l_out.take((2 if self.pcm16 else 4) * L)
            plan.append((s, pcm, N, L, mask, itf, o_a, o_m, o_i, o_c, o_w))
        o_status = l_out.take(4 * len(batch))
        ctx.stream_synchronize(stream)  # the previous call's work has left the blocks
        self._inp.reserve(l_in.size)
        self._dev.reserve(max(l_dev.size, 256))
        self._out.reserve(l_out.size)
        view, d_in, d_dev, d_out = self._inp.view, self._inp.d, self._dev.d, self._out.d

        def put(offset, array):
            view[offset:offset + array.nbytes] = np.frombuffer(array, dtype=np.uint8)

        aptr, mptr, iptr, wptr, ns, jobs = [], [], [], [], [], []
        for s, pcm, N, L, mask, itf, o_a, o_m, o_i, o_c, o_w in plan:
            if pcm:
                put(o_a, s.frames)
                jobs.append((d_in + o_a, N, d_dev + o_c))
                aptr.append(d_dev + o_c)
            else:
                put(o_a, np.ascontiguousarray(s, dtype=np.float32))
                aptr.append(d_in + o_a)
            put(o_m, mask)
            mptr.append(d_in + o_m)
            if has_itf:
                put(o_i, itf)
                iptr.append(d_in + o_i)
            wptr.append(d_out + o_w)
            ns.append(N)
        ctx.memcpy_h2d_async(d_in, self._inp.h, l_in.size, stream)
        if jobs:
            convert = ctx.pcm16_deinterleave_batch if direct else ctx.pcm16_to_float_batch
            convert(C, [p for p, _, _ in jobs], [n for _, n, _ in jobs], [o for _, _, o in jobs], stream=stream)
        flags = self.base_flags | (0 if has_itf else _ffi.FLAG_CLAMP_MASK) | (_ffi.FLAG_IN_PCM16 if direct else 0)
        ctx.enhance_online_batch(_ffi.BfOpts(flags=flags, **self.opts_kw), self.chunk_size, self.alpha, C, aptr,
                                 ns, mptr, iptr if has_itf else None, wptr, status=d_out + o_status,
                                 stream=stream)
        ctx.memcpy_d2h_async(self._out.h, d_out, l_out.size, stream)
        ctx.stream_synchronize(stream)
        out = self._out.view
        status = np.frombuffer(out[o_status:o_status + 4 * len(batch)], dtype=np.int32)
        wtype = np.int16 if self.pcm16 else np.float32
        for k, i in enumerate(batch):
            L, o_w = plan[k][3], plan[k][10]
            wave = np.frombuffer(out[o_w:o_w + np.dtype(wtype).itemsize * L], dtype=wtype).copy()
            results[i] = (wave if status[k] == 0 else None, int(status[k]))
