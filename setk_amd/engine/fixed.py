"""Fixed (data-independent) beamformers for a batch: setk_apply_weights_batch."""
import numpy as np

from .. import _ffi
from ._common import _Engine


def _weight_table(weights):
    weights = np.asarray(weights)
    if weights.ndim == 2:
        weights = weights[None]
    return np.ascontiguousarray(weights, dtype=np.complex64)  # B x F x M


class FixedBatchBeamformer(_Engine):
    """apply_fixed_beamformer.py:38-48 for a batch: FixedBeamformer.run +
    inverse_stft with the renorm to max |audio|.  weights: B x F x M complex (the
    reference's layout); run() takes [(samps C x N float32 | Pcm16Frames, beam)]
    and returns the waveforms (int16 when pcm16 else float32) in input order."""

    def __init__(self, weights, frame_len=512, frame_hop=256, center=True,
                 round_power_of_two=True, window="hann", pcm16=False, device=None,
                 max_batch_samples=1 << 29, renorm=True):
        # no GPU / no library: setk_create fails here, loudly.  The fused batch path brings
        # its own buffers and stream; torch is the plumbing of the stand-alone operators only
        # (n_fft != 512, more than 8 channels) and is imported when they are first needed.
        ctx = _ffi.default_context(device)
        self.weights = _weight_table(weights)
        super().__init__(ctx, frame_len, frame_hop, center, round_power_of_two, window)
        self._dw = 0
        # renorm=False: inverse_stft(norm=None), apply_classic_beamformer.py:109-110
        self.renorm = bool(renorm)
        if self.weights.shape[1] != self.num_bins:
            raise ValueError(f"weights have {self.weights.shape[1]} bins, the transform "
                             f"{self.num_bins}")
        self.pcm16 = pcm16
        self.max_batch_samples = max_batch_samples

    def set_weights(self, weights):
        """Swap the weight table (B x F x M) and keep everything else -- the pinned slabs, the
        device twin, the stream: what a caller does whose table grows from batch to batch
        (apply_classic_beamformer: one entry per DoA seen so far)."""
        weights = _weight_table(weights)
        if weights.shape[1:] != self.weights.shape[1:]:
            raise ValueError(f"weights {weights.shape[1:]}, engine built for {self.weights.shape[1:]}")
        if self._dw and self._slabs is not None:
            self.ctx.stream_synchronize(self._slabs.stream)  # the old table may still be read
        self._free_weights()
        self.weights = weights

    def _free_weights(self):
        if self._dw:
            self.ctx.device_free(self._dw)
            self._dw = 0

    def close(self):
        """Give the slabs and the device copy of the weights back."""
        super().close()
        self._free_weights()

    def run(self, utts):
        self._plan()
        results = [None] * len(utts)
        samps = [u[0] for u in utts]
        for C, idx in self._by_channels(samps).items():
            if C != self.weights.shape[2]:
                raise ValueError(f"Input obs do not match with weight, {self.weights.shape[1:]} "
                                 f"vs {C} channels")
            for batch in self._batches(idx, samps, self.max_batch_samples):
                self._run(utts, batch, C, results)
        return results

    def _run(self, utts, batch, C, results):
        ctx = self.ctx
        if self.n_fft != 512 or C > 8:
            return self._run_unfused(utts, batch, C, results)
        # one slab up, setk_apply_weights_batch, one slab down -- on the library's own
        # buffers and stream
        b = self._get_slabs()
        esz = 2 if self.pcm16 else 4
        aptr, ns, off_out, n_out = b.stage_audio(
            [utts[i][0] for i in batch], C, lambda N: esz * ctx.istft_num_samples(ctx.num_frames(N)))
        if not self._dw:
            self._dw = ctx.device_alloc(self.weights.nbytes)
            ctx.memcpy_h2d_async(self._dw, self.weights.ctypes.data, self.weights.nbytes, b.stream)
        ctx.apply_weights_batch(C, aptr, ns, self._dw, self.weights.shape[0],
                                [int(utts[i][1]) for i in batch], [b.out.d + o for o in off_out],
                                flags=(_ffi.FLAG_OUT_PCM16 if self.pcm16 else 0) |
                                (0 if self.renorm else _ffi.FLAG_NO_RENORM), stream=b.stream)
        b.fetch(n_out)
        for k, i in enumerate(batch):
            L = ctx.istft_num_samples(ctx.num_frames(ns[k]))
            results[i] = b.read(off_out[k], L, np.int16 if self.pcm16 else np.float32)

    def _run_unfused(self, utts, batch, C, results):
        """n_fft != 512: setk_stft -> setk_beamform -> setk_istft per utterance."""
        torch, ctx, dev, F = self.torch, self.ctx, self.dev, self.num_bins
        for i in batch:
            samps, beam = utts[i]
            a, N = self._upload(samps, C)
            T = ctx.num_frames(N)
            spec = torch.empty((C, T, F), dtype=torch.complex64, device=dev)
            ctx.stft(a, spec)
            w = torch.from_numpy(self.weights[int(beam)]).to(dev)
            enh = torch.empty((T, F), dtype=torch.complex64, device=dev)
            ctx.beamform(w, spec, C, T, F, enh)
            results[i] = self._unfused_tail(enh, T, a, renorm=self.renorm)
