"""Blind CGMM mask estimation for a batch: setk_cgmm_estimate_batch and its fall-backs."""
import os

import numpy as np

from .. import _ffi
from ._common import _Engine, Pcm16Frames, host_samples


class CgmmEstimator(_Engine):
    """Batched blind mask estimation (estimate_cgmm_masks.py:19-71, K = 2): STFT
    and all EM iterations on the device, n utterances per kernel launch
    (setk_cgmm_masks_batch).  n_fft must be 512 for the device STFT used here."""

    _no_gpu = "CgmmEstimator needs an MI355X (no CPU fallback)"

    def __init__(self, frame_len=512, frame_hop=256, center=True, round_power_of_two=True,
                 window="hann", num_iters=20, device=None, ctx=None, update_alpha=False):
        self.update_alpha = bool(update_alpha)
        # no GPU / no library: setk_create fails here, loudly.  torch is the plumbing of
        # estimate_device() (tensors in, tensors out); estimate() brings its own buffers.
        super().__init__(ctx or _ffi.default_context(device), frame_len, frame_hop, center,
                         round_power_of_two, window)
        self.num_iters = num_iters
        self.force_streaming = os.environ.get("SETK_CGMM_STREAMING", "") not in ("", "0")

    def estimate_device(self, audio, init_masks=None):
        """audio: list of device float32 tensors C x N (same C).  Returns the
        list of device speech masks T x F (float32)."""
        torch, ctx, dev, F = self.torch, self.ctx, self.dev, self.num_bins
        self._plan()
        C = audio[0].shape[0]
        if self.n_fft == 512 and C <= 8 and not self.force_streaming:
            # audio -> masks in one call: the spectrograms are written in the layout the
            # bin-resident EM reads (no [C][T][F] intermediate, no transpose pass)
            masks = [torch.empty((ctx.num_frames(a.shape[1]), F), dtype=torch.float32, device=dev)
                     for a in audio]
            init = None
            if init_masks is not None:
                init = [0 if m is None else m.data_ptr() for m in init_masks]
            try:
                ctx.cgmm_estimate_batch(C, [a.data_ptr() for a in audio],
                                        [a.shape[1] for a in audio], self.num_iters, init,
                                        [t.data_ptr() for t in masks],
                                        update_alpha=self.update_alpha)
                # no host synchronisation: the scratch lives in the handle's arena, whose
                # reuse by the next call is ordered on the stream
                return masks
            except _ffi.SetkUnsupported:
                pass  # a bin of the longest utterance does not fit a CU: streaming kernels
        if C > 8:
            # 9 - 16 channels: the general float64 EM (setk_cgmm_masks_k), one utterance at a time
            # on spectrograms of the stand-alone transform (any n_fft the plan accepts)
            masks = []
            for k, a in enumerate(audio):
                T = ctx.num_frames(a.shape[1])
                spec = torch.empty((C, T, F), dtype=torch.complex64, device=dev)
                ctx.stft(a, spec)
                gamma = torch.empty((2, T, F), dtype=torch.float32, device=dev)
                init = None if init_masks is None else init_masks[k]
                ctx.cgmm_masks_k(spec, C, T, F, 2, self.num_iters, None, init, gamma,
                                 update_alpha=self.update_alpha)
                masks.append(gamma[0])
            torch.cuda.current_stream().synchronize()
            return masks
        specs, masks, frames = [], [], []
        # rows padded to 128 bytes: the EM kernels stream 32-bin (256-byte) segments per
        # wavefront and a 2056-byte row pitch makes every segment straddle an extra line
        Fp = (F + 15) // 16 * 16
        for a in audio:
            T = ctx.num_frames(a.shape[1])
            specs.append(torch.empty((C, T, Fp), dtype=torch.complex64, device=dev))
            masks.append(torch.empty((T, F), dtype=torch.float32, device=dev))
            frames.append(T)
        # all spectrograms in one launch
        ctx.stft_batch(C, [a.data_ptr() for a in audio], [a.shape[1] for a in audio],
                       [t.data_ptr() for t in specs], spec_pitch=Fp)
        init = None
        if init_masks is not None:
            init = [0 if m is None else m.data_ptr() for m in init_masks]
        ctx.cgmm_masks_batch(C, [t.data_ptr() for t in specs], frames, F, self.num_iters, init,
                             [t.data_ptr() for t in masks], update_alpha=self.update_alpha,
                             spec_pitch=Fp)
        torch.cuda.current_stream().synchronize()  # specs must outlive the launches
        return masks

    def estimate(self, utts):
        """utts: list of C x N float32 numpy arrays or Pcm16Frames (16-bit frames as stored:
        converted on the device) -> list of T x F float32 masks.  Per channel count: the
        samples go up in ONE copy out of a page-locked slab, the masks come down in one; the
        buffers, the stream and the copies are the library's (no torch in this path).  Shapes
        the one-call estimator does not take (n_fft != 512, more than 8 channels, a bin that
        does not fit a CU) go through estimate_device()."""
        out = [None] * len(utts)
        for C, idx in self._by_channels(utts).items():
            if self.n_fft != 512 or C > 8 or self.force_streaming:
                self._estimate_torch(utts, C, idx, out)
                continue
            try:
                self._estimate_native(utts, C, idx, out)
            except _ffi.SetkUnsupported:
                self._estimate_torch(utts, C, idx, out)
        return out

    def _estimate_torch(self, utts, C, idx, out):
        torch, ctx, dev = self.torch, self.ctx, self.dev
        audio, pcm = [], []
        for i in idx:
            s = utts[i]
            if isinstance(s, Pcm16Frames):  # (converted in one launch for the group, below)
                a = torch.empty((C, s.frames.shape[0]), dtype=torch.float32, device=dev)
                pcm.append((torch.from_numpy(s.frames).to(dev), a))
            else:
                a = torch.from_numpy(host_samples(s)).to(dev)
            audio.append(a)
        if pcm:
            ctx.pcm16_to_float_batch(C, [p.data_ptr() for p, _ in pcm], [a.shape[1] for _, a in pcm],
                                     [a.data_ptr() for _, a in pcm])
        masks = self.estimate_device(audio)
        host = torch.cat([m.reshape(-1) for m in masks]).cpu().numpy()
        off = 0
        for i, m in zip(idx, masks):
            out[i] = host[off:off + m.numel()].reshape(m.shape)
            off += m.numel()

    def _estimate_native(self, utts, C, idx, out):
        ctx, F = self.ctx, self.num_bins
        self._plan()
        b = self._get_slabs()
        aptr, ns, off_out, n_out = b.stage_audio([utts[i] for i in idx], C,
                                                 lambda N: 4 * ctx.num_frames(N) * F)
        ctx.cgmm_estimate_batch(C, aptr, ns, self.num_iters, None, [b.out.d + o for o in off_out],
                                stream=b.stream, update_alpha=self.update_alpha)
        b.fetch(n_out)
        for k, i in enumerate(idx):
            T = ctx.num_frames(ns[k])
            out[i] = b.read(off_out[k], T * F, np.float32, (T, F))
