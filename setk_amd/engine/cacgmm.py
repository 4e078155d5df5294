"""Blind CACGMM mask estimation for a batch: setk_cacgmm_estimate_batch and the stand-alone path."""
import numpy as np

from .. import _ffi
from ._common import _Engine, _Layout, _Twin


class CacgmmEstimator(_Engine):
    """Batched CACGMM mask estimation (estimate_cacgmm_masks.py:19-69 up to the aligner): STFT and
    every EM iteration on the device, one STFT launch and one EM launch per group of utterances
    with the same channel count (setk_cacgmm_estimate_batch, n_fft = 512); any other n_fft
    goes through the stand-alone STFT and setk_cacgmm_masks, one utterance at a time.

    The start of utterance i is starts[i], K x F x T float64 (the caller draws it: the
    reference's comes from numpy's global generator in table order), or the CGMM-like start
    with cgmm_init (two classes; starts is then None).  1 - 8 channels."""

    _no_gpu = "CacgmmEstimator needs an MI355X (no CPU fallback)"

    def __init__(self, frame_len=512, frame_hop=256, center=True, round_power_of_two=True,
                 window="hann", num_classes=2, num_iters=50, update_alpha=True, cgmm_init=False,
                 device=None, ctx=None):
        super().__init__(ctx or _ffi.default_context(device), frame_len, frame_hop, center,
                         round_power_of_two, window)
        if not 2 <= int(num_classes) <= 4:
            raise _ffi.SetkUnsupported(f"the device CACGMM implements 2 <= num_classes <= 4, got {num_classes}")
        self.num_classes, self.num_iters = int(num_classes), int(num_iters)
        self.update_alpha = bool(update_alpha)
        self.cgmm_init = bool(cgmm_init) and self.num_classes == 2
        self._starts = None  # page-locked slab of the starts and its device twin

    def _check_starts(self, n, starts):
        if self.cgmm_init:
            if starts is not None:
                raise ValueError("cgmm_init takes no starts")
        elif starts is None or len(starts) != n:
            raise ValueError("CacgmmEstimator needs one start (K x F x T) per utterance, or cgmm_init")

    def estimate_device(self, audio, starts=None):
        """audio: list of device float32 tensors C x N (same C); starts: list of device float64
        tensors K x F x T or None (cgmm_init).  Returns (list of device masks K x T x F float32,
        int32 numpy array: the worst SETK_NUM_* status of every utterance)."""
        torch, ctx, dev, F, K = self.torch, self.ctx, self.dev, self.num_bins, self.num_classes
        self._plan()
        self._check_starts(len(audio), starts)
        C = audio[0].shape[0]
        frames = [ctx.num_frames(a.shape[1]) for a in audio]
        masks = [torch.empty((K, T, F), dtype=torch.float32, device=dev) for T in frames]
        status = np.zeros(len(audio), dtype=np.int32)
        for T, g in zip(frames, starts or []):
            if tuple(g.shape) != (K, F, T) or g.dtype != torch.float64 or not g.is_contiguous():
                raise ValueError(f"a start must be a contiguous float64 K x F x T tensor ({K} x {F} x {T})")
        if self.n_fft == 512:
            ctx.cacgmm_estimate_batch(C, [a.data_ptr() for a in audio], [a.shape[1] for a in audio], K,
                                      self.num_iters, None if starts is None else [g.data_ptr() for g in starts],
                                      [m.data_ptr() for m in masks], update_alpha=self.update_alpha,
                                      cgmm_init=self.cgmm_init, status=status)
            return masks, status
        for k, (a, T) in enumerate(zip(audio, frames)):
            spec = torch.empty((C, T, F), dtype=torch.complex64, device=dev)
            ctx.stft(a, spec)
            st = np.zeros(F, dtype=np.int32)
            ctx.cacgmm_masks(spec, C, T, F, K, self.num_iters, None if starts is None else starts[k],
                             masks[k], update_alpha=self.update_alpha, cgmm_init=self.cgmm_init, status=st)
            status[k] = st.max()
        return masks, status

    def estimate(self, utts, starts=None, return_status=False):
        """utts: list of C x N float32 numpy arrays or Pcm16Frames (16-bit frames as stored:
        converted on the device); starts: list of K x F x T float64 numpy arrays, or None with
        cgmm_init -> list of K x T x F float32 masks.  A non-zero SETK_NUM_* status of an utterance
        is numpy.linalg.eigh's LinAlgError and raised as such; with return_status the worst
        status of every utterance is returned beside the masks instead.
        Per channel count the samples and the starts go up in one copy each out of page-locked
        slabs and the masks come down in one; n_fft != 512 goes through estimate_device()."""
        self._check_starts(len(utts), starts)
        out = [None] * len(utts)
        status = np.zeros(len(utts), dtype=np.int32)
        for C, idx in self._by_channels(utts).items():
            if self.n_fft != 512:
                self._estimate_torch(utts, starts, C, idx, out, status)
            else:
                self._estimate_native(utts, starts, C, idx, out, status)
        if return_status:
            return out, status
        if status.any():
            bad = [i for i in range(len(utts)) if status[i]]
            raise np.linalg.LinAlgError(f"Eigenvalues did not converge (utterances {bad})")
        return out

    def _estimate_torch(self, utts, starts, C, idx, out, status):
        torch, dev = self.torch, self.dev
        audio = [self._upload(utts[i], C)[0] for i in idx]
        g0 = None
        if starts is not None:
            g0 = [torch.from_numpy(np.ascontiguousarray(starts[i], dtype=np.float64)).to(dev) for i in idx]
        masks, st = self.estimate_device(audio, g0)
        for k, i in enumerate(idx):
            out[i] = masks[k].cpu().numpy()
            status[i] = st[k]

    def _estimate_native(self, utts, starts, C, idx, out, status):
        ctx, F, K = self.ctx, self.num_bins, self.num_classes
        self._plan()
        b = self._get_slabs()
        aptr, ns, off_out, n_out = b.stage_audio([utts[i] for i in idx], C,
                                                 lambda N: 4 * K * ctx.num_frames(N) * F)
        frames = [ctx.num_frames(n) for n in ns]
        gptr = None
        if starts is not None:
            lay = _Layout()
            offs = [lay.take(8 * K * F * T) for T in frames]
            if self._starts is None:
                self._starts = _Twin(ctx, 0)
                self._owned.append(self._starts)
            self._starts.reserve(max(lay.size, 256), stream=b.stream)
            for i, T, o in zip(idx, frames, offs):
                g = np.ascontiguousarray(starts[i], dtype=np.float64)
                if g.shape != (K, F, T):
                    raise ValueError(f"start of utterance {i} must be K x F x T = {K} x {F} x {T}, got {g.shape}")
                self._starts.view[o:o + g.nbytes] = np.frombuffer(g, dtype=np.uint8)
            ctx.memcpy_h2d_async(self._starts.d, self._starts.h, lay.size, b.stream)
            gptr = [self._starts.d + o for o in offs]
        st = np.zeros(len(idx), dtype=np.int32)
        ctx.cacgmm_estimate_batch(C, aptr, ns, K, self.num_iters, gptr, [b.out.d + o for o in off_out],
                                  stream=b.stream, update_alpha=self.update_alpha, cgmm_init=self.cgmm_init,
                                  status=st)
        b.fetch(n_out)
        for k, i in enumerate(idx):
            out[i] = b.read(off_out[k], K * frames[k] * F, np.float32, (K, frames[k], F))
            status[i] = st[k]
