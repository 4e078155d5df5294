"""
Batched front end of the fused hot path (setk_enhance_batch): takes decoded
utterances (numpy), keeps them resident in HBM through torch tensors, runs the
four kernel stages for the whole batch and hands back PCM16 / float32 waves.

This is the compute body of apply_adaptive_beamformer.py:130-178 for many
utterances at once -- per-utterance work is microseconds on an MI355X, so the
engineering unit is the batch, not the utterance.
"""
import numpy as np

from .. import _ffi
from ._common import (_Engine, BEAMFORMER_KINDS, RANK1, Pcm16Frames, channels_and_size, compute_vad_masks,
                      host_samples)


class BatchEnhancer(_Engine):
    _no_gpu = "BatchEnhancer needs an MI355X (no CPU fallback)"

    def __init__(self, beamformer="mvdr", frame_len=512, frame_hop=256, center=True,
                 round_power_of_two=True, window="hann", ban=False, pmwf_ref=-1, rank1_appro="",
                 post_mask=False, vad_proportion=1, pcm16=False, device=None, ctx=None,
                 max_batch_samples=1 << 28, strict_reference=False, max_wide_bytes=3 << 30):
        """strict_reference: refuse (status SETK_NUM_SINGULAR -> the CLI's LinAlgError branch)
        exactly where the reference's numpy.linalg.solve meets an exactly zero pivot
        (SETK_FLAG_STRICT_REFERENCE, include/setk_hip.h); default: regularise and go through.
        max_wide_bytes: 9 to 16 channels keep their spectra on the device between the stages of
        the batched call; a batch is cut where what its utterances take (_wide_bytes) would pass
        this."""
        if beamformer not in BEAMFORMER_KINDS:
            raise ValueError(f"unknown beamformer {beamformer}")
        # no GPU / no library: setk_create fails here, loudly (there is no CPU fallback).
        # torch is the plumbing of enhance() only -- the streaming pipeline brings its own
        # buffers and streams -- and is imported when enhance() first needs it.
        super().__init__(ctx or _ffi.default_context(device), frame_len, frame_hop, center,
                         round_power_of_two, window)
        kind, beta = BEAMFORMER_KINDS[beamformer]
        flags = 0
        if ban:
            flags |= _ffi.FLAG_BAN
        if post_mask:
            flags |= _ffi.FLAG_POST_MASK
        if pcm16:
            flags |= _ffi.FLAG_OUT_PCM16
        if strict_reference:
            flags |= _ffi.FLAG_STRICT_REFERENCE
        self.base_flags = flags
        self.opts_kw = dict(kind=kind, pmwf_beta=beta, pmwf_ref=int(pmwf_ref),
                            rank1=RANK1[rank1_appro])
        self.pcm16 = pcm16
        # wave files' 16-bit samples go into the fused kernels as stored (de-interleaved, never
        # widened to float32) when the geometry is the matrix-core pass 2's: hop = n_fft / 2
        # (the two library switches are read the way csrc/capi_fused.hip and csrc/capi_handle.hip
        #  read them -- atoi -- so that e.g. SETK_MC_PASS2=false disables the form on both sides
        #  of the ABI)
        self.pcm_direct_ok = self.n_fft == 512 and 2 * frame_hop == self.n_fft and \
            _ffi.env_atoi("SETK_PCM16_DIRECT", 1) != 0 and \
            _ffi.env_atoi("SETK_MC_PASS2", 1) != 0 and _ffi.env_atoi("SETK_LEGACY_FFT", 0) == 0
        self.vad_proportion = vad_proportion
        self.max_batch_samples = max_batch_samples
        self.max_wide_bytes = max_wide_bytes

    def frames_and_length(self, num_samples):
        """(T, L) of the planned transform for a signal of num_samples, evaluated on
        the host (librosa's framing: SURVEY appendix A)."""
        s = self.stft
        hop, n_fft = s["frame_hop"], s["n_fft"]
        if s["center"]:
            if num_samples < n_fft // 2 + 1:
                raise ValueError("signal shorter than n_fft/2+1 (reflect padding)")
            T = 1 + num_samples // hop
            return T, hop * (T - 1)
        if num_samples < n_fft:
            raise ValueError("signal shorter than n_fft")
        T = 1 + (num_samples - n_fft) // hop
        return T, n_fft + hop * (T - 1)

    def condition_mask(self, mask, num_frames):
        """apply_adaptive_beamformer.py:146-151: masks arrive T x F or F x T."""
        F = self.num_bins
        mask = np.asarray(mask)
        if mask.ndim != 2:
            raise ValueError(f"mask must be 2D, got {mask.shape}")
        if mask.shape[0] == F and mask.shape[1] != F:
            mask = np.transpose(mask)
        if mask.shape[1] != F:
            raise ValueError("Input mask matrix should be shape as " +
                             f"[num_frames x num_bins], now is {mask.shape}")
        if mask.shape[0] != num_frames:
            raise ValueError("Shape of input obs do not match with mask matrix, " +
                             f"{num_frames} frames vs {mask.shape}")
        return mask

    def enhance(self, utts):
        """utts: list of (samps C x N float32 | Pcm16Frames, speech mask, interferer mask|None).
        Returns list of (wave ndarray | None, status) in input order; status != 0
        is the reference's LinAlgError case (the utterance is to be skipped)."""
        self._plan()
        results = [None] * len(utts)
        samps = [u[0] for u in utts]
        groups = self._by_channels(samps, also=[u[2] is not None for u in utts])
        for (C, has_itf), idx in groups.items():
            if self._wide(C):
                batches = self._wide_batches(idx, samps, C)
            else:
                batches = self._batches(idx, samps, self.max_batch_samples)
            for batch in batches:
                self._run(utts, batch, C, has_itf, results)
        return results

    def _wide(self, C):
        """9 to 16 channels on the 512-point transform go through the batched call's wide path
        (csrc/wide.hip); the VAD filter needs the spectrogram on the host and stays unfused."""
        return self.n_fft == 512 and 8 < C <= 16 and not (0.5 < self.vad_proportion < 1)

    def _wide_bytes(self, samps, C):
        """What an utterance of the wide path takes on the device: samples, two masks, the wave,
        and the call's scratch as include/setk_hip.h states it -- the bin-major spectra, the
        beamformed spectrogram, a covariance slab per 128 frames, the planes and the weights."""
        n = channels_and_size(samps)[1]
        T, L = self.frames_and_length(n // C)
        F, Tp, slabs = self.num_bins, (T + 3) & ~3, -(-T // 128)
        scratch = 8 * F * C * Tp + 8 * T * F + slabs * F * 824 * 4 + 264 * 4 * (6 * 136 + 2 * 16) + 4 * L
        return 4 * n + 2 * 4 * T * F + 4 * L + scratch

    def _wide_batches(self, idx, samps, C):
        batch, load = [], 0
        for i in idx:
            n = self._wide_bytes(samps[i], C)
            if batch and load + n > self.max_wide_bytes:
                yield batch
                batch, load = [], 0
            batch.append(i)
            load += n
        if batch:
            yield batch

    def _run_unfused(self, utts, batch, C, has_itf, results):
        """n_fft != 512, more than 16 channels, or 9 to 16 with the VAD filter: the same stages
        through the stand-alone operators (setk_stft -> setk_covar x2 -> setk_weights ->
        setk_beamform -> setk_istft), everything resident on the device, one
        utterance at a time."""
        torch, ctx, dev, F = self.torch, self.ctx, self.dev, self.num_bins
        mpdr = self.opts_kw["kind"] in (_ffi.BF_MPDR, _ffi.BF_MPDR_WHITEN)
        for i in batch:
            samps, mask, itf = utts[i]
            samps = host_samples(samps)
            N = samps.shape[1]
            T = ctx.num_frames(N)
            mask = self.condition_mask(mask, T)
            if has_itf:
                itf = self.condition_mask(itf, T)
            else:
                mask = np.minimum(mask, 1)
            a = torch.from_numpy(samps).to(dev)
            spec = torch.empty((C, T, F), dtype=torch.complex64, device=dev)
            ctx.stft(a, spec)
            if 0.5 < self.vad_proportion < 1:
                vad, _ = compute_vad_masks(spec[0].cpu().numpy().T, self.vad_proportion)
                mask = np.where(vad, 1.0e-4, mask)
                if has_itf:
                    itf = np.where(vad, 1.0e-4, itf)
            ms = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev)
            mn = torch.from_numpy(np.ascontiguousarray(itf, dtype=np.float32)).to(dev) \
                if has_itf else (1 - ms).contiguous()
            Rs = torch.empty((F, C, C), dtype=torch.complex64, device=dev)
            Rn = torch.empty_like(Rs)
            ctx.covar(spec, mn, C, T, F, Rn)
            ctx.covar(spec, ms, C, T, F, Rs)
            Ry = None
            if mpdr:
                Ry = torch.empty_like(Rs)
                ctx.covar(spec, torch.ones_like(ms), C, T, F, Ry)
            w = torch.empty((F, C), dtype=torch.complex64, device=dev)
            status = np.zeros(F, dtype=np.int32)
            flags = self.base_flags & (_ffi.FLAG_BAN | _ffi.FLAG_STRICT_REFERENCE)
            ctx.weights(_ffi.BfOpts(flags=flags, **self.opts_kw), Rs, Rn, Ry, F, C, w, status)
            if status.any():
                results[i] = (None, int(status.max()))
                continue
            enh = torch.empty((T, F), dtype=torch.complex64, device=dev)
            ctx.beamform(w, spec, C, T, F, enh)
            if self.base_flags & _ffi.FLAG_POST_MASK:
                enh = (enh * ms).contiguous()
            results[i] = (self._unfused_tail(enh, T, a), 0)

    def _run(self, utts, batch, C, has_itf, results):
        if self.n_fft != 512 or (C > 8 and not self._wide(C)):
            # the batched call is specialised for n_fft = 512 and C <= 16 (9 to 16: csrc/wide.hip)
            return self._run_unfused(utts, batch, C, has_itf, results)
        kind = self.opts_kw["kind"]
        if has_itf and kind == _ffi.BF_MPDR_WHITEN:
            # the fused kernel forms Ry from mask_s + (1 - mask_s); with a separate
            # interferer mask Rn and Ry are independent (libs/beamformer.py:573-590)
            return self._run_unfused(utts, batch, C, has_itf, results)
        drop_itf = has_itf and kind == _ffi.BF_MPDR  # plain MPDR never reads mask_n
        torch, ctx, dev = self.torch, self.ctx, self.dev
        audio, masks, itfs, waves, ns = [], [], [], [], []
        flags = self.base_flags | (0 if has_itf else _ffi.FLAG_CLAMP_MASK)
        # 16-bit PCM all the way into the kernels (SETK_FLAG_IN_PCM16): no float32 copy exists
        direct = self.pcm_direct_ok and C <= 8 and all(isinstance(utts[i][0], Pcm16Frames) for i in batch) \
            and not (0.5 < self.vad_proportion < 1)
        if direct:
            flags |= _ffi.FLAG_IN_PCM16
        staged = []  # (interleaved frames on the device, N, planar destination)
        for i in batch:
            samps, mask, itf = utts[i]
            if direct:
                pcm = torch.from_numpy(samps.frames).to(dev)
                N = samps.frames.shape[0]
                a = torch.empty((C, ctx.pcm16_channel_stride(N)), dtype=torch.int16, device=dev)
                staged.append((pcm, N, a))
            else:
                a, N = self._upload(samps, C)
            T = ctx.num_frames(N)
            mask = self.condition_mask(mask, T)
            if has_itf:
                itf = self.condition_mask(itf, T)
            if 0.5 < self.vad_proportion < 1:
                spec0 = torch.empty((1, T, self.num_bins), dtype=torch.complex64, device=dev)
                ctx.stft(a[:1], spec0)
                vad, _ = compute_vad_masks(spec0[0].cpu().numpy().T, self.vad_proportion)
                if not has_itf:
                    mask = np.minimum(mask, 1)
                mask = np.where(vad, 1.0e-4, mask)
                if has_itf:
                    itf = np.where(vad, 1.0e-4, itf)
            audio.append(a)
            masks.append(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev))
            if has_itf and not drop_itf:
                itfs.append(torch.from_numpy(np.ascontiguousarray(itf, dtype=np.float32)).to(dev))
            L = ctx.istft_num_samples(T)
            waves.append(torch.empty(L, dtype=torch.int16 if self.pcm16 else torch.float32,
                                     device=dev))
            ns.append(N)
        if staged:
            ctx.pcm16_deinterleave_batch(C, [p.data_ptr() for p, _, _ in staged], [n for _, n, _ in staged],
                                         [a.data_ptr() for _, _, a in staged])
        opts = _ffi.BfOpts(flags=flags, **self.opts_kw)
        status = ctx.enhance_batch(opts, C, [t.data_ptr() for t in audio], ns,
                                   [t.data_ptr() for t in masks],
                                   [t.data_ptr() for t in itfs] if itfs else None,
                                   [t.data_ptr() for t in waves], want_status=True)
        for j, i in enumerate(batch):
            results[i] = (waves[j].cpu().numpy() if status[j] == 0 else None, status[j])
