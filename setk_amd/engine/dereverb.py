"""Dereverberation for a batch: WPE (setk_wpe_batch) and the factorised WPD around it."""
import os

import numpy as np

from .. import _ffi
from ._common import _Engine, _Layout, _Twin, Pcm16Frames, align256, host_samples


class BatchDereverb(_Engine):
    """apply_wpe.py:30-66 for a batch, resident on the device: the STFT of every channel,
    num_iters WPE steps over every (bin, utterance) per launch (setk_wpe_batch, fp64) and
    the inverse STFT of every channel (inverse_stft with norm = None), one upload of the
    samples and one download of the waveforms per batch.  run() takes a list of C x N
    float32 arrays or Pcm16Frames with the same channel count and returns C x L float32
    arrays (pcm16: L x C int16 frames, ready for the wav writer), None where the tap
    correlation of a bin is singular (the reference's LinAlgError, apply_wpe.py:55-57)."""

    def __init__(self, taps=10, delay=3, context=1, num_iters=3, frame_len=512, frame_hop=256,
                 center=True, round_power_of_two=True, window="hann", device=None, pcm16=False):
        # no GPU / no library: setk_create fails here, loudly.  The n_fft = 512 path brings its
        # own buffers and stream; torch is the plumbing of the other transform sizes only.
        super().__init__(_ffi.default_context(device), frame_len, frame_hop, center,
                         round_power_of_two, window)
        self._scratch = _Twin(self.ctx, 0, host=False)  # spectrograms (and float waveforms)
        self._owned.append(self._scratch)
        # pcm16: hand back interleaved int16 frames L x C, quantised on the device by the
        # writer's rule (wavio.float_to_pcm16: rint(x * 32767) in float64, wrapping)
        self.pcm16 = bool(pcm16)
        self.taps, self.delay, self.context, self.num_iters = taps, delay, context, num_iters
        self.rank_deficient_bins = 0  # SETK_NUM_RANKDEF notes seen so far (apply_wpe logs them)

    def run(self, utts):
        if not len(utts):
            return []
        self._plan()
        C = self._same_channels(utts)
        if self.n_fft == 512 and C <= 8:
            return self._run_native(utts, C)
        return self._run_torch(utts, C)

    def _run_native(self, utts, C):
        """One slab of samples up, setk_stft_batch -> setk_wpe_batch -> setk_istft (->
        setk_float_to_pcm16), one slab of waveforms down: the library's own buffers and stream."""
        ctx, F = self.ctx, self.num_bins
        b = self._get_slabs()
        esz = 2 if self.pcm16 else 4
        aptr, ns, off_out, n_out = b.stage_audio(
            utts, C, lambda N: esz * C * ctx.istft_num_samples(ctx.num_frames(N)))
        frames = [ctx.num_frames(N) for N in ns]
        lens = [ctx.istft_num_samples(T) for T in frames]
        # scratch: spectrogram in / out per utterance, float waveforms when PCM16 goes out
        lay, spec_in, spec_out, wav32 = _Layout(), [], [], []
        for T, L in zip(frames, lens):
            spec_in.append(lay.take(8 * C * T * F))
            spec_out.append(lay.take(8 * C * T * F))
            wav32.append(lay.take(4 * C * L if self.pcm16 else 0))
        self._scratch.reserve(lay.size, b.stream)
        base = self._scratch.d
        ctx.stft_batch(C, aptr, ns, [base + o for o in spec_in], stream=b.stream)
        status = np.zeros((len(utts), F), dtype=np.int32)
        ctx.wpe_batch([base + o for o in spec_in], C, frames, F, self.taps, self.delay, self.context,
                      self.num_iters, [base + o for o in spec_out], status=status, stream=b.stream)
        for k, (T, L) in enumerate(zip(frames, lens)):
            self._istft_out(base + spec_out[k], C, T, L, None, base + wav32[k], b.out.d + off_out[k],
                            b.stream)
        b.fetch(n_out)
        out = []
        self.rank_deficient_bins += int(np.count_nonzero(status == _ffi.NUM_RANKDEF))
        for k, L in enumerate(lens):
            if _ffi.wpe_failed(status[k]).any():
                out.append(None)
            elif self.pcm16:
                out.append(b.read(off_out[k], C * L, np.int16, (L, C)))
            else:
                out.append(b.read(off_out[k], C * L, np.float32, (C, L)))
        return out

    def _run_torch(self, utts, C):
        torch, ctx, dev, F = self.torch, self.ctx, self.dev, self.num_bins
        audio, ns = [], []
        for samps in utts:
            a, N = self._upload(samps, C)
            audio.append(a)
            ns.append(N)
        frames = [ctx.num_frames(N) for N in ns]
        specs = [torch.empty((C, T, F), dtype=torch.complex64, device=dev) for T in frames]
        if self.n_fft == 512 and C <= 8:
            ctx.stft_batch(C, [a.data_ptr() for a in audio], ns, [t.data_ptr() for t in specs])
        else:
            for a, t in zip(audio, specs):
                ctx.stft(a, t)
        outs = [torch.empty_like(t) for t in specs]
        status = np.zeros((len(utts), F), dtype=np.int32)
        ctx.wpe_batch(specs, C, frames, F, self.taps, self.delay, self.context, self.num_iters,
                      outs, status=status)
        lens = [ctx.istft_num_samples(T) for T in frames]
        waves = torch.empty((C * sum(lens),), dtype=torch.float32, device=dev)
        views, off = [], 0
        for t, T, L in zip(outs, frames, lens):
            w = waves[off:off + C * L].view(C, L)
            ctx.istft(t, C, T, None, None, w)
            views.append((off, L))
            off += C * L
        if self.pcm16:
            q = torch.round(waves.double() * 32767.0).to(torch.int64).to(torch.int16)
            # channel-major C x L per utterance -> interleaved frames L x C
            host = torch.cat([q[o:o + C * L].view(C, L).t().reshape(-1) for o, L in views]).cpu().numpy()
            return [None if _ffi.wpe_failed(status[u]).any() else host[o:o + C * L].reshape(L, C)
                    for u, (o, L) in enumerate(views)]
        host = waves.cpu().numpy()
        return [None if _ffi.wpe_failed(status[u]).any() else host[o:o + C * L].reshape(C, L)
                for u, (o, L) in enumerate(views)]


class BatchWpd(_Engine):
    """Factorised WPD (joint dereverberation and denoising) for a batch, resident on the device.

    Replaces the per-utterance body of funcwj/setk scripts/sptk/apply_wpd.py:31-57 around
    libs/wpe.py:113-177 (facted_wpd): per outer iteration one WPE step with the variances of the
    previous enhanced signal, a K = 2 CGMM on the dereverberated channels, the power-weighted
    and the mask-weighted covariance, the MVDR weights and the beamformer.  Where the numpy
    mirror (setk_amd.libs.wpe.facted_wpd) carries every intermediate through host arrays, here
    the samples of a batch go up once, setk_stft_batch writes the spectrograms, and every stage
    works on device pointers of one scratch block, outer iteration by outer iteration: setk_wpe per
    utterance, ONE setk_cgmm_masks_batch for the batch, setk_covar x 2 -> setk_weights ->
    setk_beamform per utterance, then setk_istft with the renorm to max |samples|
    (SpectrogramReader.maxabs) and the float -> PCM_16 conversion; one slab comes down per batch:
    [wave | status words | speech mask].  run() takes C x N float32 arrays or Pcm16Frames of one
    channel count and returns [(wave, mask T x F float32) | None]; None is the reference's
    LinAlgError (singular tap correlation or power-weighted covariance).  The transform sizes the
    fused STFT does not serve (n_fft != 512, more than 8 channels) go through the numpy mirror."""

    def __init__(self, taps=10, delay=3, context=1, wpd_iters=3, cgmm_iters=20, update_alpha=False,
                 frame_len=512, frame_hop=256, center=True, round_power_of_two=True, window="hann",
                 device=None, pcm16=False):
        ctx = _ffi.default_context(device)
        self.taps, self.delay, self.context = int(taps), int(delay), int(context)
        self.wpd_iters, self.cgmm_iters = int(wpd_iters), int(cgmm_iters)
        self.update_alpha = bool(update_alpha)
        self.pcm16 = bool(pcm16)
        super().__init__(ctx, frame_len, frame_hop, center, round_power_of_two, window)
        self.rank_deficient_bins = 0
        self._scratch = _Twin(ctx, 0, host=False)
        self._owned.append(self._scratch)
        self._cgmm_per_utt = os.environ.get("SETK_WPD_CGMM_PER_UTT") == "1"

    def run(self, utts):
        if not len(utts):
            return []
        self._plan()
        C = self._same_channels(utts)
        if self.n_fft == 512 and C <= 8:
            return self._run_resident(utts, C)
        return [self._one_by_mirror(u) for u in utts]

    @staticmethod
    def _peak(samps):
        if isinstance(samps, Pcm16Frames):
            return float(np.abs(samps.frames.astype(np.int32)).max()) / 32768.0 if samps.frames.size else 0.0
        return float(np.max(np.abs(samps))) if np.size(samps) else 0.0

    def _run_resident(self, utts, C):
        ctx, F, K = self.ctx, self.num_bins, self.wpd_iters
        b = self._get_slabs()
        al = align256
        esz = 2 if self.pcm16 else 4
        n_status = K * F  # per outer iteration: the MVDR solve (WPE's words come back with its call)

        def out_bytes(N):
            T = ctx.num_frames(N)
            return al(esz * ctx.istft_num_samples(T)) + al(4 * n_status) + al(4 * T * F) + 256

        aptr, ns, off_out, n_out = b.stage_audio(utts, C, out_bytes)
        frames = [ctx.num_frames(N) for N in ns]
        lens = [ctx.istft_num_samples(T) for T in frames]
        # scratch per utterance: spectrogram, dereverberated channels, 1 / lambda,
        # two covariances, weights, enhanced spectrum, float wave (PCM16 output)
        lay, scratch = [], _Layout()
        take = scratch.take
        for T, L in zip(frames, lens):
            lay.append(dict(spec=take(8 * C * T * F), der=take(8 * C * T * F), inv=take(4 * T * F),
                            Rd=take(8 * F * C * C), Rs=take(8 * F * C * C),
                            w=take(8 * F * C), enh=take(8 * T * F), wav=take(4 * L), norm=take(256)))
        self._scratch.reserve(scratch.size, b.stream)
        base, st = self._scratch.d, b.stream
        ctx.stft_batch(C, aptr, ns, [base + q["spec"] for q in lay], stream=st)
        mvdr = _ffi.BfOpts(kind=_ffi.BF_MVDR)
        peaks = [np.array([self._peak(u)], dtype=np.float32) for u in utts]  # (kept alive until the fetch)
        # the output slab per utterance: [wave | status words | speech mask]
        o_wave = off_out
        o_stat = [o + al(esz * L) for o, L in zip(o_wave, lens)]
        o_mask = [o + al(4 * n_status) for o in o_stat]
        d_wave, d_stat, d_mask = ([b.out.d + o for o in offs] for offs in (o_wave, o_stat, o_mask))
        # iteration-major: the CGMM of an outer iteration is ONE launch over (bin, utterance) for
        # the whole batch -- 257 workgroups of one 10 s utterance fill an eighth of the chip, and the
        # EM's 22 passes are latency, not throughput, at that size
        wpe_status = np.zeros((K, len(utts), F), dtype=np.int32)
        for it in range(K):
            # (the WPE step too: one launch over (bin, utterance); its status words come back with
            # the call, which drains the stream as every setk_wpe* call does)
            ctx.wpe_batch_var([base + q["spec"] for q in lay], C, frames, F, self.taps, self.delay,
                              self.context, 1, [base + q["der"] for q in lay],
                              lambda_enh=[base + q["enh"] for q in lay] if it else None,
                              inv_lambda_outs=[base + q["inv"] for q in lay], status=wpe_status[it],
                              stream=st)
            if self._cgmm_per_utt:  # A/B only (SETK_WPD_CGMM_PER_UTT=1): one EM launch per utterance
                for k, (q, T) in enumerate(zip(lay, frames)):
                    ctx.cgmm_masks_batch(C, [base + q["der"]], [T], F, self.cgmm_iters, None, [d_mask[k]],
                                         stream=st, update_alpha=self.update_alpha)
            else:
                ctx.cgmm_masks_batch(C, [base + q["der"] for q in lay], frames, F, self.cgmm_iters, None,
                                     d_mask, stream=st, update_alpha=self.update_alpha)
            for k, (q, T) in enumerate(zip(lay, frames)):
                p = lambda name: base + q[name]  # noqa: E731
                # the mask 1 / lambda gives the power-weighted covariance up to a per-bin scale
                # that cancels in the MVDR weight
                ctx.covar(p("der"), p("inv"), C, T, F, p("Rd"), stream=st)
                ctx.covar(p("der"), d_mask[k], C, T, F, p("Rs"), stream=st)
                ctx.weights(mvdr, p("Rs"), p("Rd"), None, F, C, p("w"), d_stat[k] + 4 * F * it, stream=st)
                ctx.beamform(p("w"), p("der"), C, T, F, p("enh"), stream=st)
        for k, (q, T, L) in enumerate(zip(lay, frames, lens)):
            ctx.memcpy_h2d_async(base + q["norm"], peaks[k].ctypes.data, 4, st)
            self._istft_out(base + q["enh"], 1, T, L, base + q["norm"], base + q["wav"], d_wave[k], st)
        b.fetch(n_out)
        out = []
        for k, (T, L) in enumerate(zip(frames, lens)):
            status = b.read(o_stat[k], n_status, np.int32, (K, F))
            self.rank_deficient_bins += int(np.count_nonzero(wpe_status[:, k] == _ffi.NUM_RANKDEF))
            if _ffi.wpe_failed(wpe_status[:, k]).any() or status.any():
                out.append(None)
                continue
            wave = b.read(o_wave[k], L, np.int16 if self.pcm16 else np.float32)
            out.append((wave, b.read(o_mask[k], T * F, np.float32, (T, F))))
        return out

    def _one_by_mirror(self, samps):
        from ..libs.utils import forward_stft, inverse_stft
        from ..libs.wpe import facted_wpd
        from ..libs import wavio
        samps = host_samples(samps)
        s = self.stft
        kw = dict(frame_len=s["frame_len"], frame_hop=s["frame_hop"], center=s["center"], window=self.window_name)
        obs = np.stack([forward_stft(ch, round_power_of_two=self.round_power_of_two, transpose=True, **kw)
                        for ch in samps])  # N x T x F
        try:
            tf_mask, enh = facted_wpd(obs, wpd_iters=self.wpd_iters, cgmm_iters=self.cgmm_iters,
                                      update_alpha=self.update_alpha, context=self.context,
                                      taps=self.taps, delay=self.delay)
        except np.linalg.LinAlgError:
            return None
        wave = inverse_stft(enh, norm=float(np.max(np.abs(samps))), transpose=True, **kw)
        if self.pcm16:
            wave = wavio.float_to_pcm16(wave)
        return wave, tf_mask[..., 0].astype(np.float32)
