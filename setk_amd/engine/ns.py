"""OM-LSA noise suppression for a batch of single-channel utterances: setk_ns_batch."""
import numpy as np

from .. import _ffi
from ..libs.wavio import float_to_pcm16 as wavio_float_to_pcm16
from ._common import _Engine, channels_and_size, host_samples


class BatchNoiseSuppressor(_Engine):
    """apply_ns.py:37-49 for a batch, resident on the device: the samples of the batch go up in
    one slab, ONE STFT launch, ONE launch of the MCRA / iMCRA recursion (a workgroup per
    utterance, float64), ONE inverse-STFT launch (setk_ns_batch), one slab comes down.

    suppressor  a libs.ns.MCRA or libs.ns.iMCRA (the CLI builds iMCRA(**conf))
    output      "wave": the enhanced waveform inverse_stft(gain * stft) of every utterance, float32
                (pcm16: int16, rounded on the device by the writer's rule); "gain": the T x F
                float64 gain
    run() takes [samps N (or 1 x N) float32 | Pcm16Frames with one channel] and returns the list
    of results (16-bit frames go up as stored and are converted on the device in front of the
    call, as in the other engines); `status` then holds the SETK_NUM_* value of every utterance
    of the last run() (SETK_NUM_NONFINITE: NaN / inf in the samples; the result of such an
    utterance is None).
    Transform sizes other than 512 go through the stand-alone operators (setk_stft ->
    setk_ns_gain -> setk_istft), one utterance at a time."""

    def __init__(self, suppressor, output="wave", eps=1e-7, frame_len=512, frame_hop=256, center=True,
                 round_power_of_two=True, window="hann", device=None, pcm16=False, max_batch_samples=1 << 26):
        super().__init__(_ffi.default_context(device), frame_len, frame_hop, center, round_power_of_two, window)
        if output not in ("wave", "gain"):
            raise ValueError(f"output must be wave or gain, got {output}")
        self.suppressor = suppressor
        self.output = output
        self.eps = eps
        self.pcm16 = bool(pcm16)
        self.max_batch_samples = max_batch_samples
        self.status = []
        # refusals that do not depend on the input come at construction, not per batch
        for name in ("w_mcra", "w_local", "w_global"):
            w = suppressor._fields.get(name)
            if w is not None and len(w) > self.num_bins:
                raise _ffi.SetkUnsupported(f"{name}: {len(w)} taps for {self.num_bins} bins")

    def _opts(self):
        return self.suppressor.opts(self.eps, gain=self.output == "gain", spec=self.output == "wave")

    def run(self, utts):
        out = [None] * len(utts)
        self.status = [_ffi.NUM_OK] * len(utts)
        if not len(utts):
            return out
        if any(channels_and_size(u)[0] != 1 for u in utts):
            raise ValueError("noise suppression takes single-channel utterances")
        self._plan()
        idx = list(range(len(utts)))
        if self.n_fft != 512:
            self._run_operators(utts, idx, out)
            return out
        for batch in self._batches(idx, utts, self.max_batch_samples):
            self._run_native(utts, batch, out)
        return out

    def _run_native(self, utts, idx, out):
        ctx, F = self.ctx, self.num_bins
        b = self._get_slabs()
        wave = self.output == "wave"
        esz = 2 if self.pcm16 else 4

        def out_bytes(N):
            T = ctx.num_frames(N)
            return esz * ctx.istft_num_samples(T) if wave else 8 * T * F

        aptr, ns, off_out, n_out = b.stage_audio([utts[i] for i in idx], 1, out_bytes)
        frames = [ctx.num_frames(N) for N in ns]
        status = np.zeros(len(idx), dtype=np.int32)
        optr = [b.out.d + o for o in off_out]
        ctx.ns_batch(self._opts(), aptr, ns, wave_ptrs=optr if wave else None, gain_ptrs=None if wave else optr,
                     status=status, flags=_ffi.FLAG_OUT_PCM16 if wave and self.pcm16 else 0, stream=b.stream)
        b.fetch(n_out)
        for k, i in enumerate(idx):
            self.status[i] = int(status[k])
            if status[k] != _ffi.NUM_OK:
                continue
            if wave:
                L = ctx.istft_num_samples(frames[k])
                out[i] = b.read(off_out[k], L, np.int16 if self.pcm16 else np.float32)
            else:
                out[i] = b.read(off_out[k], frames[k] * F, np.float64, (frames[k], F))

    def _run_operators(self, utts, idx, out):
        ctx, F = self.ctx, self.num_bins
        wave = self.output == "wave"
        for i in idx:
            samps = host_samples(utts[i])
            T = ctx.num_frames(samps.shape[1])
            spec = np.empty((1, T, F), dtype=np.complex64)
            ctx.stft(samps, spec)
            status = np.zeros(1, dtype=np.int32)
            if wave:
                enh = np.empty((1, T, F), dtype=np.complex64)
                ctx.ns_gain(self._opts(), spec, T, F, out=enh, status=status)
            else:
                gain = np.empty((T, F), dtype=np.float64)
                ctx.ns_gain(self._opts(), spec, T, F, gain=gain, status=status)
            self.status[i] = int(status[0])
            if status[0] != _ffi.NUM_OK:
                continue
            if not wave:
                out[i] = gain
                continue
            wav = np.empty((1, ctx.istft_num_samples(T)), dtype=np.float32)
            ctx.istft(enh, 1, T, None, None, wav)
            out[i] = wavio_float_to_pcm16(wav)[0] if self.pcm16 else wav[0]
