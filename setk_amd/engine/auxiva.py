"""AuxIVA blind source separation for a batch: setk_auxiva_batch."""
import numpy as np

from .. import _ffi
from ..libs.wavio import float_to_pcm16 as wavio_float_to_pcm16
from ._common import _Engine, host_samples


class BatchSeparator(_Engine):
    """apply_auxiva.py:60-79 for a batch, resident on the device: the STFT of every channel
    straight into the bin-major layout, num_epochs AuxIVA epochs over every (bin, utterance)
    per launch (fp64), the inverse STFT of every source and the renorm to max |input|
    (setk_auxiva_batch), one upload of the samples and one download of the waveforms per
    channel count.  run() takes a list of C x N float32 arrays or Pcm16Frames (any mix of
    channel counts) and returns, per utterance, the C separated sources as a C x L float32
    array (pcm16: int16, quantised on the device by the writer's rule), or None where a bin was
    singular or non-finite (the reference's LinAlgError, apply_auxiva.py:51); `status` then
    holds the SETK_NUM_* value of every utterance of the last run()."""

    def __init__(self, num_epochs=20, frame_len=512, frame_hop=256, center=True,
                 round_power_of_two=True, window="hann", device=None, pcm16=False):
        # no GPU / no library: setk_create fails here, loudly
        super().__init__(_ffi.default_context(device), frame_len, frame_hop, center,
                         round_power_of_two, window)
        self.pcm16 = bool(pcm16)
        self.num_epochs = int(num_epochs)
        self.status = []

    def run(self, utts):
        out = [None] * len(utts)
        self.status = [_ffi.NUM_OK] * len(utts)
        if not len(utts):
            return out
        self._plan()
        groups = self._by_channels(utts)
        if max(groups) > 8:
            raise _ffi.SetkUnsupported(
                f"AuxIVA on the device needs 1 <= channels <= 8 (got {max(groups)} channels)")
        for C, idx in groups.items():
            if self.n_fft == 512:
                self._run_native(utts, C, idx, out)
            else:
                self._run_operators(utts, C, idx, out)
        return out

    def _run_native(self, utts, C, idx, out):
        ctx = self.ctx
        b = self._get_slabs()
        esz = 2 if self.pcm16 else 4
        aptr, ns, off_out, n_out = b.stage_audio(
            [utts[i] for i in idx], C, lambda N: esz * C * ctx.istft_num_samples(ctx.num_frames(N)))
        lens = [ctx.istft_num_samples(ctx.num_frames(N)) for N in ns]
        status = np.zeros(len(idx), dtype=np.int32)
        ctx.auxiva_batch(C, aptr, ns, self.num_epochs, [b.out.d + o for o in off_out], status=status,
                         flags=_ffi.FLAG_OUT_PCM16 if self.pcm16 else 0, stream=b.stream)
        b.fetch(n_out)
        for k, i in enumerate(idx):
            self.status[i] = int(status[k])
            if status[k] == _ffi.NUM_OK:
                L = lens[k]
                out[i] = b.read(off_out[k], C * L, np.int16 if self.pcm16 else np.float32, (C, L))

    def _run_operators(self, utts, C, idx, out):
        """Transform sizes the batched call is not built for: the stand-alone operators
        (setk_stft -> setk_auxiva -> setk_istft), one utterance at a time."""
        ctx, F = self.ctx, self.num_bins
        for i in idx:
            samps = host_samples(utts[i])
            T = ctx.num_frames(samps.shape[1])
            spec = np.empty((C, T, F), dtype=np.complex64)
            ctx.stft(samps, spec)
            sep = np.empty_like(spec)
            status = np.zeros(F, dtype=np.int32)
            ctx.auxiva(spec, C, T, F, self.num_epochs, sep, status=status)
            self.status[i] = int(status.max())
            if self.status[i] != _ffi.NUM_OK:
                continue
            wav = np.empty((C, ctx.istft_num_samples(T)), dtype=np.float32)
            norm = np.full(C, np.max(np.abs(samps)), dtype=np.float32)
            ctx.istft(sep, C, T, None, norm, wav)
            out[i] = wavio_float_to_pcm16(wav) if self.pcm16 else wav
