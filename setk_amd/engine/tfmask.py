"""Oracle TF masks, mask-based separation and oracle separation for batches of utterances:
setk_tf_mask_batch, setk_tf_separate_batch, setk_oracle_separate_batch."""
import numpy as np

from .. import _ffi
from ..libs.wavio import float_to_pcm16 as wavio_float_to_pcm16
from ._common import Pcm16Frames, _Engine, _Layout, channels_and_size, host_samples


def first_channel(u):
    """Channel 0 of an utterance (`clean[0]` in the reference's tools): 16-bit frames stay 16-bit
    (N x 1), anything else becomes N float32 samples."""
    if isinstance(u, Pcm16Frames):
        return u if u.num_channels == 1 else Pcm16Frames(u.frames[:, :1])
    return np.ascontiguousarray(host_samples(u)[0])


def _length(u):
    return u.frames.shape[0] if isinstance(u, Pcm16Frames) else u.shape[0]


def _maxabs(u):
    """WaveReader.maxabs of a first channel: max |x| of the float32 samples."""
    if isinstance(u, Pcm16Frames):
        return float(np.float32(np.abs(u.frames.astype(np.int32)).max()) / np.float32(32768.0))
    return float(np.abs(u).max())


class _TfEngine(_Engine):
    """What the three engines share: channel 0 of every signal, one upload slab holding the
    signals of a batch as they are (all 16-bit: the kernel reads them as stored; otherwise all
    float32), one download slab, `status` per utterance of the last run()."""

    def __init__(self, frame_len, frame_hop, center, round_power_of_two, window, device, max_batch_samples):
        super().__init__(_ffi.default_context(device), frame_len, frame_hop, center, round_power_of_two, window)
        self.max_batch_samples = max_batch_samples
        self.status = []

    @staticmethod
    def _same_length(key, signals):
        n = _length(signals[0])
        if any(_length(s) != n for s in signals[1:]):
            raise ValueError(f"utterance {key}: the signals are of different length "
                             f"({[_length(s) for s in signals]})")
        return n

    def _stage(self, signals, arrays, out_bytes):
        """signals: first channels (the whole batch 16-bit, or float32 samples); arrays: float32
        arrays that go up behind them.  Returns (slabs, 16-bit?, signal pointers, array pointers,
        output offsets)."""
        b = self._get_slabs()
        pcm = all(isinstance(s, Pcm16Frames) for s in signals)
        if not pcm:
            signals = [s.to_float()[0] if isinstance(s, Pcm16Frames) else s for s in signals]
        l_in, l_out = _Layout(), _Layout()
        o_sig = [l_in.take((2 if pcm else 4) * _length(s)) for s in signals]
        o_arr = [l_in.take(a.nbytes) for a in arrays]
        o_out = [l_out.take(n) for n in out_bytes]
        b.reserve(max(l_in.size, 256), 256, max(l_out.size, 256))
        view = b.inp.view
        for s, o in zip(signals, o_sig):
            raw = np.frombuffer(s.frames if pcm else np.ascontiguousarray(s, dtype=np.float32), dtype=np.uint8)
            view[o:o + raw.shape[0]] = raw
        for a, o in zip(arrays, o_arr):
            view[o:o + a.nbytes] = np.frombuffer(a, dtype=np.uint8)
        self.ctx.memcpy_h2d_async(b.inp.d, b.inp.h, l_in.size, b.stream)
        self._out_size = l_out.size
        return b, pcm, [b.inp.d + o for o in o_sig], [b.inp.d + o for o in o_arr], o_out

    def _frames(self, n):
        return self.ctx.num_frames(n)

    def _spec(self, x):
        """setk_stft of one first channel on the host path: [T][F] complex64."""
        x = host_samples(x.to_float()[0] if isinstance(x, Pcm16Frames) else x)
        S = np.empty((1, self._frames(x.shape[1]), self.num_bins), dtype=np.complex64)
        self.ctx.stft(x, S)
        return S[0]

    def _wave(self, spec, nsamps, norm, pcm16):
        T = spec.shape[0]
        wav = np.empty((1, self.ctx.istft_num_samples(T, nsamps)), dtype=np.float32)
        self.ctx.istft(np.ascontiguousarray(spec[None]), 1, T, nsamps,
                       None if norm is None else np.array([norm], dtype=np.float32), wav)
        return wavio_float_to_pcm16(wav[0]) if pcm16 else wav[0]


class BatchMaskComputer(_TfEngine):
    """compute_mask.py:128-153 for a batch of (clean, noisy) pairs: both signals of every pair go up
    in one slab, ONE fused launch transforms them and stores the masks alone (setk_tf_mask_batch),
    one slab comes down.

    kind    ibm | irm | iam | psm | psa | crm
    cutoff  > 0: min(mask, cutoff); max(mask, 0) is applied to every kind, as the tool does
    run([(clean, noisy), ...]) -> the masks, float32 T x F (T x 2F for crm); `stats` then holds
    (cells over the cutoff, cells below zero, their sum) and `status` the SETK_NUM_* value of every
    pair (SETK_NUM_NONFINITE: the mask holds NaN / inf -- it is returned all the same, as the
    reference writes it).  Channel 0 of a multi-channel signal is taken.  Transform sizes other
    than 512 go through the stand-alone operators (setk_stft -> setk_tf_mask), one pair at a time."""

    def __init__(self, kind, cutoff=-1.0, frame_len=512, frame_hop=256, center=True, round_power_of_two=True,
                 window="hann", device=None, max_batch_samples=1 << 26):
        super().__init__(frame_len, frame_hop, center, round_power_of_two, window, device, max_batch_samples)
        _ffi.tfmask_kind(kind)
        self.kind, self.cutoff = kind, float(cutoff)
        self.width = self.num_bins * (2 if kind == "crm" else 1)
        self.stats = []

    def run(self, pairs):
        out = [None] * len(pairs)
        self.status = [_ffi.NUM_OK] * len(pairs)
        self.stats = [(0, 0, 0.0)] * len(pairs)
        if not len(pairs):
            return out
        pairs = [(first_channel(t), first_channel(m)) for t, m in pairs]
        for i, p in enumerate(pairs):
            self._same_length(i, p)
        self._plan()
        if self.n_fft != 512:
            for i, (t, m) in enumerate(pairs):
                St, Sm = self._spec(t), self._spec(m)
                mask = np.empty((St.shape[0], self.width), dtype=np.float32)
                self.stats[i] = self.ctx.tf_mask(self.kind, St, Sm, St.shape[0], self.num_bins, mask, self.cutoff)
                self.status[i] = _ffi.NUM_OK if np.isfinite(mask).all() else _ffi.NUM_NONFINITE
                out[i] = mask
            return out
        mixes = [m for _, m in pairs]
        for batch in self._batches(list(range(len(pairs))), mixes, self.max_batch_samples // 2):
            self._run_native(pairs, batch, out)
        return out

    def _run_native(self, pairs, idx, out):
        ns = [_length(pairs[i][1]) for i in idx]
        frames = [self._frames(n) for n in ns]
        signals = [pairs[i][0] for i in idx] + [pairs[i][1] for i in idx]
        b, pcm, sig, _, o_out = self._stage(signals, [], [4 * T * self.width for T in frames])
        n = len(idx)
        status = np.zeros(n, dtype=np.int32)
        stats = self.ctx.tf_mask_batch(self.kind, sig[:n], sig[n:], ns, [b.out.d + o for o in o_out],
                                       cutoff=self.cutoff, status=status, flags=_ffi.FLAG_IN_PCM16 if pcm else 0,
                                       stream=b.stream)
        b.fetch(self._out_size)
        for k, i in enumerate(idx):
            self.status[i], self.stats[i] = int(status[k]), stats[k]
            out[i] = b.read(o_out[k], frames[k] * self.width, np.float32, (frames[k], self.width))


class BatchMaskSeparator(_TfEngine):
    """wav_separate.py:39-75 for a batch: the mixtures (and the phase references) and the masks go
    up in one slab, ONE fused forward launch masks the spectra in registers, ONE inverse-STFT
    launch and one scaling launch (setk_tf_separate_batch), one slab comes down.

    keep_length  the waves have their mixture's length (--keep-length)
    mixed_norm   the waves are scaled to the mixture's max-abs (--use-mixed-norm)
    pcm16        int16 waves, rounded on the device by the writer's rule
    run(mixtures, masks, phase_refs=None) -> the waves.  A mask is T x F; an F x T mask is
    transposed, any other shape is a ValueError (the reference's).  `status`: SETK_NUM_NONFINITE
    where the masked spectrum held NaN / inf."""

    def __init__(self, keep_length=False, mixed_norm=True, pcm16=False, frame_len=512, frame_hop=256, center=True,
                 round_power_of_two=True, window="hann", device=None, max_batch_samples=1 << 26):
        super().__init__(frame_len, frame_hop, center, round_power_of_two, window, device, max_batch_samples)
        self.keep_length, self.mixed_norm, self.pcm16 = bool(keep_length), bool(mixed_norm), bool(pcm16)

    def _mask(self, mask, T):
        mask = np.asarray(mask, dtype=np.float32)
        if mask.ndim == 2 and mask.shape[0] == self.num_bins:
            mask = mask.T
        if mask.shape != (T, self.num_bins):
            raise ValueError("Dimention mismatch between mask and spectrogram"
                             f"({mask.shape[0]} x {mask.shape[-1]} vs {T} x {self.num_bins}), need check configures")
        return np.ascontiguousarray(mask)

    def run(self, mixtures, masks, phase_refs=None):
        n = len(mixtures)
        out = [None] * n
        self.status = [_ffi.NUM_OK] * n
        if not n:
            return out
        if len(masks) != n or (phase_refs is not None and len(phase_refs) != n):
            raise ValueError("one mask (and one phase reference) per mixture")
        self._plan()
        mixes = [first_channel(m) for m in mixtures]
        refs = None if phase_refs is None else [None if r is None else first_channel(r) for r in phase_refs]
        if refs is not None:
            for i, r in enumerate(refs):
                if r is not None:
                    self._same_length(i, (mixes[i], r))
        masks = [self._mask(k, self._frames(_length(m))) for k, m in zip(masks, mixes)]
        if self.n_fft != 512:
            for i, m in enumerate(mixes):
                S = self._spec(m)
                enh = np.empty_like(S)
                self.ctx.tf_apply(S, masks[i], S.shape[0], self.num_bins, enh,
                                  phase_ref=None if refs is None or refs[i] is None else self._spec(refs[i]))
                self.status[i] = _ffi.NUM_OK if np.isfinite(enh.view(np.float32)).all() else _ffi.NUM_NONFINITE
                out[i] = self._wave(enh, _length(m) if self.keep_length else None,
                                    _maxabs(m) if self.mixed_norm else None, self.pcm16)
            return out
        for batch in self._batches(list(range(n)), mixes, self.max_batch_samples // 2):
            self._run_native(mixes, refs, masks, batch, out)
        return out

    def _run_native(self, mixes, refs, masks, idx, out):
        ctx = self.ctx
        ns = [_length(mixes[i]) for i in idx]
        keep = ns if self.keep_length else None
        L = [ctx.istft_num_samples(self._frames(n), n if self.keep_length else None) for n in ns]
        have = [] if refs is None else [k for k, i in enumerate(idx) if refs[i] is not None]
        signals = [mixes[i] for i in idx] + [refs[idx[k]] for k in have]
        esz = 2 if self.pcm16 else 4
        b, pcm, sig, arr, o_out = self._stage(signals, [masks[i] for i in idx], [esz * max(n, 1) for n in L])
        n = len(idx)
        phase = None
        if have:
            phase = [None] * n
            for j, k in enumerate(have):
                phase[k] = sig[n + j]
        status = np.zeros(n, dtype=np.int32)
        norm = [_maxabs(mixes[i]) for i in idx] if self.mixed_norm else None
        ctx.tf_separate_batch(sig[:n], ns, arr, [b.out.d + o for o in o_out], phase_ptrs=phase, norm=norm,
                              nsamps=keep, status=status,
                              flags=(_ffi.FLAG_IN_PCM16 if pcm else 0) | (_ffi.FLAG_OUT_PCM16 if self.pcm16 else 0),
                              stream=b.stream)
        b.fetch(self._out_size)
        for k, i in enumerate(idx):
            self.status[i] = int(status[k])
            out[i] = b.read(o_out[k], L[k], np.int16 if self.pcm16 else np.float32)


class BatchOracleSeparator(_TfEngine):
    """oracle_separate.py:65-82 for a batch: the mixture and its K references go up in one slab,
    ONE fused forward launch runs K + 1 transforms per frame and stores the K masked spectra, ONE
    inverse-STFT launch takes them as (utterance, speaker) items (setk_oracle_separate_batch), one
    slab comes down.

    kind  iam | irm | ibm | psm (the tool's choices; anything else is a ValueError)
    run([(mixture, [reference 1 .. K]), ...]) -> per utterance the list of K waves
    (inverse_stft(mixture x mask_k), no norm); every utterance of a call has the same K <= 8."""

    def __init__(self, kind, keep_length=False, pcm16=False, frame_len=512, frame_hop=256, center=True,
                 round_power_of_two=True, window="hann", device=None, max_batch_samples=1 << 26):
        super().__init__(frame_len, frame_hop, center, round_power_of_two, window, device, max_batch_samples)
        if kind not in _ffi.ORACLE_MASKS:
            raise ValueError(f"oracle separation takes one of {_ffi.ORACLE_MASKS}, got {kind!r}")
        self.kind, self.keep_length, self.pcm16 = kind, bool(keep_length), bool(pcm16)

    def run(self, utts):
        out = [None] * len(utts)
        self.status = [_ffi.NUM_OK] * len(utts)
        if not len(utts):
            return out
        utts = [(first_channel(m), [first_channel(t) for t in ts]) for m, ts in utts]
        K = len(utts[0][1])
        if K < 1 or any(len(ts) != K for _, ts in utts):
            raise ValueError("BatchOracleSeparator.run needs the same number of references in every utterance")
        if K > _ffi.TFMASK_MAX_TARGETS:
            raise _ffi.SetkUnsupported(f"at most {_ffi.TFMASK_MAX_TARGETS} targets, got {K}")
        for i, (m, ts) in enumerate(utts):
            self._same_length(i, [m] + ts)
        self._plan()
        if self.n_fft != 512:
            self._run_operators(utts, out)
            return out
        mixes = [m for m, _ in utts]
        for batch in self._batches(list(range(len(utts))), mixes, self.max_batch_samples // (K + 1)):
            self._run_native(utts, K, batch, out)
        return out

    def _run_native(self, utts, K, idx, out):
        ctx = self.ctx
        ns = [_length(utts[i][0]) for i in idx]
        L = [ctx.istft_num_samples(self._frames(n), n if self.keep_length else None) for n in ns]
        signals = [utts[i][0] for i in idx] + [t for i in idx for t in utts[i][1]]
        esz = 2 if self.pcm16 else 4
        b, pcm, sig, _, o_out = self._stage(signals, [], [esz * max(n, 1) for n in L for _ in range(K)])
        n = len(idx)
        status = np.zeros(n, dtype=np.int32)
        ctx.oracle_separate_batch(self.kind, K, sig[:n], sig[n:], ns, [b.out.d + o for o in o_out],
                                  nsamps=ns if self.keep_length else None, status=status,
                                  flags=(_ffi.FLAG_IN_PCM16 if pcm else 0) | (_ffi.FLAG_OUT_PCM16 if self.pcm16 else 0),
                                  stream=b.stream)
        b.fetch(self._out_size)
        for k, i in enumerate(idx):
            self.status[i] = int(status[k])
            out[i] = [b.read(o_out[k * K + j], L[k], np.int16 if self.pcm16 else np.float32) for j in range(K)]

    def _run_operators(self, utts, out):
        """Other transform sizes: setk_stft of every signal, the masks of the batch kinds on the
        stored spectra (an oracle mask is the two-signal mask of its kind only for iam / psm; irm
        and ibm need all K magnitudes and are formed here on the host from the device's spectra),
        setk_tf_apply, setk_istft."""
        eps = np.float32(np.finfo(np.float32).eps)
        for i, (m, ts) in enumerate(utts):
            Sm = self._spec(m)
            St = [self._spec(t) for t in ts]
            masks = oracle_masks(self.kind, Sm, St, eps)
            waves = []
            for mask in masks:
                enh = np.empty_like(Sm)
                self.ctx.tf_apply(Sm, np.ascontiguousarray(mask, dtype=np.float32), Sm.shape[0], self.num_bins, enh)
                if not np.isfinite(enh.view(np.float32)).all():
                    self.status[i] = _ffi.NUM_NONFINITE
                waves.append(self._wave(enh, _length(m) if self.keep_length else None, None, self.pcm16))
            out[i] = waves


def _mag(z):
    return np.sqrt(z.real ** 2 + z.imag ** 2)


def oracle_masks(kind, mix, targets, eps=np.float32(np.finfo(np.float32).eps)):
    """The K masks of oracle separation on stored spectra (host arrays), float32 like the spectra."""
    if kind not in _ffi.ORACLE_MASKS:
        raise ValueError(f"oracle separation takes one of {_ffi.ORACLE_MASKS}, got {kind!r}")
    with np.errstate(all="ignore"):
        mags = [_mag(t) for t in targets]
        if kind == "ibm":
            winner = np.argmax(np.stack(mags), axis=0)
            return [winner == k for k in range(len(targets))]
        den = (sum(mags) if kind == "irm" else _mag(mix)) + eps
        if kind == "psm":
            phase = np.angle(mix)
            return [a * np.cos(phase - np.angle(t)) / den for a, t in zip(mags, targets)]
        return [a / den for a in mags]
