"""Mask-based sound source localisation for a batch: setk_ssl_batch."""
import numpy as np

from .. import _ffi
from ._common import _Engine, _Layout, _Twin, host_samples


class BatchLocalizer(_Engine):
    """The loop body of do_ssl.py:80-114 for a batch, resident on the device: one upload of the
    samples (and masks) per channel count, the STFT, the frame scores of every (direction,
    frame) once, one reduction per window, one download of indices and score spectra
    (setk_ssl_batch).  Offline every utterance is the one window [0, T); online (chunk_len > 0
    and look_back > 0) the windows are [max(t - look_back, 0), t + chunk_len), t = 0, chunk_len,
    ..., cut out of the same frame scores.  run() takes a list of C x N float32 arrays or
    Pcm16Frames (any mix of channel counts up to 16) and optional T x F masks and returns, per
    utterance, the int64 index array (one index per window); `scores` then holds the W x A
    float64 score spectra and `status` the SETK_NUM_* value of every utterance of the last run
    (MUSIC: the eigen-solves).  steer_vector is one A x M x F array, or a dict of them by
    channel count M for tables that mix arrays."""

    def __init__(self, backend="ml", steer_vector=None, srp_pair=None, frame_len=512, frame_hop=256,
                 center=True, round_power_of_two=True, window="hann", chunk_len=-1, look_back=125,
                 device=None):
        if backend not in _ffi.SSL_BACKENDS:
            raise ValueError(f"unknown SSL backend {backend}")
        if backend == "srp" and not srp_pair:
            raise ValueError("srp_pair cannot be None, (list, list)")
        sets = steer_vector if isinstance(steer_vector, dict) else {None: steer_vector}
        self.sv = {}
        for sv in sets.values():
            sv = np.ascontiguousarray(sv, dtype=np.complex64)
            if sv.ndim != 3:
                raise ValueError("steer_vector: A x M x F")
            self.sv[sv.shape[1]] = sv
        ctx = _ffi.default_context(device)
        self.backend = backend
        # ml_ssl as get_doa calls it (do_ssl.py:34): compression = -1, eps = float32 eps
        self.opts = _ffi.ssl_opts(backend, srp_pair=srp_pair, compression=-1,
                                  eps=float(np.finfo(np.float32).eps))
        self.chunk_len, self.look_back = int(chunk_len), int(look_back)
        self.online = self.chunk_len > 0 and self.look_back > 0
        super().__init__(ctx, frame_len, frame_hop, center, round_power_of_two, window)
        for sv in self.sv.values():
            if sv.shape[2] != self.num_bins:
                raise ValueError(f"steer_vector has {sv.shape[2]} bins, the transform {self.num_bins}")
        self._masks = _Twin(ctx)
        self._owned.append(self._masks)
        self._sv = {}  # channel count -> the steer vectors' twin
        self.scores, self.status = [], []

    def close(self):
        """Give the slabs of run() back."""
        twins, self._sv = list(self._sv.values()), {}
        for t in twins:
            t.close()
        super().close()

    def windows(self, num_frames):
        if not self.online:
            return [(0, num_frames)]
        return [(max(t - self.look_back, 0), min(t + self.chunk_len, num_frames))
                for t in range(0, num_frames, self.chunk_len)]

    def run(self, utts, masks=None):
        out = [None] * len(utts)
        self.scores = [None] * len(utts)
        self.status = [_ffi.NUM_OK] * len(utts)
        if not len(utts):
            return out
        if masks is not None and len(masks) != len(utts):
            raise ValueError("one mask (or None) per utterance")
        self._plan()
        groups = self._by_channels(utts)
        if max(groups) > 16:
            raise _ffi.SetkUnsupported(
                f"SSL on the device needs 1 <= channels <= 16 (got {max(groups)} channels)")
        for C, idx in groups.items():
            if C not in self.sv:
                raise ValueError(f"no steer vectors for {C} channels (have {sorted(self.sv)})")
            if self.n_fft == 512:
                self._run_native(utts, masks, C, idx, out)
            else:
                self._run_operators(utts, masks, C, idx, out)
        return out

    def _mask_of(self, masks, i, T):
        if masks is None or masks[i] is None:
            return None
        m = np.ascontiguousarray(masks[i], dtype=np.float32)
        if m.shape != (T, self.num_bins):
            raise ValueError(f"mask {m.shape} does not match the spectrogram ({T}, {self.num_bins})")
        return m

    def _run_native(self, utts, masks, C, idx, out):
        ctx, sv = self.ctx, self.sv[C]
        A = sv.shape[0]
        b = self._get_slabs()
        if C not in self._sv:  # the steer vectors go up once
            d_sv = self._sv[C] = _Twin(ctx)
            d_sv.reserve(sv.nbytes, b.stream)
            d_sv.view[:sv.nbytes] = np.frombuffer(sv, dtype=np.uint8)
            ctx.memcpy_h2d_async(d_sv.d, d_sv.h, sv.nbytes, b.stream)
        nwin = lambda N: len(self.windows(ctx.num_frames(N)))  # noqa: E731
        aptr, ns, _, n_out = b.stage_audio([utts[i] for i in idx], C, lambda N: nwin(N) * (8 * A + 8))
        frames = [ctx.num_frames(N) for N in ns]
        wins = [self.windows(T) for T in frames]
        mptr = None
        ms = [self._mask_of(masks, i, T) for i, T in zip(idx, frames)]
        if any(m is not None for m in ms):
            mk, lay, mptr = self._masks, _Layout(), []
            mk.reserve(sum(m.nbytes + 256 for m in ms if m is not None), b.stream)
            for m in ms:
                if m is None:
                    mptr.append(None)
                    continue
                o = lay.take(m.nbytes)
                mk.view[o:o + m.nbytes] = np.frombuffer(m, dtype=np.uint8)
                mptr.append(mk.d + o)
            ctx.memcpy_h2d_async(mk.d, mk.h, lay.size, b.stream)
        total = sum(len(w) for w in wins)
        status = np.zeros(len(idx), dtype=np.int32)
        # the output slab: [total][A] float64 scores, then [total] int32 indices
        ctx.ssl_batch(self.opts, C, aptr, ns, mptr, self._sv[C].d, A, wins, b.out.d + 8 * A * total,
                      score=b.out.d, status=status, stream=b.stream)
        b.fetch(n_out)
        score = b.read(0, total * A, np.float64, (total, A))
        index = b.read(8 * A * total, total, np.int32)
        w0 = 0
        for k, i in enumerate(idx):
            W = len(wins[k])
            out[i] = index[w0:w0 + W].astype(np.int64)
            self.scores[i] = score[w0:w0 + W]
            self.status[i] = int(status[k])
            w0 += W

    def _run_operators(self, utts, masks, C, idx, out):
        """Transform sizes the batched call is not built for: the stand-alone operators
        (setk_stft -> setk_ssl_scores), one utterance at a time."""
        ctx, sv, F = self.ctx, self.sv[C], self.num_bins
        A = sv.shape[0]
        for i in idx:
            samps = host_samples(utts[i])
            T = ctx.num_frames(samps.shape[1])
            spec = np.empty((C, T, F), dtype=np.complex64)
            ctx.stft(samps, spec)
            wins = self.windows(T)
            score = np.empty((len(wins), A), dtype=np.float64)
            index = np.empty(len(wins), dtype=np.int32)
            status = np.zeros(1, dtype=np.int32)
            ctx.ssl_scores(self.opts, spec, self._mask_of(masks, i, T), sv, A, C, T, F, wins, score, index,
                           status=status)
            out[i], self.scores[i], self.status[i] = index.astype(np.int64), score, int(status[0])
