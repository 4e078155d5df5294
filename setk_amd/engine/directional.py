"""Directional features from TF masks for a batch: setk_covar -> setk_pevd -> setk_directional_feats."""
import threading

import numpy as np

from .. import _ffi
from ._common import _Engine, _Layout, _Slabs, _Twin, align256, host_samples


class _DfLane(object):
    """One of the two in-flight halves of BatchDirectionalFeatures: its own library handle (a handle
    orders its calls on one stream at a time), slabs, mask twin and device scratch."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.slabs = _Slabs(ctx)
        self.masks = _Twin(ctx)
        self.scratch = _Twin(ctx, 0, host=False)
        self.pending = None

    def close(self):
        self.slabs.close()
        self.masks.close()
        self.scratch.close()


class BatchDirectionalFeatures(_Engine):
    """Directional features from TF masks for a batch of utterances, resident on the device.

    Replaces the per-utterance body of funcwj/setk scripts/sptk/compute_df_on_mask.py:40-54
    (SpectrogramReader -> compute_covar -> solve_pevd -> directional_feats, libs/spatial.py:
    184-208): the samples of a chunk go up in one slab, ONE setk_stft_batch launch writes every
    spectrogram, and per utterance setk_covar -> setk_pevd -> setk_directional_feats run on
    device pointers -- the spectrogram (31 MB at 8 ch x 30 s), the covariance and the steer
    vector never visit the host; one slab of T x F features and the per-bin status words comes
    down per chunk.  Two chunks are in flight (two library handles, two streams, each driven by
    its own host thread): the staging copies, the upload and the launches of one overlap the
    kernels and the download of the other -- the path is bound by the host's copies into and out
    of the page-locked slabs and the PCIe transfer of samples, masks and feature maps.  run() takes [(samps C x N
    float32 | Pcm16Frames, mask T x F or F x T)] and returns [(features T x F float32 | None,
    status)]: status != 0 is numpy's LinAlgError case (np.linalg.eigh on a non-finite
    covariance).  Other transform sizes and more than 8 channels go through the stand-alone
    operators of setk_amd.libs (numpy in, numpy out)."""

    def __init__(self, df_pair, frame_len=512, frame_hop=256, center=True, round_power_of_two=True,
                 window="hann", device=None, max_batch_samples=1 << 28, chunk_utts=8):
        pairs = [(int(i), int(j)) for i, j in df_pair]
        if not pairs:
            raise ValueError("no microphone pair given")
        self.pairs = pairs
        super().__init__(_ffi.default_context(device), frame_len, frame_hop, center,
                         round_power_of_two, window)
        self.max_batch_samples = max_batch_samples
        self.chunk_utts = max(1, int(chunk_utts))
        self._lanes = []

    def close(self):
        lanes, self._lanes = self._lanes, []
        for k, lane in enumerate(lanes):
            lane.close()
            if k > 0:
                lane.ctx.close()  # (lane 0 runs on the process-wide context)

    def condition_mask(self, mask, T, out=None):
        """compute_df_on_mask.py:44-47: F x T masks are turned, values above one clipped.  With
        `out` (T x F float32, e.g. a view of the page-locked upload buffer) the clipped mask is
        written there in one pass."""
        F = self.num_bins
        m = np.asarray(mask)
        if m.ndim != 2:
            raise ValueError(f"mask must be 2-D, got {m.shape}")
        if m.shape[0] == F and m.shape != (T, F):
            m = m.T
        if m.shape != (T, F):
            raise ValueError(f"mask {np.asarray(mask).shape} does not fit {T} frames x {F} bins")
        if out is not None:
            return np.minimum(m, 1, out=out, casting="unsafe")
        return np.minimum(m, 1).astype(np.float32, copy=False)

    def _lane(self, k):
        while len(self._lanes) <= k:
            ctx = self.ctx if not self._lanes else _ffi.Context(self.ctx.device)
            self._plan(ctx)
            self._lanes.append(_DfLane(ctx))
        return self._lanes[k]

    def run(self, utts):
        self._plan()
        out = [None] * len(utts)
        samps = [u[0] for u in utts]
        chunks = []  # (channel count, utterance indices)
        for C, idx in self._by_channels(samps).items():
            if any(max(p) >= C or min(p) < 0 for p in self.pairs):
                raise ValueError(f"microphone pair out of range for {C} channels: {self.pairs}")
            if self.n_fft != 512 or C > 8:
                for i in idx:
                    out[i] = self._one_by_operators(*utts[i])
                continue
            chunks += [(C, chunk) for chunk in
                       self._batches(idx, samps, self.max_batch_samples, self.chunk_utts)]
        if len(chunks) == 1:
            lane = self._lane(0)
            self._submit(lane, utts, chunks[0][1], chunks[0][0])
            self._collect(lane, out)
        elif chunks:
            # two lanes, each driven by its own thread (the staging copies and the library calls
            # release the interpreter lock): chunk k goes to lane k & 1, a lane stages, launches and
            # fetches one chunk at a time while the other lane does the same half a period apart
            lanes = [self._lane(0), self._lane(1)]
            errors = []

            def drive(k):
                try:
                    for C, chunk in chunks[k::2]:
                        self._submit(lanes[k], utts, chunk, C)
                        self._collect(lanes[k], out)
                except BaseException as e:  # noqa: B902 (re-raised in the caller's thread)
                    errors.append(e)

            other = threading.Thread(target=drive, args=(1,), name="setk-df-lane1")
            other.start()
            drive(0)
            other.join()
            if errors:
                raise errors[0]
        return out

    def _submit(self, lane, utts, batch, C):
        """Everything of one chunk, enqueued on the lane's stream; nothing waits here."""
        ctx, F = lane.ctx, self.num_bins
        b, mk = lane.slabs, lane.masks
        # out-slab per utterance: [features T x F float32 | status int32[F]]
        aptr, ns, off_out, n_out = b.stage_audio(
            [utts[i][0] for i in batch], C, lambda N: align256(4 * ctx.num_frames(N) * F) + 4 * F)
        frames = [ctx.num_frames(N) for N in ns]
        lay = _Layout()
        moff = [lay.take(4 * T * F) for T in frames]
        mk.reserve(lay.size, b.stream)
        for i, T, o in zip(batch, frames, moff):
            # (clipped straight into the page-locked buffer: one pass over the mask)
            self.condition_mask(utts[i][1], T, out=mk.view[o:o + 4 * T * F].view(np.float32).reshape(T, F))
        ctx.memcpy_h2d_async(mk.d, mk.h, lay.size, b.stream)
        # device scratch: spectrogram [C][T][F], covariance [F][C][C], steer vector [F][C] per utterance
        lay = _Layout()
        spec, cov, sv = zip(*[(lay.take(8 * C * T * F), lay.take(8 * F * C * C), lay.take(8 * F * C))
                              for T in frames])
        lane.scratch.reserve(lay.size, b.stream)
        base = lane.scratch.d
        ctx.stft_batch(C, aptr, ns, [base + o for o in spec], stream=b.stream)
        for k, T in enumerate(frames):
            o_df = b.out.d + off_out[k]
            o_st = o_df + align256(4 * T * F)
            ctx.covar(base + spec[k], mk.d + moff[k], C, T, F, base + cov[k], stream=b.stream)
            ctx.pevd(base + cov[k], None, F, C, 0, base + sv[k], o_st, stream=b.stream)
            ctx.directional_feats(base + spec[k], base + sv[k], self.pairs, C, T, F, o_df, stream=b.stream)
        ctx.memcpy_d2h_async(b.out.h, b.out.d, n_out, b.stream)
        lane.pending = (batch, frames, off_out)

    def _collect(self, lane, out):
        if lane.pending is None:
            return
        batch, frames, off_out = lane.pending
        lane.pending = None
        F = self.num_bins
        lane.ctx.stream_synchronize(lane.slabs.stream)
        for k, (i, T) in enumerate(zip(batch, frames)):
            status = lane.slabs.read(off_out[k] + align256(4 * T * F), F, np.int32)
            code = int(status.max()) if F else 0
            df = lane.slabs.read(off_out[k], T * F, np.float32, (T, F)) if code == 0 else None
            out[i] = (df, code)

    def _one_by_operators(self, samps, mask):
        """n_fft != 512 or more than 8 channels: the mirrored operators, one utterance at a time."""
        from ..libs.beamformer import compute_covar, solve_pevd
        from ..libs.spatial import directional_feats
        from ..libs.utils import forward_stft
        samps = host_samples(samps)
        s = self.stft
        obs = np.stack([forward_stft(ch, frame_len=s["frame_len"], frame_hop=s["frame_hop"],
                                     round_power_of_two=self.round_power_of_two, center=s["center"],
                                     window=self.window_name, transpose=False) for ch in samps])
        m = self.condition_mask(mask, obs.shape[2])
        try:
            sv = solve_pevd(compute_covar(obs, m))
        except np.linalg.LinAlgError:
            return None, _ffi.NUM_NONFINITE
        return directional_feats(obs, sv.T, df_pair=self.pairs), 0
