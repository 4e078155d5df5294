"""Geometry-driven spatial features for a batch: setk_stft_batch -> setk_spatial_batch."""
import threading

import numpy as np

from .. import _ffi
from ._common import _Engine, _Layout, _Slabs, _Twin, host_samples


class _SpatialLane(object):
    """One of the two in-flight halves of BatchSpatialFeatures: its own library handle (a handle
    orders its calls on one stream at a time), slabs and device scratch."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.slabs = _Slabs(ctx)
        self.scratch = _Twin(ctx, 0, host=False)
        self.pending = None

    def close(self):
        self.slabs.close()
        self.scratch.close()


class BatchSpatialFeatures(_Engine):
    """SRP-PHAT angular spectra, IPD maps and geometry directional features for a batch of
    utterances, resident on the device.

    Replaces the per-utterance bodies of funcwj/setk scripts/sptk/compute_ipd_and_linear_srp.py:
    52-73, compute_circular_srp.py:38-55 and compute_df_on_geometry.py:47-69: the samples of a
    chunk go up in one slab, ONE setk_stft_batch launch writes every spectrogram, ONE
    setk_spatial_batch call computes every feature map, one slab of T x width float32 features
    comes down per chunk -- the spectrogram never visits the host.  The SRP table (float64 on the
    host, rounded once) and the steer vectors go up once per engine.  Two chunks are in flight (two
    library handles, two streams, each driven by its own host thread).  The device scratch of a
    chunk -- SRP keeps s_p [P][T][Dpad] and the observation tiles per utterance, about 150 MB for
    8 channels x 30 s x 28 pairs -- is bounded by chunk_utts and max_batch_samples.

    kind, and what it takes:
      "srp_linear"    topo (list / tuple of positions), num_doa, samp_tdoa, sample_rate
      "srp_circular"  diag_pair [(i, j), ...], n (microphones around), d (diameter), sample_rate, num_doa
      "ipd"           pairs [(l, r), ...], cos, sin
      "df"            steer_vector A x M x F, pairs; run() then takes doa_index, one list of
                      direction indices per utterance (all of one length)
    run() takes [samps C x N float32 | Pcm16Frames] and returns [features T x width float32].
    Other transform sizes and more than 8 channels go through forward_stft and the operators of
    setk_amd.libs.spatial, one utterance at a time."""

    def __init__(self, kind, pairs=None, topo=None, num_doa=None, samp_tdoa=False, sample_rate=16000,
                 diag_pair=None, n=6, d=0.07, cos=False, sin=False, steer_vector=None, frame_len=512,
                 frame_hop=256, center=True, round_power_of_two=True, window="hann", device=None,
                 max_batch_samples=1 << 26, chunk_utts=8):
        super().__init__(_ffi.default_context(device), frame_len, frame_hop, center, round_power_of_two, window)
        from ..libs import spatial as sp
        F = self.num_bins
        self.kind = kind
        self.table = self.weight = self.sv = None
        self.channels = None  # the channel count the geometry fixes (linear topology, steer vectors)
        if kind == "srp_linear":
            if type(topo) is not list and type(topo) is not tuple:
                raise ValueError("Now only support linear arrays(in python list/tuple type)")
            self.num_doa = 181 if num_doa is None else int(num_doa)
            self.channels = len(topo)
            self.pairs, self.table, self.weight = sp.linear_srp_tables(
                topo, num_bins=F, samp_doa=not samp_tdoa, sample_frequency=sample_rate, num_doa=self.num_doa)
            self.opts_kind = "srp"
        elif kind == "srp_circular":
            self.num_doa = 121 if num_doa is None else int(num_doa)
            self.pairs, self.table, self.weight = sp.circular_srp_tables(
                diag_pair, n, d, num_bins=F, sr=sample_rate, num_doas=self.num_doa)
            self.opts_kind = "srp"
        elif kind == "ipd":
            self.pairs = [(int(i), int(j)) for i, j in pairs]
            self.opts_kind = "ipd" if not cos else ("cos_sin_ipd" if sin else "cos_ipd")
        elif kind == "df":
            self.pairs = [(int(i), int(j)) for i, j in pairs]
            self.sv = np.ascontiguousarray(steer_vector, dtype=np.complex64)
            if self.sv.ndim != 3 or self.sv.shape[2] != F:
                raise ValueError(f"steer_vector {self.sv.shape} does not fit {F} bins (A x M x F)")
            self.channels = self.sv.shape[1]
            self.opts_kind = "df"
        else:
            raise ValueError(f"unknown kind of spatial feature: {kind}")
        if not self.pairs:
            raise ValueError("no microphone pair given")
        self.max_batch_samples = max_batch_samples
        self.chunk_utts = max(1, int(chunk_utts))
        self._lanes = []
        self._const = _Twin(self.ctx, 0)  # the SRP table / the steer vectors, uploaded once
        self._owned.append(self._const)

    def close(self):
        lanes, self._lanes = self._lanes, []
        for lane in lanes:
            lane.ctx.stream_synchronize(lane.slabs.stream)
        super().close()
        for k, lane in enumerate(lanes):
            lane.close()
            if k > 0:
                lane.ctx.close()  # (lane 0 runs on the process-wide context)

    def _lane(self, k):
        while len(self._lanes) <= k:
            ctx = self.ctx if not self._lanes else _ffi.Context(self.ctx.device)
            self._plan(ctx)
            self._lanes.append(_SpatialLane(ctx))
        return self._lanes[k]

    def _const_ptr(self):
        """The device copy of the table or the steer vectors (plain device memory: both lanes read it)."""
        const = self.table if self.table is not None else self.sv
        if const is None:
            return 0
        if not self._const.d:
            raw = const.view(np.uint8).reshape(-1)
            self._const.reserve(raw.size)
            self._const.view[:raw.size] = raw
            stream = self._lane(0).slabs.stream
            self.ctx.memcpy_h2d_async(self._const.d, self._const.h, raw.size, stream)
            self.ctx.stream_synchronize(stream)
        return self._const.d

    def _opts(self, const, doa_index=None):
        if self.opts_kind == "srp":
            return _ffi.spatial_opts("srp", self.pairs, table=const, num_doas=self.num_doa, pair_weight=self.weight)
        if self.opts_kind == "df":
            return _ffi.spatial_opts("df", self.pairs, steer_vector=const, num_sv=self.sv.shape[0],
                                     doa_index=doa_index)
        return _ffi.spatial_opts(self.opts_kind, self.pairs)

    def _check_channels(self, C):
        if self.kind == "srp_linear" and C != self.channels:
            raise ValueError("{:d} microphones available, while get {:d}-channel STFT".format(self.channels, C))
        if self.kind == "df" and C != self.channels:
            raise ValueError(f"steer_vector {self.sv.shape} does not match {C} channels")
        if C < 2:
            raise ValueError("Only one-channel STFT available")
        if any(max(p) >= C or min(p) < 0 for p in self.pairs):
            raise ValueError(f"microphone pair out of range for {C} channels: {self.pairs}")

    def run(self, utts, doa_index=None):
        if self.kind == "df":
            if doa_index is None or len(doa_index) != len(utts):
                raise ValueError("df needs one list of direction indices per utterance")
            doa_index = [[int(v) for v in row] for row in doa_index]
            if any(v < 0 or v >= self.sv.shape[0] for row in doa_index for v in row):
                raise ValueError(f"direction index outside the {self.sv.shape[0]} steer vectors")
        self._plan()
        out = [None] * len(utts)
        also = [len(row) for row in doa_index] if self.kind == "df" else None
        chunks = []  # (channel count, utterance indices)
        for key, idx in self._by_channels(utts, also).items():
            C = key if also is None else key[0]
            self._check_channels(C)
            if self.n_fft != 512 or C > 8:
                for i in idx:
                    out[i] = self._one_by_operators(utts[i], doa_index[i] if doa_index else None)
                continue
            chunks += [(C, chunk) for chunk in self._batches(idx, utts, self.max_batch_samples, self.chunk_utts)]
        if not chunks:
            return out
        const = self._const_ptr()
        if len(chunks) == 1:
            lane = self._lane(0)
            self._submit(lane, utts, chunks[0][1], chunks[0][0], const, doa_index)
            self._collect(lane, out)
            return out
        # two lanes, each driven by its own thread (the staging copies and the library calls release
        # the interpreter lock): chunk k goes to lane k & 1
        lanes = [self._lane(0), self._lane(1)]
        errors = []

        def drive(k):
            try:
                for C, chunk in chunks[k::2]:
                    self._submit(lanes[k], utts, chunk, C, const, doa_index)
                    self._collect(lanes[k], out)
            except BaseException as e:  # noqa: B902 (re-raised in the caller's thread)
                errors.append(e)

        other = threading.Thread(target=drive, args=(1,), name="setk-spatial-lane1")
        other.start()
        drive(0)
        other.join()
        if errors:
            raise errors[0]
        return out

    def _width(self, n_index):
        F = self.num_bins
        if self.opts_kind == "srp":
            return self.num_doa
        if self.opts_kind == "df":
            return n_index * F
        return (2 if self.opts_kind == "cos_sin_ipd" else 1) * len(self.pairs) * F

    def _submit(self, lane, utts, batch, C, const, doa_index):
        """Everything of one chunk, enqueued on the lane's stream; nothing waits here."""
        ctx, F = lane.ctx, self.num_bins
        b = lane.slabs
        rows = [doa_index[i] for i in batch] if doa_index else None
        width = self._width(len(rows[0]) if rows else 0)
        aptr, ns, off_out, n_out = b.stage_audio([utts[i] for i in batch], C,
                                                 lambda N: 4 * ctx.num_frames(N) * width)
        frames = [ctx.num_frames(N) for N in ns]
        lay = _Layout()
        spec = [lay.take(8 * C * T * F) for T in frames]
        lane.scratch.reserve(lay.size, b.stream)
        base = lane.scratch.d
        ctx.stft_batch(C, aptr, ns, [base + o for o in spec], stream=b.stream)
        ctx.spatial_batch(self._opts(const, rows), C, [base + o for o in spec], frames, F,
                          [b.out.d + o for o in off_out], stream=b.stream)
        ctx.memcpy_d2h_async(b.out.h, b.out.d, n_out, b.stream)
        lane.pending = (batch, frames, off_out, width)

    def _collect(self, lane, out):
        if lane.pending is None:
            return
        batch, frames, off_out, width = lane.pending
        lane.pending = None
        lane.ctx.stream_synchronize(lane.slabs.stream)
        for k, (i, T) in enumerate(zip(batch, frames)):
            out[i] = lane.slabs.read(off_out[k], T * width, np.float32, (T, width))

    def spectrogram(self, samps):
        """The C x T x F spectrogram of one utterance through forward_stft (the operators' path)."""
        from ..libs.utils import forward_stft
        s = self.stft
        return np.stack([forward_stft(ch, frame_len=s["frame_len"], frame_hop=s["frame_hop"],
                                      round_power_of_two=self.round_power_of_two, center=s["center"],
                                      window=self.window_name, transpose=True) for ch in host_samples(samps)])

    def by_operators(self, S, doa_index=None):
        """The features of one C x T x F spectrogram through the stand-alone operator."""
        from ..libs import spatial as sp
        if self.opts_kind == "srp":
            return sp.srp_feats(S, self.pairs, self.table, self.weight, self.num_doa)
        if self.opts_kind == "df":
            return sp.geometry_df(S, self.sv, doa_index, self.pairs)
        return sp.ipd_feats(S, self.pairs, cos=self.opts_kind != "ipd", sin=self.opts_kind == "cos_sin_ipd")

    def _one_by_operators(self, samps, doa_index):
        """n_fft != 512 or more than 8 channels: the mirrored operators, one utterance at a time."""
        return self.by_operators(self.spectrogram(samps), doa_index)
