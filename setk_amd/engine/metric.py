"""SI-SNR scoring with permutation alignment for a batch of utterances: setk_si_snr_batch."""
import numpy as np

from .. import _ffi
from ._common import Pcm16Frames, _Engine, _Layout


def signal_length(sig):
    """Samples of one signal as score() takes it: a vector, C x N (channel 0 is scored) or
    Pcm16Frames."""
    if isinstance(sig, Pcm16Frames):
        return sig.frames.shape[0]
    return np.shape(sig)[-1]


class BatchSiSnr(_Engine):
    """The loop bodies of compute_si_snr.py:80-105 for a batch, resident on the device: the samples
    of the batch go up in one slab, three tile-parallel phases (means, centred Gram sums,
    per-sample residuals; float64) and the search over the K! orders run as six launches for the
    whole batch (setk_si_snr_batch), the tables come down in one slab.

    score(utts) takes [(est_list, ref_list)] with K estimates and K references of one length per
    utterance, 1 <= K <= 8, and returns per utterance (best, order, table, status): the best average
    SI-SNR, the assignment (estimate n belongs to reference order[n]), the K x K float64 table
    table[i, j] = si_snr(est[i], ref[j]) and the SETK_NUM_* value (SETK_NUM_NONFINITE: NaN / inf
    among the samples; the figures of such an utterance are not to be used).
    A signal is a float32 vector, a C x N array (channel 0 is scored, compute_si_snr.py:36) or
    Pcm16Frames, whose 16-bit frames go up as stored and are read through their stride: a batch of
    them alone is scored as stored, in a mixed batch they are widened on the host first (the same
    values, the same bits out)."""

    def __init__(self, eps=1e-8, remove_dc=True, device=None, max_batch_bytes=3 << 30):
        super().__init__(_ffi.default_context(device), 512, 256, True, True, "hann")
        self.eps = float(eps)
        self.remove_dc = bool(remove_dc)
        self.max_batch_bytes = max_batch_bytes

    @staticmethod
    def _check(est, ref):
        if len(est) != len(ref):
            raise RuntimeError("size do not match between xlist " + f"and slist: {len(est)} vs {len(ref)}")
        if not len(est):
            raise ValueError("an utterance needs at least one estimate and one reference")
        sizes = {signal_length(s) for s in list(est) + list(ref)}
        if len(sizes) != 1:
            raise ValueError(f"the signals of an utterance differ in length: {sorted(sizes)}")
        if 0 in sizes:
            raise ValueError("an utterance needs at least one sample")

    @staticmethod
    def _device_bytes(est, ref):
        """What an utterance takes on the device: its samples as they go up, the partial slab (a
        row of at most 72 float64 per 8192 samples), the tables."""
        n = sum(s.frames.nbytes if isinstance(s, Pcm16Frames) else 4 * signal_length(s) for s in list(est) + list(ref))
        K = len(est)
        return n + (signal_length(est[0]) // 8192 + 1) * 72 * 8 + 8 * K * K + 4 * K + 2048

    def score(self, utts):
        results = [None] * len(utts)
        for est, ref in utts:
            self._check(est, ref)
        batch, load = [], 0
        for i, (est, ref) in enumerate(utts):
            n = self._device_bytes(est, ref)
            if batch and load + n > self.max_batch_bytes:
                self._run(utts, batch, results)
                batch, load = [], 0
            batch.append(i)
            load += n
        if batch:
            self._run(utts, batch, results)
        return results

    def _run(self, utts, batch, results):
        ctx = self.ctx
        b = self._get_slabs()
        sigs = [s for i in batch for part in utts[i] for s in part]
        pcm = all(isinstance(s, Pcm16Frames) for s in sigs)
        l_in, l_out = _Layout(), _Layout()
        plan = []  # per utterance: (K, L, [(array, offset, stride)] of the estimates, of the references)

        def place(s):
            if isinstance(s, Pcm16Frames):
                a = s.frames if pcm else s.to_float()[0]
            else:
                a = np.asarray(s)
                a = np.ascontiguousarray(a if a.ndim == 1 else a[0], dtype=np.float32)
            return a, l_in.take(a.nbytes), (a.shape[1] if a.ndim == 2 else 1)

        for i in batch:
            est, ref = utts[i]
            plan.append((len(est), signal_length(est[0]), [place(s) for s in est], [place(s) for s in ref]))
        n, n_sig, n_cell = len(batch), sum(p[0] for p in plan), sum(p[0] ** 2 for p in plan)
        o_pair, o_best, o_perm, o_status = (l_out.take(8 * n_cell), l_out.take(8 * n), l_out.take(4 * n_sig),
                                            l_out.take(4 * n))
        b.reserve(max(l_in.size, 256), 256, l_out.size)
        view, d_in, d_out = b.inp.view, b.inp.d, b.out.d
        eptr, estr, rptr, rstr = [], [], [], []
        for _, _, est, ref in plan:
            for ptrs, strides, part in ((eptr, estr, est), (rptr, rstr, ref)):
                for a, off, stride in part:
                    view[off:off + a.nbytes] = np.frombuffer(a, dtype=np.uint8)
                    ptrs.append(d_in + off)
                    strides.append(stride)
        ctx.memcpy_h2d_async(d_in, b.inp.h, l_in.size, b.stream)
        flags = (_ffi.FLAG_IN_PCM16 if pcm else 0) | (0 if self.remove_dc else _ffi.FLAG_KEEP_DC)
        ctx.si_snr_batch([p[0] for p in plan], eptr, estr, rptr, rstr, [p[1] for p in plan], d_out + o_pair,
                         best=d_out + o_best, perm=d_out + o_perm, status=d_out + o_status, eps=self.eps,
                         flags=flags, stream=b.stream)
        b.fetch(l_out.size)
        pair, best = b.read(o_pair, n_cell, np.float64), b.read(o_best, n, np.float64)
        perm, status = b.read(o_perm, n_sig, np.int32), b.read(o_status, n, np.int32)
        cell = sig = 0
        for k, i in enumerate(batch):
            K = plan[k][0]
            results[i] = (float(best[k]), tuple(int(v) for v in perm[sig:sig + K]),
                          pair[cell:cell + K * K].reshape(K, K).copy(), int(status[k]))
            cell += K * K
            sig += K
