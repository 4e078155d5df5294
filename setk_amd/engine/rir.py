"""Image-method room impulse responses for a batch of (room, source, array) settings:
setk_rir_generate_batch."""
import numpy as np

from .. import _ffi
from ..libs.rir import make_spec
from ._common import _Engine, _Layout


class BatchRirGenerator(_Engine):
    """RirGenerator::GenerateRir (rir-generator.cc:108-192) for a ragged batch, resident on the
    device: the settings go up as the library's tables, two launches (the images; fold, high-pass
    and rounding) run for the whole batch (setk_rir_generate_batch), the RIRs come down in one slab.

    run(settings) takes a list of dicts with the arguments of libs.rir.generate_rir (room, src, mics,
    beta_or_rt60 and optionally sr, rir_nsamps, v, order, hp_filter, mic_type, angle) and returns per
    entry the float32 [n_mics][rir_nsamps] matrix, unscaled; self.status holds the SETK_NUM_* value
    per entry (SETK_NUM_NONFINITE: NaN / inf among the inputs or a source on a microphone)."""

    def __init__(self, device=None, max_batch_bytes=1 << 30, split=True):
        super().__init__(_ffi.default_context(device), 512, 256, True, True, "hann")
        self.max_batch_bytes = max_batch_bytes
        self.flags = 0 if split else _ffi.RIR_NO_SPLIT
        self.status = []

    def run(self, settings):
        specs = [make_spec(**s) for s in settings]
        results, self.status = [None] * len(specs), [0] * len(specs)
        batch, load = [], 0
        for i, sp in enumerate(specs):
            n = 4 * sp.n_mics * sp.num_samples
            if batch and load + n > self.max_batch_bytes:
                self._run(specs, batch, results)
                batch, load = [], 0
            batch.append(i)
            load += n
        if batch:
            self._run(specs, batch, results)
        return results

    def _run(self, specs, batch, results):
        b = self._get_slabs()
        l_out = _Layout()
        offs = [l_out.take(4 * specs[i].n_mics * specs[i].num_samples) for i in batch]
        o_status = l_out.take(4 * len(batch))
        b.reserve(256, 256, l_out.size)
        d_out = b.out.d
        self.ctx.rir_generate_batch([specs[i] for i in batch], [d_out + o for o in offs], status=d_out + o_status,
                                    flags=self.flags, stream=b.stream)
        b.fetch(l_out.size)
        status = b.read(o_status, len(batch), np.int32)
        for k, i in enumerate(batch):
            sp = specs[i]
            results[i] = b.read(offs[k], sp.n_mics * sp.num_samples, np.float32, (sp.n_mics, sp.num_samples))
            self.status[i] = int(status[k])
