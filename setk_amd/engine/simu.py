"""Data simulation for a batch of mixture recipes: setk_simu_batch."""
import numpy as np

from .. import _ffi
from ._common import _Engine, _Layout


class Source(object):
    """One speaker or point noise of a recipe: what read_wav returned (N float32, or C x N for the
    close-talk forms), its RIR (R or N x R float32) or None, where it begins in the mixture, its SDR
    against the first speaker / its SNR, and for a noise whether it repeats."""

    def __init__(self, audio, rir=None, begin=0, snr=0.0, repeat=False):
        self.audio = np.ascontiguousarray(audio, dtype=np.float32)
        self.rir = None if rir is None else np.ascontiguousarray(rir, dtype=np.float32)
        if self.rir is not None and self.rir.ndim == 1:
            self.rir = self.rir[None]
        self.begin, self.snr, self.repeat = int(begin), float(snr), bool(repeat)

    @property
    def channels(self):
        return 1 if self.audio.ndim == 1 else self.audio.shape[0]

    def image_channels(self, dump_channel):
        """Channels of the image (:69-81): the RIR's, one when a channel is dumped, the source's
        without a RIR."""
        if self.rir is None:
            return self.channels
        return 1 if dump_channel >= 0 else self.rir.shape[0]


class Recipe(object):
    """One mixture: the arguments of the reference's run_simu after its files are read
    (libs.simu.load_recipe builds it from an argument list)."""

    def __init__(self, speakers, noises=(), iso=None, iso_snr=0.0, dump_channel=-1, norm_factor=0.9):
        self.speakers, self.noises = list(speakers), list(noises)
        self.iso = None if iso is None else np.ascontiguousarray(iso, dtype=np.float32)
        self.iso_snr, self.dump_channel, self.norm_factor = float(iso_snr), int(dump_channel), float(norm_factor)
        if not self.speakers:
            raise ValueError("a recipe needs at least one speaker")

    @property
    def num_samples(self):
        """max(b + s.size) (:195: `size` counts every channel)."""
        return max(s.begin + s.audio.size for s in self.speakers)

    @property
    def num_channels(self):
        return self.speakers[0].image_channels(self.dump_channel)

    def check(self):
        """What the reference raises as RuntimeError while it mixes (:38-39, :266-269, :277-291)."""
        for s in self.speakers + self.noises:
            if s.rir is not None and s.audio.ndim != 1:
                raise RuntimeError(f"Can not convolve rir with {s.audio.ndim}D signals")
        N = self.num_channels
        if self.noises:
            Nn = self.noises[0].image_channels(self.dump_channel)
            if N != Nn:
                raise RuntimeError("Channel mismatch between source speaker configuration and pointsource "
                                   f"noise's, {N} vs {Nn}")
        if self.iso is not None:
            if N == 1:
                if self.iso.ndim != 1 and self.dump_channel < 0:
                    raise RuntimeError("Single channel mixture vs multi-channel isotropic noise")
            elif self.iso.shape[0] != N:
                raise RuntimeError("Channel number mismatch between mixture and isotropic noise, "
                                   f"{N} vs {self.iso.shape[0]}")


class Result(object):
    """mix N x L (float32) or L x N / L frames (int16); spk: channel 0 of every scaled speaker image;
    noise: channel 0 of the scaled noise or None; status: SETK_NUM_*."""

    def __init__(self, mix, spk, noise, iso_only, status):
        self.mix, self.spk, self.noise, self.iso_only, self.status = mix, spk, noise, iso_only, status


class BatchSimulator(_Engine):
    """wav_simulate.py's run_simu for a batch of recipes, resident on the device: every distinct
    array of the batch (a RIR or a noise that several recipes share goes up once) is laid into one
    page-locked slab and copied up in one piece, ONE setk_simu_batch call runs the transforms, the
    partitioned convolutions, the powers, coefficients, peaks and the scaling for all mixtures --
    ragged in length, source count, tap count and channel count -- and one slab comes down.

    pcm16  the results as 16-bit samples, rounded on the device by the writer's rule (mix then
           comes as the frames of a wave file, L x N, or L for one channel)
    run() takes a list of Recipe and returns a list of Result; `status` holds the SETK_NUM_* value
    of every mixture of the last run() (SETK_NUM_NONFINITE: NaN / inf reached the mixture)."""

    def __init__(self, device=None, pcm16=False, max_batch_samples=1 << 27):
        super().__init__(_ffi.default_context(device), 512, 256, True, True, "hann")
        self.pcm16 = bool(pcm16)
        self.max_batch_samples = max_batch_samples
        self.status = []

    def run(self, recipes):
        out = [None] * len(recipes)
        self.status = [_ffi.NUM_OK] * len(recipes)
        for r in recipes:
            r.check()
        batch, load = [], 0
        for i, r in enumerate(recipes):
            n = r.num_samples * r.num_channels * (2 + len(r.speakers) + len(r.noises))
            if batch and load + n > self.max_batch_samples:
                self._run_batch(recipes, batch, out)
                batch, load = [], 0
            batch.append(i)
            load += n
        if batch:
            self._run_batch(recipes, batch, out)
        return out

    def _run_batch(self, recipes, idx, out):
        ctx, b = self.ctx, self._get_slabs()
        esz = 2 if self.pcm16 else 4
        l_in, l_out = _Layout(), _Layout()
        placed = {}  # id(array) -> offset: shared RIRs and noises go up once

        def place(a):
            if id(a) not in placed:
                placed[id(a)] = (l_in.take(a.nbytes), a)
            return placed[id(a)][0]

        plan = []
        for i in idx:
            r = recipes[i]
            N, L = r.num_channels, r.num_samples
            srcs = [[(place(s.audio), None if s.rir is None else place(s.rir), s) for s in group]
                    for group in (r.speakers, r.noises)]
            o_iso = None if r.iso is None else place(r.iso)
            has_noise = bool(r.noises) or r.iso is not None
            plan.append((r, N, L, srcs, o_iso, l_out.take(esz * N * L), [l_out.take(esz * L) for _ in r.speakers],
                         l_out.take(esz * L) if has_noise else None))
        b.reserve(max(l_in.size, 256), 256, max(l_out.size, 256))
        for off, a in placed.values():
            b.inp.view[off:off + a.nbytes] = np.frombuffer(a, dtype=np.uint8)
        ctx.memcpy_h2d_async(b.inp.d, b.inp.h, l_in.size, b.stream)
        d_in, d_out = b.inp.d, b.out.d
        structs = []
        for r, N, L, srcs, o_iso, o_mix, o_spk, o_noise in plan:

            def source(o_a, o_r, s):
                return _ffi.simu_source(d_in + o_a, s.audio.shape[-1], s.channels,
                                        rir=None if o_r is None else d_in + o_r,
                                        rir_channels=0 if s.rir is None else s.rir.shape[0],
                                        rir_taps=0 if s.rir is None else s.rir.shape[1], begin=s.begin, snr=s.snr,
                                        repeat=s.repeat)

            rec = _ffi.simu_recipe([source(*t) for t in srcs[0]], [source(*t) for t in srcs[1]],
                                   iso=None if o_iso is None else d_in + o_iso,
                                   iso_samples=0 if r.iso is None else r.iso.shape[-1],
                                   iso_channels=0 if r.iso is None else (1 if r.iso.ndim == 1 else r.iso.shape[0]),
                                   iso_snr=r.iso_snr, dump_channel=r.dump_channel, norm_factor=r.norm_factor)
            _ffi.simu_recipe_outputs(rec, d_out + o_mix, [d_out + o for o in o_spk],
                                     None if o_noise is None else d_out + o_noise)
            if _ffi.simu_shape(rec) != (N, L):
                raise _ffi.SetkError("recipe shape disagrees with the library's")
            structs.append(rec)
        status = np.zeros(len(idx), dtype=np.int32)
        ctx.simu_batch(structs, status=status, flags=_ffi.FLAG_OUT_PCM16 if self.pcm16 else 0, stream=b.stream)
        b.fetch(l_out.size)
        dt = np.int16 if self.pcm16 else np.float32
        for k, (i, (r, N, L, _, _, o_mix, o_spk, o_noise)) in enumerate(zip(idx, plan)):
            self.status[i] = int(status[k])
            if self.pcm16:
                mix = b.read(o_mix, N * L, dt, (L, N) if N > 1 else (L,))
            else:
                mix = b.read(o_mix, N * L, dt, (N, L))
            out[i] = Result(mix, [b.read(o, L, dt) for o in o_spk], None if o_noise is None else b.read(o_noise, L, dt),
                            not r.noises and r.iso is not None, int(status[k]))
