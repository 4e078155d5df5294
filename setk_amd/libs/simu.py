"""
Data simulation: the functions of the reference's scripts/sptk/wav_simulate.py (:17-312) with
their signatures, on the C ABI.  The convolutions run on the device (setk_fir_reverb: a
partitioned overlap-save convolution, float32), run_simu as one setk_simu_batch call through
engine.BatchSimulator.  Results are float32 where the reference returns float64 built from float32
images; what is kept of the reference's quirks, and what is refused where it raises, is listed in
tests/PARITY_NOTES_SIMU.md.
"""
import numpy as np

from .. import _ffi
from .utils import EPSILON, read_wav


def coeff_snr(sig_pow, ref_pow, snr):
    """alpha of mix = Sa + alpha * Sb for SNR = 10 log10(Pa / (Pb alpha^2)) (:17-26)."""
    return (ref_pow / (sig_pow * 10**(snr / 10) + EPSILON))**0.5


def _reverb(spk, rir, want_power=True):
    spk = np.ascontiguousarray(spk, dtype=np.float32)
    rir = np.ascontiguousarray(rir, dtype=np.float32)
    N, R = rir.shape
    S = spk.shape[-1]
    revb = np.empty((N, S), dtype=np.float32)
    power = np.zeros(1, dtype=np.float64) if want_power else None
    _ffi.default_context().fir_reverb(spk, S, rir, N, R, revb, power)
    return revb, (np.float32(power[0]) if want_power else None)


def add_room_response(spk, rir, early_energy=False, sr=16000):
    """Convolve a source S with RIRs N x R: (revb N x S float32, power of channel 0) (:29-54).
    early_energy: the power of the source convolved with the first channel's direct path and
    early reflections (1 ms before to 50 ms behind the peak) instead."""
    spk = np.asarray(spk)
    if spk.ndim != 1:
        raise RuntimeError(f"Can not convolve rir with {spk.ndim}D signals")
    rir = np.asarray(rir)
    revb, power = _reverb(spk, rir)
    if early_energy:
        rir_ch0 = rir[0]
        rir_peak = np.argmax(rir_ch0)
        rir_beg_idx = max(0, int(rir_peak - 0.001 * sr))
        rir_end_idx = min(rir_ch0.size, int(rir_peak + 0.05 * sr))
        early_rir = np.zeros_like(rir_ch0)
        early_rir[rir_beg_idx:rir_end_idx] = rir_ch0[rir_beg_idx:rir_end_idx]
        _, power = _reverb(spk, early_rir[None])
    return revb, power


def _pick(rir, channel):
    if rir.ndim == 1:
        rir = rir[None, ...]
    if channel >= 0 and rir.ndim == 2:
        rir = rir[channel:channel + 1]
    return rir


def add_speaker(mix_nsamps, src_spk, src_begin, sdr, src_rir=None, channel=-1, sr=16000):
    """Mix source speakers (:57-93): one N x mix_nsamps float64 array per speaker."""
    spk_image, spk_power = [], []
    for i, spk in enumerate(src_spk):
        if src_rir is None:
            src = spk[None, ...] if spk.ndim == 1 else spk
            spk_image.append(src)
            spk_power.append(np.mean(src[0]**2))
        else:
            revb, p = add_room_response(spk, _pick(src_rir[i], channel), sr=sr)
            spk_image.append(revb)
            spk_power.append(p)
    N, _ = spk_image[0].shape
    mix = [np.zeros([N, mix_nsamps]) for _ in src_spk]
    ref_power = spk_power[0]
    for i, image in enumerate(spk_image):
        dur = image.shape[-1]
        beg = src_begin[i]
        coeff = 1 if i == 0 else coeff_snr(spk_power[i], ref_power, sdr[i])
        mix[i][..., beg:beg + dur] += coeff * image
    return mix


def add_point_noise(mix_nsamps, ref_power, noise, noise_begin, snr, noise_rir=None, channel=-1, repeat=False,
                    sr=16000):
    """Add pointsource noises (:96-143): N x mix_nsamps float64.  As in the reference every noise
    is mixed over the duration the LAST one left behind."""
    image = []
    image_power = []
    for i, noise in enumerate(noise):
        beg = noise_begin[i]
        if not repeat:
            dur = min(noise.shape[-1], mix_nsamps - beg)
        else:
            dur = mix_nsamps - beg
            if noise.shape[-1] < dur:
                noise = np.pad(noise, (0, dur - noise.shape[-1]), mode="wrap")
        if noise_rir is None:
            src = noise[None, ...] if noise.ndim == 1 else noise
            image.append(src)
            image_power.append(np.mean(src[0, :dur]**2))
        else:
            revb, revb_power = add_room_response(noise[:dur], _pick(noise_rir[i], channel), sr=sr)
            image.append(revb)
            image_power.append(revb_power)
    N, _ = image[0].shape
    mix = np.zeros([N, mix_nsamps])
    for i, img in enumerate(image):
        beg = noise_begin[i]
        coeff = coeff_snr(image_power[i], ref_power, snr[i])
        mix[..., beg:beg + dur] += coeff * img[..., :dur]
    return mix


def load_audio(src_args, beg=None, end=None, sr=16000):
    """Load audio from args.xxx (:146-163); a sample-rate mismatch raises (read_wav)."""
    if src_args:
        src_path = src_args.split(",")
        beg_int = [None for _ in src_path]
        end_int = [None for _ in src_path]
        if beg:
            beg_int = [int(v) for v in beg.split(",")]
        if end:
            end_int = [int(v) for v in end.split(",")]
        return [read_wav(s, sr=sr, beg=b, end=e) for s, b, e in zip(src_path, beg_int, end_int)]
    else:
        return None


def load_recipe(args):
    """The first half of run_simu (:166-242): the files of one argument list read, its errors
    raised, as an engine.Recipe."""
    from ..engine.simu import Recipe, Source

    def arg_float(src_args):
        return [float(s) for s in src_args.split(",")] if src_args else None

    src_spk = load_audio(args.src_spk, sr=args.sr)
    src_rir = load_audio(args.src_rir, sr=args.sr)
    if src_rir:
        if len(src_rir) != len(src_spk):
            raise RuntimeError(f"Number of --src-rir={args.src_rir} do not match with " +
                               f"--src-spk={args.src_spk} option")
    sdr = arg_float(args.src_sdr)
    if len(src_spk) > 1 and not sdr:
        raise RuntimeError("--src-sdr need to be assigned for " + f"--src-spk={args.src_spk}")
    if sdr:
        if len(src_spk) - 1 != len(sdr):
            raise RuntimeError("Number of --src-snr - 1 do not match with " + "--src-snr option")
        sdr = [0] + sdr
    else:
        sdr = [0]
    src_begin = arg_float(args.src_begin)
    if src_begin:
        src_begin = [int(v) for v in src_begin]
    else:
        src_begin = [0 for _ in src_spk]
    mix_nsamps = max([b + s.size for b, s in zip(src_begin, src_spk)])

    point_noise_rir = load_audio(args.point_noise_rir, sr=args.sr)
    # (split on whitespace here, on commas inside load_audio: :199-201 against :154-157)
    point_noise_end = [str(int(v) + mix_nsamps) for v in args.point_noise_offset.split()]
    point_noise = load_audio(args.point_noise, beg=args.point_noise_offset, end=",".join(point_noise_end),
                             sr=args.sr)
    noises = []
    if args.point_noise:
        if point_noise_rir:
            if len(point_noise) != len(point_noise_rir):
                raise RuntimeError(f"Number of --point-noise-rir={args.point_noise_rir} do not match with " +
                                   f"--point-noise={args.point_noise} option")
        point_snr = arg_float(args.point_noise_snr)
        if not point_snr:
            raise RuntimeError("--point-noise-snr need to be assigned for " + f"--point-noise={args.point_noise}")
        if len(point_noise) != len(point_snr):
            raise RuntimeError(f"Number of --point-noise-snr={args.point_noise_snr} do not match with " +
                               f"--point-noise={args.point_noise} option")
        point_begin = arg_float(args.point_noise_begin)
        if point_begin:
            point_begin = [int(v) for v in point_begin]
        else:
            point_begin = [0 for _ in point_noise]
        noises = [Source(n, rir=point_noise_rir[i] if point_noise_rir else None, begin=point_begin[i],
                         snr=point_snr[i], repeat=bool(args.point_noise_repeat))
                  for i, n in enumerate(point_noise)]

    isotropic_noise = load_audio(args.isotropic_noise, beg=str(args.isotropic_noise_offset),
                                 end=str(args.isotropic_noise_offset + mix_nsamps), sr=args.sr)
    isotropic_snr = 0.0
    if isotropic_noise:
        isotropic_noise = isotropic_noise[0]
        isotropic_snr = arg_float(args.isotropic_noise_snr)
        if not isotropic_snr:
            raise RuntimeError("--isotropic-snr need to be assigned for " +
                               f"--isotropic-noise={args.isotropic_noise} option")
        isotropic_snr = isotropic_snr[0]
    else:
        isotropic_noise = None
    speakers = [Source(s, rir=src_rir[i] if src_rir else None, begin=src_begin[i], snr=sdr[i])
                for i, s in enumerate(src_spk)]
    return Recipe(speakers, noises, iso=isotropic_noise, iso_snr=isotropic_snr, dump_channel=args.dump_channel,
                  norm_factor=args.norm_factor)


def finish(result):
    """An engine result as run_simu returns it (:304-312): mix.squeeze(), the channel-0 speaker
    references, the channel-0 noise reference or None.  A recipe whose only noise is isotropic gets
    what the reference's `noise[0] * factor` is there: the FIRST SAMPLE of the scaled chunk (its
    noise is one-dimensional at that point, :299-300)."""
    mix, spk, noise = result.mix, result.spk, result.noise
    if noise is not None and result.iso_only:
        noise = noise[0]
    return mix.squeeze(), spk, noise


def run_simu(args, engine=None):
    """(mix, [speaker references], noise reference or None) of one argument list (:166-312),
    float32."""
    from ..engine.simu import BatchSimulator
    recipe = load_recipe(args)
    own = engine is None
    engine = BatchSimulator() if own else engine
    try:
        return finish(engine.run([recipe])[0])
    finally:
        if own:
            engine.close()
