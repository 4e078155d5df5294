"""
Room impulse responses by the image method on the device: what the reference's ``rir-simulate``
(src/rir-simulate.cc over include/rir-generator.{h,cc}) computes for one command line, and the host
pre-processing in front of it.

    generate_rir(room, src, mics, beta_or_rt60, ...)   RirGenerator::GenerateRir (rir-generator.cc:108-192)
    beta_from_rt60(room, rt60, v)                      ComputeDerived's T60 branch (:78-92), in float32
    three_decimals(values)                             the "{:.3f}" of Room.rir (rir_generate_1d.py:151-168)

The generator's inputs are float32 (Kaldi's BaseFloat after parsing); so is the T60 branch, which is
kept in the reference's float32 steps here.  From the float32 inputs on the device computes in
float64 (setk_rir_generate of libsetk_hip.so; tests/PARITY_NOTES_RIR.md).
"""
import numpy as np

from .. import _ffi

MIC_TYPES = tuple(_ffi.RIR_MIC_TYPES)


def three_decimals(values):
    """Values as they reach the generator through Room.rir's command line: formatted "{:.3f}" and
    parsed again (rir_generate_1d.py:151-168).  float64 here; the generator narrows to float32."""
    return [float("{:.3f}".format(v)) for v in values]


def beta_from_rt60(room, rt60, v=340.0):
    """The six equal reflection coefficients sqrt(1 - alfa) of a reverberation time, Sabine's
    formula as rir-generator.cc:78-92 evaluates it: float32 V, S and alfa (the products in float32,
    24 V log(10) / (v S T60) in double, narrowed).  rt60 == 0: no reflections.  alfa > 1 raises the
    reference's error."""
    f32 = np.float32
    x, y, z = (f32(t) for t in room)
    rt60, v = f32(rt60), f32(v)
    if rt60 == 0:
        return np.zeros(6, dtype=np.float32)
    V = x * y * z
    S = f32(2) * (x * y + x * z + y * z)
    alfa = f32(np.float64(f32(24) * V) * np.log(10.0) / np.float64(v * S * rt60))
    if alfa > 1:
        raise RuntimeError(f"{alfa:g} > 1: The reflection coefficients cannot be calculated using the current"
                           " room parameters, i.e. room size and reverberation time.")
    return np.full(6, np.sqrt(f32(1) - alfa), dtype=np.float32)


def make_spec(room, src, mics, beta_or_rt60, sr=16000, rir_nsamps=4096, v=340.0, order=-1, hp_filter=True,
              mic_type="omnidirectional", angle=None):
    """The setk_rir_spec of one RIR: --beta with one value is a reverberation time (:78-92), with six
    the coefficients; any other count is refused as the reference refuses it (:77)."""
    beta = np.atleast_1d(np.asarray(beta_or_rt60, dtype=np.float32))
    if beta.size == 1:
        beta = beta_from_rt60(room, beta[0], v)
    elif beta.size != 6:
        raise ValueError(f"--beta takes a reverberation time or six coefficients, got {beta.size} values")
    if angle is not None and np.size(angle) == 1:
        angle = (float(np.ravel(angle)[0]), 0.0)  # (:69)
    return _ffi.rir_spec(room, src, mics, beta, rir_nsamps, samp_frequency=sr, sound_velocity=v, order=order,
                         hp_filter=hp_filter, mic_type=mic_type, angle=angle)


def generate_rir(room, src, mics, beta_or_rt60, sr=16000, rir_nsamps=4096, v=340.0, order=-1, hp_filter=True,
                 mic_type="omnidirectional", angle=None, with_status=False):
    """The generator's matrix for one source: float32 [n_mics][rir_nsamps], unscaled (rir-simulate
    writes it times 32767, rir-simulate.cc:64).  room, src: 3 values in metres; mics: n x 3."""
    spec = make_spec(room, src, mics, beta_or_rt60, sr, rir_nsamps, v, order, hp_filter, mic_type, angle)
    rir, status = _ffi.default_context().rir_generate(spec)
    return (rir, status) if with_status else rir
