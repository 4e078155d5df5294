"""
Image-method RIR generation on the MI355X (setk_amd/csrc/rir.hip, libs/rir.py, engine/rir.py)
against the reference's recorded RIRs in tests/golden/ref_rir.npz (tools/make_rir_golden.py: the
reference's unmodified rir-generator.cc) and the float64 model of tests/rir_model.py.

The unit of the bounds is each case's recorded e_ref = max |reference - model| / peak, the
reference's own float32 noise: the device stays within 4 e_ref of the reference (the convention of
test_gpu_simu.py; the factor covers a different rounding path) and is no worse than the reference
against the model (e_ref).  Measured figures: tests/PARITY_NOTES_RIR.md.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rir_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = rm.load_fixture()
NAMES = sorted(FIXTURE)


def spec_of(case, **change):
    from setk_amd import _ffi
    c = dict(case, **change)
    return _ffi.rir_spec(c["room"], c["src"], c["mics"], c["beta"], c["num_samples"], samp_frequency=c["fs"],
                         sound_velocity=c["c"], order=c["order"], hp_filter=c["hp"], mic_type=c["mic_type"],
                         angle=c["angle"])


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    return _ffi.default_context()


@pytest.fixture(scope="module")
def models():
    return {name: rm.generate(FIXTURE[name][0]) for name in NAMES}


@pytest.fixture(scope="module")
def singles(ctx):
    """Every case through the single call, once."""
    out = {}
    for name in NAMES:
        rir, status = ctx.rir_generate(spec_of(FIXTURE[name][0]))
        assert status == 0, name
        out[name] = rir
    return out


def batch_call(ctx, names, flags=0):
    specs = [spec_of(FIXTURE[n][0]) for n in names]
    outs = [np.full((s.n_mics, s.num_samples), np.nan, np.float32) for s in specs]
    status = np.full(len(specs), -1, np.int32)
    ctx.rir_generate_batch(specs, outs, status=status, flags=flags)
    assert not status.any()
    return outs


@pytest.mark.parametrize("name", NAMES)
def test_every_case_against_the_reference_and_the_model(ctx, models, name):
    c, ref, e_ref, _ = FIXTURE[name]
    (dev,) = batch_call(ctx, [name])
    peak = np.max(np.abs(ref))
    to_ref = np.max(np.abs(dev.astype(np.float64) - ref)) / peak
    to_model = np.max(np.abs(dev - models[name])) / peak
    print(f"[{name}] device against the reference {to_ref:.3e}, against the model {to_model:.3e} of the peak "
          f"(e_ref {e_ref:.3e})")
    assert dev.dtype == np.float32 and dev.shape == ref.shape and np.isfinite(dev).all()
    assert to_ref <= 4 * e_ref
    assert to_model <= e_ref  # no worse than the reference


def test_integer_delay_puts_the_bare_gain_on_one_tap(ctx):
    """d = 0: the direct path of the integer_delay case without the filter and the reflections is
    1 / (4 pi 0.5) at tap 32 and nothing else (Sinc(0) = 1, rir-generator.h:156)."""
    rir, status = ctx.rir_generate(spec_of(FIXTURE["integer_delay"][0], hp=False, order=0))
    want = np.zeros(rir.shape[1], np.float32)
    want[32] = np.float32(1.0 / (4 * np.pi * 0.5))
    assert status == 0 and np.array_equal(rir[0], want)


def test_one_ragged_batch_has_the_bits_of_the_single_calls(ctx, singles):
    first = batch_call(ctx, NAMES)
    again = batch_call(ctx, NAMES[::-1])[::-1]
    unsplit = batch_call(ctx, NAMES, flags=1)  # SETK_RIR_NO_SPLIT: one workgroup per (RIR, microphone)
    for name, a, b, u in zip(NAMES, first, again, unsplit):
        assert np.array_equal(a, singles[name]), name  # alone (split over workgroups) or in a batch
        assert np.array_equal(a, b), name              # run to run, in another batch order
        assert np.array_equal(a, u), name              # however the images are cut


def test_libs_generate_rir_with_a_reverberation_time(singles):
    """The float32 pre-processing (rir-generator.cc:78-92): from the T60 the fixture's reference was
    given to the bits of the call on the recorded coefficients."""
    from setk_amd.libs.rir import generate_rir
    for name in ("small", "anechoic", "pattern_cardioid", "integer_delay"):
        c = FIXTURE[name][0]
        rir = generate_rir(c["room"], c["src"], c["mics"], c["rt60"], sr=c["fs"], rir_nsamps=c["num_samples"],
                           v=c["c"], order=c["order"], hp_filter=c["hp"], mic_type=c["mic_type"], angle=c["angle"])
        assert np.array_equal(rir, singles[name]), name
    c = FIXTURE["six_betas"][0]
    rir = generate_rir(c["room"], c["src"], c["mics"], c["beta"], rir_nsamps=c["num_samples"])
    assert np.array_equal(rir, singles["six_betas"])


def test_engine_equals_the_c_call(singles):
    from setk_amd.engine import BatchRirGenerator
    names = ["array16", "small", "taps_1", "pattern_bidirectional", "no_hp"]
    for kw in (dict(), dict(max_batch_bytes=20000), dict(split=False)):  # one batch; several; unsplit
        e = BatchRirGenerator(**kw)
        res = e.run([dict(room=c["room"], src=c["src"], mics=c["mics"], beta_or_rt60=c["beta"], sr=c["fs"],
                          rir_nsamps=c["num_samples"], v=c["c"], order=c["order"], hp_filter=c["hp"],
                          mic_type=c["mic_type"], angle=c["angle"]) for c in (FIXTURE[n][0] for n in names)])
        e.close()
        assert e.status == [0] * len(names)
        for name, r in zip(names, res):
            assert np.array_equal(r, singles[name]), (kw, name)
    assert BatchRirGenerator().run([]) == []


def test_status_and_refusals(ctx, singles):
    from setk_amd import _ffi
    c = FIXTURE["small"][0]
    with pytest.raises(_ffi.SetkUnsupported, match="16 microphones"):
        ctx.rir_generate(spec_of(c, mics=np.tile(c["mics"], (17, 1))))
    with pytest.raises(_ffi.SetkUnsupported, match="16384 taps"):
        ctx.rir_generate(spec_of(c, num_samples=16385))
    with pytest.raises(ValueError, match="order >= -1"):
        ctx.rir_generate(spec_of(c, order=-2))
    with pytest.raises(ValueError, match="six reflection coefficients"):
        ctx.rir_generate(spec_of(c, beta=c["beta"][:5]))
    with pytest.raises(ValueError, match="samp_frequency >= 1"):
        ctx.rir_generate(spec_of(c, fs=0.5))
    with pytest.raises(ValueError, match="sound_velocity >= 1"):
        ctx.rir_generate(spec_of(c, c=0.0))
    # NaN in a position flags that RIR only; its neighbours in the batch keep their bits
    bad_src = c["src"].copy()
    bad_src[1] = np.nan
    specs = [spec_of(c), spec_of(c, src=bad_src), spec_of(FIXTURE["no_hp"][0])]
    outs = [np.full((s.n_mics, s.num_samples), np.nan, np.float32) for s in specs]
    status = np.full(3, -1, np.int32)
    ctx.rir_generate_batch(specs, outs, status=status)
    assert list(status) == [0, _ffi.NUM_NONFINITE, 0]
    assert np.array_equal(outs[0], singles["small"]) and np.array_equal(outs[2], singles["no_hp"])
    # a source on the microphone: the reference divides by zero there; that image is left out and flagged
    rir, st = ctx.rir_generate(spec_of(c, src=c["mics"][0]))
    assert st == _ffi.NUM_NONFINITE and np.isfinite(rir).all()


def test_the_largest_tap_count(ctx):
    """16384 taps (131 072 bytes of sums in LDS, one workgroup per CU), reflections up to order 1 to keep it to
    milliseconds.  The bound is the arithmetic's: float64 on both sides, so what is left is the final
    rounding to float32, 2^-24 of a tap, and the 2^-41 grid of a handful of images: 2^-23 of the peak."""
    c = dict(FIXTURE["small"][0], num_samples=16384, order=1)
    dev, st = ctx.rir_generate(spec_of(c))
    model = rm.generate(c)
    assert st == 0 and dev.shape == (1, 16384)
    assert np.max(np.abs(dev - model)) <= 2.0**-23 * np.max(np.abs(model))


@pytest.mark.parametrize("name", ["rir_generate_1d", "rir_generate_2d"])
def test_command_line_reproduces_the_reference_run(name, tmp_path, monkeypatch):
    """With the seed the reference's script was recorded under: its rir.json to the byte, and the RIR
    it got from rir-simulate to one LSB of the 16-bit file (the generator's matrix x 32767; the writers
    may round differently, tests/PARITY_NOTES_RIR.md).  A RIR it wrote goes through wav_simulate.py."""
    import importlib
    import json
    import scipy.io.wavfile
    from setk_amd.sptk import wav_simulate
    cli = importlib.import_module("setk_amd.sptk." + name)
    args, seed, want_json, want_rir = rm.load_cli_fixture(name)
    monkeypatch.chdir(tmp_path)
    cli.main(args + ["--seed", str(seed)])
    dump = args[args.index("--dump-dir") + 1]
    got = open(os.path.join(dump, "rir.json")).read()
    assert got == want_json
    loc = json.loads(got)[0]["spk"][0]["loc"]
    sr, wav = scipy.io.wavfile.read(loc)
    assert sr == 16000 and wav.dtype == np.int16 and wav.shape == want_rir.T.shape
    lsb = np.max(np.abs(wav.astype(np.float64) - want_rir.T.astype(np.float64) * 32767.0))
    print(f"[{name}] Room1-1.wav against the reference's matrix x 32767: {lsb:.3f} LSB")
    assert lsb <= 1.0
    rng = np.random.default_rng(5)
    scipy.io.wavfile.write("spk.wav", 16000, (3000 * rng.standard_normal(16000)).astype(np.int16))
    wav_simulate.main(["mix.wav", "--src-spk", "spk.wav", "--src-rir", loc])
    sr, mix = scipy.io.wavfile.read("mix.wav")
    assert sr == 16000 and mix.shape == (16000, 4) and np.abs(mix).max() > 0
