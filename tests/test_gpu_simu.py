"""
Data simulation on the MI355X (setk_amd/csrc/simu.hip, libs/simu.py, engine/simu.py and the
command line) against the float64 model of tests/simu_model.py and the reference's recorded
results in tests/golden/ref_simu*.npz (tools/make_simu_golden.py).  The bounds and the measured
figures are in tests/PARITY_NOTES_SIMU.md.

Bounds.  A mixture is held to 4 x its case's e_ref of the peak, e_ref being the REFERENCE's own
worst error against the float64 model, recorded in the fixture (1.8e-7 to 4.8e-7 on the far-field
cases).  The factor 4 covers the device's different rounding path: two 512-point transforms and up
to 32 accumulated products against one long pocketfft transform.  The stand-alone operator, whose
inputs are not fixture cases, is held to the float64 model within 4 x the SMALLEST far-field
e_ref of the fixture.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import simu_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu
FAR = ("far", "far_repeat", "far_ch1", "far_ch1_repeat")


@pytest.fixture(scope="module")
def gold():
    return sm._golden("ref_simu.npz")


@pytest.fixture(scope="module")
def op_bound(gold):
    return 4.0 * min(float(gold[f"{n}_e_ref"]) for n in FAR)


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    return _ffi.default_context()


@pytest.fixture(scope="module")
def engine():
    from setk_amd.engine import BatchSimulator
    e = BatchSimulator()
    yield e
    e.close()


def reverb(ctx, spk, rir, flags=0):
    N, R = rir.shape
    out = np.full((N, spk.size), np.nan, dtype=np.float32)
    power = np.zeros(1)
    ctx.fir_reverb(spk, spk.size, rir, N, R, out, power, flags=flags)
    return out, float(power[0])


def recipe_of(case):
    """A fixture case as an engine.Recipe (what libs.simu.load_recipe builds from its files)."""
    from setk_amd.engine.simu import Recipe, Source
    L = sm.mix_nsamps(case)
    sdr = [0.0] + list(case.get("sdr", []))
    spk = [Source(sm.pcm_to_float(s), rir=None if case.get("spk_rir") is None else sm.pcm_to_float(case["spk_rir"][i]),
                  begin=case["spk_begin"][i], snr=sdr[i]) for i, s in enumerate(case["spk"])]
    noises = [Source(sm.pcm_to_float(n)[:L],
                     rir=None if case.get("noise_rir") is None else sm.pcm_to_float(case["noise_rir"][i]),
                     begin=case["noise_begin"][i], snr=case["noise_snr"][i], repeat=bool(case.get("repeat")))
              for i, n in enumerate(case.get("noise") or [])]
    iso = None
    if case.get("iso") is not None:
        o = case.get("iso_offset", 0)
        iso = sm.pcm_to_float(case["iso"])[..., o:o + L]
    return Recipe(spk, noises, iso=iso, iso_snr=case.get("iso_snr", 0.0), dump_channel=case["dump_channel"],
                  norm_factor=case["norm_factor"])


# ---------------------------------------------------------------- the operator
@pytest.mark.parametrize("tap", [0, 255, 256, 257, 599])
def test_unit_tap_at_block_boundaries(ctx, tap):
    """N = 1, S = 768, a RIR that is one unit tap: the output is the shifted input; a misplaced
    partition or frame gives an error of order 1."""
    rng = np.random.default_rng(tap)
    x = rng.standard_normal(768).astype(np.float32)
    h = np.zeros((1, 600), np.float32)
    h[0, tap] = 1.0
    out, _ = reverb(ctx, x, h)
    want = np.concatenate([np.zeros(tap, np.float32), x])[:768]
    err = float(np.max(np.abs(out[0] - want)) / np.max(np.abs(x)))
    print(f"unit tap at {tap}: {err:.3e} of the peak")
    assert err < 1e-6


@pytest.mark.parametrize("S,R,N", [(4000, 600, 4), (300, 601, 2), (768, 256, 3), (16000, 8000, 8)])
def test_reverb_ragged_ends_against_float64(ctx, op_bound, S, R, N):
    """Source and RIR lengths that are no multiple of the block, a source shorter than its RIR
    (P = 3), one partition, and the workload's 32 partitions at 8 channels."""
    rng = np.random.default_rng(S + R)
    x = sm.pcm_to_float(sm._speech(rng, S))
    h = sm.pcm_to_float(sm._rir(rng, N, R))
    out, power = reverb(ctx, x, h)
    want = sm.fftconvolve64(x, h)
    peak = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(out - want))) / peak
    p64 = float(np.mean(want[0]**2))
    # |d mean(y^2)| <= 2 eps peak mean|y| + eps^2 peak^2 <= 2 eps peak rms for a pointwise error eps peak
    p_bound = 2.0 * op_bound * peak / np.sqrt(p64) + 1e-12
    print(f"S {S} R {R} N {N}: {err:.3e} of the peak (bound {op_bound:.3e}); power {abs(power - p64) / p64:.3e} "
          f"(bound {p_bound:.3e})")
    assert np.isfinite(out).all() and err <= op_bound
    assert abs(power - p64) / p64 <= p_bound
    # 16-bit samples in: the same bits as their float32 values
    pcm = np.rint(x * 32768.0).astype(np.int16)
    from setk_amd import _ffi
    out16, power16 = reverb(ctx, pcm, h, flags=_ffi.FLAG_IN_PCM16)
    assert np.array_equal(out16, out) and power16 == power


def test_operator_limits(ctx):
    from setk_amd import _ffi
    x = np.zeros(100, np.float32)
    for N, R in ((17, 10), (1, 16385)):
        with pytest.raises(_ffi.SetkUnsupported):
            ctx.fir_reverb(x, 100, np.zeros((N, R), np.float32), N, R, np.zeros((N, 100), np.float32))
    with pytest.raises(_ffi.SetkUnsupported):
        ctx.fir_reverb(x, 0, np.zeros((1, 8), np.float32), 1, 8, np.zeros((1, 100), np.float32))


def test_mirror_functions(ctx, op_bound):
    """libs.simu's add_room_response (both powers), add_speaker and add_point_noise keep the
    reference's shapes and values."""
    from setk_amd.libs import simu
    rng = np.random.default_rng(5)
    x, y = sm.pcm_to_float(sm._speech(rng, 1500)), sm.pcm_to_float(sm._speech(rng, 1200))
    h = sm.pcm_to_float(sm._rir(rng, 2, 900))
    revb, p = simu.add_room_response(x, h)
    want = sm.convolve64(x, h)
    assert revb.shape == (2, 1500) and abs(p - np.mean(want[0]**2)) / p < 1e-5
    _, pe = simu.add_room_response(x, h, early_energy=True)
    peak = int(np.argmax(h[0]))
    early = np.zeros_like(h[0])
    early[max(0, peak - 16):min(900, peak + 800)] = h[0][max(0, peak - 16):min(900, peak + 800)]
    assert abs(pe - np.mean(sm.convolve64(x, early)[0]**2)) / pe < 1e-5
    spk = simu.add_speaker(2000, [x, y], [0, 300], [0, 3.0], src_rir=[h, h])
    assert len(spk) == 2 and spk[0].shape == (2, 2000) and spk[0].dtype == np.float64
    pw = [np.sum(s[0]**2) / n for s, n in zip(spk, (1500, 1200))]
    assert abs(10 * np.log10(pw[0] / pw[1]) - 3.0) < 1e-3
    assert np.max(np.abs(spk[0][:, :1500] - want)) / np.max(np.abs(want)) <= op_bound
    ref_power = np.mean(sum(spk)[0]**2)
    nz = simu.add_point_noise(2000, ref_power, [y], [100], [7.0], noise_rir=[h], repeat=True)
    assert nz.shape == (2, 2000) and not nz[:, :100].any()
    assert abs(10 * np.log10(ref_power / (np.sum(nz[0]**2) / 1900)) - 7.0) < 1e-3


# ---------------------------------------------------------------- mixing
@pytest.fixture(scope="module")
def device_results(gold, engine):
    """Every fixture case run alone, once, shared by the tests below."""
    out = {}
    for name in sm.CASES:
        case, ref = sm.load_case(gold, name)
        out[name] = (case, ref, engine.run([recipe_of(case)])[0])
    return out


@pytest.mark.parametrize("name", list(sm.CASES))
def test_mixture_against_the_reference(device_results, name):
    """mix, the speaker references and the noise reference against the reference's recorded arrays."""
    case, ref, res = device_results[name]
    noise = res.noise
    if noise is not None and np.ndim(ref["noise"]) == 0:
        noise = noise[0]  # (isotropic noise only: the reference returns the first sample)
    err = sm.worst_error((res.mix, res.spk, noise), ref)
    bound = 4.0 * ref["e_ref"]
    print(f"{name}: device {err:.3e} of the peak (bound {bound:.3e}, e_ref {ref['e_ref']:.3e}); "
          f"peak {np.max(np.abs(res.mix)):.7f}")
    assert res.status == 0 and res.mix.dtype == np.float32
    assert res.mix.shape == np.atleast_2d(ref["mix"]).shape
    assert (res.noise is None) == (ref["noise"] is None)
    assert err <= bound


@pytest.mark.parametrize("name", ["far", "far_ch1_repeat", "close2"])
def test_requested_sdr_is_recovered(device_results, name):
    case, _, res = device_results[name]
    pw = [np.sum(np.float64(r)**2) / len(s) for r, s in zip(res.spk, case["spk"])]
    sdr = 10 * np.log10(pw[0] / pw[1])
    print(f"{name}: SDR {sdr:.6f} dB for {case['sdr'][0]}")
    assert abs(sdr - case["sdr"][0]) < 1e-3


@pytest.mark.parametrize("name,repeat", [("close2", False), ("far", False), ("far", True)])
def test_requested_snr_is_recovered(gold, engine, name, repeat):
    """From the device's own references: the power of the speaker-only mixture over the mixture,
    the noise's over its duration (:124, :54).  (Without the isotropic chunk, which shares the
    noise reference.)"""
    case, _ = sm.load_case(gold, name)
    case = dict(case, iso=None, repeat=repeat)
    res = engine.run([recipe_of(case)])[0]
    L, beg = sm.mix_nsamps(case), case["noise_begin"][0]
    dur = L - beg if repeat else min(len(case["noise"][0]), L - beg)
    spk_power = np.mean(sum(np.float64(r) for r in res.spk)**2)
    snr = 10 * np.log10(spk_power / (np.sum(np.float64(res.noise)**2) / dur))
    print(f"{name} repeat {repeat}: SNR {snr:.6f} dB for {case['noise_snr'][0]}")
    assert not res.noise[:beg].any() and not res.noise[beg + dur:].any()
    assert abs(snr - case["noise_snr"][0]) < 1e-3


def test_batch_and_repeat_identity(gold, device_results):
    """A ragged batch -- far-field and close-talk recipes, one and four channels, with and without
    noise, a RIR shared by two recipes -- equals the per-mixture calls bit for bit, float32 and
    16-bit; two runs are bit-identical."""
    from setk_amd.engine import BatchSimulator
    names = list(sm.CASES)
    recipes = [recipe_of(device_results[n][0]) for n in names]
    recipes[1].speakers[0].rir = recipes[0].speakers[0].rir  # one array, two recipes: transformed once
    alone = [device_results[n][2] for n in names]
    alone[1] = None
    for pcm16 in (False, True):
        e = BatchSimulator(pcm16=pcm16)
        first, second = e.run(recipes), e.run(recipes)
        singles = [e.run([r])[0] for r in recipes]
        e.close()
        for n, a, b, c, d in zip(names, first, second, singles, alone):
            for x, y, z in zip([a.mix] + a.spk + [a.noise], [b.mix] + b.spk + [b.noise], [c.mix] + c.spk + [c.noise]):
                assert (x is None and y is None) or (np.array_equal(x, y) and np.array_equal(x, z)), (n, pcm16)
            if d is not None and not pcm16:
                assert np.array_equal(a.mix, d.mix), n
            assert a.mix.dtype == (np.int16 if pcm16 else np.float32)
        if pcm16:
            # the device's rounding is the writer's: float32 value x 32767, to nearest
            f32 = alone[0]
            assert np.array_equal(first[0].mix, sm.to_pcm16(f32.mix.T))
            assert np.array_equal(first[0].spk[1], sm.to_pcm16(f32.spk[1]))


def test_nonfinite_input_is_reported(engine):
    from setk_amd import _ffi
    from setk_amd.engine.simu import Recipe, Source
    x = np.ones(700, np.float32)
    x[300] = np.nan
    good = Recipe([Source(np.ones(500, np.float32) * 0.1)])
    res = engine.run([Recipe([Source(x, rir=np.ones((2, 300), np.float32))]), good])
    assert [r.status for r in res] == [_ffi.NUM_NONFINITE, _ffi.NUM_OK] and engine.status == [3, 0]


def test_what_the_reference_refuses(engine):
    from setk_amd import _ffi
    from setk_amd.engine.simu import Recipe, Source
    x, h4, h2 = np.ones(600, np.float32), np.ones((4, 50), np.float32), np.ones((2, 50), np.float32)
    with pytest.raises(RuntimeError, match="Channel mismatch"):
        engine.run([Recipe([Source(x, rir=h4)], [Source(x, rir=h2, snr=5)])])
    with pytest.raises(RuntimeError, match="Can not convolve"):
        engine.run([Recipe([Source(np.ones((2, 600), np.float32), rir=h4)])])
    with pytest.raises(RuntimeError, match="Channel number mismatch"):
        engine.run([Recipe([Source(x, rir=h4)], iso=np.ones((2, 600), np.float32), iso_snr=3)])
    with pytest.raises(ValueError, match="last noise's duration"):  # numpy's broadcast error there
        engine.run([Recipe([Source(x)], [Source(np.ones(200, np.float32), snr=5), Source(np.ones(300, np.float32), snr=5)])])
    with pytest.raises(_ffi.SetkUnsupported, match="16384 taps"):
        engine.run([Recipe([Source(x, rir=np.ones((1, 16385), np.float32))])])


# ---------------------------------------------------------------- the command line
def _check_files(tag, out_dir, ref_files, n_spk):
    import scipy.io.wavfile as wavfile
    got = {"mix": wavfile.read(os.path.join(out_dir, "mix.wav"))[1],
           "noise": wavfile.read(os.path.join(out_dir, "ref", "noise", "mix.wav"))[1]}
    for i in range(n_spk):
        got[f"spk{i}"] = wavfile.read(os.path.join(out_dir, "ref", f"spk{i + 1}", "mix.wav"))[1]
    for key, pcm in got.items():
        assert pcm.dtype == np.int16 and pcm.shape == ref_files[key].shape, (tag, key, pcm.shape)
        worst, frac = sm.pcm_diff(pcm, ref_files[key])
        print(f"{tag} {key}: worst {worst} LSB, {100 * frac:.3f} % of the samples differ")
        # no sample by more than 1 LSB, at most 0.5 % at all (the reference against a float64 run
        # of itself: 1 LSB on 0.06 - 0.09 %)
        assert worst <= 1 and frac <= 0.005, (tag, key, worst, frac)


def test_command_line_and_cmd_list(gold, tmp_path):
    """The doc-derived case and one synthetic case through scripts/sptk/wav_simulate.py, one
    process each, and both as the lines of one --cmd-list, against the reference's PCM_16 files."""
    import shlex
    doc, doc_files, _ = sm.load_doc_case()
    far, far_ref = sm.load_case(gold, "far")
    script = os.path.join(ROOT, "scripts", "sptk", "wav_simulate.py")
    lines = []
    for tag, case, files in (("doc", doc, doc_files), ("far", far, far_ref["cli"])):
        src = tmp_path / f"{tag}_in"
        src.mkdir()
        paths = sm.write_case_files(case, str(src))
        one, lst = tmp_path / f"{tag}_one", tmp_path / f"{tag}_list"
        args = sm.cli_args(case, paths, str(one / "mix.wav"), str(one / "ref"))
        r = subprocess.run([sys.executable, script] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "Time cost:" in r.stdout and "RTF =" in r.stdout
        _check_files(tag + " (one process)", str(one), files, len(case["spk"]))
        lines.append(" ".join(shlex.quote(a) for a in sm.cli_args(case, paths, str(lst / "mix.wav"), str(lst / "ref"))))
    cmd = tmp_path / "cmd.list"
    cmd.write_text("\n\n".join(lines) + "\n")
    r = subprocess.run([sys.executable, script, "--cmd-list", str(cmd), "--batch-utts", "2"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("Time cost:") == 1  # one batch
    for tag, case, files in (("doc", doc, doc_files), ("far", far, far_ref["cli"])):
        _check_files(tag + " (--cmd-list)", str(tmp_path / f"{tag}_list"), files, len(case["spk"]))
