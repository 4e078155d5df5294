"""
OM-LSA noise suppression on the MI355X (setk_amd/csrc/ns.hip, libs/ns.py, engine/ns.py and the
command line) against the reference's recorded gains in tests/golden/ref_ns.npz
(tools/make_ns_golden.py) and the float64 model of tests/ns_model.py.  The bounds and the measured
figures are in tests/PARITY_NOTES_NS.md.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ns_model  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
E1_BOUND = 1e-13
# device against the float64 model: both evaluate E1 in closed form, so what is left is rounding
# (E1 to 1e-13, amplified 30 times by the recursion: 3e-12) -- the floor of the issue's bound
MODEL_BOUND = 1e-8
# |device PCM - reference command line PCM| on fixture cli_*: the measured worst difference (0) plus
# one LSB (the device STFT is float32, the reference's float64 rounded to complex64)
CLI_WAV_LSB = 1
STFT = dict(frame_len=512, frame_hop=256, window="hann", center=True, round_power_of_two=True)


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_ns.npz")


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    return _ffi.default_context()


def suppressor(kind, **conf):
    from setk_amd.libs import ns
    return (ns.MCRA if kind == "mcra" else ns.iMCRA)(**conf)


def relerr(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


# ---------------------------------------------------------------- E1
def test_expint_e1_against_scipy(ctx):
    from scipy.special import exp1
    seam = np.array([np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 1.0 - 1e-9, 1.0 + 1e-9, 0.999, 1.001])
    x = np.concatenate([np.logspace(-12, np.log10(700.0), 4001), seam, [1e-300, 745.0, 800.0, 1e308]])
    y = np.full_like(x, np.nan)
    ctx.expint_e1(x, y)
    n = 4001 + seam.size
    err = np.abs(y[:n] - exp1(x[:n])) / exp1(x[:n])
    print(f"E1: worst relative error {err.max():.3e} at x = {x[:n][np.argmax(err)]:.6g}; at the seam {err[4001:].max():.3e}")
    assert err.max() <= E1_BOUND
    # far ends: finite near zero, a clean underflow to 0 at the top
    assert abs(y[n] - exp1(1e-300)) / exp1(1e-300) <= E1_BOUND
    assert y[n + 1] >= 0 and y[n + 1] < 1e-300 and y[n + 2] == 0.0 and y[n + 3] == 0.0


# ---------------------------------------------------------------- recursion parity
@pytest.mark.parametrize("name", sorted(ns_model.CASES))
def test_gain_against_the_reference_and_the_model(gold, ctx, name):
    kind, T, F, _, conf = ns_model.CASES[name]
    stft, want = gold[name + "_stft"], gold[name + "_gain"]
    assert stft.shape == (T, F) and stft.dtype == np.complex64
    s = suppressor(kind, **conf)
    got = s.run(stft)
    assert got.shape == (T, F) and got.dtype == np.float64
    # the operator, with the gained spectrogram out of the same pass
    g2, enh, st = np.empty((T, F)), np.empty((T, F), np.complex64), np.full(1, -1, np.int32)
    ctx.ns_gain(s.opts(gain=True, spec=True), stft, T, F, gain=g2, out=enh, status=st)
    assert g2.tobytes() == got.tobytes() and st[0] == 0
    want_enh = (got * stft.real.astype(np.float64)).astype(np.float32) + \
        1j * (got * stft.imag.astype(np.float64)).astype(np.float32)
    assert enh.tobytes() == want_enh.astype(np.complex64).tobytes()
    model, margin = ns_model.run(kind, stft, **conf)
    bound = max(1e-8, 30 * float(gold["model_err_worst"]))
    e_ref, e_model = relerr(got, want), relerr(got, model)
    print(f"{name}: device vs reference {e_ref:.3e} (bound {bound:.2e}), vs model {e_model:.3e} "
          f"(bound {MODEL_BOUND:.0e}), margin {margin:.2e}")
    assert margin >= ns_model.MIN_MARGIN
    assert e_ref <= bound
    assert e_model <= MODEL_BOUND


@pytest.mark.parametrize("kind,F", [("mcra", 1025), ("imcra", 1025), ("imcra", 1024), ("mcra", 64)])
def test_two_bins_per_lane_and_full_workgroups(kind, F):
    """F = 1025 (n_fft = 2048) gives a lane two bins; 1024 and 64 fill their waves exactly."""
    stft = ns_model.synth_spectrogram(24, F, 3)
    conf = dict(V=5, U=3) if kind == "imcra" else dict(L=12)
    got = suppressor(kind, **conf).run(stft)
    model, margin = ns_model.run(kind, stft, **conf)
    print(f"{kind} F = {F}: device vs model {relerr(got, model):.3e}, margin {margin:.2e}")
    assert margin >= ns_model.MIN_MARGIN and relerr(got, model) <= MODEL_BOUND


def test_two_runs_give_the_same_bytes(gold):
    s = suppressor("imcra")
    assert s.run(gold["b_imcra_stft"]).tobytes() == s.run(gold["b_imcra_stft"]).tobytes()


# ---------------------------------------------------------------- the fused path
def by_operators(ctx, s, x, pcm16):
    """setk_stft -> setk_ns_gain -> setk_istft (-> setk_float_to_pcm16) of one utterance."""
    F = 257
    T = ctx.num_frames(x.size)
    spec = np.empty((1, T, F), np.complex64)
    ctx.stft(np.ascontiguousarray(x[None]), spec)
    gain, enh = np.empty((T, F)), np.empty((1, T, F), np.complex64)
    ctx.ns_gain(s.opts(gain=True, spec=True), spec, T, F, gain=gain, out=enh)
    L = ctx.istft_num_samples(T)
    wav = np.empty((1, L), np.float32)
    ctx.istft(enh, 1, T, None, None, wav)
    if not pcm16:
        return gain, wav[0]
    q = np.empty((L, 1), np.int16)
    ctx.float_to_pcm16(wav, 1, L, q)
    return gain, q[:, 0]


@pytest.mark.parametrize("kind", ["mcra", "imcra"])
def test_ragged_batch_equals_the_operator_path_bit_for_bit(ctx, kind):
    import torch
    from setk_amd import _ffi
    from setk_amd.libs.utils import stft_window
    hop = 128
    ctx.stft_plan(512, hop, 512, True, stft_window("hann", 512))
    frames = (150, 40, 7)
    pcm = [np.rint(ns_model.synth_samples((T - 1) * hop, 40 + k) * 32767).astype(np.int16)
           for k, T in enumerate(frames)]
    f32 = [p.astype(np.float32) / np.float32(32768.0) for p in pcm]
    assert [ctx.num_frames(x.size) for x in f32] == list(frames)
    s = suppressor(kind)
    for in16 in (False, True):
        src = [torch.from_numpy(p if in16 else x).cuda() for p, x in zip(pcm, f32)]
        for out16 in (False, True):
            lens = [ctx.istft_num_samples(T) for T in frames]
            waves = [torch.zeros(L, dtype=torch.int16 if out16 else torch.float32, device="cuda") for L in lens]
            gains = [torch.full((T, 257), float("nan"), dtype=torch.float64, device="cuda") for T in frames]
            st = np.full(3, -1, np.int32)
            flags = (_ffi.FLAG_IN_PCM16 if in16 else 0) | (_ffi.FLAG_OUT_PCM16 if out16 else 0)
            ctx.ns_batch(s.opts(gain=True, spec=True), [a.data_ptr() for a in src], [x.size for x in f32],
                         wave_ptrs=[w.data_ptr() for w in waves], gain_ptrs=[g.data_ptr() for g in gains],
                         status=st, flags=flags)
            torch.cuda.synchronize()
            assert list(st) == [0, 0, 0]
            for k, x in enumerate(f32):
                gain, wav = by_operators(ctx, s, x, out16)
                assert gains[k].cpu().numpy().tobytes() == gain.tobytes(), (in16, out16, k)
                assert waves[k].cpu().numpy().tobytes() == wav.tobytes(), (in16, out16, k)
    ctx.stft_plan(512, 256, 512, True, stft_window("hann", 512))


def test_wave_and_gain_against_the_reference_command_line(gold):
    from setk_amd.engine import BatchNoiseSuppressor, Pcm16Frames
    pcm = gold["cli_pcm"]
    utt = Pcm16Frames(pcm[:, None])
    e = BatchNoiseSuppressor(suppressor("imcra"), output="wave", pcm16=True, **STFT)
    wav = e.run([utt])[0]
    e.close()
    e = BatchNoiseSuppressor(suppressor("imcra"), output="gain", **STFT)
    gain = e.run([utt])[0]
    e.close()
    want = gold["cli_wav"]
    assert wav.dtype == np.int16 and wav.shape == want.shape
    lsb = int(np.abs(wav.astype(np.int32) - want.astype(np.int32)).max())
    # the command line's own gain is a mixed float32 / float64 computation (its STFT is complex64):
    # the float64 model differs from it by cli_model_err; 30 x that, as for the stored spectrograms
    g_bound = max(1e-8, 30 * float(gold["cli_model_err"]))
    g_err = relerr(gain, gold["cli_gain"])
    print(f"cli: worst PCM difference {lsb} LSB (allowed {CLI_WAV_LSB}); gain vs the command line's "
          f"{g_err:.3e} (bound {g_bound:.2e})")
    assert gain.shape == gold["cli_gain"].shape and g_err <= g_bound
    assert lsb <= CLI_WAV_LSB


# ---------------------------------------------------------------- device tensors
@pytest.mark.parametrize("kind", ["mcra", "imcra"])
def test_device_tensors_through_the_c_abi(gold, ctx, kind):
    import torch
    stft = gold["b_" + kind + "_stft"]
    T, F = stft.shape
    s = suppressor(kind)
    g_host, e_host = np.empty((T, F)), np.empty((T, F), np.complex64)
    ctx.ns_gain(s.opts(gain=True, spec=True), stft, T, F, gain=g_host, out=e_host)
    d = torch.from_numpy(stft).cuda()
    g_dev = torch.full((T, F), float("nan"), dtype=torch.float64, device="cuda")
    e_dev = torch.zeros((T, F), dtype=torch.complex64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ctx.ns_gain(s.opts(gain=True, spec=True), d, T, F, gain=g_dev, out=e_dev, status=st.data_ptr())
    torch.cuda.synchronize()
    assert g_dev.cpu().numpy().tobytes() == g_host.tobytes()
    assert e_dev.cpu().numpy().tobytes() == e_host.tobytes()
    assert int(st.cpu()[0]) == 0
    x = torch.logspace(-6, 2, 257, dtype=torch.float64).cuda()
    y = torch.zeros_like(x)
    ctx.expint_e1(x, y)
    torch.cuda.synchronize()
    yh = np.empty(257)
    ctx.expint_e1(x.cpu().numpy(), yh)
    assert y.cpu().numpy().tobytes() == yh.tobytes()


# ---------------------------------------------------------------- silence, NaN
@pytest.mark.parametrize("kind", ["mcra", "imcra"])
def test_digital_silence_in_the_middle_stays_finite(ctx, kind):
    from setk_amd import _ffi
    from setk_amd.engine import BatchNoiseSuppressor, Pcm16Frames
    stft = ns_model.synth_spectrogram(60, 129, 8)
    stft[20:40] = 0
    s = suppressor(kind)
    T, F = stft.shape
    gain, st = np.empty((T, F)), np.full(1, -1, np.int32)
    ctx.ns_gain(s.opts(), stft, T, F, gain=gain, status=st)
    assert st[0] == _ffi.NUM_OK and np.isfinite(gain).all() and (gain > 0).all()
    model, _ = ns_model.run(kind, stft)
    assert np.isfinite(model).all()
    print(f"{kind} with 20 silent frames: device vs model {relerr(gain, model):.3e}; largest gain {gain.max():.3g}")
    # the same through the waveform path: 22 frames' worth of zero samples
    pcm = np.rint(ns_model.synth_samples(19200, 9) * 32767).astype(np.int16)
    pcm[6000:6000 + 24 * 256] = 0
    e = BatchNoiseSuppressor(s, output="wave", pcm16=True, **STFT)
    wav = e.run([Pcm16Frames(pcm[:, None])])[0]
    assert e.status == [_ffi.NUM_OK] and wav is not None and wav.dtype == np.int16
    f = BatchNoiseSuppressor(s, output="wave", **STFT)
    wav32 = f.run([pcm.astype(np.float32) / np.float32(32768.0)])[0]
    assert np.isfinite(wav32).all() and np.abs(wav32).max() < 2.0 and np.abs(wav32[7000:11000]).max() == 0
    e.close()
    f.close()


def test_nan_is_reported_for_its_utterance_only(ctx):
    from setk_amd import _ffi
    from setk_amd.engine import BatchNoiseSuppressor
    utts = [ns_model.synth_samples(n, 50 + k).astype(np.float32) for k, n in enumerate((6000, 9000, 5000))]
    e = BatchNoiseSuppressor(suppressor("imcra"), output="gain", **STFT)
    clean = e.run(utts)
    assert e.status == [0, 0, 0]
    bad = [u.copy() for u in utts]
    bad[1][4000] = np.nan
    got = e.run(bad)
    assert e.status == [_ffi.NUM_OK, _ffi.NUM_NONFINITE, _ffi.NUM_OK] and got[1] is None
    assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()
    e.close()
    stft = ns_model.synth_spectrogram(12, 33, 2)
    stft[5, 7] = np.inf
    st = np.zeros(1, np.int32)
    ctx.ns_gain(suppressor("mcra").opts(), stft, 12, 33, gain=np.empty((12, 33)), status=st)
    assert st[0] == _ffi.NUM_NONFINITE


# ---------------------------------------------------------------- refusals
def test_refusals(ctx, tmp_path):
    from setk_amd import _ffi
    from setk_amd.libs import ns
    from setk_amd.sptk import apply_ns
    x = np.ones((4, 2), np.complex64)
    with pytest.raises(_ffi.SetkUnsupported, match="more taps than bins"):
        ns.iMCRA().run(x)                      # F = 2 < 3 taps
    with pytest.raises(_ffi.SetkUnsupported, match="more taps than bins"):
        ns.MCRA().run(np.ones((4, 30), np.complex64))   # w_global: 31 taps
    with pytest.raises(_ffi.SetkUnsupported, match="at most 63"):
        ns.MCRA(w_global=32)
    with pytest.raises(_ffi.SetkUnsupported, match="at most 63 taps"):
        ctx.ns_gain(_ffi.ns_opts("imcra", w_mcra=np.ones(65), V=15, U=8), np.ones((4, 129), np.complex64), 4, 129,
                    gain=np.empty((4, 129)))
    with pytest.raises(ValueError, match="unknown window"):
        ns.iMCRA(h_mcra="kaiser")
    with pytest.raises(ValueError, match="odd number of taps"):
        ctx.ns_gain(_ffi.ns_opts("imcra", w_mcra=np.ones(4), V=15, U=8), np.ones((4, 129), np.complex64), 4, 129,
                    gain=np.empty((4, 129)))
    with pytest.raises(_ffi.SetkUnsupported, match="U <= 32"):
        ns.iMCRA(U=33).run(np.ones((4, 129), np.complex64))
    with pytest.raises(_ffi.SetkUnsupported, match="num_bins <= 1025"):
        ns.iMCRA().run(np.ones((2, 2049), np.complex64))
    with pytest.raises(ValueError, match="Now only support audio in 16kHz"):
        apply_ns.main([str(tmp_path / "wav.scp"), str(tmp_path / "out"), "--sr", "8000"])


# ---------------------------------------------------------------- the command line
def run_cli(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sptk", "apply_ns.py")] + argv,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_cli_wave_gain_and_conf(tmp_path):
    import scipy.io.wavfile
    from setk_amd.engine import BatchNoiseSuppressor, Pcm16Frames
    td = str(tmp_path)
    pcm = {}
    with open(f"{td}/wav.scp", "w") as fd:
        for k, n in enumerate((19200, 7000)):
            pcm[f"utt{k}"] = np.rint(ns_model.synth_samples(n, 60 + k) * 32767).astype(np.int16)
            scipy.io.wavfile.write(f"{td}/utt{k}.wav", 16000, pcm[f"utt{k}"])
            fd.write(f"utt{k} {td}/utt{k}.wav\n")
    with open(f"{td}/conf.yaml", "w") as fd:
        fd.write("".join(f"{k}: {v}\n" for k, v in ns_model.CONF_D.items()))
    utts = [Pcm16Frames(pcm[k][:, None]) for k in ("utt0", "utt1")]
    r = run_cli([f"{td}/wav.scp", f"{td}/wave"])
    assert "Processed 2 utterances done" in r.stderr + r.stdout
    e = BatchNoiseSuppressor(suppressor("imcra"), output="wave", pcm16=True, **STFT)
    for k, want in zip(("utt0", "utt1"), e.run(utts)):
        sr, got = scipy.io.wavfile.read(f"{td}/wave/{k}.wav")
        assert sr == 16000 and got.dtype == np.int16 and got.tobytes() == want.tobytes(), k
    e.close()
    # a second run with --skip-existing finds both files
    r = run_cli([f"{td}/wav.scp", f"{td}/wave", "--skip-existing", "true"])
    assert "2 of 2 utterances already" in r.stderr + r.stdout
    run_cli([f"{td}/wav.scp", f"{td}/gain", "--output", "gain", "--conf", f"{td}/conf.yaml", "--batch-utts", "1"])
    e = BatchNoiseSuppressor(suppressor("imcra", **ns_model.CONF_D), output="gain", **STFT)
    for k, want in zip(("utt0", "utt1"), e.run(utts)):
        got = np.load(f"{td}/gain/{k}.npy")
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), k
    plain = BatchNoiseSuppressor(suppressor("imcra"), output="gain", **STFT)
    assert plain.run(utts[:1])[0].tobytes() != np.load(f"{td}/gain/utt0.npy").tobytes()  # the conf took effect
    # a frame length the batched transforms are not built for: the operators, same interface
    run_cli([f"{td}/wav.scp", f"{td}/g256", "--output", "gain", "--frame-len", "256", "--frame-hop", "128"])
    assert np.load(f"{td}/g256/utt0.npy").shape == (151, 129)
    e.close()
    plain.close()
