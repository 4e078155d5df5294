"""
GPU parity of AuxIVA (scripts/sptk/apply_auxiva.py) against recorded outputs of the unmodified
reference (tests/golden/ref_auxiva*.npz, tools/make_auxiva_golden.py) and against the float64
numpy model of tests/auxiva_model.py (itself equal to the reference to 1e-12,
tests/test_auxiva_model.py).

Bounds (BASELINE's, as DESIGN.md section 2 uses them for every operator): Y <= 1e-4, waveforms
<= 1e-3 relative RMS per source.  Every test prints the deviations it measures before it asserts.
Measured on an MI355X, per source: Y of the operator against the recorded reference 0 (c2, c4:
the same complex64 values) to 1.5e-10 (c8), against the model 2.5e-8 .. 2.6e-8 (doc recording, one
and two epochs, the odd shapes) -- the rounding of the stored complex64; the doc recording's waves
against the reference's wav files 1.1e-6 .. 2.3e-6, through the command line 8.4e-6 .. 1.5e-5; the
engine's float waves against the model 1.3e-7 .. 8.3e-7 (device STFT in front), its PCM16 waves
5.7e-6 .. 2.1e-5.  The per-bin and per-source judgement is tests/test_gpu_auxiva_conformance.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, pcm16_rel_rms, rel_rms, rms
from oracle import np_oracle as o

sys.path.insert(0, os.path.join(ROOT, "tests"))
import auxiva_model  # noqa: E402

pytestmark = pytest.mark.gpu
STFT_KW = dict(frame_len=512, frame_hop=256, window="hann", center=True)


def spectrogram(samps, kw=STFT_KW):
    """C x N float32 -> the oracle's N x T x F complex64 (SpectrogramReader with transpose)."""
    return np.stack([o.forward_stft(c, transpose=True, **kw) for c in np.atleast_2d(samps)])


def model_waves(samps, epochs, kw=STFT_KW):
    """run() of the reference on one utterance, with the model in place of auxiva():
    inverse_stft(Y[n], norm=max |samps|) per source (apply_auxiva.py:73-77)."""
    samps = np.atleast_2d(samps)
    Y = auxiva_model.auxiva(spectrogram(samps, kw), epochs)
    norm = float(np.max(np.abs(samps)))
    return np.stack([o.inverse_stft(y, transpose=True, norm=norm, **kw) for y in Y])


def egs_samples():
    egs = load_golden("doc_adaptive_beamformer.npz")["egs"]  # N x 5 int16
    return egs, np.ascontiguousarray(egs.T.astype(np.float32) / np.float32(32768.0))


# ---- 1. auxiva() against the reference's Y ------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "c4", "c8"])
def test_auxiva_matches_reference_on_scenes(name):
    from setk_amd.sptk.apply_auxiva import auxiva
    g = load_golden("ref_auxiva_scenes.npz")
    x = g[name + "_pcm"].astype(np.float32) / np.float32(32768.0)
    X, Yref = spectrogram(x), g[name + "_Y"]
    Y = auxiva(X, int(g["epochs"]))
    assert Y.shape == Yref.shape and Y.dtype == np.complex128
    for n in range(Y.shape[0]):
        dev = rel_rms(Y[n], Yref[n].astype(np.complex128))
        print(f"auxiva {name} source {n}: {dev:.3e}")
        assert dev <= 1e-4, (name, n, dev)


def test_auxiva_matches_reference_on_doc_recording():
    """egs (5 channels, 368 frames, 20 epochs): the reference's Y is not stored (3.8 MB), its
    waves are -- inverse_stft of the device's Y against them, and Y itself against the model
    (equal to the reference to 1e-12) at the STFT-domain bound."""
    from setk_amd.sptk.apply_auxiva import auxiva
    _, samps = egs_samples()
    X = spectrogram(samps)
    Y = auxiva(X, 20)
    Ym = auxiva_model.auxiva(X, 20)
    waves = load_golden("ref_auxiva.npz")["egs_waves"]
    norm = float(np.max(np.abs(samps)))
    for n in range(5):
        dev = rel_rms(Y[n], Ym[n])
        w = o.inverse_stft(Y[n], transpose=True, norm=norm, **STFT_KW)
        wdev = rel_rms(np.rint(w * 32767.0), waves[n].astype(np.float64))
        print(f"auxiva egs source {n}: Y {dev:.3e}, wave against the reference's wav {wdev:.3e}")
        assert dev <= 1e-4, (n, dev)
        assert wdev <= 1e-3, (n, wdev)


# ---- 5. which r an epoch uses --------------------------------------------------------------
def test_zero_epochs_returns_input_and_one_epoch_matches_model():
    from setk_amd.sptk.apply_auxiva import auxiva
    X = spectrogram(auxiva_model.synth_scene(7, 3, 256 * 47))
    Y0 = auxiva(X, 0)
    assert Y0.dtype == np.complex128 and np.array_equal(Y0, X.astype(np.complex128))
    for epochs in (1, 2):
        Y, Ym = auxiva(X, epochs), auxiva_model.auxiva(X, epochs)
        dev = max(rel_rms(Y[n], Ym[n]) for n in range(3))
        print(f"auxiva {epochs} epoch(s): {dev:.3e}")
        assert dev <= 1e-4, (epochs, dev)
    # an off-by-one in the norms would be far above the bound
    assert rel_rms(auxiva_model.auxiva(X, 1), auxiva_model.auxiva(X, 2)) > 1e-2


def test_auxiva_odd_shapes_and_device_tensors():
    """Any F and T of the stand-alone operators (F = 129, T not a multiple of anything; one
    frame more than a staged chunk), numpy and torch device tensors through the C ABI."""
    import torch
    from setk_amd import _ffi
    from setk_amd.sptk.apply_auxiva import auxiva
    rng = np.random.default_rng(3)
    for C, T, F in ((2, 129, 129), (4, 37, 65)):
        src = rng.laplace(size=(C, T, F)) + 1j * rng.laplace(size=(C, T, F))
        A = rng.normal(size=(F, C, C)) + 1j * rng.normal(size=(F, C, C)) + 2 * np.eye(C)
        X = np.ascontiguousarray(np.einsum("fcn,ntf->ctf", A, src).astype(np.complex64))
        Y, Ym = auxiva(X, 4), auxiva_model.auxiva(X, 4)
        dev = max(rel_rms(Y[n], Ym[n]) for n in range(C))
        print(f"auxiva C={C} T={T} F={F}: {dev:.3e}")
        assert dev <= 1e-4
        ctx = _ffi.default_context()
        xd = torch.from_numpy(X).cuda()
        yd = torch.empty_like(xd)
        st = torch.full((F,), -1, dtype=torch.int32, device="cuda")
        ctx.auxiva(xd, C, T, F, 4, yd, status=st.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy().astype(np.complex128), Y)
        assert not st.cpu().numpy().any()


# ---- 2. setk_auxiva_batch / the engine ------------------------------------------------------
EPOCHS = 6
BATCHES = {  # channels -> utterance lengths (samples); one utterance longer than 20 s
    1: (20000, 33000),
    2: (336000, 48000, 25333),
    3: (40000, 16001),
    5: (52000, 30000),
    8: (36000, 64000, 20480),
}


@pytest.mark.parametrize("C", sorted(BATCHES))
def test_engine_matches_model_and_is_reproducible(C):
    from setk_amd.engine import BatchSeparator, Pcm16Frames
    from setk_amd.libs.wavio import float_to_pcm16
    utts = [auxiva_model.synth_scene(1000 + 10 * C + k, C, N) for k, N in enumerate(BATCHES[C])]
    eng = BatchSeparator(num_epochs=EPOCHS, **STFT_KW)
    outs = eng.run(utts)
    assert eng.status == [0] * len(utts)
    refs = [model_waves(s, EPOCHS) for s in utts]
    for k, (got, ref) in enumerate(zip(outs, refs)):
        assert got.shape == ref.shape and got.dtype == np.float32
        for n in range(C):
            dev = rel_rms(got[n], ref[n])
            print(f"engine C={C} utt {k} ({BATCHES[C][k]} samples) source {n}: {dev:.3e}")
            assert dev <= 1e-3, (C, k, n, dev)
        # renormed to the input's peak (inverse_stft(norm=maxabs))
        peak = np.max(np.abs(utts[k]))
        assert np.allclose(np.max(np.abs(got), axis=1), peak, rtol=1e-5)
    # the same call twice: the same bits
    again = eng.run(utts)
    for a, b in zip(outs, again):
        assert np.array_equal(a, b)
    # a batch of n equals n single calls, bit for bit
    for k, s in enumerate(utts):
        assert np.array_equal(eng.run([s])[0], outs[k]), k
    # 16-bit frames in (converted on the device) and 16-bit samples out (the writer's rule)
    pcm = [np.rint(s * 32767.0).astype(np.int16) for s in utts]
    eng16 = BatchSeparator(num_epochs=EPOCHS, pcm16=True, **STFT_KW)
    q = eng16.run([Pcm16Frames(np.ascontiguousarray(p.T)) for p in pcm])
    f = eng.run([p.astype(np.float32) / np.float32(32768.0) for p in pcm])
    for k, (i16, f32) in enumerate(zip(q, f)):
        assert i16.dtype == np.int16 and i16.shape == f32.shape
        # (the renorm kernel quantises the float32 sample by the writer's rule, rint(x * 32767) in
        #  float64: the 16-bit output is the writer's file of the float output, sample for sample)
        assert np.array_equal(i16, float_to_pcm16(f32)), k
        ref = model_waves(pcm[k].astype(np.float32) / np.float32(32768.0), EPOCHS)
        for n in range(C):
            dev = pcm16_rel_rms(i16[n], ref[n])
            print(f"engine PCM16 C={C} utt {k} source {n}: {dev:.3e}")
            assert dev <= 1e-3, (C, k, n, dev)


def test_engine_other_transform_size_through_the_operators():
    """n_fft != 512: BatchSeparator runs setk_stft -> setk_auxiva -> setk_istft per utterance on
    host arrays.  2 channels, 4000 samples, frame 256 / hop 128, float and 16-bit frames in, float
    and PCM16 out, against the model at the bound of the batched path (1e-3 per source)."""
    from setk_amd.engine import BatchSeparator, Pcm16Frames
    kw = dict(STFT_KW, frame_len=256, frame_hop=128)
    s = auxiva_model.synth_scene(61, 2, 4000)
    q = np.rint(s * 32767.0).astype(np.int16)
    sq = q.astype(np.float32) / np.float32(32768.0)
    eng = BatchSeparator(num_epochs=EPOCHS, **kw)
    outs = eng.run([s, Pcm16Frames(np.ascontiguousarray(q.T))])
    assert eng.status == [0, 0]
    for name, got, ref in zip(("float", "frames"), outs, (model_waves(s, EPOCHS, kw), model_waves(sq, EPOCHS, kw))):
        assert got.shape == ref.shape and got.dtype == np.float32
        for n in range(2):
            dev = rel_rms(got[n], ref[n])
            print(f"engine, operators path, {name} in, source {n}: {dev:.3e}")
            assert dev <= 1e-3, (name, n, dev)
    (i16,) = BatchSeparator(num_epochs=EPOCHS, pcm16=True, **kw).run([s])
    assert i16.dtype == np.int16 and i16.shape == outs[0].shape
    for n in range(2):
        dev = pcm16_rel_rms(i16[n], model_waves(s, EPOCHS, kw)[n])
        print(f"engine, operators path, PCM16 out, source {n}: {dev:.3e}")
        assert dev <= 1e-3, (n, dev)


def test_engine_groups_mixed_channel_counts():
    from setk_amd.engine import BatchSeparator
    a = auxiva_model.synth_scene(51, 2, 30000)
    b = auxiva_model.synth_scene(52, 3, 22000)
    c = auxiva_model.synth_scene(53, 2, 18000)
    eng = BatchSeparator(num_epochs=3, **STFT_KW)
    outs = eng.run([a, b, c])
    assert [x.shape[0] for x in outs] == [2, 3, 2]
    for s, got in zip((a, b, c), outs):
        assert np.array_equal(got, eng.run([s])[0])


# ---- 3. the command line on the doc recording ----------------------------------------------
def test_cli_on_doc_recording(tmp_path):
    import scipy.io.wavfile
    egs, _ = egs_samples()
    td = str(tmp_path)
    scipy.io.wavfile.write(f"{td}/egs.wav", 16000, egs)
    open(f"{td}/wav.scp", "w").write(f"egs {td}/egs.wav\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/sptk/apply_auxiva.py"),
                        f"{td}/wav.scp", f"{td}/out"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Processed 1 utterances over 1" in r.stderr
    waves = load_golden("ref_auxiva.npz")["egs_waves"]
    assert sorted(os.listdir(f"{td}/out")) == [f"egs.src{n}.wav" for n in range(1, 6)]
    for n in range(5):
        sr, y = scipy.io.wavfile.read(f"{td}/out/egs.src{n + 1}.wav")
        assert sr == 16000 and y.dtype == np.int16 and y.shape == waves[n].shape
        ref = waves[n].astype(np.float64)
        dev = rms(y.astype(np.float64), ref) / rms(ref)
        print(f"CLI egs.src{n + 1}.wav against the reference's: {dev:.3e}")
        assert dev <= 1e-3, (n, dev)


def test_cli_two_ranks_write_every_key_once(tmp_path):
    """python -m setk_amd.launch --nproc 2 (needs two devices: one rank per GPU); on a
    single-GPU machine the same table goes through one process in batches of two."""
    import scipy.io.wavfile
    import torch
    td = str(tmp_path)
    keys = []
    with open(f"{td}/wav.scp", "w") as fd:
        for k, N in enumerate((24000, 16000, 31000, 20000, 12000)):
            s = auxiva_model.synth_scene(300 + k, 2, N)
            scipy.io.wavfile.write(f"{td}/u{k}.wav", 16000, np.rint(s.T * 32767.0).astype(np.int16))
            fd.write(f"u{k} {td}/u{k}.wav\n")
            keys.append(f"u{k}")
    script = os.path.join(ROOT, "scripts/sptk/apply_auxiva.py")
    tail = ["--num-epochs", "3", "--batch-utts", "2", f"{td}/wav.scp", f"{td}/out"]
    if torch.cuda.device_count() >= 2:
        cmd = [sys.executable, "-m", "setk_amd.launch", "--nproc", "2", "--retries", "0", script] + tail
    else:
        cmd = [sys.executable, script] + tail
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Processed 5 utterances over 5" in r.stderr
    assert sorted(os.listdir(f"{td}/out")) == sorted(f"{k}.src{n}.wav" for k in keys for n in (1, 2))


# ---- 4. refusals ---------------------------------------------------------------------------
def test_singular_and_nonfinite_input():
    from setk_amd import _ffi
    from setk_amd.sptk.apply_auxiva import auxiva
    ctx = _ffi.default_context()
    X = spectrogram(auxiva_model.synth_scene(9, 4, 256 * 40))
    C, T, F = X.shape

    def status_of(Xin, epochs=3):
        out = np.empty_like(Xin)
        st = np.full(F, -1, dtype=np.int32)
        ctx.auxiva(np.ascontiguousarray(Xin), C, T, F, epochs, out, status=st)
        return st, out

    st, _ = status_of(X)
    assert not st.any()
    silent = X.copy()
    silent[1] = 0
    st, _ = status_of(silent)
    assert (st == _ffi.NUM_SINGULAR).all(), st
    with pytest.raises(np.linalg.LinAlgError):
        auxiva(silent, 3)
    st, _ = status_of(np.zeros_like(X))
    assert (st == _ffi.NUM_SINGULAR).all(), st
    with pytest.raises(np.linalg.LinAlgError):
        auxiva(np.zeros_like(X), 3)
    # NaN in one frame of one bin: r of that frame is NaN, so every bin's covariance is
    nan = X.copy()
    nan[2, 11, 40] = np.nan
    st, _ = status_of(nan)
    assert (st == _ffi.NUM_NONFINITE).all(), st
    with pytest.raises(np.linalg.LinAlgError):
        auxiva(nan, 3)
    # zero epochs: only the bin that holds the NaN
    st, _ = status_of(nan, 0)
    assert st[40] == _ffi.NUM_NONFINITE and np.count_nonzero(st) == 1
    # an exactly duplicated channel: the reference refuses (Singular matrix).  Whether a
    # float64 elimination meets an exact zero pivot depends on its operation order: here the
    # LU of W^H V with two equal rows / columns leaves rounding residue in some bins, which
    # then report SETK_NUM_OK with finite output or SETK_NUM_NONFINITE -- never OK with a
    # non-finite output.
    dup = X.copy()
    dup[3] = dup[0]
    st, out = status_of(dup)
    ok = st == _ffi.NUM_OK
    print(f"duplicated channel: {np.count_nonzero(st == _ffi.NUM_SINGULAR)} bins singular, "
          f"{np.count_nonzero(st == _ffi.NUM_NONFINITE)} non-finite, {np.count_nonzero(ok)} OK")
    assert np.isfinite(out[:, :, ok]).all()


def test_more_than_eight_channels_is_refused_naming_the_bound():
    from setk_amd import _ffi
    from setk_amd.engine import BatchSeparator
    from setk_amd.sptk.apply_auxiva import auxiva
    X = (np.ones((9, 12, 257)) + 0j).astype(np.complex64)
    with pytest.raises(_ffi.SetkUnsupported, match="channels <= 8"):
        auxiva(X, 1)
    ctx = _ffi.default_context()
    with pytest.raises(_ffi.SetkUnsupported, match="channels <= 8"):
        ctx.auxiva(X, 9, 12, 257, 1, np.empty_like(X))
    with pytest.raises(_ffi.SetkUnsupported, match="channels <= 8"):
        BatchSeparator(num_epochs=1, **STFT_KW).run([np.zeros((9, 8000), np.float32)])
    with pytest.raises(ValueError):
        auxiva(X[0], 1)


def test_cli_logs_and_skips_a_singular_utterance(tmp_path):
    """A silent channel and an all-zero utterance inside the table: the reference's run ends
    with LinAlgError there; this command logs, skips and writes the others (PARITY_NOTES_AUXIVA)."""
    import scipy.io.wavfile
    td = str(tmp_path)
    good = np.rint(auxiva_model.synth_scene(77, 3, 24000).T * 32767.0).astype(np.int16)
    silent = good.copy()
    silent[:, 1] = 0
    wide = np.rint(auxiva_model.synth_scene(78, 9, 9000).T * 32767.0).astype(np.int16)
    table = {"a_good": good, "b_silent": silent, "c_zero": np.zeros_like(good), "d_good": good[:20000],
             "e_wide": wide}
    with open(f"{td}/wav.scp", "w") as fd:
        for k, v in table.items():
            scipy.io.wavfile.write(f"{td}/{k}.wav", 16000, v)
            fd.write(f"{k} {td}/{k}.wav\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/sptk/apply_auxiva.py"),
                        "--num-epochs", "4", f"{td}/wav.scp", f"{td}/out"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "b_silent: Failed cause LinAlgError" in r.stderr and "c_zero: Failed cause LinAlgError" in r.stderr
    assert "e_wide: skipped" in r.stderr and "channels <= 8" in r.stderr
    assert "Processed 2 utterances over 5" in r.stderr
    assert sorted(os.listdir(f"{td}/out")) == sorted(f"{k}.src{n}.wav" for k in ("a_good", "d_good")
                                                     for n in (1, 2, 3))
