"""
GPU parity of mask-based sound source localisation (scripts/sptk/do_ssl.py, libs/ssl.py) against
recorded results of the unmodified reference (tests/golden/ref_ssl.npz,
tools/make_ssl_golden.py) and the float64 numpy model of tests/ssl_model.py (equal to the
reference on every recorded index and, for its SRP / MUSIC forms, to the device's
reformulations to 1e-9: tests/test_ssl_model.py).

Bounds.  Score spectra: max_a |device - model| <= 1e-4 x (max - min of the model's spectrum),
the operator bound of DESIGN.md section 2.  Indices: equal to the reference's wherever the
model's gap between the best and the second best direction exceeds 2 x 1e-4 of the spread; a
case below that gap is not compared but counted, and for the fixtures the count allowed is ZERO
(their smallest gap is 3.1e-4, tools/make_ssl_golden.py prints them all).  Every test prints
what it measures before it asserts; tests/PARITY_NOTES_SSL.md records the figures.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import np_oracle as o

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssl_model  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 1e-4
DOC_STFT = dict(frame_len=512, frame_hop=256, window="hann", center=True)
DOC_PAIRS = (list(range(8)), list(range(8, 16)))
DOC_PAIR_TEXT = "0,8;1,9;2,10;3,11;4,12;5,13;6,14;7,15"
BACKENDS = ("ml", "srp", "music")
ML_CLI = dict(compression=-1, eps=float(ssl_model.EPSILON))  # what get_doa passes (do_ssl.py:34)


# ---- shared inputs and model spectra (computed once) -----------------------------------------
@functools.lru_cache(maxsize=None)
def doc_inputs():
    g = load_golden("doc_wide_16ch.npz")
    x = np.ascontiguousarray(g["pcm"].T.astype(np.float32) / np.float32(32768.0))
    X = np.stack([o.forward_stft(c, transpose=True, **DOC_STFT) for c in x])
    sv = ssl_model.steer_vectors("circular", 360, 257, around=16, radius=0.05)
    return X, np.asarray(g["mask"]), sv


@functools.lru_cache(maxsize=None)
def doc_model(backend, masked):
    X, mask, sv = doc_inputs()
    return ssl_model.get_doa(backend, X, sv, mask if masked else None, DOC_PAIRS if backend == "srp" else None)


@functools.lru_cache(maxsize=None)
def doc_model_online(backend):
    X, _, sv = doc_inputs()
    return ssl_model.windowed(backend, X, sv, ssl_model.online_windows(X.shape[1], 25, 50),
                              srp_pair=DOC_PAIRS if backend == "srp" else None)


@functools.lru_cache(maxsize=None)
def scene_inputs(name):
    g = load_golden("ref_ssl.npz")
    x = np.ascontiguousarray(g[name + "_pcm"].astype(np.float32) / np.float32(32768.0))
    kw = ssl_model.scene_stft_kwargs(name)
    kw.pop("round_power_of_two")
    X = np.stack([o.forward_stft(c, transpose=True, **kw) for c in x])
    return x, X, ssl_model.scene_steer_vectors(name), ssl_model.scene_masks(name), ssl_model.scene_pairs(name)


def recorded_values(text):
    return [float(v) for v in str(text).rstrip("\n").split("\t")[1].split(" ")]


def spectrum(backend, X, sv, mask=None, pairs=None, windows=None, **kw):
    from setk_amd.libs.ssl import ssl_spectrum
    if backend == "ml" and not kw:
        kw = ML_CLI
    idx, score, status = ssl_spectrum(backend, X, sv, mask=mask, srp_pair=pairs if backend == "srp" else None,
                                      windows=windows, **kw)
    assert status == 0, status
    return idx, score


def check_spectrum(what, dev, model):
    spread = float(np.max(model) - np.min(model))
    d = float(np.max(np.abs(np.asarray(dev) - model))) / spread
    print(f"{what}: spectrum deviates by {d:.2e} of the spread")
    assert d <= BOUND, (what, d)
    return d


def check_index(what, dev_idx, want_idx, model_score, take_min, allow_close=False):
    """The gap rule.  Returns 1 when the case was too close to compare (fixtures: never)."""
    gap = ssl_model.gap(model_score, take_min)
    print(f"{what}: index {int(dev_idx)} (expected {int(want_idx)}), model gap {gap:.2e}")
    if gap <= 2 * BOUND:
        assert allow_close, (what, "closer than the gap rule allows for a fixture", gap)
        return 1
    assert int(dev_idx) == int(want_idx), (what, dev_idx, want_idx)
    return 0


# ---- 1. the doc recording: spectra against the model, indices against the reference ---------
@pytest.mark.parametrize("backend", BACKENDS)
def test_doc_recording_offline(backend):
    g = load_golden("ref_ssl.npz")
    X, mask, sv = doc_inputs()
    for masked in (False, True):
        tag = "mask" if masked else "nomask"
        _, model = doc_model(backend, masked)
        idx, score = spectrum(backend, X, sv, mask if masked else None, DOC_PAIRS)
        check_spectrum(f"doc {backend} {tag}", score[0], model)
        want = recorded_values(g[f"doc_{backend}_{tag}_index"])[0]
        assert check_index(f"doc {backend} {tag}", idx[0], want, model, backend == "music") == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_doc_recording_online_windows(backend):
    """--chunk-len 25 --look-back 50: six overlapping windows out of ONE pass of frame scores."""
    g = load_golden("ref_ssl.npz")
    X, _, sv = doc_inputs()
    wins = ssl_model.online_windows(X.shape[1], 25, 50)
    _, model = doc_model_online(backend)
    idx, score = spectrum(backend, X, sv, None, DOC_PAIRS, windows=wins)
    want = recorded_values(g[f"doc_{backend}_online_index"])
    assert len(want) == len(wins) == 6
    for w in range(6):
        check_spectrum(f"doc {backend} window {wins[w]}", score[w], model[w])
        assert check_index(f"doc {backend} window {wins[w]}", idx[w], want[w], model[w], backend == "music") == 0


# ---- 2. synthetic scenes through libs.ssl with the reference's signatures ------------------
@pytest.mark.parametrize("name", list(ssl_model.SCENES))
def test_scenes_match_reference(name):
    from setk_amd.libs import ssl
    g = load_golden("ref_ssl.npz")
    _, X, sv, masks, pairs = scene_inputs(name)
    for tag, m in (("nomask", None), ("mask", masks[0])):
        for backend in BACKENDS:
            _, model = ssl_model.get_doa(backend, X, sv, m, pairs if backend == "srp" else None)
            idx, score = spectrum(backend, X, sv, m, pairs)
            check_spectrum(f"{name} {backend} {tag}", score[0], model)
            assert check_index(f"{name} {backend} {tag}", idx[0], g[f"{name}_{backend}_{tag}"], model,
                               backend == "music") == 0
        # the reference's call surface returns the bare index
        assert ssl.ml_ssl(X, sv, mask=m, **ML_CLI) == g[f"{name}_ml_{tag}"]
        assert ssl.srp_ssl(X, sv, srp_pair=pairs, mask=m) == g[f"{name}_srp_{tag}"]
        assert ssl.music_ssl(X, sv, mask=m) == g[f"{name}_music_{tag}"]


def test_two_masks_and_compression_with_norm():
    from setk_amd.libs import ssl
    g = load_golden("ref_ssl.npz")
    _, X, sv, masks, _ = scene_inputs("c4")
    idx = ssl.ml_ssl(X, sv, mask=np.stack(masks), **ML_CLI)
    _, model = ssl_model.ml_ssl(X, sv, mask=np.stack(masks), **ML_CLI)
    assert idx.shape == (2,)
    for n in range(2):
        _, score = spectrum("ml", X, sv, masks[n])
        check_spectrum(f"c4 mask {n} of two", score[0], model[n])
        assert check_index(f"c4 mask {n} of two", idx[n], g["c4_ml_twomask"][n], model[n], False) == 0
    kw = dict(compression=0.5, norm=True, eps=float(g["c4_ml_compress_eps"]))
    _, model = ssl_model.ml_ssl(X, sv, mask=masks[0], **kw)
    i, score = spectrum("ml", X, sv, masks[0], **kw)
    check_spectrum("c4 compression 0.5, norm", score[0], model)
    assert check_index("c4 compression 0.5, norm", i[0], g["c4_ml_compress"], model, False) == 0
    assert ssl.ml_ssl(X, sv, mask=masks[0], **kw) == g["c4_ml_compress"]


# ---- 3. shapes where a kernel can go wrong ---------------------------------------------------
def random_case(seed, C, A, T, F):
    """A plane wave in the STFT domain plus noise (so that every backend has a peak), random
    steer vectors of non-unit modulus around it, a random mask."""
    rng = np.random.default_rng(seed)
    sv = rng.normal(size=(A, C, F)) + 1j * rng.normal(size=(A, C, F))
    src = rng.laplace(size=(T, F)) + 1j * rng.laplace(size=(T, F))
    X = sv[A // 2][:, None, :] * src[None] + 0.3 * (rng.normal(size=(C, T, F)) + 1j * rng.normal(size=(C, T, F)))
    mask = rng.uniform(0.05, 1.0, size=(T, F)).astype(np.float32)
    return X.astype(np.complex64), sv.astype(np.complex64), mask


# C = 2 .. 16; A = 5, 37, 360 (no multiple of the wave); T = 1, one more than a frame tile (33),
# 37; F = 129 and 257
@pytest.mark.parametrize("C,A,T,F", [(2, 5, 1, 129), (3, 37, 33, 129), (4, 360, 37, 257), (8, 37, 33, 257),
                                     (16, 5, 37, 129), (16, 360, 65, 257)])
def test_shapes_against_model(C, A, T, F):
    X, sv, mask = random_case(100 + C + A + T, C, A, T, F)
    pairs = (list(range(C - 1)), list(range(1, C)))
    close = 0
    for m in (None, mask):
        for backend in BACKENDS:
            # (MUSIC with fewer frames than channels: a zero eigenvalue of multiplicity C - T, but the
            #  principal one is simple -- still defined for T = 1, v = x / |x|)
            widx, model = ssl_model.get_doa(backend, X, sv, m, pairs if backend == "srp" else None)
            idx, score = spectrum(backend, X, sv, m, pairs)
            what = f"C={C} A={A} T={T} F={F} {backend} {'mask' if m is not None else 'nomask'}"
            check_spectrum(what, score[0], model)
            close += check_index(what, idx[0], widx, model, backend == "music", allow_close=True)
    print(f"cases closer than the gap rule (not compared): {close}")


def test_srp_zero_sample():
    """np.angle(0) = 0: a zero observation (one microphone, and a whole cell) and a zero steer
    vector entry count as phase 0."""
    _, X, sv, masks, pairs = scene_inputs("c4")
    X, sv = X.copy(), sv.astype(np.complex64).copy()
    X[1, 3, 10] = 0
    X[:, 5, 20] = 0
    sv[7, 2, 30] = 0
    for wins in (None, [(0, 17), (3, 7)]):
        if wins is None:
            model = ssl_model.srp_ssl(X, sv, pairs, masks[0])[1][None]
        else:
            model = ssl_model.windowed("srp", X, sv, wins, mask=masks[0], srp_pair=pairs)[1]
        _, score = spectrum("srp", X, sv, masks[0], pairs, windows=wins)
        for w in range(len(model)):
            check_spectrum(f"srp with zero samples, windows {wins} [{w}]", score[w], model[w])


@pytest.mark.parametrize("backend", BACKENDS)
def test_window_table_against_model(backend):
    """Overlapping, single-frame, tile-straddling and full-length windows, window by window, with a mask."""
    _, X, sv, masks, pairs = scene_inputs("odd")  # T = 37, F = 129, C = 3
    T = X.shape[1]
    wins = [(0, T), (0, 1), (36, 37), (5, 20), (10, 36), (31, 34), (0, 32), (32, 37)]
    widx, model = ssl_model.windowed(backend, X, sv, wins, mask=masks[1], srp_pair=pairs if backend == "srp" else None)
    idx, score = spectrum(backend, X, sv, masks[1], pairs, windows=wins)
    close = 0
    for w, win in enumerate(wins):
        check_spectrum(f"odd {backend} window {win}", score[w], model[w])
        close += check_index(f"odd {backend} window {win}", idx[w], widx[w], model[w], backend == "music",
                             allow_close=True)
    print(f"windows closer than the gap rule (not compared): {close}")
    # the model's gaps decide this, not the device: window (0, 1) is the one window of this table
    # under 2e-4, for every backend -- frame 0 of a centred transform is its own mirror image, its
    # spectrum real, and two directions tie exactly in the model (tests/PARITY_NOTES_SSL.md)
    assert close <= 1, (backend, close)


def test_lowest_index_wins_a_tie():
    """Two identical steer vectors: np.argmax / np.argmin take the first."""
    _, X, sv, _, pairs = scene_inputs("c2")
    for backend in BACKENDS:
        best = int(ssl_model.get_doa(backend, X, sv, None, pairs if backend == "srp" else None)[0])
        dup = np.concatenate([sv[best:best + 1], sv, sv[best:best + 1]]).astype(np.complex64)
        idx, score = spectrum(backend, X, dup, None, pairs)
        assert score[0][0] == score[0][best + 1] == score[0][-1]
        assert idx[0] == 0, (backend, idx)


# ---- 4. the batched entry point ----------------------------------------------------------------
def test_batch_is_deterministic_and_equals_single():
    """Mixed channel counts and lengths in one run(), Pcm16Frames and float input, with and
    without masks: bit-identical scores on a second run, and the stand-alone operator's indices
    and (to the bound) scores.  The batch transforms on the device, the stand-alone call here
    gets the oracle's spectrogram."""
    from setk_amd.engine import BatchLocalizer, Pcm16Frames
    g = load_golden("ref_ssl.npz")
    names = ["c2", "c4", "c8", "c4"]
    ins = [scene_inputs(n) for n in names]
    utts = [ins[0][0], Pcm16Frames(g["c4_pcm"].T), ins[2][0], ins[3][0][:, :256 * 20]]
    masks = [None, ins[1][3][0], ins[2][3][1], None]
    sets = {2: ins[0][2], 4: ins[1][2], 8: ins[2][2]}
    for backend in BACKENDS:
        pair_of = {n: ins[k][4] for k, n in enumerate(names)}
        for online in (False, True):
            # one pair table per engine: the c4 scenes' neighbours fit every array here but c2
            sel = [k for k, n in enumerate(names) if backend != "srp" or n == "c4"]
            eng = BatchLocalizer(backend=backend, steer_vector=sets, srp_pair=pair_of["c4"],
                                 chunk_len=8 if online else -1, look_back=12)
            out = eng.run([utts[k] for k in sel], [masks[k] for k in sel])
            scores = [s.copy() for s in eng.scores]
            out2 = eng.run([utts[k] for k in sel], [masks[k] for k in sel])
            for a, b, sa, sb in zip(out, out2, scores, eng.scores):
                assert np.array_equal(a, b) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
            assert all(st == 0 for st in eng.status)
            for j, k in enumerate(sel):
                # (the shortened utterance has its own reflected last frames)
                X = ins[k][1] if k != 3 else np.stack([o.forward_stft(c, transpose=True, **DOC_STFT) for c in utts[3]])
                T = X.shape[1]
                m = masks[k]
                wins = eng.windows(T)
                assert out[j].shape == (len(wins),) and (len(wins) > 1) == online
                idx, score = spectrum(backend, X, sets[X.shape[0]], m, pair_of["c4"], windows=wins)
                for w in range(len(wins)):
                    check_spectrum(f"batch {backend} {names[k]} window {wins[w]} against the operator",
                                   eng.scores[j][w], score[w])
                    check_index(f"batch {backend} {names[k]} window {wins[w]}", out[j][w], idx[w], score[w],
                                backend == "music", allow_close=True)
            eng.close()


def test_batch_other_transform_size_through_the_operators():
    """n_fft != 512: BatchLocalizer runs setk_stft -> setk_ssl_scores per utterance on host arrays.
    2 channels, 4000 samples, frame 256 / hop 128, online windows, float input with a mask and
    16-bit frames without: against the stand-alone operator on the oracle's spectrogram, by the
    checks of the batched path."""
    from setk_amd.engine import BatchLocalizer, Pcm16Frames
    kw = dict(DOC_STFT, frame_len=256, frame_hop=128)
    pcm = np.ascontiguousarray(load_golden("ref_ssl.npz")["c2_pcm"][:, :4000])
    x = pcm.astype(np.float32) / np.float32(32768.0)
    X = np.stack([o.forward_stft(c, transpose=True, **kw) for c in x])
    C, T, F = X.shape
    assert (C, T, F) == (2, 32, 129)
    rng = np.random.default_rng(5)
    sv = np.exp(1j * rng.uniform(-np.pi, np.pi, size=(24, C, F)))
    mask = rng.uniform(0.1, 1.0, size=(T, F)).astype(np.float32)
    eng = BatchLocalizer(backend="ml", steer_vector=sv, chunk_len=8, look_back=12, **kw)
    out = eng.run([x, Pcm16Frames(np.ascontiguousarray(pcm.T))], [mask, None])
    assert eng.status == [0, 0]
    wins = eng.windows(T)
    assert len(wins) == 4
    for j, m in enumerate((mask, None)):
        idx, score = spectrum("ml", X, sv, m, None, windows=wins)
        assert out[j].shape == (len(wins),) and out[j].dtype == np.int64
        for w in range(len(wins)):
            check_spectrum(f"operators path, utterance {j}, window {wins[w]}", eng.scores[j][w], score[w])
            check_index(f"operators path, utterance {j}, window {wins[w]}", out[j][w], idx[w], score[w], False,
                        allow_close=True)
    eng.close()


def test_device_tensors_through_the_c_abi():
    """setk_ssl_scores and setk_ssl_batch on torch device tensors: same bits as from host arrays."""
    import torch
    from setk_amd import _ffi
    ctx = _ffi.default_context()
    x, X, sv, masks, pairs = scene_inputs("c8")
    C, T, F = X.shape
    A = sv.shape[0]
    sv64 = np.ascontiguousarray(sv, dtype=np.complex64)
    wins = [(0, T), (4, 19)]
    for backend in BACKENDS:
        opts = _ffi.ssl_opts(backend, srp_pair=pairs, **ML_CLI)
        score = np.empty((2, A))
        index = np.empty(2, dtype=np.int32)
        ctx.ssl_scores(opts, X, masks[0], sv64, A, C, T, F, wins, score, index)
        dX, dm, dsv = torch.from_numpy(X).cuda(), torch.from_numpy(masks[0]).cuda(), torch.from_numpy(sv64).cuda()
        dscore = torch.zeros((2, A), dtype=torch.float64, device="cuda")
        dindex = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        dst = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        ctx.ssl_scores(opts, dX, dm, dsv, A, C, T, F, wins, dscore, dindex, status=dst.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(dscore.cpu().numpy().view(np.uint64), score.view(np.uint64)), backend
        assert np.array_equal(dindex.cpu().numpy(), index) and int(dst.cpu()[0]) == 0
        # the batch: audio in
        ctx.stft_plan(512, 256, 512, True, None)
        da = torch.from_numpy(x).cuda()
        bscore = torch.zeros((2, A), dtype=torch.float64, device="cuda")
        bindex = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        ctx.ssl_batch(opts, C, [da.data_ptr()], [x.shape[1]], [dm.data_ptr()], dsv, A, [wins], bindex.data_ptr(),
                      score=bscore.data_ptr())
        torch.cuda.synchronize()
        for w in range(2):
            check_spectrum(f"ssl_batch {backend} on device tensors, window {wins[w]}", bscore.cpu().numpy()[w], score[w])
            check_index(f"ssl_batch {backend} window {wins[w]}", bindex.cpu().numpy()[w], index[w], score[w],
                        backend == "music", allow_close=True)


def test_sixteen_channels_through_the_batch():
    """More than 8 channels: the stand-alone transform per utterance in front of the same scores
    (the doc recording, Pcm16Frames)."""
    from setk_amd.engine import BatchLocalizer, Pcm16Frames
    g = load_golden("ref_ssl.npz")
    X, mask, sv = doc_inputs()
    pcm = load_golden("doc_wide_16ch.npz")["pcm"]
    eng = BatchLocalizer(backend="ml", steer_vector=sv)
    out = eng.run([Pcm16Frames(pcm)], [mask])
    _, model = doc_model("ml", True)
    check_spectrum("doc ml masked through BatchLocalizer", eng.scores[0][0], model)
    assert check_index("doc ml masked through BatchLocalizer", out[0][0],
                       recorded_values(g["doc_ml_mask_index"])[0], model, False) == 0
    eng.close()


def test_profiled_stages_are_reported():
    from setk_amd import _ffi
    from setk_amd.engine import BatchLocalizer
    x, _, sv, _, _ = scene_inputs("c4")
    eng = BatchLocalizer(backend="ml", steer_vector=sv)
    ctx = eng.ctx
    ctx.set_profiling(True)
    try:
        eng.run([x])
        ms = ctx.last_stage_ms()
    finally:
        ctx.set_profiling(False)
        eng.close()
    print(f"stages (ms): STFT {ms[0]:.3f}, frame scores {ms[1]:.3f}, reduce {ms[2]:.3f}")
    assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0


# ---- 5. limits ---------------------------------------------------------------------------------
def test_unsupported_and_invalid_requests():
    from setk_amd import _ffi
    from setk_amd.engine import BatchLocalizer
    ctx = _ffi.default_context()
    C, T, F, A = 17, 4, 9, 3
    X = np.ones((C, T, F), dtype=np.complex64)
    sv = np.ones((A, C, F), dtype=np.complex64)
    score, index = np.empty((1, A)), np.empty(1, dtype=np.int32)
    with pytest.raises(_ffi.SetkUnsupported, match="<= 16"):
        ctx.ssl_scores(_ffi.ssl_opts("ml"), X, None, sv, A, C, T, F, None, score, index)
    with pytest.raises(_ffi.SetkUnsupported, match="<= 16"):
        BatchLocalizer(backend="ml", steer_vector=np.ones((A, C, 257), dtype=np.complex64)).run(
            [np.zeros((C, 4096), dtype=np.float32)])
    X, sv = X[:4].copy(), sv[:, :4].copy()
    with pytest.raises(ValueError, match="window"):
        ctx.ssl_scores(_ffi.ssl_opts("ml"), X, None, sv, A, 4, T, F, [(2, 2)], score, index)
    with pytest.raises(ValueError, match="window"):
        ctx.ssl_scores(_ffi.ssl_opts("ml"), X, None, sv, A, 4, T, F, [(0, T + 1)], score, index)
    with pytest.raises(ValueError, match="pair"):
        ctx.ssl_scores(_ffi.ssl_opts("srp", srp_pair=([0], [4])), X, None, sv, A, 4, T, F, None, score, index)


# ---- 6. the command lines ----------------------------------------------------------------------
def test_command_lines_on_doc_recording(tmp_path):
    """compute_steer_vector.py writes the steer vectors, do_ssl.py the reference's text lines byte
    for byte: offline with and without the mask (stored F x T, which the command line
    transposes), as degrees and as indices, and online."""
    import scipy.io.wavfile
    import torch  # noqa: F401  (keeps this process on torch's runtime: the in-process calls below
    #                            would otherwise switch the library's loader to torch-free mode)
    from setk_amd.sptk import compute_steer_vector, do_ssl
    g = load_golden("ref_ssl.npz")
    doc = load_golden("doc_wide_16ch.npz")
    td = str(tmp_path)
    scipy.io.wavfile.write(f"{td}/egs.wav", 16000, doc["pcm"])
    with open(f"{td}/wav.scp", "w") as fd:
        fd.write(f"egs {td}/egs.wav\n")
    np.save(f"{td}/mask.npy", np.ascontiguousarray(doc["mask"].T))  # F x T
    with open(f"{td}/mask.scp", "w") as fd:
        fd.write(f"egs {td}/mask.npy\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/sptk/compute_steer_vector.py"),
                        "--num-doas", "360", "--num-bins", "257", "--sr", "16000", "--geometry", "circular",
                        "--circular-radius", "0.05", "--circular-around", "16", f"{td}/sv.npy"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.load(f"{td}/sv.npy"), doc_inputs()[2])
    small = f"{td}/small.npy"
    compute_steer_vector.main([small, "--num-doas", "7", "--num-bins", "33", "--geometry", "circular"])
    assert np.max(np.abs(np.load(small) - g["sv_circular"])) <= 1e-12

    def run(backend, *extra, script=False):
        argv = ["--frame-len", "512", "--frame-hop", "256", "--backend", backend, "--doa-range", "0,360"]
        if backend == "srp":
            argv += ["--srp-pair", DOC_PAIR_TEXT]
        argv += list(extra) + [f"{td}/wav.scp", f"{td}/sv.npy", f"{td}/doa.scp"]
        if script:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/sptk/do_ssl.py")] + argv,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
        else:
            do_ssl.main(argv)
        return open(f"{td}/doa.scp").read()

    assert run("ml", "--output", "degree", script=True) == str(g["doc_ml_nomask_degree"])
    for backend in BACKENDS:
        got = run(backend, "--output", "index", "--mask-scp", f"{td}/mask.scp")
        print(backend, "masked, index:", repr(got))
        assert got == str(g[f"doc_{backend}_mask_index"])
        got = run(backend, "--output", "degree", "--chunk-len", "25", "--look-back", "50")
        print(backend, "online, degree:", repr(got))
        assert got == str(g[f"doc_{backend}_online_degree"])
    got = run("music", "--output", "radian")
    assert got == "egs\t{:.4f}\n".format(np.linspace(0, 2 * np.pi, 361)[60])
