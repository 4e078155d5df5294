"""
Sound source localisation without a GPU: the numpy model (tests/ssl_model.py) against recorded
results of the unmodified reference (tests/golden/ref_ssl.npz, tools/make_ssl_golden.py); the
two reformulations the device relies on (factorised SRP-PHAT, MUSIC on the principal
eigenvector) restated in numpy against the model's own forms; compute_steer_vector.py against
the reference's stored arrays; the command-line surface of do_ssl.py.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import np_oracle as o

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssl_model  # noqa: E402

DOC_STFT = dict(frame_len=512, frame_hop=256, window="hann", center=True)
DOC_PAIRS = (list(range(8)), list(range(8, 16)))
BACKENDS = ("ml", "srp", "music")


@functools.lru_cache(maxsize=None)
def doc_inputs():
    """The doc recording: spectrogram 16 x 126 x 257, its CGMM mask, the 360 steer vectors of
    doc/ssl/README.md (circular, 16 around, 0.05 m)."""
    g = load_golden("doc_wide_16ch.npz")
    x = g["pcm"].T.astype(np.float32) / np.float32(32768.0)
    X = np.stack([o.forward_stft(c, transpose=True, **DOC_STFT) for c in x])
    sv = ssl_model.steer_vectors("circular", 360, 257, around=16, radius=0.05)
    return X, np.asarray(g["mask"]), sv


@functools.lru_cache(maxsize=None)
def scene_inputs(name):
    g = load_golden("ref_ssl.npz")
    x = g[name + "_pcm"].astype(np.float32) / np.float32(32768.0)
    kw = ssl_model.scene_stft_kwargs(name)
    kw.pop("round_power_of_two")
    X = np.stack([o.forward_stft(c, transpose=True, **kw) for c in x])
    return X, ssl_model.scene_steer_vectors(name), ssl_model.scene_masks(name), ssl_model.scene_pairs(name)


def recorded_values(text):
    """ "egs\\t61.0000 60.0000\\n" -> [61.0, 60.0] """
    key, vals = str(text).rstrip("\n").split("\t")
    assert key == "egs"
    return [float(v) for v in vals.split(" ")]


# ---- 1. the model's index equals every recorded index --------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_model_matches_reference_on_doc_recording(backend):
    g = load_golden("ref_ssl.npz")
    X, mask, sv = doc_inputs()
    pairs = DOC_PAIRS if backend == "srp" else None
    for tag, m in (("nomask", None), ("mask", mask)):
        idx, score = ssl_model.get_doa(backend, X, sv, m, pairs)
        gap = ssl_model.gap(score, backend == "music")
        print(f"doc {backend} {tag}: index {idx}, gap {gap:.2e}")
        # --doa-range 0,360 with 360 directions: the angle in degrees IS the index
        assert recorded_values(g[f"doc_{backend}_{tag}_index"]) == [float(idx)]
        assert recorded_values(g[f"doc_{backend}_{tag}_degree"]) == [float(idx)]
    wins = ssl_model.online_windows(X.shape[1], 25, 50)
    assert len(wins) == 6
    idx, scores = ssl_model.windowed(backend, X, sv, wins, srp_pair=pairs)
    print(f"doc {backend} online: {idx}, smallest gap "
          f"{min(ssl_model.gap(s, backend == 'music') for s in scores):.2e}")
    assert recorded_values(g[f"doc_{backend}_online_index"]) == [float(i) for i in idx]
    assert recorded_values(g[f"doc_{backend}_online_degree"]) == [float(i) for i in idx]


def test_doc_recording_is_where_the_reference_found_it():
    g = load_golden("ref_ssl.npz")
    assert [recorded_values(g[f"doc_{b}_nomask_index"]) for b in BACKENDS] == [[59.0], [59.0], [60.0]]
    assert recorded_values(g["doc_ml_online_index"]) == [61.0, 60.0, 60.0, 59.0, 58.0, 57.0]
    assert recorded_values(g["doc_srp_online_index"]) == [60.0, 60.0, 60.0, 59.0, 58.0, 57.0]
    assert recorded_values(g["doc_music_online_index"]) == [61.0, 60.0, 60.0, 60.0, 58.0, 57.0]


@pytest.mark.parametrize("name", list(ssl_model.SCENES))
def test_model_matches_reference_on_scenes(name):
    g = load_golden("ref_ssl.npz")
    X, sv, masks, pairs = scene_inputs(name)
    assert X.shape[0] == ssl_model.SCENES[name][2] and X.shape[1] == ssl_model.SCENES[name][4]
    for tag, m in (("nomask", None), ("mask", masks[0])):
        for backend in BACKENDS:
            idx, score = ssl_model.get_doa(backend, X, sv, m, pairs if backend == "srp" else None)
            print(f"{name} {backend} {tag}: index {idx}, gap {ssl_model.gap(score, backend == 'music'):.2e}")
            assert int(idx) == int(g[f"{name}_{backend}_{tag}"]), (name, backend, tag)
    if name == "c4":
        idx, score = ssl_model.ml_ssl(X, sv, mask=np.stack(masks), compression=-1, eps=ssl_model.EPSILON)
        assert score.shape == (2, sv.shape[0]) and np.array_equal(idx, g["c4_ml_twomask"])
        idx, score = ssl_model.ml_ssl(X, sv, compression=0.5, norm=True, eps=float(g["c4_ml_compress_eps"]),
                                      mask=masks[0])
        assert int(idx) == int(g["c4_ml_compress"]) and not np.isnan(score).any()


# ---- 2. the device's reformulations, in numpy, against the model's own forms ------------------
def factorised_srp(X, sv, pairs, mask):
    """u_p = phasor(x_l) conj(phasor(x_r)), d likewise for sv, folded over the frames first:
    score[a] = (1 / P) sum_{p,f} Re(conj(d[a,p,f]) U[p,f]), U = sum_t mask u_p.  No angle, no cos."""
    def phasor(z):
        n = np.abs(z)
        return np.where(n > 0, z / np.where(n > 0, n, 1), 1.0)
    left, right = pairs
    mask = np.ones(X.shape[1:]) if mask is None else mask
    px, ps = phasor(X.astype(np.complex128)), phasor(sv.astype(np.complex128))
    U = np.sum(px[left] * px[right].conj() * mask[None], axis=1)             # P x F
    d = ps[:, left] * ps[:, right].conj()                                     # A x P x F
    return np.sum(np.real(d.conj() * U[None]), axis=(1, 2)) / len(left)


def pevd_music(X, sv, mask):
    """E_n E_n^H = I - v v^H: score[a] = sum_f | ||sv||^2 - |v^H sv|^2 |, v the principal
    eigenvector of the covariance with the SQUARED mask (any positive per-bin scale)."""
    mask = np.ones(X.shape[1:]) if mask is None else mask.astype(np.float64)
    x = X.astype(np.complex128).transpose(2, 0, 1)                            # F x M x T
    w = (mask**2).T[:, None, :]                                               # F x 1 x T
    R = np.matmul(x * w, x.conj().transpose(0, 2, 1)) / np.maximum(np.sum(w, axis=2), 1e-6)[..., None]
    v = np.linalg.eigh(R)[1][..., -1]                                         # F x M
    s = sv.astype(np.complex128).transpose(2, 0, 1)                           # F x A x M
    return np.sum(np.abs(np.sum(np.abs(s)**2, axis=2) - np.abs(np.einsum("fm,fam->fa", v.conj(), s))**2), axis=0)


@pytest.mark.parametrize("name", ["doc"] + list(ssl_model.SCENES))
def test_reformulations_equal_the_reference_forms(name):
    if name == "doc":
        X, mask, sv = doc_inputs()
        pairs = DOC_PAIRS
    else:
        X, sv, masks, pairs = scene_inputs(name)
        mask = masks[0]
    for tag, m in (("nomask", None), ("mask", mask)):
        _, ref = ssl_model.srp_ssl(X, sv, pairs, m)
        dev = np.max(np.abs(factorised_srp(X, sv, pairs, m) - ref)) / (ref.max() - ref.min())
        print(f"{name} {tag}: factorised SRP against the cosine form {dev:.2e} of the spread")
        assert dev <= 1e-9
        _, ref = ssl_model.music_ssl(X, sv, m)
        dev = np.max(np.abs(pevd_music(X, sv, m) - ref)) / (ref.max() - ref.min())
        print(f"{name} {tag}: MUSIC on the principal eigenvector against the noise subspace {dev:.2e}")
        assert dev <= 1e-9


def test_srp_zero_sample_counts_as_phase_zero():
    """np.angle(0) = 0: a zero sample contributes the other microphone's phase alone."""
    X, sv, masks, pairs = scene_inputs("c4")
    X = X.copy()
    X[1, 3, 10] = 0
    X[:, 5, 20] = 0
    _, ref = ssl_model.srp_ssl(X, sv, pairs, None)
    dev = np.max(np.abs(factorised_srp(X, sv, pairs, None) - ref)) / (ref.max() - ref.min())
    assert dev <= 1e-9


# ---- 3. compute_steer_vector.py ---------------------------------------------------------------
@pytest.mark.parametrize("name,argv", [
    ("sv_linear", ["--geometry", "linear", "--linear-topo", "0,0.05,0.1,0.15"]),
    ("sv_circular", ["--geometry", "circular"]),
    ("sv_circular_center", ["--geometry", "circular", "--circular-center", "true"]),
    ("sv_circular_normalize", ["--geometry", "circular", "--normalize", "true"]),
])
def test_compute_steer_vector_matches_reference(name, argv, tmp_path):
    from setk_amd.sptk import compute_steer_vector as csv
    ref = load_golden("ref_ssl.npz")[name]
    out = str(tmp_path / "sv.npy")
    csv.main([out, "--num-doas", "7", "--num-bins", "33"] + argv)
    sv = np.load(out)
    assert sv.shape == ref.shape and sv.dtype == ref.dtype
    dev = np.max(np.abs(sv - ref))
    print(f"{name}: {dev:.2e}")
    assert dev <= 1e-12


def test_compute_steer_vector_defaults_equal_the_references():
    from setk_amd.sptk import compute_steer_vector as csv
    a = csv.build_parser().parse_args(["sv.npy"])
    assert (a.num_doas, a.num_bins, a.sr, a.speed, a.linear_topo, a.circular_around, a.circular_radius,
            bool(a.circular_center), a.geometry, bool(a.normalize)) == \
        (181, 257, 16000, 343, (), 6, 0.05, False, "linear", False)


# ---- 4. do_ssl.py's surface ---------------------------------------------------------------------
@pytest.mark.parametrize("script", ["do_ssl.py", "compute_steer_vector.py"])
def test_cli_help_exits_zero(script):
    path = os.path.join(ROOT, "scripts", "sptk", script)
    assert os.access(path, os.X_OK)
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    opts = ("wav_scp", "steer_vector", "doa_scp", "--backend", "--srp-pair", "--doa-range", "--mask-scp",
            "--output", "--mask-eps", "--chunk-len", "--look-back", "--frame-len") if script == "do_ssl.py" \
        else ("steer_vector", "--num-doas", "--num-bins", "--linear-topo", "--circular-around", "--geometry")
    for opt in opts:
        assert opt in r.stdout, opt


def test_do_ssl_defaults_equal_the_references():
    """do_ssl.py:124-170."""
    from setk_amd.libs.opts import StftParser
    from setk_amd.sptk import do_ssl
    a = do_ssl.build_parser().parse_args(["wav.scp", "sv.npy", "doa.scp"])
    assert (a.wav_scp, a.steer_vector, a.doa_scp) == ("wav.scp", "sv.npy", "doa.scp")
    assert (a.backend, a.srp_pair, a.doa_range, a.mask_scp, a.output, a.mask_eps, a.chunk_len, a.look_back) == \
        ("ml", "", "0,360", "", "degree", -1, -1, 125)
    for k, v in vars(StftParser.parser.parse_args([])).items():
        assert getattr(a, k) == v, k
    with pytest.raises(SystemExit):
        do_ssl.build_parser().parse_args(["a", "b", "c", "--backend", "gcc"])
    assert do_ssl.parse_srp_pair("0,8;1,9") == ([0, 1], [8, 9])


def test_mask_rules_of_the_command_line():
    """Winner-take-all over several readers (add_wta), the first mask, transposed to T x F."""
    from setk_amd.sptk import do_ssl
    a = np.array([[0.9, 0.2], [0.4, 0.5]])
    b = np.array([[0.1, 0.8], [0.4, 0.3]])
    wa, wb = do_ssl.add_wta([a, b], eps=1e-4)
    assert np.array_equal(wa, [[0.9, 1e-4], [0.4, 0.5]]) and np.array_equal(wb, [[1e-4, 0.8], [0.4, 1e-4]])
    ft = np.arange(6.0).reshape(3, 2)  # F x T with F = 3
    assert do_ssl.load_mask([{"k": ft}], "k", -1, 3).shape == (2, 3)
    assert do_ssl.load_mask([{"k": ft.T}], "k", -1, 3).shape == (2, 3)
    assert np.array_equal(do_ssl.load_mask([{"k": a}, {"k": b}], "k", 1e-4, 2), wa)
    assert np.array_equal(do_ssl.load_mask([{"k": a}, {"k": b}], "k", -1, 2), a)
    assert do_ssl.load_mask(None, "k", -1, 2) is None


def test_argument_checks_need_no_device():
    from setk_amd._ffi import SetkUnsupported
    from setk_amd.libs import ssl
    X = np.zeros((2, 5, 9), dtype=np.complex64)
    sv = np.ones((3, 2, 9), dtype=np.complex64)
    with pytest.raises(ValueError, match="srp_pair cannot be None"):
        ssl.srp_ssl(X, sv)
    with pytest.raises(ValueError):
        ssl.ml_ssl(X, np.ones((3, 4, 9), dtype=np.complex64))
    with pytest.raises(ValueError):
        ssl.music_ssl(X, sv, mask=np.ones((4, 9)))
    with pytest.raises(SetkUnsupported, match="<= 16"):
        ssl.ml_ssl(np.zeros((17, 5, 9), dtype=np.complex64), np.ones((3, 17, 9), dtype=np.complex64))


def test_product_modules_do_not_import_test_infrastructure():
    for rel in ("setk_amd/sptk/do_ssl.py", "setk_amd/sptk/compute_steer_vector.py", "setk_amd/libs/ssl.py",
                "scripts/sptk/do_ssl.py", "scripts/sptk/compute_steer_vector.py"):
        src = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(from|import)\s+(oracle|tests|ssl_model|conftest)\b", src, re.M), rel
