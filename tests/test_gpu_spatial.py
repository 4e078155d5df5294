"""
The geometry-driven spatial features on the MI355X (setk_amd/csrc/spatial.hip, libs/spatial.py,
engine/spatial.py and the three command lines) against the reference's recorded results in
tests/golden/ref_spatial.npz (tools/make_spatial_golden.py; the expected maps are stored as
float32, 6e-8 below the bar).  Operators: BASELINE's bar of 1e-4 absolute, raw IPD on the circle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spatial_model as sm  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-4
STFT = dict(frame_len=512, frame_hop=256, window="hann", center=True, round_power_of_two=True)


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_spatial.npz")


def maxdiff(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


# ---------------------------------------------------------------- operator parity
@pytest.mark.parametrize("name", sorted(sm.LINEAR))
def test_srp_phat_linear(gold, name):
    from setk_amd.libs.spatial import srp_phat_linear
    C, T, F, D, topo, samp_doa = sm.LINEAR[name]
    S = sm.spec_of(gold[name.split("_")[0] + "_S"])
    got = srp_phat_linear(S, list(topo), sample_frequency=16000, num_doa=D, num_bins=F, samp_doa=samp_doa)
    assert got.shape == (T, D) and got.dtype == np.float32
    dev = maxdiff(got, gold[name + "_srp"])
    print(f"{name}: max |device - reference| = {dev:.3e}")
    assert dev <= BAR


def test_gcc_phat_diag_mean_is_the_circular_spectrum(gold):
    from setk_amd.libs import spatial as sp
    C, T, F, D, pairs, n, d = sm.CIRCULAR["circ6"]
    S = sm.spec_of(gold["circ6_S"])
    # as compute_circular_srp.py does it, pair by pair ...
    one = np.average(np.stack([sp.gcc_phat_diag(S[i], S[j], min(i, j) * np.pi * 2 / n, d, num_bins=F, sr=16000,
                                                num_doas=D) for i, j in pairs]), axis=0)
    # ... and in one call, as the engine does
    p, table, w = sp.circular_srp_tables(pairs, n, d, num_bins=F, num_doas=D)
    got = sp.srp_feats(S, p, table, w, D)
    print(f"circ6: per pair {maxdiff(one, gold['circ6_srp']):.3e}, one call {maxdiff(got, gold['circ6_srp']):.3e}")
    assert one.shape == got.shape == (T, D)
    assert maxdiff(one, gold["circ6_srp"]) <= BAR and maxdiff(got, gold["circ6_srp"]) <= BAR


def test_gcc_phat_linear_is_the_two_microphone_spectrum(gold):
    from setk_amd.libs.spatial import gcc_phat_linear
    S = sm.spec_of(gold["lin2_S"])
    got = gcc_phat_linear(S[0], S[1], 0.1, num_doa=7, num_bins=33)
    assert got.shape == (1, 7) and maxdiff(got, gold["lin2_srp"]) <= BAR


@pytest.mark.parametrize("key,kw", [("ipd_raw", {}), ("ipd_cos", dict(cos=True)),
                                    ("ipd_cossin", dict(cos=True, sin=True))])
def test_ipd(gold, key, kw):
    from setk_amd.libs.spatial import ipd, ipd_feats
    S = sm.spec_of(gold["lin4_S"])
    one = np.hstack([ipd(S[l], S[r], **kw) for l, r in sm.IPD_PAIRS])
    got = ipd_feats(S, sm.IPD_PAIRS, **kw)
    assert np.array_equal(one, got) and got.shape == gold[key].shape and got.dtype == np.float32
    if key == "ipd_raw":
        dev = float(sm.circle_distance(got, gold[key]).max())
        assert got.min() >= -np.float32(np.pi) and got.max() < np.float32(np.pi)
    else:
        dev = maxdiff(got, gold[key])
    print(f"{key}: max |device - reference| = {dev:.3e}")
    assert dev <= BAR


@pytest.mark.parametrize("key", sorted(sm.DF_CASES))
def test_geometry_df(gold, key):
    from setk_amd.libs.spatial import geometry_df
    idx, pairs = sm.DF_CASES[key]
    S = sm.spec_of(gold["lin4_S"])
    if pairs is None:
        pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    got = geometry_df(S, gold["df_sv"], idx, pairs)
    dev = maxdiff(got, gold[key])
    print(f"{key}: max |device - reference| = {dev:.3e}")
    assert got.shape == gold[key].shape and dev <= BAR


def test_all_zero_spectrogram(gold):
    from setk_amd.libs.spatial import srp_phat_linear
    got = srp_phat_linear(np.zeros((4, 37, 33), np.complex64), list(sm.LINEAR["lin4"][4]), num_doa=181, num_bins=33)
    assert np.isfinite(got).all() and maxdiff(got, gold["zero_srp"]) <= BAR


def test_two_runs_give_the_same_bytes(gold):
    from setk_amd.libs.spatial import srp_phat_linear
    C, T, F, D, topo, _ = sm.LINEAR["lin8"]
    S = sm.spec_of(gold["lin8_S"])
    a = srp_phat_linear(S, list(topo), num_doa=D, num_bins=F)
    b = srp_phat_linear(S, list(topo), num_doa=D, num_bins=F)
    assert a.tobytes() == b.tobytes()


def test_limits_are_refused():
    from setk_amd import _ffi
    from setk_amd.libs import spatial as sp
    with pytest.raises(_ffi.SetkUnsupported, match="2 <= num_channels <= 16"):
        sp.ipd_feats(np.ones((17, 2, 4), np.complex64), [(0, 1)])
    with pytest.raises(_ffi.SetkUnsupported, match="num_bins >= 2"):
        sp.ipd_feats(np.ones((2, 2, 1), np.complex64), [(0, 1)])
    with pytest.raises(_ffi.SetkUnsupported, match="MSC is not ported"):
        sp.msc(np.ones((2, 4, 4), np.complex64))
    with pytest.raises(ValueError, match="3 microphones available, while get 2-channel STFT"):
        sp.srp_phat_linear(np.ones((2, 4, 4), np.complex64), [0, 0.1, 0.2])


# ---------------------------------------------------------------- the batch entry
def test_batch_entry_equals_the_operator_bit_for_bit(gold):
    import torch
    from setk_amd import _ffi
    from setk_amd.libs import spatial as sp
    ctx = _ffi.default_context()
    rng = np.random.default_rng(5)
    F, D = 33, 181
    specs = [sm.spec_of(rng.integers(-7, 8, size=(4, T, F, 2))) for T in (1, 37, 64)]
    pairs, table, weight = sp.linear_srp_tables(sm.LINEAR["lin4"][4], num_bins=F, num_doa=D)
    sv = np.ascontiguousarray(gold["df_sv"])
    idx = [[2, 0, 5], [1, 1, 6], [0, 3, 4]]
    cases = [
        (_ffi.spatial_opts("srp", pairs, table=table, num_doas=D, pair_weight=weight),
         lambda k: sp.srp_feats(specs[k], pairs, table, weight, D)),
        (_ffi.spatial_opts("cos_sin_ipd", sm.IPD_PAIRS), lambda k: sp.ipd_feats(specs[k], sm.IPD_PAIRS, True, True)),
        (_ffi.spatial_opts("ipd", sm.IPD_PAIRS), lambda k: sp.ipd_feats(specs[k], sm.IPD_PAIRS)),
        (_ffi.spatial_opts("df", pairs, steer_vector=sv, num_sv=7, doa_index=idx),
         lambda k: sp.geometry_df(specs[k], sv, idx[k], pairs)),
    ]
    dev = [torch.from_numpy(s).cuda() for s in specs]
    for opts, operator in cases:
        outs = [torch.full((s.shape[1], _ffi.spatial_width(opts, F)), float("nan"), dtype=torch.float32,
                           device="cuda") for s in specs]
        ctx.spatial_batch(opts, 4, [d.data_ptr() for d in dev], [s.shape[1] for s in specs], F,
                          [o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert o.cpu().numpy().tobytes() == operator(k).tobytes(), (opts.kind, k)


# ---------------------------------------------------------------- engine and command lines
def write_waves(td, channels, seed):
    """Four ragged 16-bit files, 0.2 - 1.2 s; returns (wav.scp, {key: frames N x C int16})."""
    import scipy.io.wavfile
    rng = np.random.default_rng(seed)
    pcm = {}
    with open(f"{td}/wav.scp", "w") as fd:
        for k, (N, C) in enumerate(zip((3200, 19200, 8000, 12345), channels)):
            pcm[f"utt{k}"] = (1000 * rng.standard_normal((N, C))).astype(np.int16)
            scipy.io.wavfile.write(f"{td}/utt{k}.wav", 16000, pcm[f"utt{k}"])
            fd.write(f"utt{k} {td}/utt{k}.wav\n")
    return f"{td}/wav.scp", pcm


def run_cli(name, argv, expect_ok=True):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sptk", name + ".py")] + argv,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    if expect_ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def check_archive(td, engine, pcm, keys, doa_index=None):
    """Every row equals the operator on forward_stft of the same file, bit for bit; the --scp
    offsets address the same rows."""
    from setk_amd.engine import Pcm16Frames
    from setk_amd.libs.data_handler import ArchiveReader, ScriptReader
    rows = list(ArchiveReader(f"{td}/out.ark"))
    assert [k for k, _ in rows] == keys
    by_scp = ScriptReader(f"{td}/out.scp")
    assert list(by_scp.index_keys) == keys
    for key, mat in rows:
        want = engine.by_operators(engine.spectrogram(Pcm16Frames(pcm[key])),
                                   doa_index[key] if doa_index else None)
        assert mat.dtype == np.float32 and mat.shape == want.shape, (key, mat.shape, want.shape)
        assert mat.tobytes() == want.tobytes(), key
        assert np.array_equal(by_scp[key], mat), key
    engine.close()


def test_cli_linear_srp_and_the_refusal_of_msc(tmp_path):
    from setk_amd.engine import BatchSpatialFeatures
    td = str(tmp_path)
    scp, pcm = write_waves(td, (4, 4, 4, 4), 31)
    r = run_cli("compute_ipd_and_linear_srp", [scp, f"{td}/out.ark", "--scp", f"{td}/out.scp", "--batch-utts", "3",
                                               "--srp.num_doa", "91", "--srp.sample-tdoa", "true"])
    assert "Processed SRP for 4 utterances" in r.stderr + r.stdout
    check_archive(td, BatchSpatialFeatures("srp_linear", topo=(0.0, 0.2, 0.4, 0.8), num_doa=91, samp_tdoa=True),
                  pcm, ["utt0", "utt1", "utt2", "utt3"])
    r = run_cli("compute_ipd_and_linear_srp", [scp, f"{td}/msc.ark", "--type", "msc"], expect_ok=False)
    assert r.returncode != 0 and "MSC is not ported" in r.stderr


def test_cli_ipd_with_four_and_six_channels(tmp_path):
    from setk_amd.engine import BatchSpatialFeatures
    td = str(tmp_path)
    scp, pcm = write_waves(td, (4, 6, 6, 4), 32)
    r = run_cli("compute_ipd_and_linear_srp", [scp, f"{td}/out.ark", "--scp", f"{td}/out.scp", "--batch-utts", "3",
                                               "--type", "ipd", "--ipd.pair", "0,3;1,2", "--ipd.cos", "true",
                                               "--ipd.sin", "true"])
    assert "Processed IPD for 4 utterances" in r.stderr + r.stdout
    check_archive(td, BatchSpatialFeatures("ipd", pairs=[(0, 3), (1, 2)], cos=True, sin=True), pcm,
                  ["utt0", "utt1", "utt2", "utt3"])


def test_cli_circular_srp(tmp_path):
    from setk_amd.engine import BatchSpatialFeatures
    td = str(tmp_path)
    scp, pcm = write_waves(td, (6, 6, 6, 6), 33)
    r = run_cli("compute_circular_srp", [scp, f"{td}/out.ark", "--scp", f"{td}/out.scp", "--batch-utts", "3"])
    assert "Processd 4 utterances done" in r.stderr + r.stdout
    check_archive(td, BatchSpatialFeatures("srp_circular", diag_pair=[(0, 3), (1, 4), (2, 5)], n=6, d=0.07),
                  pcm, ["utt0", "utt1", "utt2", "utt3"])


def test_cli_df_on_geometry_with_doa_idx_and_utt2idx(tmp_path, gold):
    from setk_amd.engine import BatchSpatialFeatures
    td = str(tmp_path)
    scp, pcm = write_waves(td, (4, 4, 4, 4), 34)
    sv = (np.random.default_rng(7).standard_normal((7, 4, 257)) +
          1j * np.random.default_rng(8).standard_normal((7, 4, 257))).astype(np.complex64)
    np.save(f"{td}/sv.npy", sv)
    run_cli("compute_df_on_geometry", [scp, f"{td}/sv.npy", f"{td}/out.ark", "--scp", f"{td}/out.scp",
                                       "--batch-utts", "3", "--doa-idx", "2,0,5", "--df-pair", "0,1;1,3"])
    keys = ["utt0", "utt1", "utt2", "utt3"]
    check_archive(td, BatchSpatialFeatures("df", pairs=[(0, 1), (1, 3)], steer_vector=sv), pcm, keys,
                  {k: [2, 0, 5] for k in keys})
    with open(f"{td}/utt2idx", "w") as fd:
        fd.write("utt0 6\nutt1 0\nutt3 3\n")
    r = run_cli("compute_df_on_geometry", [scp, f"{td}/sv.npy", f"{td}/out.ark", "--scp", f"{td}/out.scp",
                                           "--batch-utts", "3", "--utt2idx", f"{td}/utt2idx"])
    assert "Missing utt2idx for utterance utt2" in r.stderr + r.stdout
    assert "Processed 3 utterances over 4" in r.stderr + r.stdout
    check_archive(td, BatchSpatialFeatures("df", pairs=[(0, 1)], steer_vector=sv), pcm, ["utt0", "utt1", "utt3"],
                  {"utt0": [6], "utt1": [0], "utt3": [3]})


# ---------------------------------------------------------------- end to end against the reference's command lines
@pytest.mark.parametrize("name", ["e2e_lin", "e2e_circ"])
def test_end_to_end_srp_against_the_reference_cli(gold, name):
    """The bound is derived, not chosen (spatial_model.e2e_bound): E = max |X_dev - X_ref| is
    measured here, X_dev from forward_stft, X_ref the reference's STFT (oracle.np_oracle, which
    the generator asserted to be bit-identical to it and whose max and sum the fixture holds)."""
    from oracle import np_oracle as o
    from setk_amd.engine import BatchSpatialFeatures, Pcm16Frames
    pcm = gold[name + "_pcm"]
    if name == "e2e_lin":
        engine = BatchSpatialFeatures("srp_linear", topo=(0.0, 0.2, 0.4, 0.8), num_doa=181)
    else:
        engine = BatchSpatialFeatures("srp_circular", diag_pair=[(0, 3), (1, 4), (2, 5)], n=6, d=0.07, num_doa=121)
    got = engine.run([Pcm16Frames(pcm)])[0]
    X_dev = engine.spectrogram(Pcm16Frames(pcm))
    weights = engine.weight
    pairs = engine.pairs
    engine.close()
    x = pcm.T.astype(np.float32) / np.float32(32768.0)
    X_ref = np.stack([o.forward_stft(c, **STFT, transpose=True) for c in x])
    xmax, xsum = gold[name + "_xabs"]
    assert np.abs(X_ref).max() == xmax and np.isclose(np.abs(X_ref).astype(np.float64).sum(), xsum, rtol=1e-12)
    E = float(np.abs(X_dev.astype(np.complex128) - X_ref).max())
    bound = sm.e2e_bound(X_ref, E, pairs, gold[name + "_norms"], weights)
    want = gold[name + "_srp"]
    diff = np.abs(got.astype(np.float64) - want)
    print(f"{name}: E = {E:.3e} ({E / xmax:.2e} of max |X|), max |device - reference CLI| = {diff.max():.3e}, "
          f"bound {bound.min():.3e} .. {bound.max():.3e}")
    assert got.shape == want.shape
    assert bound.max() < 0.05
    assert (diff <= bound[:, None]).all()
