"""
CPU tests of the CACGMM path: the float64 model of tests/cacgmm_model.py against the reference's
recorded posteriors (tests/golden/ref_cacgmm*.npz) and, where the reference tree is present,
against the unmodified CacgmmTrainer run live; the command line's surface; the multi-rank walk
of the random draws, with a stub trainer and no device.
"""
from pathlib import Path

import numpy as np
import pytest

import cacgmm_model as cm
from conftest import load_golden
from oracle import ref_harness as rh

needs_reference = pytest.mark.skipif(not rh.available(), reason="the reference tree is not present")


@pytest.fixture(scope="module")
def record():
    return load_golden("ref_cacgmm.npz")


@pytest.mark.parametrize("name", sorted(cm.CASES))
def test_model_matches_the_recorded_reference_at_every_snapshot(record, name):
    x, g0, K, N, cgmm_init, ua = cm.case_inputs(name)
    assert np.array_equal(x, record[name + "_spec"])
    if g0 is not None:
        assert np.array_equal(g0, record[name + "_gamma0"])
    model = cm.cacgmm_em(x, K, N, g0, cgmm_init=cgmm_init, update_alpha=ua)
    assert len(model) == N + 1
    for n in cm.snapshots(N):
        ref = record[f"{name}_ref128_{n}"]
        assert model[n].shape == ref.shape == (K, cm.CASE_BINS, x.shape[2])
        # the same arithmetic on the same float64 input (another BLAS may order its sums differently)
        assert np.abs(model[n] - ref).max() <= 1e-9, (name, n)
        assert np.abs(model[n].sum(0) - 1).max() <= 1e-12


def test_zero_iterations_return_the_start(record):
    x, g0, K, _, _, _ = cm.case_inputs("c7_chunk")
    (only,) = cm.cacgmm_em(x, K, 0, g0)
    assert np.array_equal(only, g0)
    x, _, K, _, _, ua = cm.case_inputs("c4_cgmm_init_fixed_alpha")
    (only,) = cm.cacgmm_em(x, K, 0, None, cgmm_init=True, update_alpha=ua)
    assert np.abs(only - record["c4_cgmm_init_fixed_alpha_ref128_0"]).max() <= 1e-9


@needs_reference
@pytest.mark.parametrize("name", sorted(cm.CASES))
def test_model_matches_the_live_reference(name):
    """complex128 input: the same arithmetic, 1e-9.  complex64 input: the reference normalises in
    float32, the model (as the device) in float64; that distance is printed -- the figures of
    PARITY_NOTES_CACGMM.md -- and held to the record's."""
    libs = rh.load()
    x, g0, K, N, cgmm_init, ua = cm.case_inputs(name)
    model = cm.cacgmm_em(x, K, N, g0, cgmm_init=cgmm_init, update_alpha=ua)

    def live(obs):
        tr = libs.cluster.CacgmmTrainer(obs, K, gamma=None if g0 is None else g0.copy(), cgmm_init=cgmm_init,
                                        update_alpha=ua)
        start = np.array(tr.gamma)
        return start, np.array(tr.train(N))

    start, last = live(x.astype(np.complex128))
    assert np.abs(start - model[0]).max() <= 1e-9 and np.abs(last - model[N]).max() <= 1e-9
    _, last64 = live(x)
    d = np.abs(last64 - model[N])
    print(f"[{name}] float32-normalisation deviation after {N} iterations: max {d.max():.3e}, mean {d.mean():.3e}")
    assert np.abs(last64 - load_golden("ref_cacgmm.npz")[name + "_ref64_last"]).max() <= 1e-9


@pytest.mark.parametrize("name,K,kw", [("2spk", 3, {}), ("noisy", 2, dict(cgmm_init=True, update_alpha=False))])
def test_model_on_the_doc_recipes(name, K, kw):
    """The model on the spectrogram the reference saw, against its recorded posteriors: the
    float32-normalisation deviation the GPU test's bounds are ten times of."""
    from oracle import np_oracle as o
    post = load_golden(f"ref_cacgmm_{name}.npz")[name + "_post"]
    pcm = load_golden("doc_spatial_clustering.npz")["pcm_" + name]
    samps = (pcm.astype(np.float32) / np.float32(32768.0)).T.copy()
    obs = o.multichannel_stft(samps, transpose=False, frame_len=512, frame_hop=256, window="hann", center=True)
    np.random.seed(777)
    g0 = None if kw else cm.random_start(K, obs.shape[1], obs.shape[2])
    got = np.transpose(cm.cacgmm_em(obs, K, 20, g0, **kw)[-1], (0, 2, 1))
    d = np.abs(got - post)
    print(f"[doc {name}] model against the recorded reference: max {d.max():.3e}, mean {d.mean():.3e}")
    recorded = {"2spk": (1.670e-05, 6.953e-08), "noisy": (3.561e-04, 2.032e-07)}[name]
    # (the figures of PARITY_NOTES_CACGMM.md, to the digits given there)
    assert d.max() <= 1.01 * recorded[0] and d.mean() <= 1.01 * recorded[1]


# ---- the command line ----
def _parser():
    from setk_amd.sptk import estimate_cacgmm_masks as cli
    return cli, cli.build_parser()


def test_cli_defaults_equal_the_reference():
    cli, parser = _parser()
    a = parser.parse_args(["wav.scp", "dst"])
    assert (a.wav_scp, a.dst_dir) == ("wav.scp", "dst")
    assert a.num_iters == 50 and a.num_classes == 2 and a.seed == 777 and a.init_mask == ""
    assert not a.cgmm_init and a.solve_permu and a.update_alpha and a.fmt == "numpy"
    assert (a.frame_len, a.frame_hop, a.window, bool(a.center), bool(a.round_power_of_two)) == \
        (512, 256, "hann", True, True)
    assert a.batch_utts == 1
    a = parser.parse_args(["--cgmm-init", "true", "--solve-permu", "false", "--update-alpha", "false",
                           "--mask-format", "kaldi", "--init-mask", "m.scp", "--num-classes", "3", "a", "b"])
    assert a.cgmm_init and not a.solve_permu and not a.update_alpha and a.fmt == "kaldi" and a.init_mask == "m.scp"


@needs_reference
def test_cli_options_equal_the_reference_parser():
    """Every option string, default and destination of the reference's parser, read from its
    source (the reference builds its parser under __main__)."""
    import re
    src = Path(rh.REF_SPTK, "estimate_cacgmm_masks.py").read_text()
    ref_opts = set(re.findall(r'add_argument\(\s*"(--[a-z-]+)"', src))
    _, parser = _parser()
    mine = {s for act in parser._actions for s in act.option_strings if s.startswith("--")}
    stft = {"--frame-len", "--frame-hop", "--center", "--round-power-of-two", "--window", "--help"}
    assert mine - stft - {"--batch-utts"} == ref_opts


class _Reader(object):
    """Four utterances; peek_nsamps as a wave header gives it."""
    nsamps = {"a": 2560, "b": 5120, "c": 2560 + 255, "d": 7680}

    def __init__(self):
        self.index_keys = list(self.nsamps)
        self.loaded = []

    def __len__(self):
        return len(self.index_keys)

    def peek_nsamps(self, key):
        return self.nsamps[key]

    def __getitem__(self, key):
        self.loaded.append(key)
        T = 1 + self.nsamps[key] // 256
        return np.zeros((2, 257, T), dtype=np.complex64)


class _Shard(object):
    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def assign_by_duration(self, reader):
        return reader.index_keys[self.rank::self.world]

    def barrier(self):
        pass


def _walk(tmp_path, rank, world, init_keys=(), existing=(), **opts):
    """train_table with a stub trainer that records the first draw it would have seen."""
    cli, parser = _parser()
    args = parser.parse_args(["--num-iters", "1", "--solve-permu", "false", "wav.scp", str(tmp_path)])
    for k, v in opts.items():
        setattr(args, k, v)
    seen = {}

    class Trainer(object):
        def __init__(self, obs, K, gamma=None, cgmm_init=False, update_alpha=True):
            self.K, (_, self.F, self.T) = K, obs.shape
            self.key = reader.loaded[-1]
            if gamma is None and not (cgmm_init and K == 2):
                seen[self.key] = np.random.uniform(size=[K, self.F, self.T])[0, 0, 0]

        def train(self, n):
            return np.zeros((self.K, self.F, self.T))

    reader = _Reader()
    for key in existing:
        (tmp_path / f"{key}.npy").write_bytes(b"")
    init = {k: np.zeros((args.num_classes, 1 + reader.nsamps[k] // 256, 257)) for k in init_keys}
    written = []
    np.random.seed(args.seed)
    n = cli.train_table(args, reader, init or None, _Shard(rank, world), tmp_path,
                        lambda key, m: written.append((key, m.shape, m.dtype)), trainer_cls=Trainer)
    return n, seen, written, np.random.uniform()


def _expected_first_draws(K, skip=()):
    """The first draw of every utterance in a one-process run, and the generator's next value."""
    np.random.seed(777)
    out = {}
    for key, n in _Reader.nsamps.items():
        if key not in skip:
            out[key] = np.random.uniform(size=[K, 257, 1 + n // 256])[0, 0, 0]
    return out, np.random.uniform()


@pytest.mark.parametrize("K", [2, 3])
def test_multi_rank_walk_discards_the_foreign_draws(tmp_path, K):
    want, after = _expected_first_draws(K)
    n, seen, written, nxt = _walk(tmp_path, 0, 1, num_classes=K)
    assert n == 4 and seen == want and nxt == after
    assert [w[0] for w in written] == list("abcd") and written[0][1:] == ((K, 11, 257), np.float32)
    total = 0
    for rank in range(3):
        n, seen, written, nxt = _walk(tmp_path, rank, 3, num_classes=K)
        mine = _Reader().index_keys[rank::3]
        assert seen == {k: want[k] for k in mine} and [w[0] for w in written] == mine
        # every rank has consumed exactly K * F * T draws per utterance of the table
        assert nxt == after
        total += n
    assert total == 4


def test_walk_draws_nothing_for_init_masks_existing_files_and_cgmm_init(tmp_path):
    want, after = _expected_first_draws(3, skip=("b", "d"))
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        d = tmp_path / f"r{rank}{world}"
        d.mkdir()
        n, seen, written, nxt = _walk(d, rank, world, init_keys=("b",), existing=("d",), num_classes=3)
        mine = [k for k in _Reader().index_keys[rank::world] if k != "d"]
        assert [w[0] for w in written] == mine and n == len(mine)
        assert seen == {k: want[k] for k in mine if k != "b"} and nxt == after
    # --cgmm-init true with two classes: no draw at all, on any rank; with three classes it falls
    # through to the random start (cluster.py:496)
    np.random.seed(777)
    untouched = np.random.uniform()
    for rank, world in ((0, 1), (1, 2)):
        d = tmp_path / f"c{rank}{world}"
        d.mkdir()
        n, seen, _, nxt = _walk(d, rank, world, num_classes=2, cgmm_init=1)
        assert seen == {} and nxt == untouched and n == len(_Reader().index_keys[rank::world])
    d = tmp_path / "c3"
    d.mkdir()
    _, seen, _, nxt = _walk(d, 1, 2, num_classes=3, cgmm_init=1)
    want3, after3 = _expected_first_draws(3)
    assert seen == {k: want3[k] for k in ("b", "d")} and nxt == after3


def test_failed_utterance_is_logged_and_the_run_goes_on(tmp_path, caplog):
    cli, parser = _parser()
    args = parser.parse_args(["--num-classes", "2", "--cgmm-init", "true", "--solve-permu", "false", "w", str(tmp_path)])

    class Trainer(object):
        def __init__(self, obs, K, **kw):
            self.shape = (K,) + obs.shape[1:]
            self.fail = obs.shape[2] == 21  # utterance b

        def train(self, n):
            if self.fail:
                raise np.linalg.LinAlgError("Eigenvalues did not converge")
            return np.zeros(self.shape)

    written = []
    cli.logger.propagate = True
    with caplog.at_level("INFO"):
        n = cli.train_table(args, _Reader(), None, _Shard(0, 1), tmp_path, lambda k, m: written.append(k),
                            trainer_cls=Trainer)
    assert n == 3 and written == ["a", "c", "d"]
    assert "Training utterance b ... Failed" in caplog.text and "Training utterance c ... Done" in caplog.text


def test_trainer_refuses_what_the_device_does_not_implement():
    from setk_amd import _ffi
    from setk_amd.libs.cluster import CacgmmTrainer, norm_observation
    x = np.ones((2, 3, 4), dtype=np.complex64)
    with pytest.raises(_ffi.SetkUnsupported):
        CacgmmTrainer(x, 2, cacgmm="model.pkl")
    with pytest.raises(_ffi.SetkUnsupported):
        CacgmmTrainer(x, 5)
    with pytest.raises(_ffi.SetkUnsupported):
        CacgmmTrainer(np.ones((9, 3, 4), dtype=np.complex64), 2)
    with pytest.raises(ValueError):
        CacgmmTrainer(x, 2, gamma=np.ones((2, 4, 3)))
    z = norm_observation(np.array([[3.0, 0.0], [4.0, 0.0]]), axis=0)
    assert np.allclose(z, [[0.6, 0.0], [0.8, 0.0]])
