"""
SI-SNR scoring with permutation alignment on the MI355X (setk_amd/csrc/metric.hip, libs/metric.py,
engine/metric.py and the command line) against the float64 statement of tests/metric_model.py and
the reference's recorded figures in tests/golden/ref_metric.npz (tools/make_golden_metric.py).  The
bounds and the measured figures are in tests/PARITY_NOTES_METRIC.md.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import metric_model as model  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

# Device against model.  Both form n per sample in float64 and differ only in the order of their
# sums: a term's error relative to |n| is about 1e-16 |x| / |n|, 1e-11 at 100 dB, so the true gap
# is near 1e-10 dB.  1e-6 leaves four decades and still fails a closed-form residual at 100 dB
# (4e-5 dB) or a float32 accumulator.
MODEL_BAR_DB = 1e-6
REF_BAR_DB = 4 * 6.584e-6   # the reference's float32 arithmetic against the model (test_metric_model.py)
TILE = 8192                 # kMetricTile
LENGTHS = [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 70001]
LEVELS = [-20.0, 0.0, 20.0, 60.0, 100.0]
NUMBER = re.compile(r"-?\d+\.\d+")


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_metric.npz")


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    return _ffi.default_context()


@pytest.fixture(scope="module")
def engine():
    from setk_amd.engine import BatchSiSnr
    e = BatchSiSnr()
    yield e
    e.close()


def utterance(rng, K, L, first_level=0, order=None):
    """K references with an offset of +0.05 and K estimates 0.7 s + noise - 0.02, estimate n planted
    on reference order[n] at LEVELS[(first_level + n) % 5]."""
    order = list(range(K)) if order is None else order
    pairs = {}
    for n in range(K):
        pairs[n] = model.planted(rng, L, LEVELS[(first_level + n) % len(LEVELS)])
    refs = [None] * K
    for n in range(K):
        refs[order[n]] = pairs[n][1]
    return [pairs[n][0] for n in range(K)], refs


def in_pcm(signals):
    return [np.clip(np.rint(np.asarray(s, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16) for s in signals]


# ---------------------------------------------------------------- 1. the pair table
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_pair_table_against_the_model(engine, K):
    rng = np.random.default_rng(100 + K)
    utts = [utterance(rng, K, L, first_level=li) for li, L in enumerate(LENGTHS)]
    results = engine.score(utts)
    worst, checked, high = 0.0, 0, 0
    for L, (est, ref), (_, _, table, status) in zip(LENGTHS, utts, results):
        want = model.pair_table(est, ref)
        keep = (want >= -150.0) & (want <= 100.0)
        gap = float(np.max(np.abs(table - want)[keep])) if keep.any() else 0.0
        print(f"K={K} L={L}: {int(keep.sum())} of {K * K} cells in [-150, 100], diagonal "
              f"{np.array2string(np.diag(want), precision=3)}, largest gap {gap:.3e} dB")
        assert status == 0 and table.shape == (K, K)
        worst, checked, high = max(worst, gap), checked + int(keep.sum()), high + int((keep & (want > 90.0)).sum())
        if L == 1:
            assert np.all(table == model.FLOOR_DB)
    print(f"K={K}: largest |device - model| {worst:.3e} dB over {checked} cells, {high} of them above 90 dB")
    assert checked >= 10 * K * K and high >= 1
    assert worst <= MODEL_BAR_DB


# ---------------------------------------------------------------- 2. edges
def test_edges_give_the_floor_exactly(engine):
    rng = np.random.default_rng(7)
    s = (0.1 * rng.standard_normal(300)).astype(np.float32)
    zero, const = np.zeros(300, np.float32), np.full(300, 0.25, np.float32)
    cases = [("silent reference", s, zero), ("silent estimate", zero, s), ("both silent", zero, zero),
             ("constant estimate", const, s), ("one sample", s[:1], s[1:2])]
    results = engine.score([([x], [r]) for _, x, r in cases])
    for (name, _, _), (best, order, table, status) in zip(cases, results):
        print(f"{name}: table {table[0, 0]!r} best {best!r}")
        assert table[0, 0] == model.FLOOR_DB and best == model.FLOOR_DB and order == (0,) and status == 0
    twice = engine.score([([2 * s], [s])])[0][2][0, 0]
    print(f"x = 2 s: device {twice:.3f} dB, model {model.si_snr(2 * s, s):.3f} dB")
    assert twice >= 150.0


def test_remove_dc_false_reaches_the_kernel():
    from setk_amd.engine import BatchSiSnr
    from setk_amd.libs import metric
    rng = np.random.default_rng(8)
    est, ref = utterance(rng, 3, 5000, first_level=1)
    keep, drop = BatchSiSnr(remove_dc=False), BatchSiSnr()
    try:
        kept, dropped = keep.score([(est, ref)])[0][2], drop.score([(est, ref)])[0][2]
    finally:
        keep.close()
        drop.close()
    want = model.pair_table(est, ref, remove_dc=False)
    gap, apart = float(np.max(np.abs(kept - want))), np.abs(np.diag(kept) - np.diag(dropped))
    print(f"remove_dc=False: largest |device - model| {gap:.3e} dB; |kept - removed| on the diagonal {apart}")
    assert gap <= MODEL_BAR_DB and np.all(apart > 1.0)
    one = metric.si_snr(est[0], ref[0], remove_dc=False)
    assert isinstance(one, float) and one == kept[0, 0]


# ---------------------------------------------------------------- 3. permutations
def check_orders(engine, K, orders, seed):
    rng = np.random.default_rng(seed)
    utts = [utterance(rng, K, 3000 + 11 * k, first_level=2, order=list(order)) for k, order in enumerate(orders)]
    for order, (est, ref), (best, perm, table, status) in zip(orders, utts, engine.score(utts)):
        want_best, want_perm = model.best_order(model.pair_table(est, ref))
        print(f"K={K} planted {tuple(order)}: device {perm} {best:.9f}, model {want_perm} {want_best:.9f}")
        assert status == 0 and perm == tuple(order) and perm == want_perm
        assert abs(best - want_best) <= MODEL_BAR_DB
        assert model.best_order(table) == (best, perm)  # the device's own additions are the model's


def test_all_six_orders_of_three_sources(engine):
    from itertools import permutations
    check_orders(engine, 3, list(permutations(range(3))), 31)


@pytest.mark.parametrize("K", [4, 8])
def test_reversed_and_drawn_orders(engine, K):
    rng = np.random.default_rng(40 + K)
    drawn = [tuple(int(v) for v in rng.permutation(K)) for _ in range(2)]
    check_orders(engine, K, [tuple(range(K))[::-1]] + drawn, 50 + K)


def test_ties_go_to_the_first_order(engine):
    rng = np.random.default_rng(9)
    L = 2000
    refs = [(0.1 * rng.standard_normal(L)).astype(np.float32) for _ in range(3)]
    silent = [np.zeros(L, np.float32)] * 3
    best, perm, table, _ = engine.score([(refs, silent)])[0]
    assert np.all(table == model.FLOOR_DB) and best == model.FLOOR_DB and perm == (0, 1, 2)
    same = (0.5 * refs[0] + 0.3 * refs[1]).astype(np.float32)
    best, perm, table, _ = engine.score([([same, same], refs[:2])])[0]
    want = model.best_order(model.pair_table([same, same], refs[:2]))
    print(f"identical estimates: table {table.tolist()}, device {perm} {best!r}, model {want}")
    assert np.array_equal(table[0], table[1]) and perm == (0, 1) == want[1] and abs(best - want[0]) <= MODEL_BAR_DB


def test_nine_sources_are_refused_naming_the_bound(engine):
    from setk_amd import _ffi
    from setk_amd.libs import metric
    rng = np.random.default_rng(10)
    sig = [(0.1 * rng.standard_normal(500)).astype(np.float32) for _ in range(9)]
    with pytest.raises(_ffi.SetkUnsupported, match="num_sources <= 8"):
        engine.score([(sig, sig)])
    with pytest.raises(_ffi.SetkUnsupported, match="num_sources <= 8"):
        metric.permute_si_snr(sig, sig)
    best, perm, _, status = engine.score([(sig[:8], sig[:8])])[0]  # the handle is usable afterwards
    assert perm == tuple(range(8)) and status == 0 and best > 100.0


# ---------------------------------------------------------------- 4. forms
@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(11)
    shapes = [(2, 5000), (8, TILE + 77), (1, 300), (3, 2 * TILE + 5), (4, 999)]
    return [utterance(rng, K, L, first_level=k, order=list(rng.permutation(K))) for k, (K, L) in enumerate(shapes)]


def same_results(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_ragged_batch_equals_single_calls_and_a_cut_batch(engine, ragged):
    from setk_amd.engine import BatchSiSnr
    whole = engine.score(ragged)
    single = [engine.score([u])[0] for u in ragged]
    small = BatchSiSnr(max_batch_bytes=200000)  # the second utterance alone is above it
    try:
        cut = small.score(ragged)
    finally:
        small.close()
    for k, (w, s, c) in enumerate(zip(whole, single, cut)):
        print(f"utterance {k}: K={len(w[1])} best {w[0]:.6f} order {w[1]}")
        assert same_results(w, s) and same_results(w, c)


def test_sixteen_bit_and_strided_input_have_the_bits_of_float32(engine, ctx, ragged):
    from setk_amd import _ffi
    from setk_amd.engine import Pcm16Frames
    rng = np.random.default_rng(12)
    est, ref = [in_pcm(part) for part in ragged[3]]
    as_float = [[v.astype(np.float32) / np.float32(32768) for v in part] for part in (est, ref)]
    mono = [[Pcm16Frames(v[:, None]) for v in part] for part in (est, ref)]
    # channel 0 of interleaved three-channel frames, read through its stride
    wide = [[Pcm16Frames(np.stack([v, in_pcm([0.1 * rng.standard_normal(v.size)])[0], v[::-1]], axis=1)) for v in part]
            for part in (est, ref)]
    planar = [[np.stack([v, v[::-1]]) for v in part] for part in as_float]  # C x N: channel 0
    mixed = ([mono[0][0]] + as_float[0][1:], as_float[1])                   # widened on the host
    want = engine.score([tuple(as_float)])[0]
    for name, form in (("16-bit mono", mono), ("16-bit, 3 channels", wide), ("float32 C x N", planar), ("mixed", mixed)):
        got = engine.score([tuple(form)])[0]
        print(f"{name}: best {got[0]!r} against {want[0]!r}")
        assert same_results(got, want)
    # float32 through a stride: the library call itself, on torch tensors
    import torch
    K, L = len(est), est[0].size
    dev = torch.device("cuda", ctx.device)
    inter = [torch.from_numpy(np.stack([v, v[::-1], 0 * v], axis=1).copy()).to(dev) for v in as_float[0] + as_float[1]]
    pair = np.empty(K * K)
    ctx.si_snr_batch([K], [t.data_ptr() for t in inter[:K]], [3] * K, [t.data_ptr() for t in inter[K:]], [3] * K, [L],
                     pair, stream=0)
    assert np.array_equal(pair.reshape(K, K), want[2])
    with pytest.raises(ValueError, match="flags"):
        ctx.si_snr_batch([K], [t.data_ptr() for t in inter[:K]], [3] * K, [t.data_ptr() for t in inter[K:]], [3] * K,
                         [L], pair, flags=_ffi.FLAG_OUT_PCM16, stream=0)


# ---------------------------------------------------------------- 5. status
def test_one_nan_marks_its_utterance_alone(engine, ragged):
    from setk_amd import _ffi
    clean = engine.score(ragged)
    est, ref = ragged[1]
    bad = ref[2].copy()
    bad[TILE + 5] = np.nan  # in the second tile
    dirty = list(ragged)
    dirty[1] = (est, ref[:2] + [bad] + ref[3:])
    got = engine.score(dirty)
    print("status:", [r[3] for r in got])
    assert [r[3] for r in got] == [0, _ffi.NUM_NONFINITE, 0, 0, 0]
    for k in (0, 2, 3, 4):
        assert same_results(got[k], clean[k])
    assert np.isnan(got[1][2][:, 2]).all() and got[1][1] in set(__import__("itertools").permutations(range(8)))


# ---------------------------------------------------------------- 6. libs.metric and the command line
def test_libs_metric_on_the_fixture(gold):
    from setk_amd.libs import metric
    bar = REF_BAR_DB + MODEL_BAR_DB
    for k, db in enumerate(gold["pair_db"]):
        x, s = gold[f"pair{k}_x"], gold[f"pair{k}_s"]
        for name, dc in (("dc", True), ("nodc", False)):
            got, ref = metric.si_snr(x, s, remove_dc=dc), float(gold[f"pair{k}_{name}"])
            print(f"planted {db:+.0f} dB remove_dc={dc}: device {got:.9f} reference {ref:.9f} gap {abs(got - ref):.3e}")
            assert isinstance(got, float) and abs(got - ref) <= bar
    for k, K in enumerate(gold["perm_k"]):
        xs, ss = list(gold[f"perm{k}_x"]), list(gold[f"perm{k}_s"])
        best, order = metric.permute_si_snr(xs, ss, align=True)
        print(f"K={K}: device {best:.9f} {order}, reference {float(gold[f'perm{k}_best']):.9f}")
        assert order == tuple(int(v) for v in gold[f"perm{k}_order"]) and isinstance(order, tuple)
        assert abs(best - float(gold[f"perm{k}_best"])) <= bar
        assert metric.permute_si_snr(xs, ss) == best


def write_cli_inputs(gold, tmp):
    import scipy.io.wavfile
    keys = [str(k) for k in gold["cli_keys"]]
    for name in ("sep1", "sep2", "ref1", "ref2"):
        with open(tmp / f"{name}.scp", "w") as f:
            for key in keys:
                scipy.io.wavfile.write(str(tmp / f"{name}_{key}.wav"), 16000, gold[f"cli_{name}_{key}"])
                f.write(f"{key}\t{tmp / (name + '_' + key + '.wav')}\n")
    (tmp / "spk2class").write_text("".join(f"{k}\t{c}\n" for k, c in zip(keys, gold["cli_classes"])))


def run_cli(argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sptk", "compute_si_snr.py")] + argv,
                          capture_output=True, text=True, timeout=300, cwd=ROOT)


def same_text_to(mine, theirs, bar):
    """Equal line shapes, every printed number within `bar`."""
    assert NUMBER.sub("#", mine) == NUMBER.sub("#", theirs), mine + "\n---\n" + theirs
    for a, b in zip(NUMBER.findall(mine), NUMBER.findall(theirs)):
        assert abs(float(a) - float(b)) <= bar, (a, b)


def test_command_line_on_the_fixture(gold, tmp_path):
    write_cli_inputs(gold, tmp_path)
    join = lambda names: ",".join(str(tmp_path / n) for n in names.split(","))  # noqa: E731
    modes = {"single": ("sep1.scp", "ref1.scp", []), "multi": ("sep1.scp,sep2.scp", "ref1.scp,ref2.scp", []),
             "multi_class": ("sep1.scp,sep2.scp", "ref1.scp,ref2.scp", ["--spk2class", str(tmp_path / "spk2class")])}
    for tag, (sep, ref, more) in modes.items():
        files = {}
        for batch in ([], ["--batch-utts", "2"]):
            snr, ali = tmp_path / f"{tag}{len(batch)}.snr", tmp_path / f"{tag}{len(batch)}.ali"
            r = run_cli([join(sep), join(ref), "--per-utt", str(snr), "--utt-ali", str(ali)] + more + batch)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
            files[len(batch)] = (r.stdout, snr.read_text(), ali.read_text())
        report, per_utt, utt_ali = files[0]
        print(f"{tag}:\n{report}{per_utt}{utt_ali}")
        assert utt_ali == str(gold[f"cli_{tag}_utt_ali"])
        # one unit of the last printed digit plus the reference's distance from the model
        same_text_to(per_utt, str(gold[f"cli_{tag}_per_utt"]), 0.011)
        same_text_to(report, str(gold[f"cli_{tag}_report"]), 0.011)
        assert files[2] == files[0]  # --batch-utts 2 gives the same files and report


def test_command_line_fails_on_a_non_finite_utterance_naming_the_key(gold, tmp_path):
    import scipy.io.wavfile
    write_cli_inputs(gold, tmp_path)
    bad = gold["cli_sep1_utt_c"].astype(np.float32) / np.float32(32768)
    bad[17] = np.inf
    scipy.io.wavfile.write(str(tmp_path / "sep1_utt_c.wav"), 16000, bad)
    r = run_cli([str(tmp_path / "sep1.scp"), str(tmp_path / "ref1.scp")])
    print(r.stderr[-600:])
    assert r.returncode != 0 and "utt_c" in r.stderr and "Report" not in r.stdout
