"""
SI-SNR scoring without a device: the float64 statement (tests/metric_model.py) against what the
unmodified reference returned (tests/golden/ref_metric.npz, tools/make_golden_metric.py), its edge
semantics, and the host-only parts of the product -- the refusals of libs.metric, the command
line's truncation rule, parser and report text.

The reference computes in float32; how far that puts it from the float64 statement was measured
when the fixture was made (REF_GAP_DB, numpy 2.2.6) and the reference is held to four times it.
Alignments are equal outright.
"""
import os
import re

import numpy as np
import pytest

import metric_model as model
from setk_amd import _ffi
from setk_amd.engine import Pcm16Frames
from setk_amd.libs import metric
from setk_amd.sptk import compute_si_snr as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_metric.npz")
REF_GAP_DB = 6.584e-6       # largest |reference - model| over the fixture's figures, as measured
BAR_DB = 4 * REF_GAP_DB


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def cli_signals(golden, key):
    """What the command line scores for one key: float32 channel 0 of every file, cut by its rule."""
    def chan0(name):
        v = golden[f"cli_{name}_{key}"].astype(np.float32) / np.float32(32768)
        return v if v.ndim == 1 else np.ascontiguousarray(v[:, 0])
    return cli.truncate([chan0("sep1"), chan0("sep2")], [chan0("ref1"), chan0("ref2")])


def test_reference_si_snr_lies_within_four_times_its_measured_gap(golden):
    worst = 0.0
    for k, db in enumerate(golden["pair_db"]):
        x, s = golden[f"pair{k}_x"], golden[f"pair{k}_s"]
        for name, dc in (("dc", True), ("nodc", False)):
            got, ref = model.si_snr(x, s, remove_dc=dc), float(golden[f"pair{k}_{name}"])
            print(f"planted {db:+.0f} dB remove_dc={dc}: model {got:.9f} reference {ref:.9f} gap {abs(got - ref):.3e}")
            worst = max(worst, abs(got - ref))
    print(f"largest gap {worst:.3e} dB, recorded {float(golden['ref_gap_db']):.3e}, bar {BAR_DB:.3e}")
    assert float(golden["ref_gap_db"]) <= REF_GAP_DB * 1.001
    assert worst <= BAR_DB


def test_reference_alignments_are_the_models(golden):
    for k, K in enumerate(golden["perm_k"]):
        best, order = model.permute_si_snr(list(golden[f"perm{k}_x"]), list(golden[f"perm{k}_s"]), align=True)
        ref_best, ref_order = float(golden[f"perm{k}_best"]), tuple(int(v) for v in golden[f"perm{k}_order"])
        print(f"K={K}: model {best:.9f} {order} reference {ref_best:.9f} {ref_order}")
        assert order == ref_order
        assert abs(best - ref_best) <= BAR_DB


def test_edges_give_the_floor_exactly():
    rng = np.random.default_rng(3)
    s = (0.1 * rng.standard_normal(300)).astype(np.float32)
    zero, const = np.zeros(300, np.float32), np.full(300, 0.25, np.float32)
    cases = {"silent reference": (s, zero), "silent estimate": (zero, s), "both silent": (zero, zero),
             "constant estimate": (const, s), "one sample": (s[:1], s[1:2])}
    for name, (x, ref) in cases.items():
        v = model.si_snr(x, ref)
        print(f"{name}: {v!r}")
        assert v == model.FLOOR_DB
    twice = model.si_snr(2 * s, s)
    print(f"x = 2 s: {twice:.3f} dB")
    assert twice >= 150.0


def test_dropping_the_mean_removal_is_visible_on_offset_signals():
    x, s = model.planted(np.random.default_rng(4), 4000, 20.0)
    with_dc, without = model.si_snr(x, s), model.si_snr(x, s, remove_dc=False)
    print(f"remove_dc=True {with_dc:.4f}  remove_dc=False {without:.4f}")
    assert abs(with_dc - 20.0) < 0.5 and abs(with_dc - without) > 1.0


def test_ties_go_to_the_first_order():
    assert model.best_order(np.full((3, 3), model.FLOOR_DB)) == (model.FLOOR_DB, (0, 1, 2))
    # two identical estimates: (0, 1) and (1, 0) add the same two numbers in the other order
    table = np.array([[7.25, 3.5], [7.25, 3.5]])
    assert model.best_order(table) == (5.375, (0, 1))
    table = np.array([[1.0, 9.0, 2.0], [8.0, 1.0, 2.0], [0.0, 1.0, 7.0]])
    assert model.best_order(table) == (8.0, (1, 0, 2))


def test_libs_metric_refuses_on_the_host():
    v = np.zeros(8, np.float32)
    with pytest.raises(RuntimeError, match="size do not match between xlist and slist: 2 vs 1"):
        metric.permute_si_snr([v, v], [v])
    with pytest.raises(ValueError, match="differ in length"):
        metric.si_snr(v, v[:5])
    with pytest.raises(_ffi.SetkUnsupported, match="editdistance"):
        metric.permute_ed([[1]], [[1]])


def test_truncation_follows_the_first_signals_only():
    a, b = np.arange(10, dtype=np.float32), np.arange(7, dtype=np.float32)
    sep, ref = cli.truncate([a, a + 1], [b, b + 1])
    assert [v.size for v in sep + ref] == [7, 7, 7, 7] and np.array_equal(sep[1], (a + 1)[:7])
    # equal first signals: nothing is cut, whatever the others are (the reference then fails in numpy;
    # the engine refuses with ValueError)
    sep, ref = cli.truncate([a, b], [a, a])
    assert [v.size for v in sep + ref] == [10, 7, 10, 10]
    # 16-bit frames are cut along the frames, C x N arrays along the samples
    frames = Pcm16Frames(np.arange(24, dtype=np.int16).reshape(12, 2))
    sep, ref = cli.truncate([frames], [np.zeros((2, 9), np.float32)])
    assert sep[0].frames.shape == (9, 2) and np.array_equal(sep[0].frames, frames.frames[:9])
    assert ref[0].shape == (2, 9)


def test_parser_takes_the_reference_arguments():
    args = cli.build_parser().parse_args(["a.scp,b.scp", "c.scp,d.scp", "--spk2class", "s2c", "--per-utt", "snr",
                                          "--utt-ali", "ali", "--batch-utts", "2"])
    assert (args.sep_scp, args.ref_scp, args.spk2class, args.per_utt, args.utt_ali, args.batch_utts) == \
        ("a.scp,b.scp", "c.scp,d.scp", "s2c", "snr", "ali", 2)
    args = cli.build_parser().parse_args(["a.scp", "c.scp"])
    assert (args.spk2class, args.per_utt, args.utt_ali, args.batch_utts) == ("", "", "", 16)


NUMBER = re.compile(r"-?\d+\.\d+")


def test_report_text_is_the_references(golden, tmp_path):
    s2c = tmp_path / "spk2class"
    s2c.write_text("".join(f"{k}\t{c}\n" for k, c in zip(golden["cli_keys"], golden["cli_classes"])))
    for tag, classes in (("multi", ""), ("multi_class", str(s2c))):
        report = cli.Report(classes)
        for key in golden["cli_keys"]:
            report.add(str(key), model.permute_si_snr(*cli_signals(golden, str(key))))
        mine, theirs = report.lines(), str(golden[f"cli_{tag}_report"]).rstrip("\n").split("\n")
        print("\n".join(mine))
        assert [NUMBER.sub("#", line) for line in mine] == [NUMBER.sub("#", line) for line in theirs]
        for a, b in zip(mine, theirs):
            for va, vb in zip(NUMBER.findall(a), NUMBER.findall(b)):
                assert abs(float(va) - float(vb)) <= 0.0011  # one unit of the last printed digit + the bar
