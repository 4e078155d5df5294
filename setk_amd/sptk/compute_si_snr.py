#!/usr/bin/env python
"""
SI-SNR (Si-SDR) scoring with permutation alignment on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/compute_si_snr.py`` (same positional arguments, options,
report lines and --per-utt / --utt-ali files, :71-141).  One scp on either side is the
single-speaker mode (si_snr per utterance); comma-separated scps are the multi-speaker mode: the
best average over the assignments of separated signals to references, and with --utt-ali the
assignment itself -- for ``apply_auxiva.py`` the answer to which ``src{n}`` is which speaker.  The
reference scores one utterance at a time in float32 numpy and walks the K! orders in Python; this
front end hands batches of WAVE SAMPLES to ``engine.BatchSiSnr``: the samples go up once per
batch (16-bit files as stored), every sum is float64 on the device, the tables come down once.
Utterances are scored and reported in the order of the first separated scp.  A non-finite
utterance fails the run and names its key.  The report is one, so under ``setk_amd.launch`` with
more than one rank the tool runs on one rank only.
"""
import argparse
import sys
from collections import defaultdict

from setk_amd import _ffi
from setk_amd.engine import BatchSiSnr, Pcm16Frames
from setk_amd.engine.metric import signal_length
from setk_amd.libs.data_handler import ScpReader, WaveReader
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import read_samples, run_batches

logger = get_logger(__name__)


class SpeakersReader(object):
    """One WaveReader per comma-separated scp (compute_si_snr.py:17-42); the first one gives the
    keys and their order.  Multi-channel audio is scored on channel 0 (:34-36), which the engine
    selects on the device."""

    def __init__(self, scps, at_least=2):
        split_scps = scps.split(",")
        if len(split_scps) < at_least:
            raise RuntimeError("Construct SpeakersReader need more than one script, got {}".format(scps))
        self.readers = [WaveReader(scp) for scp in split_scps]
        self.index_keys = self.readers[0].index_keys

    def __len__(self):
        return len(self.readers[0])

    def __getitem__(self, key):
        return [read_samples(reader, key) for reader in self.readers]


def cut(sig, end):
    """The first `end` samples of a signal (a vector, C x N or Pcm16Frames)."""
    if isinstance(sig, Pcm16Frames):
        return Pcm16Frames(sig.frames[:end])
    return sig[..., :end]


def truncate(sep_list, ref_list):
    """compute_si_snr.py:82-85 / :95-98: when the FIRST separated signal and the FIRST reference
    differ in length, every signal is cut to the shorter of the two."""
    a, b = signal_length(sep_list[0]), signal_length(ref_list[0])
    if a != b:
        end = min(a, b)
        sep_list = [cut(s, end) for s in sep_list]
        ref_list = [cut(s, end) for s in ref_list]
    return sep_list, ref_list


class Report(object):
    """compute_si_snr.py:45-68: sums and counts per class in the order of first appearance."""

    def __init__(self, spk2class=None):
        self.s2c = ScpReader(spk2class) if spk2class else None
        self.snr = defaultdict(float)
        self.cnt = defaultdict(int)

    def add(self, key, val):
        cls_str = "NG"
        if self.s2c:
            cls_str = self.s2c[key]
        self.snr[cls_str] += val
        self.cnt[cls_str] += 1

    def lines(self):
        tot_utt = sum([self.cnt[cls_str] for cls_str in self.cnt])
        tot_snr = sum([self.snr[cls_str] for cls_str in self.snr])
        out = ["Si-SDR(dB) Report: ", "Total: {:d}/{:.3f}".format(tot_utt, tot_snr / tot_utt)]
        for cls_str in self.snr:
            out.append("\t{}: {:d}/{:.3f}".format(cls_str, self.cnt[cls_str], self.snr[cls_str] / self.cnt[cls_str]))
        return out

    def report(self, file=None):
        print("\n".join(self.lines()), file=file or sys.stdout)


def run(args):
    single_speaker = len(args.sep_scp.split(",")) == 1
    reporter = Report(args.spk2class)
    utt_snr = open(args.per_utt, "w") if args.per_utt else None
    utt_ali = open(args.utt_ali, "w") if args.utt_ali else None
    sep_reader = SpeakersReader(args.sep_scp, at_least=1 if single_speaker else 2)
    ref_reader = SpeakersReader(args.ref_scp, at_least=1 if single_speaker else 2)
    _ffi.set_torch_free()  # the engine brings its own buffers and stream
    engine = BatchSiSnr()

    def flush(pending):
        results = engine.score([(sep, ref) for _, sep, ref in pending])
        for (key, _, _), (snr, ali, _, status) in zip(pending, results):
            if status != _ffi.NUM_OK:
                raise RuntimeError(f"{key}: NaN / inf among the samples (status {status}), no score")
            reporter.add(key, snr)
            if utt_snr:
                utt_snr.write("{}\t{:.2f}\n".format(key, snr))
            if utt_ali and not single_speaker:
                utt_ali.write("{}\t{}\n".format(key, " ".join(map(str, ali))))
        return len(pending)

    def utterances():
        for key in sep_reader.index_keys:
            sep, ref = truncate(sep_reader[key], ref_reader[key])
            yield key, sep, ref

    try:
        run_batches(utterances(), args.batch_utts, flush)
    finally:
        engine.close()
        for f in (utt_snr, utt_ali):
            if f:
                f.close()
    reporter.report()


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to compute SI-SDR, as metric of the separation quality",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("sep_scp", type=str,
                        help="Separated speech scripts, waiting for measure"
                        "(support multi-speaker, egs: spk1.scp,spk2.scp)")
    parser.add_argument("ref_scp", type=str,
                        help="Reference speech scripts, as ground truth for Si-SDR computation")
    parser.add_argument("--spk2class", type=str, default="",
                        help="If assigned, report results per class (gender or degree)")
    parser.add_argument("--per-utt", type=str, default="",
                        help="If assigned, report snr improvement for each utterance")
    parser.add_argument("--utt-ali", type=str, default="", help="If assigned, output audio alignments")
    parser.add_argument("--batch-utts", type=int, default=16,
                        help="[setk_amd] utterances per batched call")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
