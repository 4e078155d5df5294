#!/usr/bin/env python
"""
Training-target TF masks (IBM / IRM / IAM / PSM / PSA / CRM) from clean / noisy pairs on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/compute_mask.py`` (same positional arguments, options and
defaults, :159-202; Kaldi archive, optional script file, the two clip lines of :136-152 in the
log).  The reference transforms both files with librosa and forms the mask in numpy; this front
end hands batches of WAVE SAMPLES to ``engine.BatchMaskComputer``: both signals of every pair go
up once per batch, one fused launch transforms them and stores the mask alone, the masks and the
three logged numbers (the device's counters) come down once.

What differs on purpose: ``--format exraw`` is refused (SetkUnsupported); channel 0 of a
multi-channel file is taken (the reference's ``clean[0]``).
"""
import argparse
from contextlib import closing

import numpy as np

from setk_amd import _ffi
from setk_amd.engine import BatchMaskComputer
from setk_amd.libs.data_handler import ArchiveWriter, WaveReader
from setk_amd.libs.opts import StftParser
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import read_samples, run_batches, set_torch_free, stft_kwargs

logger = get_logger(__name__)

MASKS = ["irm", "ibm", "iam", "psm", "psa", "crm"]


def compute_mask(tgt, mix, mask):
    """The reference's module-level function on stored spectra (T x F complex, host arrays): the
    mask as compute_mask.py:59-107 returns it, without the clips of run(), computed on the device
    in float32 (T x 2F for crm)."""
    tgt = np.ascontiguousarray(tgt, dtype=np.complex64)
    mix = np.ascontiguousarray(mix, dtype=np.complex64)
    if tgt.shape != mix.shape or tgt.ndim != 2:
        raise ValueError(f"compute_mask: T x F spectra of one shape, got {tgt.shape} and {mix.shape}")
    T, F = tgt.shape
    out = np.empty((T, 2 * F if mask == "crm" else F), dtype=np.float32)
    _ffi.default_context().tf_mask(mask, tgt, mix, T, F, out, cutoff=float("nan"), want_stats=False)
    return out


def run(args):
    if args.format != "kaldi":
        raise _ffi.SetkUnsupported("--format exraw (libs/exraw.py) is not built; write Kaldi archives")
    clean_reader = WaveReader(args.clean_scp)
    noisy_reader = WaveReader(args.noisy_scp)
    set_torch_free(args, None)
    cutoff = args.cutoff
    engine = BatchMaskComputer(args.mask, cutoff=cutoff, **stft_kwargs(args))
    with closing(engine), ArchiveWriter(args.mask_ark, args.scp) as writer:

        def flush(pending):
            masks = engine.run([(c, n) for _, c, n in pending])
            for (key, _, _), mask, (over, below, below_sum), status in zip(pending, masks, engine.stats,
                                                                          engine.status):
                if over:
                    logger.info(f"Clip {over:d}({float(over) / mask.size:.2f}) items over "
                                f"{cutoff:.2f} for utterance {key}")
                if below:
                    logger.info(f"Clip {below}({float(below) / mask.size:.2f}, {below_sum / below:.2f}) "
                                f"items below zero for utterance {key}")
                if status != _ffi.NUM_OK:
                    logger.warning(f"{key}: the mask holds NaN / inf (a silent cell); written as it is")
                writer.write(key, mask)
            return len(pending)

        def utterances():
            for key in clean_reader.index_keys:
                if key in noisy_reader:
                    yield key, read_samples(clean_reader, key), read_samples(noisy_reader, key)
                else:
                    logger.warning(f"Missing bg-noise for utterance {key}")

        num_utts = run_batches(utterances(), args.batch_utts, flush)
    logger.info(f"Processed {num_utts} utterances")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to compute Tf-mask(as targets for Kaldi's nnet3, only for 2 component case, "
        "egs: speech & noise)",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("clean_scp", type=str, help="Scripts for clean speech in Kaldi format")
    parser.add_argument("noisy_scp", type=str, help="Scripts for noisy speech in Kaldi format")
    parser.add_argument("mask_ark", type=str, help="Location to dump mask archives")
    parser.add_argument("--format", type=str, default="kaldi", choices=["kaldi", "exraw"],
                        help="Output archive format ([setk_amd] exraw is refused)")
    parser.add_argument("--scp", type=str, default="", help="If assigned, generate corresponding mask scripts")
    parser.add_argument("--mask", type=str, default="irm", choices=MASKS,
                        help="Type of masks(irm/ibm/iam(FFT-mask,smm)/psm/psa/crm) to compute. 'psa' is the "
                        "nominator of psm. For iam/psm the second .scp is the noisy component.")
    parser.add_argument("--cutoff", type=float, default=-1,
                        help="Cutoff values(<=0, not cutoff) for some non-bounded masks, egs: iam/psm")
    parser.add_argument("--batch-utts", type=int, default=32, help="[setk_amd] pairs per batched call")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
