#!/usr/bin/env python
"""
SRP angular spectrum of circular arrays on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/compute_circular_srp.py`` (same positional arguments,
options, defaults and Kaldi archive output): batches of WAVE SAMPLES go to
``engine.BatchSpatialFeatures`` (setk_stft_batch -> setk_spatial_batch on device pointers, one
download of the T x D spectra).  Under ``torchrun`` every rank would write the same archive, so
the tool runs on one rank only.
"""
import argparse

import numpy as np

from setk_amd import _ffi
from setk_amd.engine import BatchSpatialFeatures
from setk_amd.libs.data_handler import ArchiveWriter, WaveReader
from setk_amd.libs.opts import StftParser
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import stft_kwargs
from setk_amd.sptk.compute_ipd_and_linear_srp import feed

logger = get_logger(__name__)


def run(args):
    srp_pair = [tuple(map(int, p.split(","))) for p in args.diag_pair.split(";")]
    if not len(srp_pair):
        raise RuntimeError(f"Bad configurations with --pair {args.diag_pair}")
    logger.info(f"Compute gcc with {srp_pair}")
    engine = BatchSpatialFeatures("srp_circular", diag_pair=srp_pair, n=args.n, d=args.d, sample_rate=args.sr,
                                  num_doa=args.num_doas, **stft_kwargs(args))
    waves = WaveReader(args.wav_scp)
    _ffi.set_torch_free(waves.first_channels_at_most(8))
    num_done = 0
    with ArchiveWriter(args.srp_ark, args.scp) as writer:

        def on_result(key, srp):
            nonlocal num_done
            num_done += 1
            nan = np.sum(np.isnan(srp))
            if nan:
                raise RuntimeError(f"Matrix {key} has nan ({nan:d}) items)")
            writer.write(key, srp)
            if not num_done % 1000:
                logger.info(f"Processed {num_done:d} utterances...")

        feed(engine, waves, waves.index_keys, args.batch_utts, on_result)
    engine.close()
    logger.info(f"Processd {len(waves):d} utterances done")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to compute SRP augular spectrum for circular arrays",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Rspecifier for multi-channel wave")
    parser.add_argument("srp_ark", type=str, help="Location to dump features")
    parser.add_argument("--scp", type=str, default="", help="If assigned, generate corresponding scripts")
    parser.add_argument("--n", type=int, default=6, help="Number of arrays")
    parser.add_argument("--d", type=float, default=0.07, help="Diameter of circular array")
    parser.add_argument("--diag-pair", type=str, default="0,3;1,4;2,5",
                        help="Compute gcc between those diagonal arrays")
    parser.add_argument("--sr", type=int, default=16000, help="Sample rate of input wave")
    parser.add_argument("--num-doas", type=int, default=121,
                        help="Number of DoA to sample between 0 and 2pi")
    parser.add_argument("--batch-utts", type=int, default=32, help="[setk_amd] utterances per GPU batch")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
