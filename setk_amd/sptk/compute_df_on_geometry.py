#!/usr/bin/env python
"""
Directional / angle features from steer vectors (array geometry) on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/compute_df_on_geometry.py`` (same positional arguments,
options, defaults and Kaldi archive output): batches of WAVE SAMPLES go to
``engine.BatchSpatialFeatures``; the steer vectors go up once, one launch covers all utterances
and all chosen directions of a batch (setk_stft_batch -> setk_spatial_batch).  Utterances
without an entry in --utt2idx are reported and left out, as the reference does.  Under
``torchrun`` every rank would write the same archive, so the tool runs on one rank only.
"""
import argparse

import numpy as np

from setk_amd import _ffi
from setk_amd.engine import BatchSpatialFeatures
from setk_amd.libs.data_handler import ArchiveWriter, ScpReader, WaveReader
from setk_amd.libs.opts import StftParser
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import stft_kwargs
from setk_amd.sptk.compute_ipd_and_linear_srp import feed

logger = get_logger(__name__)


def run(args):
    waves = WaveReader(args.wav_scp)
    if args.utt2idx:
        utt2idx = ScpReader(args.utt2idx, value_processor=int)
        logger.info(f"Using --utt2idx={args.utt2idx}")
    else:
        utt2idx = None
        logger.info(f"Using --doa-idx={args.doa_idx}")
    df_pair = [tuple(map(int, p.split(","))) for p in args.df_pair.split(";")]
    if not len(df_pair):
        raise RuntimeError(f"Bad configurations with --pair {args.df_pair}")
    logger.info(f"Compute directional feature with {df_pair}")
    # A x M x F
    steer_vector = np.load(args.steer_vector)
    engine = BatchSpatialFeatures("df", pairs=df_pair, steer_vector=steer_vector, **stft_kwargs(args))
    _ffi.set_torch_free(waves.first_channels_at_most(8))
    keys, doa_index = [], {}
    for key in waves.index_keys:
        if utt2idx is None:
            doa_index[key] = [int(v) for v in str(args.doa_idx).split(",")]
        elif key in utt2idx:
            doa_index[key] = [utt2idx[key]]
        else:
            logger.warning(f"Missing utt2idx for utterance {key}")
            continue
        keys.append(key)
    num_done = 0
    with ArchiveWriter(args.dup_ark, args.scp) as writer:

        def on_result(key, df):
            nonlocal num_done
            writer.write(key, df)
            num_done += 1
            if not num_done % 1000:
                logger.info(f"Processed {num_done:d} utterance...")

        feed(engine, waves, keys, args.batch_utts, on_result, doa_index=doa_index)
    engine.close()
    logger.info(f"Processed {num_done:d} utterances over {len(waves):d}")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to compute directional features for linear arrays, "
        "based on given steer vector. Also see scripts/sptk/compute_steer_vector.py",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Multi-Channel wave scripts in kaldi format")
    parser.add_argument("steer_vector", type=str,
                        help="Pre-computed steer vector in each directions (in shape A x M x F, A: number "
                        "of DoAs, M: microphone number, F: FFT bins)")
    parser.add_argument("dup_ark", type=str, help="Location to dump features (in ark format)")
    parser.add_argument("--utt2idx", type=str, default="",
                        help="utt2idx for index (between [0, A - 1]) of the DoA.")
    parser.add_argument("--doa-idx", type=str, default=0,
                        help="DoA index for all utterances if --utt2idx=\"\"")
    parser.add_argument("--scp", type=str, default="",
                        help="If assigned, generate corresponding feature scripts")
    parser.add_argument("--df-pair", type=str, default="0,1",
                        help="Microphone pairs for directional feature computation")
    parser.add_argument("--batch-utts", type=int, default=32, help="[setk_amd] utterances per GPU batch")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
