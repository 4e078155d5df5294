#!/usr/bin/env python
"""
Mask-based sound source localisation (ML / SRP-PHAT / MUSIC) on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/do_ssl.py`` (same positional arguments, options,
defaults and output file: ``key\\t{doa:.4f}``, online mode one value per chunk separated by
blanks, :118-172).  The reference walks a SpectrogramReader and scores one utterance -- online
one overlapping window -- at a time in numpy; this front end hands batches of WAVE SAMPLES and
masks to ``engine.BatchLocalizer``: the samples go up once per batch, the STFT, the frame
scores and the window reductions run on the GPU, the indices come down once.  Lines are
written in the table's order.  The tool runs on one rank (one output file).

One deliberate difference (tests/PARITY_NOTES_SSL.md): in online mode the mask is cut along
the FRAMES of each window; the reference cuts the mask's last axis after bringing it to T x F,
i.e. the bins, and then fails to broadcast for any real input.
"""
import argparse

import numpy as np

from setk_amd import _ffi
from setk_amd.engine import BatchLocalizer
from setk_amd.libs.data_handler import NumpyReader, WaveReader
from setk_amd.libs.opts import StftParser, str2tuple
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import n_fft, read_samples, run_batches, set_torch_free, stft_kwargs

logger = get_logger(__name__)


def add_wta(masks_list, eps=1e-4):
    """Winner-take-all masks (do_ssl.py:17-27): a speaker keeps its mask where it is the
    largest of all, eps elsewhere."""
    max_mask = np.max(np.stack(masks_list, axis=-1), -1)
    return [np.where(m == max_mask, m, eps) for m in masks_list]


def parse_srp_pair(text):
    """ "0,8;1,9" -> ([0, 1], [8, 9])  (do_ssl.py:70-74)."""
    pairs = [tuple(map(int, p.split(","))) for p in text.split(";")]
    return [t[0] for t in pairs], [t[1] for t in pairs]


def load_mask(readers, key, mask_eps, num_bins):
    """do_ssl.py:83-93: the first reader's mask (after the winner-take-all rule when several
    readers and --mask-eps >= 0), as T x F."""
    if not readers:
        return None
    mask = [np.asarray(r[key]) for r in readers]
    if mask_eps >= 0 and len(readers) > 1:
        mask = add_wta(mask, eps=mask_eps)
    mask = mask[0]
    if mask.shape[-1] != num_bins:
        mask = mask.transpose()
    return mask


def run(args):
    steer_vector = np.load(args.steer_vector)
    logger.info(f"Shape of the steer vector: {steer_vector.shape}")
    num_doa, _, _ = steer_vector.shape
    min_doa, max_doa = str2tuple(args.doa_range)
    if args.output == "radian":
        angles = np.linspace(min_doa * np.pi / 180, max_doa * np.pi / 180, num_doa + 1)
    else:
        angles = np.linspace(min_doa, max_doa, num_doa + 1)
    waves = WaveReader(args.wav_scp)
    readers = [NumpyReader(scp) for scp in args.mask_scp.split(",")] if args.mask_scp else None
    online = args.chunk_len > 0 and args.look_back > 0
    if online:
        logger.info(f"Set up in online mode: chunk_len = {args.chunk_len}, look_back = {args.look_back}")
    srp_pair = None
    if args.backend == "srp":
        srp_pair = parse_srp_pair(args.srp_pair)
        logger.info(f"Choose srp-based algorithm, srp pair is {srp_pair}")
    set_torch_free(args, None)  # the engine brings its own buffers and stream
    engine = BatchLocalizer(backend=args.backend, steer_vector=steer_vector, srp_pair=srp_pair,
                            chunk_len=args.chunk_len if online else -1, look_back=args.look_back,
                            **stft_kwargs(args))
    with open(args.doa_scp, "w") as doa_out:

        def flush(pending):
            results = engine.run([s for _, s, _ in pending], [m for _, _, m in pending])
            for (key, _, _), idx, st in zip(pending, results, engine.status):
                if st != _ffi.NUM_OK:
                    logger.warning(f"{key}: eigen-solve status {st} in some bin (zero or non-finite covariance)")
                doa = [float(i) if args.output == "index" else angles[i] for i in idx]
                if not online:
                    logger.info(f"Processing utterance {key}: {doa[0]:.4f}")
                doa_out.write(f"{key}\t" + " ".join(f"{d:.4f}" for d in doa) + "\n")
            return len(pending)

        def utterances():
            for key in waves.index_keys:
                if online:
                    logger.info(f"Processing utterance {key}...")
                yield key, read_samples(waves, key), load_mask(readers, key, args.mask_eps, n_fft(args) // 2 + 1)

        done = run_batches(utterances(), args.batch_utts, flush)
    engine.close()
    logger.info(f"Processing {done} utterance done")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to ML/SRP based sound souce localization (SSL)."
        "Also see scripts/sptk/compute_steer_vector.py",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Multi-channel wave rspecifier")
    parser.add_argument("steer_vector", type=str,
                        help="Pre-computed steer vector in each directions (in shape A x M x F, A: number "
                        "of DoAs, M: microphone number, F: FFT bins)")
    parser.add_argument("doa_scp", type=str, help="Wspecifier for estimated DoA")
    parser.add_argument("--backend", type=str, default="ml", choices=["ml", "srp", "music"],
                        help="Which algorithm to choose for SSL")
    parser.add_argument("--srp-pair", type=str, default="",
                        help="Microphone index pair to compute srp response")
    parser.add_argument("--doa-range", type=str, default="0,360", help="DoA range")
    parser.add_argument("--mask-scp", type=str, default="",
                        help="Rspecifier for TF-masks in numpy format")
    parser.add_argument("--output", type=str, default="degree", choices=["radian", "degree", "index"],
                        help="Output type of the DoA")
    parser.add_argument("--mask-eps", type=float, default=-1,
                        help="Value of eps used in masking winner-take-all")
    parser.add_argument("--chunk-len", type=int, default=-1,
                        help="Number frames per chunk (for online setups)")
    parser.add_argument("--look-back", type=int, default=125,
                        help="Number of frames to look back (for online setups)")
    parser.add_argument("--batch-utts", type=int, default=16,
                        help="[setk_amd] utterances per batched call")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
