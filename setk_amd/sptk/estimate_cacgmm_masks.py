#!/usr/bin/env python
"""
Speaker mask estimation with the CACGMM model on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/estimate_cacgmm_masks.py`` (same positional arguments,
options, defaults, outputs {dst_dir}/{key}.npy float32 K x T x F for every K, :62; skip-if-exists
:38; an utterance whose eigendecomposition fails is logged as Failed and the run goes on,
:64-65).  The start is the reference's: --init-mask, the CGMM-like start (--cgmm-init true with
two classes) or the seeded random posteriors (--seed), drawn on the host from numpy's legacy
generator in table order exactly as the reference does.  The whole EM runs in one launch of
csrc/cacgmm.hip; --solve-permu (default true) aligns the classes over frequency on the host
(libs/cluster.permu_aligner).

--batch-utts N > 1 [setk_amd] hands N utterances at a time to engine.CacgmmEstimator (n_fft =
512, no --init-mask): one STFT launch straight into the kernel's layout and one EM launch per
batch.  That STFT (stft_binmajor_kernel) and the stand-alone one behind SpectrogramReader are two
kernels over the same float32 butterflies; they gave the same bits where the tests compare them,
but nothing holds that for every shape, so the default stays one utterance at a time:
CacgmmTrainer on SpectrogramReader's spectrogram.
"""
import argparse
from contextlib import closing

import numpy as np

from setk_amd import _ffi
from setk_amd.dist import Shard
from setk_amd.libs.cluster import CacgmmTrainer, permu_aligner
from setk_amd.libs.data_handler import (NumpyReader, NumpyWriter, ScriptReader, SpectrogramReader,
                                        WaveReader)
from setk_amd.libs.opts import StftParser, strtobool
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import finish, n_fft, num_frames, read_samples, run_batches, stft_kwargs, walk

logger = get_logger(__name__)


def build_parser():
    parser = argparse.ArgumentParser(
        description="Speaker masks estimation using Complex Angular Central Gaussian Mixture Model (CACGMM)",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Multi-channel wave scripts in kaldi format")
    parser.add_argument("dst_dir", type=str, help="Where to dump estimated speech masks")
    parser.add_argument("--num-iters", type=int, default=50, help="Number of iterations to train Cacgmm")
    parser.add_argument("--num-classes", type=int, default=2,
                        help="Number of the cluster used in cacgmm model")
    parser.add_argument("--seed", type=int, default=777, help="Random seed for initialization")
    parser.add_argument("--init-mask", type=str, default="", dest="init_mask",
                        help="Mask scripts for cacgmm initialization")
    parser.add_argument("--cgmm-init", type=strtobool, default=False,
                        help="For 2 classes, using the cgmm init way")
    parser.add_argument("--solve-permu", type=strtobool, default=True,
                        help="If true, solving permutation problems")
    parser.add_argument("--update-alpha", type=strtobool, default=True,
                        help="If true, update alpha in M-step")
    parser.add_argument("--mask-format", type=str, dest="fmt", default="numpy",
                        choices=["kaldi", "numpy"], help="Mask storage format")
    parser.add_argument("--batch-utts", type=int, default=1,
                        help="[setk_amd] utterances per EM launch (above 1: n_fft = 512, no --init-mask)")
    return parser


def _finish(masks, args):
    """K x F x T posteriors -> what the reference writes (:54-62)."""
    masks = np.transpose(masks, (0, 2, 1))
    if args.solve_permu:
        masks = permu_aligner(masks)
        logger.info("Permutation alignment done on each frequency")
    return masks.astype(np.float32)


def train_table(args, reader, init_reader, shard, dst_dir, write, trainer_cls=CacgmmTrainer):
    """The loop of estimate_cacgmm_masks.py:37-67 over this rank's share of the table; returns
    how many utterances were trained.

    The random start comes out of ONE generator that the reference advances utterance by
    utterance in table order (:28, cluster.py:509-511).  With the table dealt over several ranks
    every rank walks the whole table and DISCARDS the draws of the utterances that are not its
    own (K x F x T doubles each, T from the wave header), so an N-rank run starts every
    utterance exactly as the one-process run does.  No draw is made for a key that has an init
    mask, and none under --cgmm-init true with two classes (cluster.py:496)."""
    K = args.num_classes
    num_bins = n_fft(args) // 2 + 1
    num_done = 0
    for key, mine in walk(shard, reader, dst_dir, draws=not (args.cgmm_init and K == 2)):
        has_init = bool(init_reader) and key in init_reader
        if not mine:
            if not has_init:
                np.random.uniform(size=K * num_bins * num_frames(reader, key, args, n_fft(args)))
            continue
        stft = reader[key]
        if stft.ndim == 2:
            stft = stft[None]
        init_mask = None
        if has_init:
            # K x T x F => K x F x T (:42-43)
            init_mask = np.transpose(init_reader[key], (0, 2, 1))
            logger.info("Using external mask to initialize cacgmm")
        try:
            trainer = trainer_cls(stft, K, gamma=init_mask, cgmm_init=bool(args.cgmm_init),
                                  update_alpha=bool(args.update_alpha))
            masks = _finish(trainer.train(args.num_iters), args)
            num_done += 1
            write(key, masks)
            logger.info(f"Training utterance {key} ... Done")
        except np.linalg.LinAlgError:
            logger.warning(f"Training utterance {key} ... Failed")
    return num_done


def train_batched(args, reader, shard, dst_dir, write):
    """--batch-utts N > 1: waves in, masks out, N utterances per STFT + EM launch."""
    from setk_amd.engine import CacgmmEstimator
    K = args.num_classes
    cgmm_init = bool(args.cgmm_init) and K == 2
    est = CacgmmEstimator(**dict(stft_kwargs(args), round_power_of_two=True), num_classes=K,
                          num_iters=args.num_iters, update_alpha=bool(args.update_alpha), cgmm_init=cgmm_init,
                          device=shard.device if shard.world > 1 else None)

    def flush(pending):
        num_done = 0
        starts = None if cgmm_init else [g for _, _, g in pending]
        masks, status = est.estimate([s for _, s, _ in pending], starts, return_status=True)
        for (key, _, _), m, st in zip(pending, masks, status):
            if st != 0 or not np.isfinite(m).all():
                logger.warning(f"Training utterance {key} ... Failed")
                continue
            write(key, _finish(np.transpose(m, (0, 2, 1)), args))
            logger.info(f"Training utterance {key} ... Done")
            num_done += 1
        return num_done

    def utterances():
        for key, mine in walk(shard, reader, dst_dir, draws=not cgmm_init):
            T = num_frames(reader, key, args, n_fft(args))
            g0 = None
            if not cgmm_init:  # (every rank draws for every utterance it walks; its own are kept)
                g0 = np.random.uniform(size=[K, est.num_bins, T])
                if mine:
                    g0 = g0 / np.sum(g0, 0, keepdims=True)
                    logger.info(f"Random initialized, num_classes = {K}")
            if mine:
                yield key, read_samples(reader, key, at_least_2d=True), g0

    with closing(est):
        return run_batches(utterances(), args.batch_utts, flush)


def run(args):
    # estimate_cacgmm_masks.py:28 of the reference: the random start is drawn from numpy's legacy
    # global generator, seeded once per run
    np.random.seed(args.seed)
    if not 2 <= args.num_classes <= 4:
        raise _ffi.SetkUnsupported(f"--num-classes {args.num_classes}: the device EM implements 2 .. 4")
    with closing(Shard()) as shard:
        with NumpyWriter(args.dst_dir) as writer:
            if args.batch_utts > 1 and n_fft(args) == 512 and not args.init_mask:
                reader = WaveReader(args.wav_scp)
                num_done = train_batched(args, reader, shard, args.dst_dir, writer.write)
            else:
                reader = SpectrogramReader(args.wav_scp, frame_len=args.frame_len, frame_hop=args.frame_hop,
                                           round_power_of_two=args.round_power_of_two, window=args.window,
                                           center=args.center, transpose=False)
                MaskReader = {"numpy": NumpyReader, "kaldi": ScriptReader}
                init_reader = MaskReader[args.fmt](args.init_mask) if args.init_mask else None
                num_done = train_table(args, reader, init_reader, shard, args.dst_dir, writer.write)
        finish(shard, num_done, f"Train %d utterances over {len(reader):d}")


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
