#!/usr/bin/env python
"""
Separate the target from a mixture with a given TF mask on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/wav_separate.py`` (same positional arguments, options and
defaults, :80-122; ``{dst_dir}/{key}.wav`` PCM_16).  The reference walks a SpectrogramReader, masks
the stored spectrogram in numpy and inverts with librosa; this front end hands batches of WAVE
SAMPLES and masks to ``engine.BatchMaskSeparator``: mixtures, phase references and masks go up once
per batch, one fused launch transforms and masks, one launch inverts, one scales and rounds to 16
bits, the waves come down once.  --skip-existing resumes.
"""
import argparse
import os
from contextlib import closing

from setk_amd import _ffi
from setk_amd.dist import Shard
from setk_amd.engine import BatchMaskSeparator
from setk_amd.libs.data_handler import NumpyReader, ScriptReader, WaveReader, WaveWriter
from setk_amd.libs.opts import StftParser, strtobool
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import complete_wav, deal, finish, read_samples, run_batches, set_torch_free, stft_kwargs

logger = get_logger(__name__)


def run(args):
    with closing(Shard()) as shard:
        reader = WaveReader(args.wav_scp, sr=args.sr)
        phase_reader = None
        if args.phase_ref:
            phase_reader = WaveReader(args.phase_ref, sr=args.sr)
            logger.info(f"Using phase reference from {args.phase_ref}")
        mask_reader = {"numpy": NumpyReader, "kaldi": ScriptReader}[args.fmt](args.mask_scp)
        set_torch_free(args, shard)
        engine = BatchMaskSeparator(keep_length=args.keep_length, mixed_norm=args.mixed_norm, pcm16=True,
                                    device=shard.device if shard.world > 1 else None, **stft_kwargs(args))
        with closing(engine), WaveWriter(args.dst_dir, sr=args.sr) as writer:

            def flush(pending):
                outs = engine.run([s for _, s, _, _ in pending], [m for _, _, m, _ in pending],
                                  None if phase_reader is None else [r for _, _, _, r in pending])
                for (key, _, _, _), wave, status in zip(pending, outs, engine.status):
                    if status != _ffi.NUM_OK:
                        logger.warning(f"{key}: NaN / inf in the masked spectrum")
                    writer.write_pcm16(key, wave)
                return len(pending)

            def utterances():
                for key in deal(args, shard, reader, lambda k: complete_wav(os.path.join(args.dst_dir, f"{k}.wav"))):
                    if key not in mask_reader:
                        continue
                    logger.info(f"Processing utterance {key}...")
                    yield (key, read_samples(reader, key), mask_reader[key],
                           None if phase_reader is None else read_samples(phase_reader, key))

            num_done = run_batches(utterances(), args.batch_utts, flush)
        finish(shard, num_done, f"Processed %d utterances over {len(reader):d}")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to separate target component from mixtures given Tf-masks",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Mixture wave scripts in kaldi format")
    parser.add_argument("mask_scp", type=str, help="Scripts of masks in kaldi's archive or numpy's ndarray")
    parser.add_argument("dst_dir", type=str, help="Location to dump separated wave files")
    parser.add_argument("--sr", type=int, default=16000, help="Waveform data sample rate")
    parser.add_argument("--phase-ref", type=str, default="", help="If assigned, use phase of it instead of mixture")
    parser.add_argument("--mask-format", dest="fmt", choices=["kaldi", "numpy"], default="kaldi",
                        help="Define format of masks, kaldi's archives or numpy's ndarray")
    parser.add_argument("--keep-length", type=strtobool, default=False,
                        help="If ture, keep result the same length as orginal")
    parser.add_argument("--use-mixed-norm", type=strtobool, default=True, dest="mixed_norm",
                        help="If true, keep norm of separated same as mixed one")
    parser.add_argument("--batch-utts", type=int, default=32, help="[setk_amd] utterances per batched call")
    parser.add_argument("--skip-existing", type=strtobool, default=False,
                        help="[setk_amd] resume: utterances whose output already exists (complete) "
                             "are not processed again")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
