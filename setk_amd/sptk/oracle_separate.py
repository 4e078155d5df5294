#!/usr/bin/env python
"""
Oracle speech separation (IAM / IBM / IRM / PSM from the speakers' references) on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/oracle_separate.py`` (same positional arguments, options
and defaults, :86-119; ``{dump_dir}/spk{k}/{key}.wav`` PCM_16).  The reference transforms the
mixture and every reference with librosa, forms the masks in numpy and inverts one speaker at a
time; this front end hands batches of WAVE SAMPLES to ``engine.BatchOracleSeparator``: the mixture
and its K references go up once per batch, one fused launch runs the K + 1 transforms of a frame
and stores the K masked spectra, one launch inverts them all, the waves come down once.
--skip-existing resumes.  At most 8 references.
"""
import argparse
import os
from contextlib import closing

import numpy as np

from setk_amd import _ffi
from setk_amd.dist import Shard
from setk_amd.engine import BatchOracleSeparator
from setk_amd.engine.tfmask import oracle_masks
from setk_amd.libs.data_handler import WaveReader
from setk_amd.libs.opts import StftParser, strtobool
from setk_amd.libs.utils import get_logger
from setk_amd.libs.wavio import write_pcm16
from setk_amd.sptk._common import complete_wav, deal, finish, read_samples, run_batches, set_torch_free, stft_kwargs

logger = get_logger(__name__)


def compute_mask(mixture, targets_list, mask_type):
    """The reference's module-level function on stored spectra (oracle_separate.py:19-45): the list
    of masks, float32 like complex64 spectra."""
    return oracle_masks(mask_type, np.asarray(mixture), [np.asarray(t) for t in targets_list])


def run(args):
    logger.info(f"Using mask: {args.mask.upper()}")
    with closing(Shard()) as shard:
        reader = WaveReader(args.mix_scp, sr=args.sr)
        ref_scps = args.ref_scp.split(",")
        logger.info(f"Number of speakers: {len(ref_scps)}")
        if len(ref_scps) > _ffi.TFMASK_MAX_TARGETS:
            raise _ffi.SetkUnsupported(f"at most {_ffi.TFMASK_MAX_TARGETS} targets, got {len(ref_scps)}")
        targets = [WaveReader(scp, sr=args.sr) for scp in ref_scps]
        set_torch_free(args, shard)
        engine = BatchOracleSeparator(args.mask, keep_length=args.keep_length, pcm16=True,
                                      device=shard.device if shard.world > 1 else None, **stft_kwargs(args))

        def path(key, k):
            return os.path.join(args.dump_dir, f"spk{k + 1}", f"{key}.wav")

        with closing(engine):

            def flush(pending):
                outs = engine.run([(m, ts) for _, m, ts in pending])
                for (key, _, _), waves, status in zip(pending, outs, engine.status):
                    if status != _ffi.NUM_OK:
                        logger.warning(f"{key}: NaN / inf in a masked spectrum")
                    for k, wave in enumerate(waves):
                        os.makedirs(os.path.dirname(path(key, k)), exist_ok=True)
                        write_pcm16(path(key, k), wave, args.sr)
                return len(pending)

            def utterances():
                done = lambda key: all(complete_wav(path(key, k)) for k in range(len(targets)))  # noqa: E731
                args.dst_dir = args.dump_dir
                for key in deal(args, shard, reader, done):
                    if any(key not in t for t in targets):
                        logger.info(f"Skip utterance {key}, missing targets")
                        continue
                    yield key, read_samples(reader, key), [read_samples(t, key) for t in targets]

            num_utts = run_batches(utterances(), args.batch_utts, flush)
        finish(shard, num_utts, "Processed %d utterance")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to do oracle speech separation, using specified mask(IAM|IBM|IRM|PSM)",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("mix_scp", type=str, help="Location of mixture wave scripts in kaldi format")
    parser.add_argument("--ref-scp", type=str, required=True,
                        help="Reference speaker wave scripts in kaldi format, separated using ','")
    parser.add_argument("--dump-dir", type=str, default="sep", help="Location to dump seperated speakers")
    parser.add_argument("--mask", type=str, default="irm", choices=list(_ffi.ORACLE_MASKS),
                        help="Type of mask to use for speech separation")
    parser.add_argument("--sr", type=int, default=16000, help="Waveform data sample rate")
    parser.add_argument("--keep-length", type=strtobool, default=False,
                        help="If ture, keep result the same length as orginal")
    parser.add_argument("--batch-utts", type=int, default=16, help="[setk_amd] utterances per batched call")
    parser.add_argument("--skip-existing", type=strtobool, default=False,
                        help="[setk_amd] resume: utterances whose outputs already exist (complete) "
                             "are not processed again")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
