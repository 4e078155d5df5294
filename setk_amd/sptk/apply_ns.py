#!/usr/bin/env python
"""
Single-channel OM-LSA noise suppression (iMCRA) on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/apply_ns.py`` (same positional arguments, options and
defaults, :53-79; ``{dst_dir}/{key}.wav`` PCM_16 or ``{dst_dir}/{key}.npy`` float64 gains).  The
reference walks a SpectrogramReader and runs the recursion as a python loop over frames with a
numerical integral per spectrogram cell (about 0.3 ms per cell); this front end hands batches of
WAVE SAMPLES to ``engine.BatchNoiseSuppressor``: the samples go up once per batch, the STFT, the
recursion (float64, one workgroup per utterance, --batch-utts utterances per launch) and the
inverse STFT run on the GPU, the results come down once.  Utterances are dealt over the ranks
of a ``python -m setk_amd.launch`` run by duration; --skip-existing resumes.

What differs on purpose is listed in tests/PARITY_NOTES_NS.md (digital silence stays finite).
"""
import argparse
import os
from contextlib import closing

from setk_amd.dist import Shard
from setk_amd.engine import BatchNoiseSuppressor, channels_and_size
from setk_amd.libs.data_handler import NumpyWriter, WaveReader, WaveWriter
from setk_amd.libs.ns import iMCRA
from setk_amd.libs.opts import StftParser, strtobool
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import (complete_npy, complete_wav, deal, finish, read_samples, run_batches,
                                   set_torch_free, stft_kwargs)

logger = get_logger(__name__)


def run(args):
    if args.sr != 16000:
        raise ValueError("Now only support audio in 16kHz")
    if args.conf:
        import yaml
        with open(args.conf, "r") as conf:
            suppressor = iMCRA(**(yaml.full_load(conf) or {}))
    else:
        suppressor = iMCRA()
    wave = args.output == "wave"

    def complete(key):
        if wave:
            return complete_wav(os.path.join(args.dst_dir, f"{key}.wav"))
        return complete_npy(os.path.join(args.dst_dir, f"{key}.npy"))

    with closing(Shard()) as shard:
        reader = WaveReader(args.wav_scp)  # 16 kHz tables like the reference (SpectrogramReader)
        set_torch_free(args, shard)  # the engine brings its own buffers and stream
        engine = BatchNoiseSuppressor(suppressor, output=args.output, pcm16=True,
                                      device=shard.device if shard.world > 1 else None, **stft_kwargs(args))
        with closing(engine), (WaveWriter(args.dst_dir, sr=args.sr) if wave else NumpyWriter(args.dst_dir)) as writer:

            def flush(pending):
                done = 0
                ok = []
                for key, samps in pending:
                    if channels_and_size(samps)[0] != 1:
                        logger.warning(f"{key}: skipped, noise suppression takes single-channel audio "
                                       f"(got {channels_and_size(samps)[0]} channels)")
                    else:
                        ok.append((key, samps))
                if not ok:
                    return 0
                outs = engine.run([s for _, s in ok])
                for (key, _), res in zip(ok, outs):
                    if res is None:
                        logger.warning(f"{key}: skipped, non-finite values in the samples")
                        continue
                    if wave:
                        writer.write_pcm16(key, res)  # rounded on the device by the writer's rule
                    else:
                        writer.write(key, res)
                    done += 1
                return done

            def utterances():
                for key in deal(args, shard, reader, complete):
                    logger.info(f"Processing utterance {key}...")
                    yield key, read_samples(reader, key)

            num_done = run_batches(utterances(), args.batch_utts, flush)
        finish(shard, num_done, "Processed %d utterances done")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to do single channel noise suppression",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Noisy audio scripts in Kaldi format")
    parser.add_argument("dst_dir", type=str, help="Location to dump enhanced audio or gain coefficients")
    parser.add_argument("--conf", type=str, default="", help="Yaml configurations for OMLSA")
    parser.add_argument("--output", type=str, choices=["gain", "wave"], default="wave",
                        help="Output type of the command")
    parser.add_argument("--sr", type=int, default=16000, help="Waveform data sample frequency")
    parser.add_argument("--batch-utts", type=int, default=32,
                        help="[setk_amd] utterances per batched call (one workgroup each)")
    parser.add_argument("--skip-existing", type=strtobool, default=False,
                        help="[setk_amd] resume: utterances whose output already exists (complete) "
                             "are not processed again")
    parser.add_argument("--requeue", type=strtobool, default=False,
                        help="[setk_amd] with --skip-existing: deal only the MISSING utterances over the "
                             "ranks (what `python -m setk_amd.launch` passes on its retries)")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
