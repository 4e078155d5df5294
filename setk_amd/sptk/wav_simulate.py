#!/usr/bin/env python
"""
Audio data simulation on the MI355X: reverberate, mix at an SDR / SNR, normalise the peak.

Drop-in for funcwj/setk ``scripts/sptk/wav_simulate.py`` (same arguments and defaults, :345-421;
the same "Time cost / RTF" line; ``mix`` and ``--dump-ref-dir/{noise,clean,spk1..}/basename`` as
PCM_16).  The reference runs one mixture per process and convolves on one CPU core; here the
convolutions are a partitioned overlap-save convolution on the GPU and the mixing runs there too
(``engine.BatchSimulator``).

One extension, ``--cmd-list FILE``: every non-empty line of FILE is one reference argument list
(split with shlex, parsed by the same parser).  The lines are batched (--batch-utts mixtures per
library call), dealt over the ranks of a ``python -m setk_amd.launch`` run by the length of their
first speaker, and --skip-existing resumes: a line whose mixture file is complete is not run again.

What is kept of the reference's quirks is listed in tests/PARITY_NOTES_SIMU.md.
"""
import argparse
import os
import pathlib
import shlex
import time
from contextlib import closing

from setk_amd import _ffi
from setk_amd.dist import Shard
from setk_amd.engine import BatchSimulator
from setk_amd.libs import wavio
from setk_amd.libs.opts import strtobool
from setk_amd.libs.simu import finish as finish_result
from setk_amd.libs.simu import load_recipe
from setk_amd.libs.utils import get_logger, write_wav
from setk_amd.sptk._common import complete_wav, deal, finish, run_batches

logger = get_logger(__name__)


def dump(args, mix, spk_ref, noise):
    """The output layout of the reference's run (:326-341)."""
    write_wav(args.mix, mix, sr=args.sr)
    if args.dump_ref_dir:
        basename = os.path.basename(args.mix)
        ref_dir = pathlib.Path(args.dump_ref_dir)
        ref_dir.mkdir(parents=True, exist_ok=True)
        if noise is not None:
            write_wav(str(ref_dir / "noise" / basename), noise, sr=args.sr)
        if len(spk_ref) == 1:
            # (the reference hands the LIST over, :338, and its writer's .astype raises: written here)
            write_wav(str(ref_dir / "clean" / basename), spk_ref[0], sr=args.sr)
        else:
            for i, s in enumerate(spk_ref):
                write_wav(str(ref_dir / f"spk{i + 1}" / basename), s, sr=args.sr)


def run_one(args, engine):
    start = time.time()
    mix, spk_ref, noise = finish_result(engine.run([load_recipe(args)])[0])
    utt_dur = mix.shape[-1] / float(args.sr)
    time_cost = float(time.time() - start)
    print(f"Time cost: {time_cost:.4f}s, Utterance duration: {utt_dur:.2f}s, "
          f"RTF = {time_cost / utt_dur:.4f}", flush=True)
    dump(args, mix, spk_ref, noise)


class CmdTable(object):
    """The lines of a --cmd-list file as the table the shared deal walks: keys are line numbers,
    the weight of a line is the length of its first speaker (from the wave header)."""

    def __init__(self, path, parser):
        self.args = {}
        with open(path, "r") as fd:
            for n, line in enumerate(fd, 1):
                if not line.strip():
                    continue
                sub = parser.parse_args(shlex.split(line))
                if sub.cmd_list or not sub.mix:
                    raise ValueError(f"{path}:{n}: a line is one argument list with its mix, without --cmd-list")
                self.args[str(n)] = sub
        self.index_keys = list(self.args)

    def peek_nsamps(self, key):
        try:
            with open(self.args[key].src_spk.split(",")[0], "rb") as fd:
                info = wavio.read_header(fd)
            return info["data_bytes"] // max(1, info["align"])
        except (OSError, wavio.WaveFormatError):
            return None


def run_list(args, parser):
    table = CmdTable(args.cmd_list, parser)
    args.dst_dir = "place"  # (the deal's log line: every line names its own mix)
    with closing(Shard()) as shard:
        if shard.torch_free_ok:
            _ffi.set_torch_free(True)  # the engine brings its own buffers and stream
        engine = BatchSimulator(device=shard.device if shard.world > 1 else None)
        with closing(engine):

            def flush(pending):
                start = time.time()
                outs = engine.run([r for _, r in pending])
                time_cost = float(time.time() - start)
                utt_dur = sum(o.mix.shape[-1] for o in outs) / float(args.sr)
                print(f"Time cost: {time_cost:.4f}s, Utterance duration: {utt_dur:.2f}s, "
                      f"RTF = {time_cost / utt_dur:.4f}", flush=True)
                for (sub, _), o in zip(pending, outs):
                    dump(sub, *finish_result(o))
                return len(pending)

            def mixtures():
                for key in deal(args, shard, table, lambda k: complete_wav(table.args[k].mix)):
                    sub = table.args[key]
                    yield sub, load_recipe(sub)

            num_done = run_batches(mixtures(), args.batch_utts, flush)
        finish(shard, num_done, "Simulated %d mixtures done")


def run(args, parser):
    if args.cmd_list:
        return run_list(args, parser)
    if not args.mix:
        parser.error("the following arguments are required: mix (or --cmd-list)")
    _ffi.set_torch_free(True)
    with closing(BatchSimulator()) as engine:
        run_one(args, engine)


def build_parser():
    parser = argparse.ArgumentParser(description="Command to do audio data simulation",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("mix", type=str, nargs="?", default="", help="Audio to output")
    parser.add_argument("--dump-ref-dir", type=str, default="", help="Directory of the reference audio to output")
    parser.add_argument("--src-spk", type=str, default="", help="Source speakers, e.g., spk1.wav,spk2.wav")
    parser.add_argument("--src-rir", type=str, default="", help="RIRs for each source speakers")
    parser.add_argument("--src-sdr", type=str, default="", help="SDR for each speakers (if needed)")
    parser.add_argument("--src-begin", type=str, default="", help="Begining samples on the mixture utterances")
    parser.add_argument("--point-noise", type=str, default="", help="Add pointsource noises")
    parser.add_argument("--point-noise-rir", type=str, default="",
                        help="RIRs of the pointsource noises (if needed)")
    parser.add_argument("--point-noise-snr", type=str, default="", help="SNR of the pointsource noises")
    parser.add_argument("--point-noise-begin", type=str, default="",
                        help="Begining samples of the pointsource noises on the mixture utterances (if needed)")
    parser.add_argument("--point-noise-offset", type=str, default="",
                        help="Add from the offset position of the pointsource noise")
    parser.add_argument("--point-noise-repeat", type=strtobool, default="false",
                        help="Repeat the pointsource noise or not")
    parser.add_argument("--isotropic-noise", type=str, default="", help="Add isotropic noises")
    parser.add_argument("--isotropic-noise-snr", type=str, default="", help="SNR of the isotropic noises")
    parser.add_argument("--isotropic-noise-offset", type=int, default=0,
                        help="Add noise from the offset position of the isotropic noise")
    parser.add_argument("--dump-channel", type=int, default=-1, help="Index of the channel to dump out (-1 means all)")
    parser.add_argument("--norm-factor", type=float, default=0.9, help="Normalization factor of the final output")
    parser.add_argument("--sr", type=int, default=16000, help="Value of the sample rate")
    parser.add_argument("--cmd-list", type=str, default="",
                        help="[setk_amd] a file with one argument list per line: the mixtures are batched on the GPU")
    parser.add_argument("--batch-utts", type=int, default=32, help="[setk_amd] --cmd-list: mixtures per batched call")
    parser.add_argument("--skip-existing", type=strtobool, default=False,
                        help="[setk_amd] --cmd-list resume: lines whose mix already exists (complete) are not run again")
    parser.add_argument("--requeue", type=strtobool, default=False,
                        help="[setk_amd] with --skip-existing: deal only the MISSING lines over the ranks "
                             "(what `python -m setk_amd.launch` passes on its retries)")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.cmd_list and not args.src_spk:
        parser.error("the following arguments are required: --src-spk")
    run(args, parser)


if __name__ == "__main__":
    main()
