#!/usr/bin/env python
"""
AuxIVA blind source separation on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/apply_auxiva.py`` (same positional arguments, options
and defaults, :82-102; one PCM_16 wav per source, ``{dst_dir}/{key}.src{n}.wav``).  The
reference walks a SpectrogramReader and runs the update rules as a python loop over epochs,
bins and sources; this front end hands batches of WAVE SAMPLES to
``engine.BatchSeparator``: the samples go up once per batch, the STFT, the epochs (float64,
--batch-utts utterances per launch), the inverse STFT of every source and the renorm to
max |samples| run on the GPU, the waveforms come down once.  Utterances are dealt over the
ranks of a ``python -m setk_amd.launch`` run by duration.

One deliberate difference (tests/PARITY_NOTES_AUXIVA.md): an utterance with a singular bin (a silent
or all-zero channel) is logged and skipped like apply_adaptive_beamformer.py:170-172 does;
the reference's run ends there with LinAlgError.
"""
import argparse
from contextlib import closing

import numpy as np

from setk_amd import _ffi
from setk_amd._ffi import SetkUnsupported
from setk_amd.dist import Shard
from setk_amd.engine import BatchSeparator
from setk_amd.libs.data_handler import WaveReader, WaveWriter
from setk_amd.libs.opts import StftParser
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import (finish, group_by_channels, read_samples, run_batches,
                                   set_torch_free, stft_kwargs)

logger = get_logger(__name__)

MAX_CHANNELS = 8


def auxiva(X, epochs=20):
    """auxiva() of the reference (apply_auxiva.py:24-57) on the device.
    Arguments:
        X: shape in N x T x F (complex; the device works on complex64 observations)
    Return
        Y: same shape as X, complex128
    Raises np.linalg.LinAlgError where the reference's solve does (a singular bin), ValueError
    on a bad shape, SetkUnsupported beyond 8 channels."""
    X = np.asarray(X)
    if X.ndim != 3 or 0 in X.shape or not np.iscomplexobj(X):
        raise ValueError("auxiva expects a complex array of shape N x T x F")
    if epochs < 0:
        raise ValueError("epochs must not be negative")
    N, T, F = X.shape
    if N > MAX_CHANNELS:
        raise SetkUnsupported(f"AuxIVA on the device needs 1 <= channels <= {MAX_CHANNELS} "
                              f"(got {N} channels)")
    ctx = _ffi.default_context()
    spec = np.ascontiguousarray(X, dtype=np.complex64)
    out = np.empty_like(spec)
    status = np.zeros(F, dtype=np.int32)
    ctx.auxiva(spec, N, T, F, int(epochs), out, status=status)
    if (status == _ffi.NUM_SINGULAR).any():
        raise np.linalg.LinAlgError("Singular matrix")
    if (status != _ffi.NUM_OK).any():
        raise np.linalg.LinAlgError("non-finite values in AuxIVA")
    return out.astype(np.complex128)


def run(args):
    with closing(Shard()) as shard:
        reader = WaveReader(args.wav_scp)  # 16 kHz tables like the reference (SpectrogramReader)
        set_torch_free(args, shard)
        engine = BatchSeparator(num_epochs=args.epochs, device=shard.device if shard.world > 1 else None,
                                pcm16=True, **stft_kwargs(args))
        with closing(engine), WaveWriter(args.dst_dir, sr=args.sr) as writer:

            def flush(pending):
                """--batch-utts utterances (grouped by channel count) per engine call."""
                done = 0
                for nch, items in group_by_channels(pending).items():
                    if nch > MAX_CHANNELS:
                        for key, _ in items:
                            logger.warning(f"{key}: skipped, AuxIVA on the device needs 1 <= channels "
                                           f"<= {MAX_CHANNELS} (got {nch} channels)")
                        continue
                    try:
                        outs = engine.run([s for _, s in items])
                    except SetkUnsupported as e:
                        for key, _ in items:
                            logger.warning(f"{key}: skipped, {e}")
                        continue
                    for (key, _), srcs, st in zip(items, outs, engine.status):
                        if srcs is None:
                            what = "LinAlgError (Singular matrix)" if st == _ffi.NUM_SINGULAR else "non-finite values"
                            logger.warning(f"{key}: Failed cause {what} in auxiva")
                            continue
                        for idx in range(srcs.shape[0]):
                            writer.write_pcm16(f"{key}.src{idx + 1}", srcs[idx])
                        done += 1
                return done

            def utterances():
                for key in shard.assign_by_duration(reader):
                    logger.info(f"Processing utterance {key}...")
                    yield key, read_samples(reader, key)

            num_done = run_batches(utterances(), args.batch_utts, flush)
        finish(shard, num_done, f"Processed %d utterances over {len(reader):d}")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to do AuxIVA bss algorithm",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Multi-channel wave scripts in kaldi format")
    parser.add_argument("dst_dir", type=str, help="Location to dump separated source files")
    parser.add_argument("--num-epochs", default=20, type=int, dest="epochs",
                        help="Number of epochs to run AuxIVA algorithm")
    parser.add_argument("--sr", type=int, default=16000, help="Waveform data sample rate")
    parser.add_argument("--batch-utts", type=int, default=16,
                        help="[setk_amd] utterances per batched AuxIVA call")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
