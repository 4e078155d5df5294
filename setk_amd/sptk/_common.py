"""
What the command lines share: the FFT size and the engines' STFT keywords, the torch-free
decision, the sample read, the batch loop, the deal of the utterances with its resume rules,
the closing tally and the table walk of the two mask estimators.  Plain functions; what is
particular to a tool (its flush, its log texts, its options) stays in the tool's file.

Log lines written here carry stacklevel=2: the record names the tool that called, as it did
when every tool had its own copy.
"""
import os

import numpy as np

from setk_amd import _ffi
from setk_amd.engine import Pcm16Frames, channels_and_size
from setk_amd.libs.utils import get_logger, nextpow2

logger = get_logger(__name__)


def n_fft(args):
    return nextpow2(args.frame_len) if args.round_power_of_two else args.frame_len


def stft_kwargs(args):
    """The STFT keywords every batch engine takes."""
    return dict(frame_len=args.frame_len, frame_hop=args.frame_hop, center=bool(args.center),
                window=args.window, round_power_of_two=bool(args.round_power_of_two))


def set_torch_free(args, shard, ok=True):
    """With the n_fft = 512 plan the engines bring their own buffers and stream, and a process
    (alone, or with the library's own collectives: shard None or torch_free_ok) then runs
    without torch unless the tool sees a reason in its inputs (`ok` false: e.g. more than 8
    channels, which go through torch tensors)."""
    if n_fft(args) == 512 and (shard is None or shard.torch_free_ok):
        _ffi.set_torch_free(ok)


def read_samples(reader, key, at_least_2d=False):
    """One 16-bit PCM file: its frames as stored (Pcm16Frames; the device converts and
    transposes them).  Anything else: the float samples of reader.read, N or C x N
    (at_least_2d: 1 x N for single-channel audio)."""
    pcm = reader.read_pcm16(key)
    if pcm is not None:
        return Pcm16Frames(pcm)
    samps = reader.read(key)
    return samps[None] if at_least_2d and samps.ndim == 1 else samps


def run_batches(items, batch_utts, flush):
    """Hand `items` to flush(list) in runs of batch_utts (at least one), the tail included;
    flush is never called with an empty list.  Returns the sum of what the flushes return."""
    size, done, pending = max(1, batch_utts), 0, []
    for item in items:
        pending.append(item)
        if len(pending) >= size:
            done += flush(pending)
            pending = []
    if pending:
        done += flush(pending)
    return done


def group_by_channels(pending):
    """{channel count: [(key, samples, ...), ...]} in order of first appearance: an engine call
    takes utterances of one channel count."""
    groups = {}
    for item in pending:
        groups.setdefault(channels_and_size(item[1])[0], []).append(item)
    return groups


def complete_wav(path):
    """True if `path` is a WAV file whose size is what its RIFF / data chunk headers say (the
    writer renames finished files into place; this also rejects files truncated by other
    means, e.g. a full disk under an older version)."""
    try:
        size = os.path.getsize(path)
        if size <= 44:
            return False
        with open(path, "rb") as f:
            head = f.read(44)
    except OSError:
        return False
    if len(head) < 44 or head[:4] != b"RIFF" or head[8:12] != b"WAVE" or head[36:40] != b"data":
        return False
    riff = int.from_bytes(head[4:8], "little")
    data = int.from_bytes(head[40:44], "little")
    return riff + 8 == size and data + 44 == size


def complete_npy(path):
    """True if `path` loads as a .npy file (header and size agree)."""
    try:
        np.load(path, mmap_mode="r")
        return True
    except (OSError, ValueError):
        return False


def deal(args, shard, reader, done):
    """This rank's utterances; done(key) tells whether that key's output is already complete.
    Default: the deal is computed on the FULL table (every rank keeps the utterances it had)
    and --skip-existing then drops what is already there.  --requeue (a re-launch after a
    failure): the missing utterances are found first -- by every rank, from the same directory
    listing: nobody writes before the barrier below -- and only they are dealt, so the
    leftovers of a rank that died are shared by all ranks instead of waiting for it."""
    skip = getattr(args, "skip_existing", False)
    requeue = skip and getattr(args, "requeue", False) and shard.world > 1
    keys = list(reader.index_keys) if requeue else shard.assign_by_duration(reader)
    if not skip:
        return keys
    left = [k for k in keys if not done(k)]
    if len(left) != len(keys):
        logger.info(f"--skip-existing: {len(keys) - len(left)} of {len(keys)} utterances already "
                    f"in {args.dst_dir}", stacklevel=2)
    if requeue:
        shard.barrier()
        return shard.assign_by_duration(reader, keys=left)
    return left


def finish(shard, num_done, message):
    """The closing tally, the same collectives on every rank: barrier, sum of num_done over
    the ranks, and on rank 0 the tool's line (`message` with one %d for the sum).  The caller
    closes the shard in its finally."""
    shard.barrier()
    if shard.world > 1:
        num_done = int(round(shard.sum_counts([num_done])[0]))
    if shard.rank == 0:
        logger.info(message, num_done, stacklevel=2)


def num_frames(reader, key, args, n_fft):
    """STFT frames of an utterance from its wave header (librosa's count: 1 + N // hop with
    centring, 1 + (N - n_fft) // hop without); pipes and globs are decoded for their length."""
    n = reader.peek_nsamps(key)
    if n is None:
        n = reader.read(key).shape[-1]
    if args.center:
        return 1 + n // args.frame_hop
    return 1 + (n - n_fft) // args.frame_hop


def walk(shard, reader, dst_dir, draws):
    """The table walk of the mask estimators: yields (key, mine) in table order.

    The random start comes out of ONE generator that the reference advances utterance by
    utterance in table order.  With `draws` and the table dealt over several ranks every rank
    walks the whole table and DISCARDS the draws of the utterances that are not its own
    (mine false; K x F x T doubles each, T from the wave header), so an N-rank run starts
    every utterance exactly as the one-process run does.  Without draws a rank sees its own
    keys only.  What exists is decided once, before any rank writes: the walk of every rank
    must skip the same utterances (the reference does not draw for an utterance it skips)."""
    mine = shard.assign_by_duration(reader)
    keys = list(reader.index_keys) if (draws and shard.world > 1) else mine
    own = set(mine)
    existing = {key for key in keys if os.path.exists(os.path.join(dst_dir, f"{key}.npy"))}
    shard.barrier()
    for key in keys:
        if key not in existing:
            yield key, key in own
        elif key in own:
            logger.info(f"Training utterance {key} ... Skip", stacklevel=2)
