"""
setk_amd/sptk/_common.py, the plumbing the command lines share, on the host alone: the batch
loop, the grouping by channel count, the FFT size, the deal with its resume rules and the table
walk of the mask estimators.  No library is loaded and nothing runs on a device.
"""
import argparse
import wave

import numpy as np
import pytest

from setk_amd.dist import assign_keys
from setk_amd.engine import Pcm16Frames
from setk_amd.sptk import _common as c


# ---- the batch loop ----
@pytest.mark.parametrize("size, want", [(3, [3, 3, 1]), (1, [1] * 7), (0, [1] * 7), (-2, [1] * 7)])
def test_run_batches_flushes_in_order_and_sums(size, want):
    seen = []

    def flush(items):
        seen.append(list(items))
        return 10 * len(items) + 1

    total = c.run_batches(iter(range(7)), size, flush)
    assert [len(b) for b in seen] == want
    assert [i for b in seen for i in b] == list(range(7))
    assert total == 10 * 7 + len(want)


def test_run_batches_never_flushes_an_empty_list():
    def flush(items):
        raise AssertionError(f"flush({items!r}) on an empty input")

    for size in (3, 1, 0, -2):
        assert c.run_batches([], size, flush) == 0
    # ... nor after a last full batch
    calls = []
    assert c.run_batches("abcdef", 3, lambda items: calls.append(list(items)) or 1) == 2
    assert calls == [list("abc"), list("def")]


def test_group_by_channels_keeps_the_order_inside_a_group():
    pending = [("p2", Pcm16Frames(np.zeros((50, 2), np.int16))),
               ("f1", np.zeros(40, np.float32)),
               ("r1", np.zeros((1, 30), np.float32)),
               ("f2", np.zeros((2, 60), np.float32)),
               ("p1", Pcm16Frames(np.zeros((70, 1), np.int16)))]
    groups = c.group_by_channels(pending)
    assert list(groups) == [2, 1]  # (first appearance)
    assert [k for k, _ in groups[1]] == ["f1", "r1", "p1"]
    assert [k for k, _ in groups[2]] == ["p2", "f2"]
    assert groups[1][0][1] is pending[1][1]  # the items themselves, untouched


@pytest.mark.parametrize("frame_len, rpt, want", [(400, True, 512), (400, False, 400), (512, True, 512),
                                                  (512, False, 512), (513, True, 1024)])
def test_n_fft(frame_len, rpt, want):
    args = argparse.Namespace(frame_len=frame_len, round_power_of_two=rpt, frame_hop=160, center=1, window="hann")
    assert c.n_fft(args) == want
    assert c.stft_kwargs(args) == dict(frame_len=frame_len, frame_hop=160, center=True, window="hann",
                                       round_power_of_two=rpt)


# ---- the deal ----
class _Reader(object):
    nsamps = {"a": 900, "b": 300, "c": 700, "d": 500, "e": 200, "f": 400}

    def __init__(self):
        self.index_keys = list(self.nsamps)

    def peek_nsamps(self, key):
        return self.nsamps[key]


class _Shard(object):
    """rank / world, a barrier that counts, the duration deal of dist.Shard."""

    def __init__(self, rank=0, world=1):
        self.rank, self.world, self.barriers = rank, world, 0

    def barrier(self):
        self.barriers += 1

    def assign_by_duration(self, reader, keys=None):
        keys = list(reader.index_keys if keys is None else keys)
        return assign_keys(keys, self.rank, self.world, [reader.peek_nsamps(k) for k in keys])


def _write_wav(path, nsamps=100):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(b"\0\0" * nsamps)


def _outputs(tmp_path):
    """a, c complete and b truncated as .wav; a, c complete and b, d unreadable as .npy."""
    for key in "abc":
        _write_wav(tmp_path / f"{key}.wav")
        np.save(tmp_path / f"{key}.npy", np.zeros((4, 5)))
    whole = (tmp_path / "b.wav").read_bytes()
    (tmp_path / "b.wav").write_bytes(whole[:-10])
    whole = (tmp_path / "b.npy").read_bytes()
    (tmp_path / "b.npy").write_bytes(whole[:-10])
    (tmp_path / "d.npy").write_bytes(b"not an array at all")

    def wav_done(key):
        return c.complete_wav(str(tmp_path / f"{key}.wav"))

    def npy_done(key):
        return c.complete_npy(str(tmp_path / f"{key}.npy"))

    return wav_done, npy_done


def _args(tmp_path, **kw):
    return argparse.Namespace(dst_dir=str(tmp_path), **kw)


def test_deal_without_skip_existing_is_the_plain_deal(tmp_path):
    wav_done, _ = _outputs(tmp_path)
    reader = _Reader()
    for args in (_args(tmp_path), _args(tmp_path, skip_existing=False, requeue=True)):
        assert c.deal(args, _Shard(), reader, wav_done) == list("abcdef")
        for rank in range(2):
            shard = _Shard(rank, 2)
            assert c.deal(args, shard, reader, wav_done) == shard.assign_by_duration(reader)
            assert shard.barriers == 0


def test_deal_skip_existing_drops_only_complete_outputs(tmp_path):
    wav_done, npy_done = _outputs(tmp_path)
    assert [k for k in "abcdef" if wav_done(k)] == ["a", "c"]
    assert [k for k in "abcdef" if npy_done(k)] == ["a", "c"]
    args = _args(tmp_path, skip_existing=True, requeue=False)
    for done in (wav_done, npy_done):
        assert c.deal(args, _Shard(), _Reader(), done) == list("bdef")  # (b truncated, d unreadable: kept)
    # one rank with --requeue: nothing to share, no barrier
    shard = _Shard()
    assert c.deal(_args(tmp_path, skip_existing=True, requeue=True), shard, _Reader(), wav_done) == list("bdef")
    assert shard.barriers == 0


def test_deal_requeue_shares_exactly_the_missing_keys(tmp_path):
    wav_done, _ = _outputs(tmp_path)
    args = _args(tmp_path, skip_existing=True, requeue=True)
    reader, got = _Reader(), []
    for rank in range(2):
        shard = _Shard(rank, 2)
        mine = c.deal(args, shard, reader, wav_done)
        assert mine == shard.assign_by_duration(reader, keys=list("bdef"))
        assert shard.barriers == 1  # (nobody writes before every rank has looked)
        got += mine
    assert sorted(got) == list("bdef")


def test_deal_skip_existing_without_requeue_keeps_every_ranks_share(tmp_path):
    wav_done, _ = _outputs(tmp_path)
    args = _args(tmp_path, skip_existing=True, requeue=False)
    reader, got = _Reader(), []
    for rank in range(2):
        shard = _Shard(rank, 2)
        mine = c.deal(args, shard, reader, wav_done)
        assert mine == [k for k in shard.assign_by_duration(reader) if k not in "ac"]
        assert shard.barriers == 0
        got += mine
    assert sorted(got) == list("bdef")


def test_deal_logs_what_it_skipped_in_both_branches(tmp_path, caplog):
    wav_done, _ = _outputs(tmp_path)
    for requeue, text in ((False, "1 of 3"), (True, "2 of 6")):
        caplog.clear()
        with caplog.at_level("INFO"):
            c.deal(_args(tmp_path, skip_existing=True, requeue=requeue), _Shard(0, 2), _Reader(), wav_done)
        assert f"--skip-existing: {text} utterances already in {tmp_path}" in caplog.text
        assert caplog.records[0].filename == "test_sptk_common.py"  # the line names its caller


# ---- the walk of the mask estimators ----
def test_walk_with_draws_shows_every_rank_the_whole_table(tmp_path):
    reader = _Reader()
    (tmp_path / "c.npy").write_bytes(b"")  # exists: skipped by every rank, whoever owns it
    seen = []
    for rank in range(2):
        shard = _Shard(rank, 2)
        steps = list(c.walk(shard, reader, tmp_path, draws=True))
        assert [k for k, _ in steps] == list("abdef") and shard.barriers == 1
        assert [k for k, mine in steps if mine] == [k for k in shard.assign_by_duration(reader) if k != "c"]
        seen.append(steps)
    assert all(m0 != m1 for (_, m0), (_, m1) in zip(*seen))  # complementary
    # one process: its own table
    assert list(c.walk(_Shard(), reader, tmp_path, draws=True)) == [(k, True) for k in "abdef"]


def test_walk_without_draws_shows_a_rank_its_own_keys(tmp_path, caplog):
    reader = _Reader()
    (tmp_path / "a.npy").write_bytes(b"")
    for rank in range(2):
        shard = _Shard(rank, 2)
        own = shard.assign_by_duration(reader)
        caplog.clear()
        with caplog.at_level("INFO"):
            steps = list(c.walk(shard, reader, str(tmp_path), draws=False))
        assert steps == [(k, True) for k in own if k != "a"] and shard.barriers == 1
        assert ("Training utterance a ... Skip" in caplog.text) == ("a" in own)


def test_num_frames_counts_as_the_stft_does():
    reader = _Reader()
    args = argparse.Namespace(center=True, frame_hop=256)
    assert c.num_frames(reader, "a", args, 512) == 1 + 900 // 256
    args.center = False
    assert c.num_frames(reader, "a", args, 512) == 1 + (900 - 512) // 256
