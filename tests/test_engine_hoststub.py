"""
The batch engines' torch-free paths on the plain HIP stand-in (tools/hoststub, PLAIN=1): kernels
do nothing there, so what is checked is the plumbing around them -- grouping, slab layout, growth
from a small batch to a larger one, output shapes and dtypes, the None / status conventions,
close() -- and, through hoststub_report, that launches were counted and no copy left its
allocation.  The engines run in a child process because SETK_LIB is read at import.
"""
from hoststub_case import report, run_child

HOP, F = 256, 257


def test_engines_on_the_plain_stand_in():
    run_child(__file__, "engines on the stand-in: ok")


def _child():
    import numpy as np
    import pytest
    from setk_amd import _ffi
    from setk_amd.engine import (BatchSeparator, BatchDereverb, BatchWpd, CgmmEstimator,
                                 FixedBatchBeamformer, BatchLocalizer, BatchDirectionalFeatures,
                                 Pcm16Frames, channels_and_size)

    rng = np.random.default_rng(11)

    def f32(C, N):
        return (0.1 * rng.standard_normal((C, N))).astype(np.float32)

    def pcm(C, N):
        return Pcm16Frames((3000 * rng.standard_normal((N, C))).astype(np.int16))

    def shape_of(u):  # (C, N, T, L) of the centred 512 / 256 transform
        C, size = channels_and_size(u)
        N = size // C
        T = 1 + N // HOP
        return C, N, T, HOP * (T - 1)

    def zeros(a, shape, dtype):
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dtype, (a.shape, a.dtype, shape, dtype)
        assert not a.any()  # the stand-in's kernels write nothing into calloc'ed memory

    # two calls per engine, the second larger, so that every buffer grows once
    mixed = [[f32(2, 4000), pcm(2, 4300)],
             [f32(2, 5000), pcm(2, 4800), f32(2, 4100), f32(3, 4000), pcm(3, 4700)]]
    same = [[f32(2, 4000), pcm(2, 4300)], [pcm(3, 5000), f32(3, 4800), f32(3, 4100)]]

    # the first engine also brings the process-wide handle and its plan up: what is live after its
    # close() is what must be live after every other engine's
    live = None
    for p16 in (False, True):
        e = BatchSeparator(num_epochs=2, pcm16=p16)
        assert e.run([]) == [] and e.status == []
        for batch in mixed:
            outs = e.run(batch)
            assert e.status == [_ffi.NUM_OK] * len(batch)
            for u, o in zip(batch, outs):
                C, _, _, L = shape_of(u)
                zeros(o, (C, L), np.int16 if p16 else np.float32)
        with pytest.raises(_ffi.SetkUnsupported, match="needs 1 <= channels <= 8 .got 9 channels"):
            e.run([f32(9, 4000)])
        e.close()
        e.close()  # (idempotent)
        live = report()[3] if live is None else live
        assert report()[3] == live

    for p16 in (False, True):
        e = BatchDereverb(taps=4, delay=2, num_iters=2, pcm16=p16)
        assert e.run([]) == []
        for batch in same:
            for u, o in zip(batch, e.run(batch)):
                C, _, _, L = shape_of(u)
                zeros(o, (L, C) if p16 else (C, L), np.int16 if p16 else np.float32)
        with pytest.raises(ValueError, match="BatchDereverb.run needs the same channel count in every utterance"):
            e.run(mixed[1])
        assert e.rank_deficient_bins == 0
        e.close()
        assert report()[3] == live

    for p16 in (False, True):
        e = BatchWpd(taps=4, delay=2, wpd_iters=2, cgmm_iters=2, pcm16=p16)
        assert e.run([]) == []
        for batch in same:
            for u, o in zip(batch, e.run(batch)):
                _, _, T, L = shape_of(u)
                zeros(o[0], (L,), np.int16 if p16 else np.float32)
                zeros(o[1], (T, F), np.float32)
        with pytest.raises(ValueError, match="BatchWpd.run needs the same channel count in every utterance"):
            e.run(mixed[1])
        assert e.rank_deficient_bins == 0
        e.close()
        assert report()[3] == live

    e = CgmmEstimator(num_iters=2)
    for batch in mixed:
        for u, o in zip(batch, e.estimate(batch)):
            zeros(o, (shape_of(u)[2], F), np.float32)
    e.close()
    assert report()[3] == live

    def table(B):
        return (rng.standard_normal((B, F, 2)) + 1j * rng.standard_normal((B, F, 2))).astype(np.complex64)

    for p16 in (False, True):
        e = FixedBatchBeamformer(table(2), pcm16=p16)
        two = mixed[1][:3]
        for batch, beams in ((mixed[0], (0, 1)), (two, (2, 0, 1))):
            for u, o in zip(batch, e.run(list(zip(batch, beams)))):
                zeros(o, (shape_of(u)[3],), np.int16 if p16 else np.float32)
            e.set_weights(table(3))  # a larger table between the calls: the device copy is replaced
            assert e.weights.shape == (3, F, 2)
        with pytest.raises(ValueError, match="engine built for"):
            e.set_weights(table(3)[:, :, :1])
        with pytest.raises(ValueError, match="Input obs do not match with weight"):
            e.run([(mixed[1][3], 0)])
        e.close()
        assert report()[3] == live

    A, chunk, back = 6, 10, 5
    sv = {C: (rng.standard_normal((A, C, F)) + 1j * rng.standard_normal((A, C, F))).astype(np.complex64)
          for C in (2, 3)}
    e = BatchLocalizer(backend="ml", steer_vector=sv, chunk_len=chunk, look_back=back)
    assert e.run([]) == []
    for batch in mixed:
        # every other utterance with a mask, the others without
        masks = [rng.uniform(0, 1, (shape_of(u)[2], F)).astype(np.float32) if k % 2 == 0 else None
                 for k, u in enumerate(batch)]
        outs = e.run(batch, masks)
        assert e.status == [_ffi.NUM_OK] * len(batch)
        for u, o, sc in zip(batch, outs, e.scores):
            T = shape_of(u)[2]
            W = len(range(0, T, chunk))
            assert e.windows(T)[1] == (chunk - back, min(2 * chunk, T)) and len(e.windows(T)) == W
            zeros(o, (W,), np.int64)
            zeros(sc, (W, A), np.float64)
    with pytest.raises(ValueError, match="one mask .or None. per utterance"):
        e.run(mixed[0], [None])
    with pytest.raises(ValueError, match="no steer vectors for 4 channels"):
        e.run([f32(4, 4000)])
    e.close()
    assert report()[3] == live

    # one chunk (one lane), then two channel counts in chunks of two (both lanes, two threads)
    for chunk_utts, batches in ((8, same), (2, mixed)):
        e = BatchDirectionalFeatures([(0, 1)], chunk_utts=chunk_utts)
        assert e.run([]) == []
        for batch in batches:
            pairs = [(u, rng.uniform(0, 1.5, (F, shape_of(u)[2]) if k % 2 else (shape_of(u)[2], F)))
                     for k, u in enumerate(batch)]  # masks T x F and F x T
            for u, (df, code) in zip(batch, e.run(pairs)):
                assert code == 0
                zeros(df, (shape_of(u)[2], F), np.float32)
        with pytest.raises(ValueError, match="microphone pair out of range for 1 channels"):
            e.run([(f32(1, 4000)[0], np.ones((16, F)))])
        e.close()
        assert report()[3] == live

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    assert launches > 100 and copies > 100, (launches, copies)
    print(f"engines on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child()
