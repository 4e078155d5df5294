"""
CacgmmEstimator's torch-free path on the plain HIP stand-in (tools/hoststub, PLAIN=1): kernels do
nothing there, so what is checked is the plumbing around them -- grouping by channel count, the
slabs of the samples, the starts and the masks, growth from a small batch to a larger ragged one,
16-bit and float input, output shapes and dtypes, the status convention, close() -- and, through
hoststub_report, that launches were counted and no copy left its allocation.  The engine runs in
a child process because SETK_LIB is read at import.
"""
from hoststub_case import report, run_child

HOP, F = 256, 257


def test_cacgmm_estimator_on_the_plain_stand_in():
    run_child(__file__, "cacgmm estimator on the stand-in: ok")


def _child():
    import numpy as np
    import pytest
    from setk_amd import _ffi
    from setk_amd.engine import CacgmmEstimator, Pcm16Frames, channels_and_size

    rng = np.random.default_rng(12)

    def f32(C, N):
        return (0.1 * rng.standard_normal((C, N))).astype(np.float32)

    def pcm(C, N):
        return Pcm16Frames((3000 * rng.standard_normal((N, C))).astype(np.int16))

    def frames_of(u):
        C, size = channels_and_size(u)
        return 1 + (size // C) // HOP

    def starts_of(batch, K):
        return [np.full((K, F, frames_of(u)), 1.0 / K) for u in batch]

    # two calls per engine, the second larger and ragged, so that every buffer grows once
    batches = [[f32(2, 4000), pcm(2, 4300)],
               [f32(2, 5000), pcm(2, 4800), f32(2, 4100), f32(3, 4000), pcm(3, 9700)]]
    launches0 = report()[0]
    live = None
    for K, cgmm_init in ((3, False), (2, True), (4, False)):
        e = CacgmmEstimator(num_classes=K, num_iters=2, cgmm_init=cgmm_init)
        assert e.estimate([], None if cgmm_init else []) == []
        for batch in batches:
            before = report()[0]
            starts = None if cgmm_init else starts_of(batch, K)
            outs, status = e.estimate(batch, starts, return_status=True)
            # per channel count: the 16-bit conversion (where there is 16-bit input), one STFT
            # launch and one EM launch
            groups = len({channels_and_size(u)[0] for u in batch})
            assert 2 * groups <= report()[0] - before <= 3 * groups, (report()[0] - before, groups)
            assert status.dtype == np.int32 and status.tolist() == [_ffi.NUM_OK] * len(batch)
            for u, o in zip(batch, outs):
                assert isinstance(o, np.ndarray) and o.shape == (K, frames_of(u), F) and o.dtype == np.float32
                assert not o.any()  # the stand-in's kernels write nothing into calloc'ed memory
            assert len(e.estimate(batch, starts)) == len(batch)
        if not cgmm_init:
            with pytest.raises(ValueError, match="one start"):
                e.estimate(batches[0], None)
            with pytest.raises(ValueError, match="must be K x F x T"):
                e.estimate(batches[0], [s[:, :, :-1] for s in starts_of(batches[0], K)])
        else:
            with pytest.raises(ValueError, match="cgmm_init takes no starts"):
                e.estimate(batches[0], starts_of(batches[0], K))
        with pytest.raises(_ffi.SetkUnsupported, match="1 <= num_channels <= 8"):
            e.estimate([f32(9, 4000)], None if cgmm_init else [np.full((K, F, 16), 1.0 / K)])
        e.close()
        e.close()  # (idempotent)
        live = report()[3] if live is None else live
        assert report()[3] == live
    with pytest.raises(_ffi.SetkUnsupported, match="2 <= num_classes <= 4"):
        CacgmmEstimator(num_classes=5)

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    assert launches - launches0 >= 24 and copies > 20, (launches, copies)
    print(f"cacgmm estimator on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child()
