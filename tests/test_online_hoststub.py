"""
BatchOnlineEnhancer on the plain HIP stand-in (tools/hoststub, PLAIN=1): kernels do nothing there,
so what is checked is the plumbing around them -- grouping by channel count and interferer mask,
the slabs of samples, masks and waves, growth from a small batch to a larger ragged one, 16-bit
and float input, output shapes and dtypes, the status convention, the refusals that need no
device, close() -- and, through hoststub_report, that launches were counted and no copy left its
allocation.  The engine runs in a child process because SETK_LIB is read at import.
"""
from hoststub_case import report, run_child

HOP, F = 256, 257


def test_online_enhancer_on_the_plain_stand_in():
    run_child(__file__, "online enhancer on the stand-in: ok")


def _child():
    import numpy as np
    import pytest
    from setk_amd import _ffi
    from setk_amd.engine import BatchOnlineEnhancer, Pcm16Frames, channels_and_size

    rng = np.random.default_rng(12)

    def f32(C, N):
        return (0.1 * rng.standard_normal((C, N))).astype(np.float32)

    def pcm(C, N):
        return Pcm16Frames((3000 * rng.standard_normal((N, C))).astype(np.int16))

    def frames_of(u):
        C, size = channels_and_size(u)
        return 1 + (size // C) // HOP

    def with_masks(batch, itf=False, transposed=False):
        out = []
        for u in batch:
            m = rng.uniform(0.1, 0.9, size=(frames_of(u), F)).astype(np.float32)
            out.append((u, m.T.copy() if transposed else m, rng.uniform(0.1, 0.9, size=m.shape) if itf else None))
        return out

    # two calls per engine, the second larger and ragged, so that every buffer grows once
    batches = [[f32(2, 9000), pcm(2, 9300)],
               [f32(2, 12000), pcm(2, 9800), f32(2, 9100), f32(3, 9000), pcm(3, 19700), pcm(3, 9000)]]
    launches0 = report()[0]
    live = None
    for kind, chunk, kw in (("mvdr", 32, {}), ("gevd", 33, dict(ban=True, post_mask=True, pcm16=True)),
                            ("mvdr", 7, dict(pcm16=True, max_batch_bytes=1 << 20))):
        e = BatchOnlineEnhancer(beamformer=kind, chunk_size=chunk, alpha=0.7, **kw)
        assert e.enhance([]) == []
        for k, batch in enumerate(batches):
            before = report()[0]
            res = e.enhance(with_masks(batch, itf=(k == 1 and kind == "gevd"), transposed=(k == 0)))
            # per engine call: (16-bit conversion), pass 1, smoothing, solve, (BAN), status, pass 2, renorm
            groups = len({channels_and_size(u)[0] for u in batch})
            assert report()[0] - before >= 6 * groups, (report()[0] - before, groups)
            assert len(res) == len(batch)
            for u, (wave, status) in zip(batch, res):
                assert status == _ffi.NUM_OK
                assert isinstance(wave, np.ndarray) and wave.shape == (HOP * (frames_of(u) - 1),)
                assert wave.dtype == (np.int16 if kw.get("pcm16") else np.float32)
                assert not wave.any()  # the stand-in's kernels write nothing into calloc'ed memory
        assert e.num_chunks(65) == -(-65 // chunk)
        assert e.ctx.online_num_chunks(16384, chunk) == -(-65 // chunk)
        with pytest.raises(ValueError, match="Shape of input obs do not match with mask matrix"):
            e.enhance([(batches[0][0], np.ones((5, F), np.float32), None)])
        with pytest.raises(_ffi.SetkUnsupported, match="1 <= num_channels <= 8"):
            e.enhance(with_masks([f32(9, 9000)]))
        e.close()
        e.close()  # (idempotent)
        live = report()[3] if live is None else live
        assert report()[3] == live
    # what the library refuses without a device
    with pytest.raises(_ffi.SetkUnsupported, match="the online beamformer is MVDR or GEVD"):
        BatchOnlineEnhancer(beamformer="pmwf-0", chunk_size=32).enhance(with_masks(batches[0]))
    with pytest.raises(ValueError, match="chunk_size must be at least 1"):
        BatchOnlineEnhancer(chunk_size=0)
    ctx = _ffi.default_context()
    with pytest.raises(ValueError, match="chunk_size must be at least 1"):
        ctx.online_num_chunks(16384, 0)
    for alpha in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"alpha must lie in \[0, 1\)"):
            BatchOnlineEnhancer(chunk_size=32, alpha=alpha).enhance(with_masks(batches[0]))

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    assert launches - launches0 >= 60 and copies > 20, (launches, copies)
    print(f"online enhancer on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child()
