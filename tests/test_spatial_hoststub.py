"""
BatchSpatialFeatures and compute_ipd_and_linear_srp.py on the plain HIP stand-in (tools/hoststub,
PLAIN=1, no sanitizer): kernels do nothing there, so what is checked is the plumbing around them --
grouping by channel count, the slabs, growth from a small batch to a larger ragged one, 16-bit
and float input, output shapes and dtypes, the one upload of the table, close() -- and, through
hoststub_report, that launches were counted, no copy left its allocation and no device memory is
held after close.  The engine runs in a child process because SETK_LIB is read at import.
"""
import os
import sys

from hoststub_case import report, run_child

HOP, F = 256, 257


def test_spatial_engine_and_cli_on_the_plain_stand_in(tmp_path):
    run_child(__file__, "spatial features on the stand-in: ok", str(tmp_path))


def _child(tmp):
    import numpy as np
    import pytest
    import scipy.io.wavfile
    from setk_amd import _ffi
    from setk_amd.engine import BatchSpatialFeatures, Pcm16Frames, channels_and_size
    from setk_amd.libs.data_handler import ScriptReader
    from setk_amd.sptk import compute_ipd_and_linear_srp as cli

    rng = np.random.default_rng(21)

    def f32(C, N):
        return (0.1 * rng.standard_normal((C, N))).astype(np.float32)

    def pcm(C, N):
        return Pcm16Frames((3000 * rng.standard_normal((N, C))).astype(np.int16))

    def frames_of(u):
        C, size = channels_and_size(u)
        return 1 + (size // C) // HOP

    # two calls per engine, the second larger and ragged, so that every buffer grows once; four
    # channels throughout for the engines a geometry ties to a channel count
    small = [f32(4, 4000), pcm(4, 4300)]
    large = [f32(4, 5000), pcm(4, 4800), f32(4, 4100), f32(4, 9000), pcm(4, 9700)]
    mixed = [f32(4, 5000), pcm(6, 4800), f32(6, 4100)]
    sv = np.ones((7, 4, F), dtype=np.complex64)
    engines = [
        (dict(kind="srp_linear", topo=(0.0, 0.2, 0.4, 0.8)), 181, 3, False),
        (dict(kind="srp_circular", diag_pair=[(0, 2), (1, 3)], n=4, d=0.07), 121, 3, True),
        (dict(kind="ipd", pairs=[(0, 1), (2, 3)], cos=True, sin=True), 4 * F, 1, True),
        (dict(kind="df", pairs=[(0, 1), (0, 3)], steer_vector=sv), 3 * F, 1, False),
    ]
    launches0 = report()[0]
    live = None
    for kw, width, per_call, any_channels in engines:
        e = BatchSpatialFeatures(chunk_utts=2, **kw)
        df = kw["kind"] == "df"
        assert e.run([], doa_index=[] if df else None) == []
        batches = [small, large] + ([mixed] if any_channels else [])
        for batch in batches:
            before = report()[0]
            idx = [[2, 0, 5]] * len(batch) if df else None
            outs = e.run(batch, doa_index=idx)
            # per chunk: the 16-bit conversion (where there is 16-bit input), one STFT launch and
            # the launches of one setk_spatial_batch call (SRP: the memset is no launch)
            groups = {}
            for u in batch:
                groups[channels_and_size(u)[0]] = groups.get(channels_and_size(u)[0], 0) + 1
            chunks = sum((n + 1) // 2 for n in groups.values())
            assert (1 + per_call) * chunks <= report()[0] - before <= (2 + per_call) * chunks, \
                (kw["kind"], report()[0] - before, chunks)
            for u, o in zip(batch, outs):
                assert isinstance(o, np.ndarray) and o.shape == (frames_of(u), width) and o.dtype == np.float32
                assert not o.any()  # the stand-in's kernels write nothing into calloc'ed memory
        if kw["kind"] == "srp_linear":
            with pytest.raises(ValueError, match="4 microphones available, while get 6-channel STFT"):
                e.run(mixed)
        with pytest.raises(ValueError, match="microphone pair out of range|microphones available|does not match"):
            e.run([f32(2, 4000)], doa_index=[[0]] if df else None)
        if df:
            with pytest.raises(ValueError, match="direction index outside"):
                e.run(small, doa_index=[[0], [7]])
        e.close()
        e.close()  # (idempotent)
        live = report()[3] if live is None else live
        assert report()[3] == live, (kw["kind"], report()[3], live)
    with pytest.raises(_ffi.SetkUnsupported, match="2 <= num_channels <= 16"):
        _ffi.default_context().spatial_feats(_ffi.spatial_opts("ipd", [(0, 0)]), np.zeros((1, 3, F), np.complex64),
                                             1, 3, F, np.zeros((3, F), np.float32))
    with pytest.raises(_ffi.SetkUnsupported, match="at most 120 microphone pairs"):
        _ffi.default_context().spatial_feats(_ffi.spatial_opts("ipd", [(0, 1)] * 121),
                                             np.zeros((2, 3, F), np.complex64), 2, 3, F,
                                             np.zeros((3, 121 * F), np.float32))

    # ---- the command line: keys, shapes, --scp offsets, the refusal of --type msc ----
    with open(os.path.join(tmp, "wav.scp"), "w") as fd:
        for k, N in enumerate((3200, 9000, 5100, 19200)):
            path = os.path.join(tmp, f"u{k}.wav")
            scipy.io.wavfile.write(path, 16000, (3000 * rng.standard_normal((N, 4))).astype(np.int16))
            fd.write(f"u{k} {path}\n")
    ark, scp = os.path.join(tmp, "srp.ark"), os.path.join(tmp, "srp.scp")
    cli.main([os.path.join(tmp, "wav.scp"), ark, "--scp", scp, "--batch-utts", "3"])
    rows = ScriptReader(scp)
    assert list(rows.index_keys) == ["u0", "u1", "u2", "u3"]
    for k, N in enumerate((3200, 9000, 5100, 19200)):
        assert rows[f"u{k}"].shape == (1 + N // HOP, 181)
    with pytest.raises(_ffi.SetkUnsupported, match="MSC is not ported"):
        cli.main([os.path.join(tmp, "wav.scp"), ark, "--type", "msc"])
    assert report()[3] == live

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    assert launches - launches0 >= 40 and copies > 40, (launches, copies)
    print(f"spatial features on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child(sys.argv[1])
