"""
BatchNoiseSuppressor and apply_ns.py on the plain HIP stand-in (tools/hoststub, PLAIN=1, no
sanitizer): kernels do nothing there, so what is checked is the plumbing around them -- the slabs,
growth from a small batch to a larger ragged one, 16-bit and float input, output shapes and
dtypes of both output kinds, the operator path of other transform sizes, the refusals, close() --
and, through hoststub_report, that launches were counted, no copy left its allocation and no
device memory is held after close.  The engine runs in a child process because SETK_LIB is read at
import.
"""
import os
import sys

from hoststub_case import report, run_child

HOP, F = 256, 257


def test_ns_engine_and_cli_on_the_plain_stand_in(tmp_path):
    run_child(__file__, "noise suppression on the stand-in: ok", str(tmp_path))


def _child(tmp):
    import numpy as np
    import pytest
    import scipy.io.wavfile
    from setk_amd import _ffi
    from setk_amd.engine import BatchNoiseSuppressor, Pcm16Frames, channels_and_size
    from setk_amd.libs.ns import MCRA, iMCRA
    from setk_amd.sptk import apply_ns as cli

    rng = np.random.default_rng(23)

    def f32(N):
        return (0.1 * rng.standard_normal(N)).astype(np.float32)

    def pcm(N):
        return Pcm16Frames((3000 * rng.standard_normal((N, 1))).astype(np.int16))

    def frames_of(u):
        return 1 + channels_and_size(u)[1] // HOP

    # two calls per engine, the second larger and ragged, so that every buffer grows once
    small = [f32(4000), pcm(4300)]
    large = [f32(5000), pcm(4800), f32(4100).reshape(1, -1), f32(19000), pcm(9700)]
    launches0 = report()[0]
    live = None
    for sup in (iMCRA(), MCRA(), iMCRA(V=5, U=8, w_mcra=2)):
        for output, pcm16 in (("wave", True), ("wave", False), ("gain", False)):
            e = BatchNoiseSuppressor(sup, output=output, pcm16=pcm16)
            assert e.run([]) == []
            for batch in (small, large):
                before = report()[0]
                outs = e.run(batch)
                # the 16-bit conversion, the STFT, the recursion, and for waveforms the inverse STFT
                # and (16 bits out) the rounding of every utterance
                want = 3 + (output == "wave") + (len(batch) if output == "wave" and pcm16 else 0)
                assert report()[0] - before == want, (output, pcm16, report()[0] - before, want)
                assert e.status == [_ffi.NUM_OK] * len(batch)
                for u, o in zip(batch, outs):
                    T = frames_of(u)
                    if output == "gain":
                        assert o.shape == (T, F) and o.dtype == np.float64
                    else:
                        assert o.shape == (HOP * (T - 1),) and o.dtype == (np.int16 if pcm16 else np.float32)
                    assert not o.any()  # the stand-in's kernels write nothing into calloc'ed memory
            with pytest.raises(ValueError, match="single-channel"):
                e.run([np.zeros((2, 4000), np.float32)])
            e.close()
            e.close()  # (idempotent)
            live = report()[3] if live is None else live
            assert report()[3] == live, (output, pcm16, report()[3], live)
    # other transform sizes: the operators, one utterance at a time.  They stage through the
    # arena of the process-wide handle, which keeps its blocks: the second pass must add nothing
    for again in (False, True):
        e = BatchNoiseSuppressor(iMCRA(), output="gain", frame_len=256, frame_hop=128)
        outs = e.run(small)
        assert [o.shape for o in outs] == [(1 + 4000 // 128, 129), (1 + 4300 // 128, 129)]
        e.close()
        e = BatchNoiseSuppressor(MCRA(), output="wave", frame_len=400, frame_hop=160, round_power_of_two=False,
                                 pcm16=True)
        outs = e.run(small)
        assert [o.shape for o in outs] == [(160 * (4000 // 160),), (160 * (4300 // 160),)]
        assert outs[0].dtype == np.int16
        e.close()
        if again:
            assert report()[3] == live
        live = report()[3]
    with pytest.raises(_ffi.SetkUnsupported, match="taps for 17 bins"):
        BatchNoiseSuppressor(MCRA(), frame_len=32, frame_hop=16)
    with pytest.raises(ValueError, match="output must be wave or gain"):
        BatchNoiseSuppressor(iMCRA(), output="mask")
    ctx = _ffi.default_context()
    with pytest.raises(_ffi.SetkUnsupported, match="more taps than bins"):
        iMCRA().run(np.ones((4, 2), np.complex64))
    with pytest.raises(_ffi.SetkUnsupported, match="at most 63 taps"):
        ctx.ns_gain(_ffi.ns_opts("imcra", w_mcra=np.ones(65), V=15, U=8), np.ones((4, 129), np.complex64), 4, 129,
                    gain=np.empty((4, 129)))
    with pytest.raises(ValueError, match="a selected output is NULL"):
        ctx.ns_gain(iMCRA().opts(gain=True, spec=True), np.ones((4, 129), np.complex64), 4, 129,
                    gain=np.empty((4, 129)))
    y = np.ones(5)
    ctx.expint_e1(np.linspace(0.1, 3, 5), y)

    # ---- the command line: keys, shapes, both outputs, --conf, --skip-existing, --sr ----
    sizes = (3200, 9000, 5100, 19200)
    with open(os.path.join(tmp, "wav.scp"), "w") as fd:
        for k, N in enumerate(sizes):
            path = os.path.join(tmp, f"u{k}.wav")
            scipy.io.wavfile.write(path, 16000, (3000 * rng.standard_normal(N)).astype(np.int16))
            fd.write(f"u{k} {path}\n")
    with open(os.path.join(tmp, "conf.yaml"), "w") as fd:
        fd.write("V: 5\nU: 8\nw_mcra: 2\n")
    scp = os.path.join(tmp, "wav.scp")
    cli.main([scp, os.path.join(tmp, "wave"), "--batch-utts", "3"])
    live = report()[3]  # (the handle's arena has grown to the batch's scratch and keeps it)
    for k, N in enumerate(sizes):
        sr, w = scipy.io.wavfile.read(os.path.join(tmp, "wave", f"u{k}.wav"))
        assert sr == 16000 and w.dtype == np.int16 and w.shape == (HOP * (N // HOP),)
    before = report()[0]
    cli.main([scp, os.path.join(tmp, "wave"), "--skip-existing", "true"])
    assert report()[0] == before  # nothing left to do
    cli.main([scp, os.path.join(tmp, "gain"), "--output", "gain", "--conf", os.path.join(tmp, "conf.yaml")])
    for k, N in enumerate(sizes):
        g = np.load(os.path.join(tmp, "gain", f"u{k}.npy"))
        assert g.dtype == np.float64 and g.shape == (1 + N // HOP, F)
    with pytest.raises(ValueError, match="Now only support audio in 16kHz"):
        cli.main([scp, os.path.join(tmp, "x"), "--sr", "8000"])
    with pytest.raises(TypeError):
        with open(os.path.join(tmp, "bad.yaml"), "w") as fd:
            fd.write("no_such_parameter: 1\n")
        cli.main([scp, os.path.join(tmp, "x"), "--conf", os.path.join(tmp, "bad.yaml")])
    assert report()[3] == live

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    assert launches - launches0 >= 60 and copies > 40, (launches, copies)
    print(f"noise suppression on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child(sys.argv[1])
