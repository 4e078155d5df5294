"""
setk_rir_generate(_batch), BatchRirGenerator and rir_generate_{1d,2d}.py on the plain HIP stand-in
(tools/hoststub, PLAIN=1, no sanitizer): kernels do nothing there, so what is checked is the plumbing
around them -- the marshalling of setk_rir_spec, launch counts of a ragged batch, validation and
the limits, the command lines' sampling order and rir.json against what the reference's scripts
recorded with the same seed (tests/golden/ref_rir.npz), --batch-rirs batching, the refused --gpu --
and, through hoststub_report, that no copy left its allocation and no device memory is held after
close.  Runs in a child process because SETK_LIB is read at import.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hoststub_case import report, run_child  # noqa: E402


def test_rir_engine_and_cli_on_the_plain_stand_in(tmp_path):
    run_child(__file__, "RIR generation on the stand-in: ok", str(tmp_path))


def _child(tmp):
    import ctypes
    import json
    import numpy as np
    import pytest
    import scipy.io.wavfile
    import rir_model as rm
    from setk_amd import _ffi
    from setk_amd.engine import BatchRirGenerator
    from setk_amd.libs.rir import make_spec
    from setk_amd.sptk import rir_generate_1d, rir_generate_2d

    ctx = _ffi.default_context()
    room, src, mics = (4.0, 5.0, 2.5), (1.2, 1.7, 1.4), [(2.6, 3.1, 1.1), (2.7, 3.1, 1.1)]

    # ---- marshalling: the structure as the header lays it out, the arrays as float32 ----
    assert ctypes.sizeof(_ffi.RirSpec) == 72
    sp = make_spec(room, src, mics, (0.9, 0.8, 0.7, 0.6, 0.5, 0.85), sr=8000, rir_nsamps=700, v=343.0, order=3,
                   hp_filter=False, mic_type="cardioid", angle=(0.6, 0.3))
    assert (sp.n_mics, sp.n_beta, sp.mic_type, sp.order, sp.num_samples, sp.hp_filter) == \
        (2, 6, _ffi.RIR_MIC_CARDIOID, 3, 700, 0)
    assert (sp.samp_frequency, sp.sound_velocity) == (8000.0, 343.0)
    assert [sp.room[i] for i in range(3)] == [4.0, 5.0, 2.5] and sp.mics[3] == np.float32(2.7)
    assert sp.beta[5] == np.float32(0.85) and sp.angle[1] == np.float32(0.3)
    assert not make_spec(room, src, mics, 0.3).angle  # NULL: 0, 0

    # ---- one call: two launches whatever the batch ----
    before = report()[0]
    rir, status = ctx.rir_generate(sp)
    assert report()[0] - before == 2 and rir.shape == (2, 700) and status == 0
    specs = [make_spec(room, src, mics[:n], 0.3, rir_nsamps=ns) for n, ns in ((1, 1), (2, 300), (1, 16384))]
    outs = [np.zeros((s.n_mics, s.num_samples), np.float32) for s in specs]
    before = report()[0]
    ctx.rir_generate_batch(specs, outs, status=np.zeros(3, np.int32))
    ctx.rir_generate_batch(specs, outs, flags=_ffi.RIR_NO_SPLIT)
    assert report()[0] - before == 4

    # ---- validation and the limits, before anything is launched ----
    before = report()[0]

    def refused(exc, match, **change):
        kw = dict(room=room, src=src, mics=mics, beta_or_rt60=(0.5,) * 6, rir_nsamps=256)
        kw.update(change)
        with pytest.raises(exc, match=match):
            ctx.rir_generate(make_spec(**kw))

    refused(_ffi.SetkUnsupported, "16 microphones", mics=[mics[0]] * 17)
    refused(_ffi.SetkUnsupported, "16384 taps", rir_nsamps=16385)
    refused(_ffi.SetkUnsupported, "16384 taps", rir_nsamps=0)
    refused(_ffi.SetkUnsupported, "64 kHz", sr=96000)
    refused(_ffi.SetkUnsupported, "images per microphone", room=(0.05, 0.05, 0.05), rir_nsamps=16384)
    refused(ValueError, "samp_frequency >= 1", sr=0.5)
    refused(ValueError, "sound_velocity >= 1", v=0.9)
    refused(ValueError, "order >= -1", order=-2)
    refused(ValueError, "room dimensions > 0", room=(4.0, 0.0, 2.5))
    with pytest.raises(ValueError, match="six reflection coefficients"):
        ctx.rir_generate(_ffi.rir_spec(room, src, mics, (0.5,) * 5, 256))
    with pytest.raises(ValueError, match="flags"):
        ctx.rir_generate(sp, flags=2)
    with pytest.raises(ValueError, match="bad args"):
        ctx.rir_generate_batch([], [])
    bad = _ffi.rir_spec(room, src, mics, (0.5,) * 6, 256)
    bad.mic_type = 5
    with pytest.raises(ValueError, match="mic_type"):
        ctx.rir_generate(bad)
    assert report()[0] == before

    # ---- the engine: batches by size, idempotent close, nothing held afterwards ----
    settings = [dict(room=room, src=src, mics=mics[:n], beta_or_rt60=0.3, rir_nsamps=ns)
                for n, ns in ((2, 500), (1, 300), (2, 1), (1, 900))]
    live = None
    for kw, launches in ((dict(), 2), (dict(max_batch_bytes=4000), 6), (dict(split=False), 2)):
        e = BatchRirGenerator(**kw)
        assert e.run([]) == []
        before = report()[0]
        res = e.run(settings)
        assert report()[0] - before == launches, (kw, report()[0] - before)
        assert [r.shape for r in res] == [(2, 500), (1, 300), (2, 1), (1, 900)] and e.status == [0] * 4
        assert all(r.dtype == np.float32 for r in res)
        e.close()
        e.close()
        live = report()[3] if live is None else live
        assert report()[3] == live, (kw, report()[3], live)

    # ---- the command lines: the reference's draws, its rir.json, --batch-rirs, --gpu ----
    os.chdir(tmp)
    for name, cli in (("rir_generate_1d", rir_generate_1d), ("rir_generate_2d", rir_generate_2d)):
        args, seed, want_json, _ = rm.load_cli_fixture(name)
        dump = args[args.index("--dump-dir") + 1]
        before = report()[0]
        cli.main(args + ["--seed", str(seed), "--batch-rirs", "3"])
        assert report()[0] - before == 4  # 4 RIRs in batches of 3 and 1
        got = open(os.path.join(dump, "rir.json")).read()
        assert json.loads(got) == json.loads(want_json), name  # the sampling order and the rounding
        assert got == want_json, name                          # and the file as written
        for room_cfg in json.loads(got):
            for spk in room_cfg["spk"]:
                sr, w = scipy.io.wavfile.read(spk["loc"])
                assert sr == 16000 and w.dtype == np.int16 and w.shape == (800, 4)
        assert os.path.getsize(os.path.join(dump, "Room1.jpg")) > 0 and os.path.exists(os.path.join(dump, "Room2.jpg"))
        before = report()[0]
        cli.main(args + ["--seed", str(seed)])
        assert report()[0] - before == 2 and open(os.path.join(dump, "rir.json")).read() == want_json
        cli.main(args + ["--seed", str(seed + 1)])
        assert open(os.path.join(dump, "rir.json")).read() != want_json
        before = report()[0]
        with pytest.raises(_ffi.SetkUnsupported, match="gpuRIR"):
            cli.main(args + ["--gpu", "true"])
        assert report()[0] == before
    with pytest.raises(RuntimeError, match="Wrong format with --room-dim"):
        rir_generate_1d.main(["1", "--room-dim", "4,6;5,7", "--dump-dir", "bad"])
    assert report()[3] == live

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    print(f"RIR generation on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child(sys.argv[1])
