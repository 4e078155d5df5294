"""
setk_fir_reverb, setk_simu_batch, BatchSimulator and wav_simulate.py on the plain HIP stand-in
(tools/hoststub, PLAIN=1, no sanitizer): kernels do nothing there, so what is checked is the
plumbing around them -- argument validation and the SETK_ERR_UNSUPPORTED limits, the recipe
marshalling of _ffi.py (shapes the library derives from the structures), launch counts of a ragged
batch and of the close-talk forms, the errors the reference raises, --cmd-list parsing, batching,
sharding and resume -- and, through hoststub_report, that no copy left its allocation and no device
memory is held after close.  Runs in a child process because SETK_LIB is read at import.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hoststub_case import report, run_child  # noqa: E402


def test_simu_engine_and_cli_on_the_plain_stand_in(tmp_path):
    run_child(__file__, "data simulation on the stand-in: ok", str(tmp_path))


def _child(tmp):
    import ctypes
    import shlex
    import numpy as np
    import pytest
    import scipy.io.wavfile
    import simu_model as sm
    from setk_amd import _ffi
    from setk_amd.engine import BatchSimulator
    from setk_amd.engine.simu import Recipe, Source
    from setk_amd.sptk import wav_simulate as cli

    rng = np.random.default_rng(31)

    def f32(*shape):
        return (0.1 * rng.standard_normal(shape)).astype(np.float32)

    ctx = _ffi.default_context()
    # ---- the operator: validation and limits ----
    x, out = f32(1000), np.zeros((4, 1000), np.float32)
    before = report()[0]
    ctx.fir_reverb(x, 1000, f32(4, 600), 4, 600, out, np.zeros(1))
    assert report()[0] - before == 4  # transforms, convolution, power partials, their fold
    before = report()[0]
    ctx.fir_reverb(x, 1000, f32(3, 600), 3, 600, out[:3].copy())
    assert report()[0] - before == 2  # no power asked
    for N, R, S in ((0, 600, 1000), (17, 600, 1000), (4, 0, 1000), (4, 16385, 1000), (4, 600, 0)):
        with pytest.raises(_ffi.SetkUnsupported):
            ctx.fir_reverb(x, S, f32(max(N, 1), max(R, 1)), N, R, out)
    with pytest.raises(ValueError, match="bad args"):
        ctx.fir_reverb(x, 1000, None, 4, 600, out)

    # ---- recipe marshalling: the library reads the shapes out of the structures ----
    spk = [_ffi.simu_source(0x1000, 3000, rir=0x2000, rir_channels=4, rir_taps=600, begin=700),
           _ffi.simu_source(0x3000, 3700, rir=0x2000, rir_channels=4, rir_taps=600, snr=3.0)]
    rec = _ffi.simu_recipe(spk, [_ffi.simu_source(0x4000, 1900, rir=0x5000, rir_channels=4, rir_taps=601, begin=300,
                                                  snr=5.0, repeat=True)], dump_channel=-1)
    assert _ffi.simu_shape(rec) == (4, 3700) and rec.noises[0].flags == _ffi.SIMU_REPEAT and rec.n_noises == 1
    rec.dump_channel = 2
    assert _ffi.simu_shape(rec) == (1, 3700)
    close = _ffi.simu_recipe([_ffi.simu_source(0x1000, 500, channels=2, begin=10)])
    assert _ffi.simu_shape(close) == (2, 1010)  # `size` counts every channel (:195)
    with pytest.raises(ValueError, match="device pointers"):  # host addresses are refused
        _ffi.simu_recipe_outputs(rec, 0x6000, [0x7000, 0x8000], 0x9000)
        ctx.simu_batch([rec])
    assert ctypes.sizeof(_ffi.SimuSource) == 48 and ctypes.sizeof(_ffi.SimuRecipe) == 88

    # ---- the engine: a ragged batch, growth, the close-talk forms, shared arrays ----
    h4, h1 = f32(4, 600), f32(700)
    far = Recipe([Source(f32(3300), rir=h4, begin=700), Source(f32(3700), rir=f32(4, 520), snr=3.0)],
                 [Source(f32(1900), rir=h4, begin=300, snr=5.0, repeat=True)], iso=f32(4, 4000), iso_snr=8.0)
    mono = Recipe([Source(f32(2000), rir=h1)], [Source(f32(900), rir=h1, snr=0.0)])
    one = Recipe([Source(f32(2, 1000))])
    close2 = Recipe([Source(f32(800)), Source(f32(900), begin=50, snr=-2.0)], [Source(f32(300), snr=10.0, repeat=True)])
    live = None
    for pcm16 in (False, True):
        e = BatchSimulator(pcm16=pcm16)
        assert e.run([]) == []
        before = report()[0]
        res = e.run([one, close2])
        assert report()[0] - before == 6  # no RIR: the mixing only (powers, two folds, speaker power, peak, output)
        before = report()[0]
        res = e.run([far, mono, one, close2])
        # transforms, convolutions at 2 channels and at 1 channel per pass, and the mixing
        assert report()[0] - before == 9, report()[0] - before
        dt = np.int16 if pcm16 else np.float32
        assert [r.mix.shape for r in res] == ([(4000, 4), (2000,), (2000, 2), (950,)] if pcm16 else
                                              [(4, 4000), (1, 2000), (2, 2000), (1, 950)])
        assert all(r.mix.dtype == dt and all(s.dtype == dt for s in r.spk) for r in res)
        assert [len(r.spk) for r in res] == [2, 1, 1, 2] and [r.noise is None for r in res] == [False, False, True, False]
        assert res[0].noise.shape == (4000,) and e.status == [0, 0, 0, 0]
        e.close()
        e.close()  # (idempotent)
        live = report()[3] if live is None else live
        assert report()[3] == live, (pcm16, report()[3], live)
    e = BatchSimulator()
    # ---- what the reference raises, before anything is launched ----
    before = report()[0]
    with pytest.raises(RuntimeError, match="Channel mismatch between source speaker"):
        e.run([Recipe([Source(f32(600), rir=h4)], [Source(f32(600), rir=f32(2, 50), snr=5)])])
    with pytest.raises(RuntimeError, match="Can not convolve rir with 2D"):
        e.run([Recipe([Source(f32(2, 600), rir=h4)])])
    with pytest.raises(RuntimeError, match="Single channel mixture vs multi-channel"):
        e.run([Recipe([Source(f32(600))], iso=f32(2, 600), iso_snr=3)])
    with pytest.raises(ValueError, match="last noise's duration"):
        e.run([Recipe([Source(f32(600))], [Source(f32(200), snr=5), Source(f32(300), snr=5)])])
    with pytest.raises(_ffi.SetkUnsupported, match="behind the mixture's end"):
        e.run([Recipe([Source(f32(600))], [Source(f32(200), begin=600, snr=5)])])
    with pytest.raises(_ffi.SetkUnsupported, match="16 channels"):
        e.run([Recipe([Source(f32(600), rir=f32(17, 20))])])
    with pytest.raises(ValueError, match="dump_channel beyond"):
        e.run([Recipe([Source(f32(600), rir=h4)], dump_channel=4)])
    assert report()[0] == before
    e.close()

    # ---- the command line: the reference's errors, --cmd-list parsing, batching and resume ----
    case = sm.make_case("far")
    paths = sm.write_case_files(case, tmp)
    sr8 = os.path.join(tmp, "sr8.wav")
    scipy.io.wavfile.write(sr8, 8000, case["spk"][0])

    def args(mix, **change):
        a = sm.cli_args(dict(case, **change), paths, mix, os.path.join(os.path.dirname(mix), "ref"))
        return a

    with pytest.raises(RuntimeError, match="Number of --src-rir"):
        cli.main([os.path.join(tmp, "x.wav"), "--src-spk", ",".join(paths["spk"]), "--src-rir", paths["spk_rir"][0],
                  "--src-sdr=3"])
    with pytest.raises(RuntimeError, match="--src-sdr need to be assigned"):
        cli.main([os.path.join(tmp, "x.wav"), "--src-spk", ",".join(paths["spk"])])
    with pytest.raises(RuntimeError, match="--point-noise-snr need to be assigned"):
        cli.main([os.path.join(tmp, "x.wav"), "--src-spk", paths["spk"][0], "--point-noise", paths["noise"][0]])
    with pytest.raises(RuntimeError, match="Expect sr=16000"):
        cli.main([os.path.join(tmp, "x.wav"), "--src-spk", sr8])
    with pytest.raises(RuntimeError, match="Channel mismatch"):
        cli.main([os.path.join(tmp, "x.wav"), "--src-spk", paths["spk"][0], "--src-rir", paths["spk_rir"][0],
                  "--point-noise", paths["noise"][0], "--point-noise-snr=5"])
    with pytest.raises(SystemExit):
        cli.main(["--src-spk", paths["spk"][0]])  # neither mix nor --cmd-list
    assert not os.path.exists(os.path.join(tmp, "x.wav"))
    cli.main(args(os.path.join(tmp, "single", "mix.wav")))
    sr, w = scipy.io.wavfile.read(os.path.join(tmp, "single", "mix.wav"))
    assert sr == 16000 and w.dtype == np.int16 and w.shape == (4000, 4)
    for sub in ("noise", "spk1", "spk2"):
        assert scipy.io.wavfile.read(os.path.join(tmp, "single", "ref", sub, "mix.wav"))[1].shape == (4000,)

    lines = [" ".join(shlex.quote(a) for a in args(os.path.join(tmp, f"m{k}", "mix.wav"))) for k in range(5)]
    lst = os.path.join(tmp, "cmd.list")
    with open(lst, "w") as fd:
        fd.write("\n\n".join(lines) + "\n   \n")
    before = report()[0]
    cli.main(["--cmd-list", lst, "--batch-utts", "2"])
    assert report()[0] - before == 3 * 8  # three batches (2 + 2 + 1) of eight launches (one channel count)
    assert all(os.path.exists(os.path.join(tmp, f"m{k}", "ref", "spk2", "mix.wav")) for k in range(5))
    before = report()[0]
    cli.main(["--cmd-list", lst, "--skip-existing", "true"])
    assert report()[0] == before  # nothing left to do
    os.remove(os.path.join(tmp, "m3", "mix.wav"))
    with open(os.path.join(tmp, "m1", "mix.wav"), "r+b") as fd:
        fd.truncate(1000)  # an incomplete file is run again
    cli.main(["--cmd-list", lst, "--skip-existing", "true", "--batch-utts", "8"])
    assert report()[0] - before == 8
    assert scipy.io.wavfile.read(os.path.join(tmp, "m1", "mix.wav"))[1].shape == (4000, 4)
    # the deal over two ranks: every line to exactly one of them, by the first speaker's length
    table = cli.CmdTable(lst, cli.build_parser())
    assert table.index_keys == ["1", "3", "5", "7", "9"] and table.peek_nsamps("1") == 3300
    from setk_amd.dist import assign_keys
    w = [table.peek_nsamps(k) for k in table.index_keys]
    parts = [assign_keys(table.index_keys, r, 2, w) for r in range(2)]
    assert sorted(parts[0] + parts[1]) == sorted(table.index_keys) and parts[0] and parts[1]
    with open(lst, "a") as fd:
        fd.write("--src-spk a.wav --cmd-list other.list mix.wav\n")
    with pytest.raises(ValueError, match="one argument list with its mix"):
        cli.main(["--cmd-list", lst])

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    print(f"data simulation on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child(sys.argv[1])
