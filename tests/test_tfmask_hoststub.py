"""
BatchMaskComputer, BatchMaskSeparator, BatchOracleSeparator and their command lines on the plain HIP
stand-in (tools/hoststub, PLAIN=1, no sanitizer): kernels do nothing there, so what is checked is
the plumbing around them -- the slabs, growth from a small batch to a larger ragged one, 16-bit and
float input, shapes and dtypes, the launch counts (ONE forward launch per batch, plus one inverse
launch for the separators), the operator path of other transform sizes, an empty batch, the
refusals, close() -- and, through hoststub_report, that no copy left its allocation and no device
memory is held after close.  The engines run in a child process because SETK_LIB is read at import.
"""
import os
import sys

from hoststub_case import report, run_child

HOP, F = 256, 257


def test_tfmask_engines_and_clis_on_the_plain_stand_in(tmp_path):
    run_child(__file__, "tf masks on the stand-in: ok", str(tmp_path))


def _child(tmp):
    import numpy as np
    import pytest
    import scipy.io.wavfile
    from setk_amd import _ffi
    from setk_amd.engine import (BatchMaskComputer, BatchMaskSeparator, BatchOracleSeparator, Pcm16Frames,
                                 channels_and_size)
    from setk_amd.libs.data_handler import ScriptReader
    from setk_amd.sptk import compute_mask, oracle_separate, wav_separate

    rng = np.random.default_rng(31)

    def f32(N, C=None):
        return (0.1 * rng.standard_normal(N if C is None else (C, N))).astype(np.float32)

    def pcm(N, C=1):
        return Pcm16Frames((3000 * rng.standard_normal((N, C))).astype(np.int16))

    def frames_of(u):
        C, size = channels_and_size(u)
        return 1 + (size // C) // HOP

    sizes_small, sizes_large = (4000, 4300), (5000, 4800, 4100, 19000, 9700)
    launches0 = report()[0]
    live = None

    def settle(e):
        nonlocal live
        e.close()
        e.close()  # (idempotent)
        live = report()[3] if live is None else live
        assert report()[3] == live, (type(e).__name__, report()[3], live)

    # ---- masks: one forward launch and the fold of the statistics per batch ----
    for kind in ("irm", "psm", "crm"):
        for make in (f32, pcm):
            e = BatchMaskComputer(kind, cutoff=2.0)
            assert e.run([]) == []
            for sizes in (sizes_small, sizes_large):
                batch = [(make(n), make(n)) for n in sizes]
                before = report()[0]
                outs = e.run(batch)
                assert report()[0] - before == 2, (kind, report()[0] - before)
                assert e.status == [_ffi.NUM_OK] * len(batch) and len(e.stats) == len(batch)
                for (_, m), o in zip(batch, outs):
                    assert o.shape == (frames_of(m), F * (2 if kind == "crm" else 1)) and o.dtype == np.float32
                    assert not o.any()  # the stand-in's kernels write nothing into calloc'ed memory
            settle(e)
    # a float target with a 16-bit mixture, and two channels of which the first is taken: one float batch
    e = BatchMaskComputer("iam")
    outs = e.run([(f32(4000), pcm(4000)), (f32(5000, 2), pcm(5000, 3))])
    assert [o.shape for o in outs] == [(16, F), (20, F)]
    with pytest.raises(ValueError, match="different length"):
        e.run([(f32(4000), f32(4001))])
    settle(e)
    with pytest.raises(ValueError, match="unknown mask"):
        BatchMaskComputer("smm")

    # ---- separation with a given mask: forward, inverse, scale ----
    for pcm16, keep, ref in ((True, False, False), (False, True, True), (False, False, False)):
        e = BatchMaskSeparator(keep_length=keep, mixed_norm=not keep, pcm16=pcm16)
        assert e.run([], []) == []
        for sizes in (sizes_small, sizes_large):
            mixes = [pcm(n) if i % 2 else f32(n) for i, n in enumerate(sizes)]
            masks = [rng.random((frames_of(m), F)).astype(np.float32) for m in mixes]
            masks[0] = masks[0].T                      # an F x T mask is transposed
            refs = [f32(n) if i != 1 else None for i, n in enumerate(sizes)] if ref else None
            before = report()[0]
            outs = e.run(mixes, masks, refs)
            # forward, inverse, and the scale launch whenever something is scaled or rounded
            assert report()[0] - before == 2 + (pcm16 or not keep), (pcm16, keep, report()[0] - before)
            for n, o in zip(sizes, outs):
                assert o.shape == (n if keep else HOP * (n // HOP),) and o.dtype == (np.int16 if pcm16 else np.float32)
        with pytest.raises(ValueError, match="Dimention mismatch"):
            e.run([f32(4000)], [np.ones((5, F), np.float32)])
        settle(e)

    # ---- oracle separation: K + 1 signals per utterance, one forward and one inverse launch ----
    for K, pcm16 in ((2, True), (3, False), (8, False)):
        e = BatchOracleSeparator("irm", pcm16=pcm16)
        assert e.run([]) == []
        for sizes in (sizes_small, sizes_large):
            make = pcm if K == 2 else f32
            batch = [(make(n), [make(n) for _ in range(K)]) for n in sizes]
            before = report()[0]
            outs = e.run(batch)
            assert report()[0] - before == 2 + pcm16, (K, report()[0] - before)
            for n, waves in zip(sizes, outs):
                assert len(waves) == K
                assert all(w.shape == (HOP * (n // HOP),) and w.dtype == (np.int16 if pcm16 else np.float32)
                           for w in waves)
        settle(e)
    with pytest.raises(_ffi.SetkUnsupported, match="at most 8 targets"):
        BatchOracleSeparator("irm").run([(f32(4000), [f32(4000)] * 9)])
    with pytest.raises(ValueError, match="oracle separation takes"):
        BatchOracleSeparator("crm")
    ctx = _ffi.default_context()
    with pytest.raises(ValueError, match="ibm, irm, iam or psm"):
        ctx.oracle_separate_batch("psa", 1, [1], [1], [4000], [1])
    with pytest.raises(_ffi.SetkUnsupported, match="at most 8 targets"):
        ctx.oracle_separate_batch("irm", 9, [1], [1] * 9, [4000], [1] * 9)

    # ---- other transform sizes: the operators, one utterance at a time; the second pass adds nothing ----
    for again in (False, True):
        e = BatchMaskComputer("psm", frame_len=256, frame_hop=128)
        outs = e.run([(f32(4000), f32(4000)), (pcm(4300), pcm(4300))])
        assert [o.shape for o in outs] == [(1 + 4000 // 128, 129), (1 + 4300 // 128, 129)]
        e.close()
        e = BatchMaskSeparator(pcm16=True, frame_len=400, frame_hop=160, round_power_of_two=False)
        outs = e.run([f32(4000)], [np.ones((1 + 4000 // 160, 201), np.float32)])
        assert outs[0].shape == (160 * (4000 // 160),) and outs[0].dtype == np.int16
        e.close()
        e = BatchOracleSeparator("ibm", frame_len=256, frame_hop=128)
        outs = e.run([(f32(4000), [f32(4000), f32(4000)])])
        assert [w.shape for w in outs[0]] == [(128 * (4000 // 128),)] * 2
        e.close()
        if again:
            assert report()[3] == live
        live = report()[3]
    m = compute_mask.compute_mask(np.ones((4, 129), np.complex64), np.ones((4, 129), np.complex64), "crm")
    assert m.shape == (4, 258) and m.dtype == np.float32
    masks = oracle_separate.compute_mask(np.ones((4, 9), np.complex64), [np.ones((4, 9), np.complex64)] * 3, "irm")
    assert len(masks) == 3 and np.allclose(masks[0], 1 / 3, atol=1e-6)

    # ---- the command lines: keys, shapes, archives and wav files, --skip-existing ----
    sizes = (3200, 9000, 5100, 19200)
    for role in ("clean", "other", "noisy"):
        with open(os.path.join(tmp, f"{role}.scp"), "w") as fd:
            for k, N in enumerate(sizes):
                path = os.path.join(tmp, f"{role}{k}.wav")
                scipy.io.wavfile.write(path, 16000, (3000 * rng.standard_normal(N)).astype(np.int16))
                if role != "noisy" or k != 2:          # utterance 2 has no noisy file
                    fd.write(f"u{k} {path}\n")
    scp = {role: os.path.join(tmp, f"{role}.scp") for role in ("clean", "other", "noisy")}
    ark, mscp = os.path.join(tmp, "irm.ark"), os.path.join(tmp, "irm.scp")
    compute_mask.main([scp["clean"], scp["noisy"], ark, "--scp", mscp, "--mask", "irm", "--batch-utts", "2"])
    rd = ScriptReader(mscp)
    assert sorted(rd.index_keys) == ["u0", "u1", "u3"]
    for k in (0, 1, 3):
        assert rd[f"u{k}"].shape == (1 + sizes[k] // HOP, F)
    with pytest.raises(_ffi.SetkUnsupported, match="exraw"):
        compute_mask.main([scp["clean"], scp["noisy"], ark, "--format", "exraw"])
    wav_separate.main([scp["noisy"], mscp, os.path.join(tmp, "sep"), "--batch-utts", "2"])
    live = report()[3]  # (the handle's arena has grown to the batch's scratch and keeps it)
    for k in (0, 1, 3):
        sr, w = scipy.io.wavfile.read(os.path.join(tmp, "sep", f"u{k}.wav"))
        assert sr == 16000 and w.dtype == np.int16 and w.shape == (HOP * (sizes[k] // HOP),)
    before = report()[0]
    wav_separate.main([scp["noisy"], mscp, os.path.join(tmp, "sep"), "--skip-existing", "true"])
    assert report()[0] == before  # nothing left to do
    wav_separate.main([scp["noisy"], mscp, os.path.join(tmp, "sepk"), "--keep-length", "true", "--phase-ref",
                       scp["clean"], "--use-mixed-norm", "false"])
    assert scipy.io.wavfile.read(os.path.join(tmp, "sepk", "u3.wav"))[1].shape == (sizes[3],)
    oracle_separate.main([scp["noisy"], "--ref-scp", scp["clean"] + "," + scp["other"], "--dump-dir",
                          os.path.join(tmp, "ora"), "--mask", "psm"])
    for k in (0, 1, 3):
        for spk in (1, 2):
            sr, w = scipy.io.wavfile.read(os.path.join(tmp, "ora", f"spk{spk}", f"u{k}.wav"))
            assert sr == 16000 and w.dtype == np.int16 and w.shape == (HOP * (sizes[k] // HOP),)
    before = report()[0]
    oracle_separate.main([scp["noisy"], "--ref-scp", scp["clean"] + "," + scp["other"], "--dump-dir",
                          os.path.join(tmp, "ora"), "--mask", "psm", "--skip-existing", "true"])
    assert report()[0] == before
    assert report()[3] == live

    launches, violations, copies, _, first = report()
    assert violations == 0, first
    assert launches - launches0 >= 60 and copies > 40, (launches, copies)
    print(f"tf masks on the stand-in: ok ({launches} launches, {copies} copies)")


if __name__ == "__main__":
    _child(sys.argv[1])
