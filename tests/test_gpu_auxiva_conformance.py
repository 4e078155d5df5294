"""
Conformance of AuxIVA on the device -- auxiva_epoch_kernel<1..8> behind setk_auxiva, and the batch
entry setk_auxiva_batch -- on the constructed spectrograms of auxiva_cases.py, judged per bin and
source against auxiva() restated in np.clongdouble:

    ||got_fn - ref_fn|| <= 2^-24 ||ref_fn|| + 4 u_fn     (norms over the frames)

u the error of the float64 model under two summation orders, floored at 2^-40 ||ref_fn||; exactly
zero where the reference is; status 0 in every bin; finite.  test_auxiva_cases.py shows on the CPU
that this bar fails eight seeded faults, seven of which the per-source relative RMS of
test_gpu_auxiva.py lets pass.  Measured figures: PARITY_NOTES_AUXIVA.md.
"""
import os
import sys

import numpy as np
import pytest

import auxiva_cases as ac
from conftest import ROOT, rel_rms

sys.path.insert(0, os.path.join(ROOT, "tests"))
import auxiva_model  # noqa: E402

pytestmark = pytest.mark.gpu
STFT_KW = dict(frame_len=512, frame_hop=256, window="hann", center=True)


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    return _ffi.default_context()


def run(ctx, X, epochs):
    """setk_auxiva on host arrays -> (Y [C][T][F] complex64, status [F]); both preset so that an
    element or a status the call does not write shows."""
    C, T, F = X.shape
    out = np.full(X.shape, np.nan, np.complex64)
    st = np.full(F, -1, dtype=np.int32)
    ctx.auxiva(np.ascontiguousarray(X), C, T, F, epochs, out, status=st)
    return out, st


def run_on_device(ctx, X, epochs):
    import torch
    C, T, F = X.shape
    xd = torch.from_numpy(np.array(X)).cuda()             # (a copy: the shared reference is read-only)
    yd = torch.full_like(xd, float("nan"))
    st = torch.full((F,), -1, dtype=torch.int32, device="cuda")
    ctx.auxiva(xd, C, T, F, epochs, yd, status=st.data_ptr())
    torch.cuda.synchronize()
    return yd.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("C", ac.CHANNELS)
def test_operator(ctx, C):
    """Every case of the channel count: 4 C + 1, 31 .. 33, 127 .. 129 and 257 frames at one, two
    and three epochs, 130, 255, 256 and 385 at two."""
    tally = ac.Tally(f"setk_auxiva C={C}")
    for case in ac.cases(C):
        R = ac.reference(case)
        got, st = run(ctx, R.X, case.epochs)
        tally.add(case.name, *ac.judge(case.name, got, st, R))
        old = ac.source_rel_rms(got, R)
        assert old.max() <= 1e-4, (case.name, old)          # the older measure, for the record
        if case.T == 129 and case.epochs == 3:
            dev, dst = run_on_device(ctx, R.X, case.epochs)
            assert np.array_equal(ac.bits(dev), ac.bits(got)) and np.array_equal(dst, st), case.name
    tally.finish()


def test_hard_cases(ctx):
    """A near-duplicate channel in the white bin (cond about 1e6): the yardsticks carry the bar."""
    tally = ac.Tally("setk_auxiva, near-duplicate channel")
    for case in ac.hard_cases():
        R = ac.reference(case)
        got, st = run(ctx, R.X, case.epochs)
        ratio, fails = ac.judge(case.name, got, st, R)
        print(f"[{case.name}] worst ratio per bin " + " ".join(f"{v:.3f}" for v in ratio.max(axis=1)))
        tally.add(case.name, ratio, fails)
    tally.finish()


def test_same_bits_twice_and_across_layouts(ctx):
    """A case repeated gives the same bits; and the six bins among nine (auxiva_cases.embedded:
    extra bins that are non-zero only where the six are silent, which keeps every power the six
    bins' covariances use bit for bit -- a copy of `white` there cannot) give the bits they give
    alone, whatever block of the grid runs them: every bin, at one and at three epochs."""
    for case in (ac.Case(5, 129, 3), ac.Case(8, 33, 2)):
        R = ac.reference(case)
        a, sa = run(ctx, R.X, case.epochs)
        b, sb = run(ctx, R.X, case.epochs)
        assert np.array_equal(ac.bits(a), ac.bits(b)) and np.array_equal(sa, sb), case.name
    for C, T in ((2, 33), (3, 129), (3, 257)):
        for epochs in (1, 3):
            R = ac.reference(ac.Case(C, T, epochs))
            alone, st = run(ctx, R.X, epochs)
            big, stb = run(ctx, ac.embedded(np.array(R.X)), epochs)
            assert not st.any() and not stb.any(), (C, T, epochs, st, stb)
            for f, at in enumerate(ac.EMBED_AT):
                assert np.array_equal(ac.bits(big[:, :, at]), ac.bits(alone[:, :, f])), (C, T, epochs, f)


# ---------------------------------------------------------------- the batch entry
BATCH_FRAMES = (127, 128, 129, 33)


def model_waves(samps, epochs):
    """run() of the reference on one utterance with the float64 model in place of auxiva()."""
    from oracle import np_oracle as o
    X = np.stack([o.forward_stft(c, transpose=True, **STFT_KW) for c in np.atleast_2d(samps)])
    Y = auxiva_model.auxiva(X, epochs)
    norm = float(np.max(np.abs(samps)))
    return np.stack([o.inverse_stft(y, transpose=True, norm=norm, **STFT_KW) for y in Y])


@pytest.mark.parametrize("C", ac.CHANNELS)
def test_batch_every_count_at_the_edges(C):
    """setk_auxiva_batch at every channel count (4, 6 and 7 had no run), one call on four
    utterances whose frame counts sit on and beside the staged chunk and one past a wavefront's
    quarter.  The entry has no tap for Y: each source's waveform against the model at the
    project's 1e-3, the batch against single calls bit for bit."""
    from setk_amd.engine import BatchSeparator
    utts = [auxiva_model.synth_scene(2000 + 10 * C + k, C, 256 * (T - 1)) for k, T in enumerate(BATCH_FRAMES)]
    eng = BatchSeparator(num_epochs=3, **STFT_KW)
    outs = eng.run(utts)
    assert eng.status == [0] * len(utts)
    for k, (s, got) in enumerate(zip(utts, outs)):
        ref = model_waves(s, 3)
        assert got.shape == ref.shape and got.dtype == np.float32
        devs = [rel_rms(got[n], ref[n]) for n in range(C)]
        print(f"batch C={C} T={BATCH_FRAMES[k]}: " + " ".join(f"{d:.2e}" for d in devs))
        assert max(devs) <= 1e-3, (C, k, devs)
    for k, s in enumerate(utts):
        single = eng.run([s])
        assert eng.status == [0]
        assert np.array_equal(single[0], outs[k]), (C, k)
