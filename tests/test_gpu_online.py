"""
Block-online MVDR / GEV beamforming on the device (setk_enhance_online_batch, BatchOnlineEnhancer,
apply_adaptive_beamformer.py --online.chunk-size) against the float64 statement of
tests/online_model.py.  Inputs: o.synth_utterance(30 + C, C, N) with the mask 0.05 + 0.9 irm
(cond(Rn_c) <= 1.5e3 for every chunk and bin: no cell is left out).  Bars: the project's -- smoothed
covariances 1e-5 and weights 2e-4 per chunk (rel rms; the weights against the model evaluated in
complex128 ON THE TAPPED float32 covariances, as tests/test_gpu_wide.py does: a solve amplifies
the float32 noise of its matrices by their condition number, which is no property of the solver),
waveforms 1e-3.  Every test prints its figures before it asserts.
"""
import argparse
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import online_model as om
from conftest import ROOT, load_golden, pcm16_rel_rms, rel_rms
from oracle import np_oracle as o

pytestmark = pytest.mark.gpu

ALPHA = 0.8
N_TAPS = 16384  # T = 65: chunks of 32 and 33 frames both end in a short chunk (1 frame at 32)


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, 256, 512, True)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(C, N):
    mix, mask = om.case_inputs(C, N)
    mix.setflags(write=False)
    mask.setflags(write=False)
    return mix, mask


@functools.lru_cache(maxsize=None)
def itf_mask(T):
    m = np.random.default_rng(11).uniform(0.1, 0.9, size=(T, 257)).astype(np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def model_wave(C, N, chunk, kind, ban, post, itf):
    mix, mask = inputs(C, N)
    wav = om.enhance_online(mix, mask, chunk, ALPHA, kind=kind, ban=ban, post_mask=post,
                            itf_mask=itf_mask(mask.shape[0]) if itf else None)
    wav.setflags(write=False)
    return wav


def run_abi(ctx, kind, chunk, mix, mask, flags=0, alpha=ALPHA, taps=True):
    """One utterance through setk_enhance_online_batch; returns (wave, status, taps)."""
    import torch
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    C, N = mix.shape
    a = torch.from_numpy(np.array(mix, dtype=np.float32)).to(dev)
    m = torch.from_numpy(np.array(mask, dtype=np.float32)).to(dev)
    T = ctx.num_frames(N)
    out = torch.empty(ctx.istft_num_samples(T), dtype=torch.float32, device=dev)
    K = ctx.online_num_chunks(N, chunk)
    tp = dict(Rs=np.zeros((K, 257, C, C), np.complex64), Rn=np.zeros((K, 257, C, C), np.complex64),
              weight=np.zeros((K, 257, C), np.complex64)) if taps else None
    st = np.full(1, -1, dtype=np.int32)
    opts = _ffi.BfOpts(kind={"mvdr": _ffi.BF_MVDR, "gevd": _ffi.BF_GEVD, "pmwf-0": _ffi.BF_PMWF}[kind],
                       flags=flags | _ffi.FLAG_CLAMP_MASK, pmwf_ref=-1)
    ctx.enhance_online_batch(opts, chunk, alpha, C, [a.data_ptr()], [N], [m.data_ptr()], None, [out.data_ptr()],
                             status=st, taps=tp)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(st[0]), tp


@pytest.mark.parametrize("chunk", [32, 33])
@pytest.mark.parametrize("C", range(1, 9))
def test_taps_per_chunk(ctx, C, chunk):
    mix, mask = inputs(C, N_TAPS)
    obs = o.multichannel_stft(mix, round_power_of_two=True, transpose=False, **om.STFT_KW)
    assert obs.shape[2] == 65
    ref = om.online_parts(obs, np.minimum(mask, 1), chunk, ALPHA, kind="mvdr")
    K = ref["Rs"].shape[0]
    assert K == -(-65 // chunk) == ctx.online_num_chunks(N_TAPS, chunk)
    for kind in ("mvdr", "gevd")[:1 if C == 1 else 2]:
        _, st, tp = run_abi(ctx, kind, chunk, mix, mask)
        assert st == 0
        want = om.weights_on(kind, tp["Rs"], tp["Rn"])
        for k in range(K):
            e_rs, e_rn = rel_rms(tp["Rs"][k], ref["Rs"][k]), rel_rms(tp["Rn"][k], ref["Rn"][k])
            e_w = rel_rms(tp["weight"][k], want[k])
            print(f"C={C} chunk={chunk} {kind} k={k}: Rs {e_rs:.2e} Rn {e_rn:.2e} w {e_w:.2e}")
            assert e_rs < 1e-5 and e_rn < 1e-5, (C, chunk, kind, k, e_rs, e_rn)
            assert e_w < 2e-4, (C, chunk, kind, k, e_w)


def test_alpha_zero_and_one_long_chunk(ctx):
    """alpha = 0: every chunk's smoothed matrices are its own; one chunk >= T: the offline call."""
    from setk_amd import _ffi
    mix, mask = inputs(4, N_TAPS)
    obs = o.multichannel_stft(mix, round_power_of_two=True, transpose=False, **om.STFT_KW)
    _, st, tp = run_abi(ctx, "mvdr", 33, mix, mask, alpha=0.0)
    ref = om.online_parts(obs, np.minimum(mask, 1), 33, 0.0)
    assert st == 0 and rel_rms(tp["Rn"][1], ref["rn"][1]) < 1e-5 and rel_rms(tp["Rs"][1], ref["Rs"][1]) < 1e-5
    wav, st, _ = run_abi(ctx, "mvdr", 4000, mix, mask, flags=_ffi.FLAG_BAN, taps=False)
    off = o.enhance_utterance(mix, mask, kind="mvdr", ban=True, gauge=True)
    print("one chunk against the offline oracle", rel_rms(wav, off))
    assert st == 0 and rel_rms(wav, off) < 1e-3


WAVE_CASES = [(kind, ban, post, itf) for kind in ("mvdr", "gevd") for ban in (False, True)
              for post in (False, True) for itf in (False, True)]


def _engine(kind, chunk, ban=False, post=False, pcm16=False, **kw):
    from setk_amd.engine import BatchOnlineEnhancer
    return BatchOnlineEnhancer(beamformer=kind, chunk_size=chunk, alpha=ALPHA, ban=ban, post_mask=post,
                               pcm16=pcm16, **kw)


@pytest.mark.parametrize("kind,ban,post,itf", WAVE_CASES,
                         ids=[f"{k}{'-ban' if b else ''}{'-post' if p else ''}{'-itf' if i else ''}"
                              for k, b, p, i in WAVE_CASES])
def test_waveform_through_the_engine(kind, ban, post, itf):
    # 4 ch x 16384 samples: T = 65, the last chunk a single frame (there BAN divides by w^H rn w of
    # a rank-one rn: GEV + BAN + an interferer mask is the largest figure of the table, 4.2e-4);
    # 4 ch x 20480: T = 81, chunks of 32, 32 and 17 frames; 2 ch x 48000: T = 188, six chunks
    for C, N in ((4, 16384), (4, 20480), (2, 48000)):
        mix, mask = inputs(C, N)
        im = itf_mask(mask.shape[0]) if itf else None
        ref = model_wave(C, N, 32, kind, ban, post, itf)
        for pcm16 in (False, True):
            eng = _engine(kind, 32, ban, post, pcm16)
            (wav, st), = eng.enhance([(mix, mask, im)])
            eng.close()
            err = pcm16_rel_rms(wav, ref) if pcm16 else rel_rms(wav, ref)
            print(f"{kind} ban={ban} post={post} itf={itf} C={C} N={N} pcm16={pcm16}: {err:.2e}")
            assert st == 0 and wav.shape == ref.shape
            assert wav.dtype == (np.int16 if pcm16 else np.float32)
            assert err < 1e-3, (kind, ban, post, itf, C, N, pcm16, err)


def test_ragged_batch_equals_single_calls_and_pcm_equals_float():
    from setk_amd.engine import Pcm16Frames
    rng = np.random.default_rng(3)
    shapes = [(4, 16384), (4, 20000), (2, 48000), (4, 9000), (2, 16500)]
    utts = []
    for k, (C, N) in enumerate(shapes):
        mix, sp, nz = o.synth_utterance(60 + k, C, N, return_parts=True)
        pcm = np.clip(np.rint(mix.T * 32768.0 * 0.9), -32768, 32767).astype(np.int16)
        mask = (0.05 + 0.9 * o.irm_mask(sp, nz)).astype(np.float32)
        utts.append((Pcm16Frames(pcm), mask, None if k % 2 else rng.uniform(0.1, 0.9, size=mask.shape)))
    for kind, chunk, ban in (("mvdr", 32, True), ("gevd", 33, False)):
        for pcm16 in (False, True):
            eng = _engine(kind, chunk, ban, True, pcm16)
            batch = eng.enhance(utts)
            singles = [eng.enhance([u])[0] for u in utts]
            floats = eng.enhance([(u[0].to_float(), u[1], u[2]) for u in utts])
            # a batch cut by bytes into several calls gives the same again
            eng.close()
            small = _engine(kind, chunk, ban, True, pcm16, max_batch_bytes=1 << 22)
            cut = small.enhance(utts)
            small.close()
            for k, (b, s, f, c) in enumerate(zip(batch, singles, floats, cut)):
                assert b[1] == s[1] == f[1] == c[1] == 0
                assert np.array_equal(b[0], s[0]), (kind, pcm16, k, "batch against single")
                assert np.array_equal(b[0], f[0]), (kind, pcm16, k, "16-bit against float input")
                assert np.array_equal(b[0], c[0]), (kind, pcm16, k, "one batch against several")
                assert np.max(np.abs(b[0])) > 0


def test_per_utterance_host_loop_meets_the_model():
    """The loop the CLI keeps for the geometries the engine does not take
    (libs.beamformer.Online* under do_online_beamform): its first parity test."""
    from setk_amd.libs import utils
    from setk_amd.libs.beamformer import OnlineGevdBeamformer, OnlineMvdrBeamformer
    from setk_amd.sptk.apply_adaptive_beamformer import do_online_beamform
    mix, mask = inputs(4, 20480)
    kw = dict(frame_len=512, frame_hop=256, window="hann", center=True, transpose=False)
    obs = np.stack([utils.forward_stft(x, round_power_of_two=True, **kw) for x in mix])
    for kind, cls in (("mvdr", OnlineMvdrBeamformer), ("gevd", OnlineGevdBeamformer)):
        for ban in (False, True):
            args = argparse.Namespace(chunk_size=32, alpha=ALPHA, ban=ban)
            enh = do_online_beamform(cls(257, 4, ALPHA), np.minimum(mask, 1), None, obs, args)
            wav = utils.inverse_stft(enh, norm=float(np.max(np.abs(mix))), **kw)
            ref = model_wave(4, 20480, 32, kind, ban, False, False)
            print(f"host loop {kind} ban={ban}: {rel_rms(wav, ref):.2e}")
            assert rel_rms(wav, ref) < 1e-3, (kind, ban)


def test_cli_online(tmp_path):
    import scipy.io.wavfile
    g = load_golden("ref_cli.npz")
    td = str(tmp_path)
    scipy.io.wavfile.write(os.path.join(td, "u0.wav"), 16000, g["u0.pcm"])
    np.save(os.path.join(td, "u0.npy"), g["u0.mask"])
    with open(os.path.join(td, "wav.scp"), "w") as f:
        f.write(f"u0 {td}/u0.wav\n")
    with open(os.path.join(td, "mask.scp"), "w") as f:
        f.write(f"u0 {td}/u0.npy\n")
    samps = (g["u0.pcm"].astype(np.float32) / 32768.0).T.copy()
    C = samps.shape[0]
    script = os.path.join(ROOT, "scripts", "sptk", "apply_adaptive_beamformer.py")
    base = [sys.executable, script, "--mask-format", "numpy", "--online.chunk-size", "32",
            "--online.channels", str(C)]
    tail = [os.path.join(td, "wav.scp"), os.path.join(td, "mask.scp")]
    # the batched engine, then (--vad-proportion) the per-utterance loop
    for name, extra, okw in (("engine", ["--ban", "true"], dict(ban=True)),
                             ("gevd", ["--beamformer", "gevd", "--post-masking", "true"],
                              dict(kind="gevd", post_mask=True)),
                             ("vad", ["--vad-proportion", "0.9"], dict(vad_proportion=0.9))):
        dst = os.path.join(td, name)
        r = subprocess.run(base + extra + tail + [dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert f"Using online {okw.get('kind', 'mvdr')} beamformer, chunk size = 32" in r.stderr
        assert "Processing utterance u0, signal power" in r.stderr
        assert "Processed 1 utterances out of 1" in r.stderr
        sr, y = scipy.io.wavfile.read(os.path.join(dst, "u0.wav"))
        ref = om.enhance_online(samps, g["u0.mask"], 32, ALPHA, **okw)
        err = pcm16_rel_rms(y, ref)
        print(f"cli {name}: {err:.2e}")
        assert sr == 16000 and y.dtype == np.int16 and y.shape == ref.shape
        assert err < 1e-3, (name, err)
    # a channel count that is not --online.channels: named, not a broadcasting error
    r = subprocess.run(base[:-1] + [str(C + 1)] + tail + [os.path.join(td, "bad")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and f"has {C} channels, --online.channels says {C + 1}" in r.stderr
    # --skip-existing leaves a finished file alone
    kept = os.path.join(td, "engine", "u0.wav")
    before = (os.stat(kept).st_mtime_ns, open(kept, "rb").read())
    r = subprocess.run(base + ["--ban", "true", "--skip-existing", "true"] + tail + [os.path.join(td, "engine")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "--skip-existing: 1 of 1 utterances already" in r.stderr
    assert (os.stat(kept).st_mtime_ns, open(kept, "rb").read()) == before


def test_refusals(ctx):
    from setk_amd import _ffi
    from setk_amd.engine import BatchOnlineEnhancer
    mix, mask = inputs(4, N_TAPS)
    with pytest.raises(_ffi.SetkUnsupported, match="1 <= num_channels <= 8"):
        nine = o.synth_utterance(39, 9, N_TAPS)
        _engine("mvdr", 32).enhance([(nine, mask, None)])
    with pytest.raises(_ffi.SetkUnsupported, match="the online beamformer is MVDR or GEVD"):
        run_abi(ctx, "pmwf-0", 32, mix, mask, taps=False)
    with pytest.raises(_ffi.SetkUnsupported, match="only the n_fft = 512 kernels are built"):
        eng = BatchOnlineEnhancer(chunk_size=32, frame_len=400, frame_hop=160, round_power_of_two=False,
                                  ctx=_ffi.Context(0))
        T = 1 + N_TAPS // 160
        eng.enhance([(mix, np.full((T, 201), 0.5, np.float32), None)])
    with pytest.raises(ValueError, match="chunk_size must be at least 1"):
        run_abi(ctx, "mvdr", 0, mix, mask, taps=False)
    with pytest.raises(ValueError, match=r"alpha must lie in \[0, 1\)"):
        run_abi(ctx, "mvdr", 32, mix, mask, alpha=1.0, taps=False)
    # the handle is as usable as before
    wav, st, _ = run_abi(ctx, "mvdr", 32, mix, mask, taps=False)
    assert st == 0 and np.max(np.abs(wav)) > 0
