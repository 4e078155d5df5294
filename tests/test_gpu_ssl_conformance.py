"""
Conformance of mask-based sound source localisation on the MI355X (setk_amd/csrc/ssl.hip,
capi_ssl.hip) through libs.ssl.ssl_spectrum and the batch entry, on the constructed cases of
ssl_cases.py.  Every (window, direction) score is judged against the float64 reference there at
min(A, 1e-4 x spread of its window's reference spectrum), A the derived allowance of that cell;
where the reference is not finite the device must be non-finite in exactly the same cells; every
index must be the lowest direction attaining the extremum of the device's own scores, a non-finite
score counting as the extremum.  test_ssl_cases.py shows on the CPU that a float32 model of the
kernels passes this judge on the same cases and that twelve seeded faults fail it.  Every test
prints its worst error / allowance and the cell before it asserts.  Figures: PARITY_NOTES_SSL.md.
"""
import numpy as np
import pytest

import ssl_cases as sc

pytestmark = pytest.mark.gpu


def run_device(case):
    from setk_amd.libs.ssl import ssl_spectrum
    c = case
    return ssl_spectrum(c.backend, c.x, c.sv, mask=c.mask, srp_pair=sc.pair_lists(c.pairs) if c.pairs else None,
                        windows=c.windows, **(c.kw or {}))


def run_and_judge(tally, case):
    """-> (expected, index, scores); the input conditions of the case are asserted on the way"""
    exp = sc.expected(case)
    if case.needs_delta:
        assert exp["delta_ratio"] >= sc.DELTA_FLOOR, (case.name, exp["delta_ratio"])
    if case.backend == "music":
        assert exp["gap"] >= case.min_gap and tuple(exp["dead"]) == tuple(case.dead_bins), (case.name, exp["gap"], exp["dead"])
    idx, got, status = run_device(case)
    sc.evaluate(case, exp, idx, got, tally, status)
    return exp, idx, got


# ---------------------------------------------------------------- every channel count
@pytest.mark.parametrize("backend", sc.BACKENDS)
@pytest.mark.parametrize("C", range(1, 17))
def test_every_channel_count(C, backend):
    """C = 1 .. 16 with all pairs (K = 1 .. 120; one channel: the pair (0, 0)), every single frame and
    the whole utterance."""
    tally = sc.Tally(f"channels {backend} C={C}")
    for case in sc.channel_cases(C, backend):
        exp, idx, got = run_and_judge(tally, case)
        if C == 1 and backend != "srp":
            # one channel: the reference's spectrum does not depend on the direction, its index is 0
            assert not sc.spreads(exp["ref"]).any() and not exp["idx"].any()
            if backend == "music":
                assert not np.asarray(got).any() and not idx.any(), (idx, np.abs(got).max())
    tally.finish()


# ---------------------------------------------------------------- tile edges, one axis at a time
@pytest.mark.parametrize("backend", sc.BACKENDS)
@pytest.mark.parametrize("axis,value", sc.EDGES)
def test_tile_edges(axis, value, backend):
    """The 32-frame tile, the 32-bin patch, the 64-direction wave and the 256-thread window
    reduction: on, below and above each, at 3 and 8 channels, the other two axes held small."""
    tally = sc.Tally(f"edge {backend} {axis}={value}")
    for case in sc.edge_cases(axis, value, backend):
        run_and_judge(tally, case)
    tally.finish()


@pytest.mark.parametrize("backend", sc.BACKENDS)
def test_one_hot_bins(backend):
    """One term of the sum over the bins, at bins 0, 31, 32 and F - 1."""
    tally = sc.Tally(f"one-hot {backend}")
    for case in sc.onehot_cases(backend):
        run_and_judge(tally, case)
    tally.finish()


# ---------------------------------------------------------------- the offline SRP fold against the frame path
def test_offline_srp_fold():
    """A single window goes through the float64 fold, the same window in a table of two through the
    frame scores: both against the reference, and against each other at the sum of their allowances."""
    tally = sc.Tally("srp fold")
    for one, two in sc.fold_cases():
        e1, _, g1 = run_and_judge(tally, one)
        e2, _, g2 = run_and_judge(tally, two)
        with np.errstate(all="ignore"):
            ratio = np.abs(g1[0] - g2[0]) / (e1["A"][0] + e2["A"][0])
        a = int(np.argmax(ratio))
        print(f"{one.name}: fold against frames, worst difference / (sum of allowances) {ratio[a]:.3f} at direction {a}")
        if not ratio[a] <= 1.0:
            tally.fail([f"{one.name}: the two SRP paths differ by {abs(g1[0][a] - g2[0][a]):.3e} at direction {a}, "
                        f"allowances {e1['A'][0][a]:.3e} + {e2['A'][0][a]:.3e}"])
    tally.finish()


# ---------------------------------------------------------------- ML options
def test_ml_options():
    """The log form at three eps, the power form at three exponents, with and without norm, on the
    ladder; `extreme` (2^100 .. 2^-100) under norm; `aligned` under the range rule."""
    tally = sc.Tally("ml options")
    for case in sc.ml_option_cases():
        run_and_judge(tally, case)
    tally.finish()


# ---------------------------------------------------------------- every family
@pytest.mark.parametrize("C", [2, 5, 16])
@pytest.mark.parametrize("backend", sc.BACKENDS)
def test_families(backend, C):
    tally = sc.Tally(f"families {backend} C={C}")
    for case in sc.family_cases(backend, C):
        exp, idx, got = run_and_judge(tally, case)
        if case.family == "nan":
            assert not np.isfinite(exp["ref"]).all()
    tally.finish()


# ---------------------------------------------------------------- ties and NaN at A = 513
@pytest.mark.parametrize("backend", sc.BACKENDS)
def test_exact_ties(backend):
    """Copies of the best steer vector at directions of one thread's strided loop (44 and 300), of
    both sides of the 256-thread edge and at the last of 513: bit-equal scores, the lowest index."""
    tally = sc.Tally(f"ties {backend}")
    for case, best, pos in sc.tie_cases(backend):
        exp, idx, got = run_and_judge(tally, case)
        same = sorted(set(pos) | {best})
        bits = got[:, same].view(np.uint64)
        print(f"{case.name}: best {best}, copies at {pos}: index {idx.tolist()}")
        if not (bits == bits[:, :1]).all():
            tally.fail([f"{case.name}: the copies' scores differ: {got[:, same]!r}"])
        if int(idx[0]) != same[0]:
            tally.fail([f"{case.name}: index {int(idx[0])}, the lowest copy is {same[0]}"])
    tally.finish()


@pytest.mark.parametrize("backend", sc.BACKENDS)
def test_nan_inputs(backend):
    """A NaN in the spectrogram or the mask makes every direction of the frames it touches a NaN (index
    0); a NaN in a steer vector exactly that direction, and the index the lowest such direction."""
    tally = sc.Tally(f"nan {backend}")
    for case in sc.nan_cases(backend):
        exp, idx, got = run_and_judge(tally, case)
        bad = ~np.isfinite(exp["ref"])
        assert bad.any()
        print(f"{case.name}: non-finite cells {int(bad.sum())} (device {int((~np.isfinite(got)).sum())}), "
              f"index {idx.tolist()} (reference {exp['idx'].tolist()})")
    tally.finish()


# ---------------------------------------------------------------- MUSIC window tables
def test_music_windows():
    """Eight windows (single frames, t0 > 0, tile-straddling) at F = 33; eigenvalues 1e-3 apart; two
    bins of zero covariance (status non-OK, the other bins judged)."""
    tally = sc.Tally("music windows")
    for case in sc.music_window_cases():
        run_and_judge(tally, case)
    tally.finish()


# ---------------------------------------------------------------- the batch entry
BATCH_FRAMES = (32, 33, 64, 65)
BATCH_A = 9


def batch_geometry(C):
    """(delays in samples, gains) of the microphones: the same array for every utterance"""
    rng = np.random.default_rng([6, C])
    return rng.integers(0, 64, size=C), 0.5 + 0.5 * rng.uniform(size=C)


def batch_audio(C, T):
    """float32 [C][256 (T - 1)]: one source, delayed and scaled per microphone, plus a tenth of noise
    (MUSIC needs a principal direction in every bin)."""
    rng = np.random.default_rng([5, C, T])
    N = 256 * (T - 1)
    src = rng.standard_normal(N + 64)
    delays, gains = batch_geometry(C)
    x = np.stack([g * src[64 - d:64 - d + N] for d, g in zip(delays, gains)])
    return (0.1 * (x + 0.1 * rng.standard_normal((C, N)))).astype(np.float32)


def batch_steer(C, F, A):
    """Random steer vectors, two of them near the source: its delays and gains with the moduli moved
    by 30 % (ML's delta then stays above its floor), and that again with a phase ramp over the
    microphones.  Without them the spectra of 16 channels have next to no spread, and the float32 sum
    over 257 bins of a single frame is as large as 1e-4 of it."""
    sv = sc.random_steer(A, C, F)
    delays, gains = batch_geometry(C)
    d = gains[:, None] * np.exp(-2j * np.pi * np.arange(F)[None, :] * delays[:, None] / 512.0)
    d = d * (1 + 0.3 * np.where(np.arange(C) % 2, -1.0, 1.0))[:, None]
    sv[A // 3] = d
    sv[A // 3 + 1] = d * np.exp(0.2j * np.arange(C))[:, None]
    return sv


def batch_call(ctx, opts, C, audio, masks, sv, windows):
    """One setk_ssl_batch call on device tensors -> (index [sum W], score [sum W][A], status [n])"""
    import torch
    da = [torch.from_numpy(a).cuda() for a in audio]
    dm = [None if m is None else torch.from_numpy(m).cuda() for m in masks]
    dsv = torch.from_numpy(sv).cuda()
    W = sum(len(w) for w in windows)
    score = torch.full((W, sv.shape[0]), float("nan"), dtype=torch.float64, device="cuda")
    index = torch.full((W,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((len(audio),), -1, dtype=torch.int32, device="cuda")
    ctx.ssl_batch(opts, C, [a.data_ptr() for a in da], [a.shape[1] for a in audio],
                  [None if m is None else m.data_ptr() for m in dm], dsv, sv.shape[0], windows, index.data_ptr(),
                  score=score.data_ptr(), status=status.data_ptr())
    torch.cuda.synchronize()
    return index.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("backend", sc.BACKENDS)
@pytest.mark.parametrize("C", [1, 8, 9, 16])
def test_batch_entry(C, backend):
    """setk_ssl_batch (n_fft = 512, F = 257) on ragged utterances of 32, 33, 64 and 65 frames, two of
    them masked: one window per utterance (SRP: the fold, its grid sized by the longest utterance) and
    window tables.  The reference is evaluated on the spectrogram setk_stft returns for the same audio:
    what is judged is the localisation and the channel groups' spec_dump plumbing beyond 8 channels."""
    from setk_amd import _ffi
    ctx = _ffi.default_context()
    ctx.stft_plan(512, 256, 512, True, None)
    F, A = 257, BATCH_A
    audio = [batch_audio(C, T) for T in BATCH_FRAMES]
    masks = [sc.mask(T, F) if k % 2 == 0 else None for k, T in enumerate(BATCH_FRAMES)]
    sv = batch_steer(C, F, A)
    pairs = [(0, C - 1), (C // 2, 0), (C - 1, C // 2), (0, 0)] if C > 1 else [(0, 0)]
    kw = dict(sc.ML_CLI) if backend == "ml" else {}
    opts = _ffi.ssl_opts(backend, srp_pair=sc.pair_lists(pairs), **kw)
    specs = []
    for a, T in zip(audio, BATCH_FRAMES):
        assert ctx.num_frames(a.shape[1]) == T
        X = np.empty((C, T, F), np.complex64)
        ctx.stft(a, X)
        specs.append(X)
    tally = sc.Tally(f"batch {backend} C={C}")
    for mode in ("one window", "table"):
        tables = [[(0, T)] if mode == "one window" else [(0, T), (0, 1), (T - 1, T), (30, T), (31, 32)]
                  for T in BATCH_FRAMES]
        idx, score, status = batch_call(ctx, opts, C, audio, masks, sv, tables)
        idx2, score2, _ = batch_call(ctx, opts, C, audio, masks, sv, tables)
        if not (np.array_equal(idx, idx2) and score.tobytes() == score2.tobytes()):
            tally.fail([f"{mode}: a second run of the batch gave other bytes"])
        w0 = 0
        for k, T in enumerate(BATCH_FRAMES):
            W = len(tables[k])
            case = sc.Case(f"batch {mode} utterance {k} (T={T}) {backend} C={C}", backend, "audio", specs[k], sv,
                           masks[k], tables[k], pairs if backend == "srp" else None, kw or None,
                           rule="range" if (backend == "ml" and C == 1) else "ref",
                           needs_delta=backend == "ml" and C > 1)
            exp = sc.expected(case)
            if case.needs_delta:
                assert exp["delta_ratio"] >= sc.DELTA_FLOOR, (case.name, exp["delta_ratio"])
            if backend == "music" and C > 1:
                assert exp["gap"] >= case.min_gap and not exp["dead"], (case.name, exp["gap"], exp["dead"])
            sc.evaluate(case, exp, idx[w0:w0 + W], score[w0:w0 + W], tally, int(status[k]))
            i1, s1, _ = batch_call(ctx, opts, C, [audio[k]], [masks[k]], sv, [tables[k]])
            if not (np.array_equal(i1, idx[w0:w0 + W]) and s1.tobytes() == score[w0:w0 + W].tobytes()):
                tally.fail([f"{case.name}: the utterance alone gave other bytes than in the batch"])
            w0 += W
    tally.finish()
