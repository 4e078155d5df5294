"""
Conformance of the WPE step (setk_amd/csrc/wpe.hip) on the constructed cases of wpe_cases.py:
every kernel form -- the thirteen LDS instantiations at each chunk size they occur with, and the
global-memory form -- against an np.clongdouble restatement of the step, judged per (bin, channel):

    ||got - ref||_2 <= 2^-24 ||ref_fc||_2 + 4 u_fc

(wpe_cases.py: u is the larger error of the complex128 oracle and of a float64 model of the
kernel's arithmetic; test_wpe_cases.py shows on the CPU that the bar fails seven seeded kernel
faults).  Then the exact properties -- isolated impulses, power-of-two scalings, independence of
bins and of utterances -- the variances the device estimates itself, the [C][T][F] layout entry,
two iterations, and the degenerate inputs.  Which form a shape runs is asked of the library
(setk_wpe_form).  Measured figures: tests/PARITY_NOTES_WPE.md.
"""
import numpy as np
import pytest

import wpe_cases as wc

pytestmark = pytest.mark.gpu

CASES = wc.all_cases()
METAMORPHIC = [wc.Case(2, 4, 129), wc.Case(9, 10, 161), wc.Case(6, 16, 177), wc.Case(8, 12, 193)]


def _ctx():
    from setk_amd import _ffi
    return _ffi.default_context()


def run_step(x, lam, taps, delay):
    """x [F][N][T] complex64, lam [F][T] float64 through setk_wpe_step -> (out [F][N][T], status)"""
    F, N, T = x.shape
    spec = np.ascontiguousarray(np.transpose(x, (1, 2, 0)))
    out = np.empty_like(spec)
    st = np.full(F, -1, np.int32)
    _ctx().wpe_step(spec, N, T, F, taps, delay, np.ascontiguousarray(lam, dtype=np.float64), out, status=st)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))), st


def run_fnt(xs, taps, delay, context, iters):
    """list of [F][N][T_u] complex64 through setk_wpe_batch_fnt -> (outs, status [n][F])"""
    xs = [np.ascontiguousarray(x) for x in xs]
    F, N, _ = xs[0].shape
    outs = [np.empty_like(x) for x in xs]
    st = np.full((len(xs), F), -1, np.int32)
    _ctx().wpe_batch_fnt(xs, N, [x.shape[2] for x in xs], F, taps, delay, context, iters, outs, status=st)
    return outs, st


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(wc.bits(a), wc.bits(b))


@pytest.mark.parametrize("ch,taps", list(wc.SHAPES), ids=[f"{c}x{t}" for c, t in wc.SHAPES])
def test_step_under_the_judge(ch, taps):
    from setk_amd import _ffi
    wide, ntw, tc = _ffi.wpe_form(ch, taps)
    assert ("wide" if wide else ntw, tc) == wc.SHAPES[(ch, taps)]
    worst, fails = {}, []
    for c in CASES:
        if (c.ch, c.taps) != (ch, taps):
            continue
        R = wc.reference(c)
        got, st = run_step(R.x, R.lam, taps, c.delay)
        for f in range(wc.F):
            w, bad = wc.judge(c.name, got, st, R, bins=[f])
            fam = wc.family_of_bin(c, f)
            worst[fam] = max(worst.get(fam, 0.0), w)
            fails += bad
    form = "wide" if wide else f"NTW {ntw}"
    print(f"[step {ch}x{taps}, {form}, TC {tc}] worst ratio " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not fails, fails[:6]


def test_table_reaches_every_form():
    """Every (instantiation, chunk size) pair any supported shape selects, and the wide form, is
    run by a case of the table: a later change to the dispatcher cannot silently uncover one."""
    from setk_amd import _ffi
    reachable = set()
    for ch in range(1, 17):
        for taps in range(1, 257):
            form = _ffi.wpe_form(ch, taps)
            if form is not None:
                reachable.add(("wide", form[2]) if form[0] else (form[1], form[2]))
    run = set()
    for c in CASES:
        wide, ntw, tc = _ffi.wpe_form(c.ch, c.taps)
        run.add(("wide", tc) if wide else (ntw, tc))
    print("[forms run] " + " ".join(f"{n}/{tc}" for n, tc in sorted(run, key=str)))
    assert run == reachable, sorted(reachable - run, key=str)
    assert {n for n, _ in run} == {1, 2, 3, 4, 5, 8, 10, 12, 14, 17, 20, 23, 26, "wide"}
    assert {tc for _, tc in run} == {16, 32, 64}
    assert {(23, 64), (23, 32), (23, 16), (26, 32), (26, 16), ("wide", 64)} <= run


def test_isolated_impulses_come_back_bit_for_bit():
    for ch, taps, delay, tc in wc.IMPULSE_SHAPES:
        x, lam = wc.impulses(ch, taps, delay, tc)
        got, st = run_step(x, lam, taps, delay)
        assert not st.any(), (ch, taps, st)
        assert same_bits(got, x), (ch, taps, delay, np.argwhere(wc.bits(got) != wc.bits(x))[:4])
    print(f"[impulses] {len(wc.IMPULSE_SHAPES)} shapes: output == input, bit for bit")


@pytest.mark.parametrize("case", METAMORPHIC, ids=[c.name for c in METAMORPHIC])
def test_power_of_two_scalings_and_bin_independence(case):
    """x 2^k scales the result bit for bit (R and r scale together, the rank floor is relative);
    lambda 2^j leaves it unchanged bit for bit (j even: the square roots of the factorisation then
    scale by 2^(j/2) exactly); a bin run alone equals the same bin inside the stack."""
    R = wc.reference(case)
    base, st = run_step(R.x, R.lam, case.taps, case.delay)
    assert not st.any()
    for k in (-40, 30):
        s = np.float32(2.0 ** k)
        got, st = run_step(R.x * s, R.lam, case.taps, case.delay)
        assert not st.any() and same_bits(got, base * s), (case.name, k)
    for j in (20, -30):
        got, st = run_step(R.x, R.lam * 2.0 ** j, case.taps, case.delay)
        assert not st.any() and same_bits(got, base), (case.name, j)
    for f in range(wc.F):
        got, st = run_step(R.x[f:f + 1], R.lam[f:f + 1], case.taps, case.delay)
        assert not st.any() and same_bits(got[0], base[f]), (case.name, f)
    print(f"[metamorphic {case.name}] x 2^-40, 2^30; lambda 2^20, 2^-30; each bin alone: bit for bit")


@pytest.mark.parametrize("shape,frames", wc.RAGGED, ids=[f"{s[0]}x{s[1]}" for s, _ in wc.RAGGED])
def test_ragged_batch(shape, frames):
    """setk_wpe_batch_fnt, one iteration, context 1: every utterance of a ragged batch equals the
    same utterance run alone, bit for bit, and stands under the judge -- the variances are the
    device's own float32 estimate here, so the allowance grows by what the reference itself
    answers a relative (C + 2 ctx + 3) 2^-24 on every lambda_t with."""
    ch, taps = shape
    tc = wc.SHAPES[shape][1]
    xs = [wc.make_case(wc.Case(ch, taps, T))[0][:2] for T in frames]       # white, ladder
    outs, st = run_fnt(xs, taps, 3, 1, 1)
    assert not st.any()
    worst = 0.0
    for u, x in enumerate(xs):
        alone, st1 = run_fnt([x], taps, 3, 1, 1)
        assert not st1.any() and same_bits(alone[0], outs[u]), (shape, u)
        lam = wc.compute_lambda64(x, 1)
        R = wc.Reference(x, lam, taps, 3, tc)
        sens = wc.lambda_sensitivity(x, lam, taps, 3, wc.lambda_rel_bound(ch, 1), seed=u)
        w, fails = wc.judge(f"ragged {ch}x{taps} T={x.shape[2]}", outs[u], st[u], R, extra=sens)
        assert not fails, fails[:4]
        worst = max(worst, w)
    print(f"[ragged {ch}x{taps} T={frames}] alone == in the batch; worst ratio {worst:.3f}")


def test_estimated_variances():
    """1 / lambda as setk_wpe returns it (float32 [T][F]) against 1 / compute_lambda in float64:
    relative error (C + 2 ctx + 3) 2^-24 (wpe_cases.lambda_rel_bound); a frame whose whole
    context is silent gives exactly 1 / eps_f32 = 2^23."""
    ctx = _ctx()
    F, worst, silent = 3, 0.0, 0
    for C in (1, 3, 16):
        for cx in (0, 1, 2, 3):
            for T in sorted({1, 2, max(cx, 1), 255, 256, 257}):
                rng = np.random.default_rng([C, cx, T])
                x = wc._cnormal(rng, F, C, T)
                x[1] *= 3e-4                                   # powers around the floor
                if T > 200:
                    x[:, :, 100 - cx - 1:100 + cx + 2] = 0.0   # frame 100: a silent context
                    x[2, :, 150:] *= 1e-5                      # far below the floor
                x = x.astype(np.complex64)
                spec = np.ascontiguousarray(np.transpose(x, (1, 2, 0)))
                inv = np.full((T, F), -1.0, np.float32)
                ctx.wpe(spec, C, T, F, 1, 1, cx, 1, np.empty_like(spec), inv_lambda_out=inv)
                lam = wc.compute_lambda64(x, cx)               # [F][T]
                want = 1.0 / lam.T
                rel = np.abs(inv.astype(np.float64) - want) / want
                worst = max(worst, float(rel.max() / wc.lambda_rel_bound(C, cx)))
                assert rel.max() <= wc.lambda_rel_bound(C, cx), (C, cx, T, rel.max())
                quiet = lam.T == wc.EPS32
                assert (inv[quiet] == np.float32(2.0 ** 23)).all(), (C, cx, T)
                silent += int(quiet.sum())
                if T > 200:
                    assert quiet[100].all() and quiet[160:250, 2].all()
    assert silent > 0
    print(f"[variances] worst error {worst:.3f} of (C + 2 ctx + 3) 2^-24; {silent} floored cells exactly 2^23")
    # lambda from a previous enhanced signal: max(|enh|^2, eps) in fp64 (exact products of
    # float32 values, one fp64 rounding of the sum and one of the reciprocal), rounded once to
    # float32: 2^-24 (1 + 2^-20)
    C, T = 3, 97
    rng = np.random.default_rng(5)
    x = wc._cnormal(rng, C, T, F).astype(np.complex64)
    enh = wc._cnormal(rng, T, F)
    enh[:, 1] *= 3e-4
    enh[10:20, 2] *= 1e-6
    enh[30:33] = 0.0
    enh = enh.astype(np.complex64)
    inv = np.full((T, F), -1.0, np.float32)
    ctx.wpe(x, C, T, F, 2, 1, 1, 1, np.empty_like(x), lambda_enh=enh, inv_lambda_out=inv)
    e = enh.astype(np.complex128)
    want = 1.0 / np.maximum(e.real ** 2 + e.imag ** 2, wc.EPS32)
    rel = np.abs(inv.astype(np.float64) - want) / want
    assert rel.max() <= wc.U32 * (1 + 2.0 ** -20), rel.max()
    assert (inv[30:33] == np.float32(2.0 ** 23)).all() and (inv[10:20, 2] == np.float32(2.0 ** 23)).all()
    print(f"[variances from enh] worst error {rel.max() / wc.U32:.3f} of 2^-24")


def test_library_layout_equals_the_reference_layout():
    """setk_wpe ([C][T][F]: two tiled transposes around the step) against setk_wpe_batch_fnt
    (F x N x T, none), two iterations, bit for bit; bins and frames on both sides of the 32 x 32
    transpose tile."""
    ctx = _ctx()
    C, n = 3, 0
    for F in (1, 31, 33, 65):
        for T in (33, 63, 97):
            rng = np.random.default_rng([F, T])
            x = wc._cnormal(rng, F, C, T).astype(np.complex64)
            spec = np.ascontiguousarray(np.transpose(x, (1, 2, 0)))
            out = np.empty_like(spec)
            st = np.full(F, -1, np.int32)
            ctx.wpe(spec, C, T, F, 3, 1, 1, 2, out, status=st)
            outs, st2 = run_fnt([x], 3, 1, 1, 2)
            assert not st.any() and not st2.any()
            assert same_bits(np.ascontiguousarray(np.transpose(out, (2, 0, 1))), outs[0]), (F, T)
            n += 1
    print(f"[layout] {n} (F, T) pairs: [C][T][F] entry == F x N x T entry, bit for bit")


@pytest.mark.parametrize("case", METAMORPHIC[:2] + METAMORPHIC[3:], ids=lambda c: c.name)
def test_two_iterations(case):
    """num_iters = 2, context 1, white and ladder families, against the extended chain that rounds
    to complex64 between the steps as the device does.  Bar: the judge's, for the second step on
    the chain's own variances, plus the chain's answer to a relative (C + 2 ctx + 3) 2^-24 on
    every lambda_t of both steps -- a property of the reference alone."""
    x = wc.reference(case).x[:2]
    outs, st = run_fnt([x], case.taps, case.delay, 1, 2)
    last, lam1 = wc.chain(x, case.taps, case.delay, 1, 2)
    moved, _ = wc.chain(x, case.taps, case.delay, 1, 2, rel=wc.lambda_rel_bound(case.ch, 1))
    R = wc.Reference(x, lam1, case.taps, case.delay, case.tc)
    sens = wc._norm_t(moved - last)
    w, fails = wc.judge(f"two iterations {case.name}", outs[0], st[0], R, extra=sens)
    print(f"[two iterations {case.name}] worst ratio {w:.3f}; sensitivity / ||ref|| up to "
          f"{float((sens / R.norm).max()):.2e}, u / ||ref|| up to {float((R.u / R.norm).max()):.2e}")
    assert not fails, fails[:4]


def test_degenerate_inputs():
    from setk_amd import _ffi
    c = wc.Case(6, 5, 129)
    # a bitwise-duplicated channel: rank deficient, reported, finite; the fitted values are unique
    x, lam, want = wc.duplicated_channel(c)
    got, st = run_step(x, lam, c.taps, c.delay)
    assert list(st) == [_ffi.NUM_RANKDEF] and np.isfinite(got).all()
    twins = (wc.rel_rms(got[:, 0], want[:, 0]), wc.rel_rms(got[:, -1], want[:, -1]))
    assert max(twins) < 1e-4 and wc.rel_rms(got, want) < 1e-4, twins
    print(f"[duplicated channel] status {int(st[0])}; twins against the utterance without the twin "
          f"{twins[0]:.2e} {twins[1]:.2e}; all channels {wc.rel_rms(got, want):.2e}")
    # an all-zero channel: exactly zero out, the others as without it
    x, lam, want = wc.silent_channel(c)
    got, st = run_step(x, lam, c.taps, c.delay)
    assert list(st) == [_ffi.NUM_RANKDEF] and not wc.bits(got[0, -1]).any()
    assert wc.rel_rms(got, want) < 1e-4
    print(f"[silent channel] status {int(st[0])}; exactly zero; the others {wc.rel_rms(got, want):.2e}")
    # a NaN in one bin: that bin is singular and comes back unchanged, the others are judged
    x, lam = wc.with_nan_bin(c, f=1)
    got, st = run_step(x, lam, c.taps, c.delay)
    assert list(st) == [0, _ffi.NUM_SINGULAR, 0, 0], st
    assert same_bits(got[1], x[1])
    w, fails = wc.judge("NaN bin: the others", got, st, wc.reference(c), bins=[0, 2, 3])
    assert not fails, fails[:4]
    print(f"[NaN bin] status {list(map(int, st))}; the bin returns x; the others' worst ratio {w:.3f}")
