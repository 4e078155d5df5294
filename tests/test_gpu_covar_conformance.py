"""
Conformance of the masked spatial covariance in its device forms -- the stand-alone operator
(setk_covar: covar_spec_kernel<1..8>, covar_spec_wide_kernel at 9..16), the fused fold of pass 1
(covar_fold.h, 1..8 channels, under two slab cuts), the matrix-core fold of wide.hip (9..16,
every count) and the block-online recursion (online.hip) -- on the constructed cases of
covar_cases.py, judged per bin, entry and part against compute_covar in complex128:

    |got - ref| <= A = (T + 8) 2^-24 (S_ij + |Phi_ij| Sm) / den       (+ A_fwd for the fused forms)

and exactly 0 where A == 0; every result exactly Hermitian with a real diagonal, and finite.
test_covar_cases.py shows on the CPU that this bar fails six seeded faults in bins the global
rel_rms of the older tests cannot see.  Measured figures: PARITY_NOTES_COVAR.md.
"""
import os

import numpy as np
import pytest

import covar_cases as cc
import stft_cases as sc
from conftest import rel_rms
from oracle import np_oracle as o

pytestmark = pytest.mark.gpu
F = cc.BINS


def new_ctx():
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(512, cc.HOP, 512, True)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    c.close()


class fresh_handle:
    """A fresh handle created under an environment switch of INTEGRATION.md (read at creation)."""

    def __init__(self, switch):
        self.switch = switch

    def __enter__(self):
        self.old = {}
        for kv in filter(None, self.switch.split(",")):
            k, v = kv.split("=")
            self.old[k] = os.environ.get(k)
            os.environ[k] = v
        self.ctx = new_ctx()
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def check(tally, family, name, got, ref, A):
    tally.fail(cc.structure(name, got))
    tally.add(family, cc.judge(name, got, ref, A))


# ---------------------------------------------------------------- stand-alone setk_covar
@pytest.mark.parametrize("C", range(1, 17))
def test_standalone_covar(ctx, C):
    """The device gets the very complex64 spectrogram the reference folds: the sharp judgement of
    the arithmetic.  covar_spec_kernel<C> up to 8 channels, covar_spec_wide_kernel above."""
    tally = cc.Tally(f"setk_covar C={C}")
    for case in cc.standalone_cases(C):
        x, m = cc.standalone_inputs(case)
        got = np.full((case.F, C, C), np.nan, np.complex64)
        ctx.covar(x, m, C, case.T, case.F, got)
        ref = cc.reference(x, m)
        check(tally, f"{case.spec}/{case.mask}", case.name, got, ref, cc.allowance(x, m, ref))
    tally.finish()


# ---------------------------------------------------------------- the fused forms
def run_fused(c, C, cases, kind=None, pcm=False, audio=None, masks=None):
    """One setk_enhance_batch_taps call (MVDR unless told) on the cases, which share the plan, the
    clamp flag and whether they bring a noise mask.  Returns (status, Rs, Rn, weight)."""
    import torch
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    n = len(cases)
    flags = _ffi.FLAG_CLAMP_MASK if cases[0].clamp else 0
    if audio is None:
        audio = [cc.spectra(k.audio, C, k.T)[0] for k in cases]
        masks = [cc.fused_masks(k)[:2] for k in cases]
    ns = [a.shape[1] for a in audio]
    if pcm:
        a = [torch.zeros((C, c.pcm16_channel_stride(k)), dtype=torch.int16, device=dev) for k in ns]
        for t, u in zip(a, audio):
            t[:, :u.shape[1]] = torch.from_numpy(np.array(u)).to(dev)
        flags |= _ffi.FLAG_IN_PCM16
    else:
        a = [torch.from_numpy(cc.as_float(u) if u.dtype == np.int16 else np.array(u, dtype=np.float32)).to(dev)
             for u in audio]
    ms = [torch.from_numpy(np.ascontiguousarray(k[0])).to(dev) for k in masks]
    mn = [torch.from_numpy(np.ascontiguousarray(k[1])).to(dev) for k in masks] if masks[0][1] is not None else None
    outs = [torch.zeros(max(c.istft_num_samples(c.num_frames(k)), 1), dtype=torch.float32, device=dev) for k in ns]
    tp = dict(Rs=torch.full((n, F, C, C), float("nan"), dtype=torch.complex64, device=dev),
              Rn=torch.full((n, F, C, C), float("nan"), dtype=torch.complex64, device=dev),
              weight=torch.zeros((n, F, C), dtype=torch.complex64, device=dev))
    opts = _ffi.BfOpts(kind=_ffi.BF_MVDR if kind is None else kind, flags=flags, pmwf_ref=-1)
    st = c.enhance_batch(opts, C, [t.data_ptr() for t in a], ns, [t.data_ptr() for t in ms],
                         [t.data_ptr() for t in mn] if mn else None, [t.data_ptr() for t in outs], taps=tp)
    torch.cuda.synchronize()
    return st, tp["Rs"].cpu().numpy(), tp["Rn"].cpu().numpy(), tp["weight"].cpu().numpy()


def groups_of(cases, by_frames=False):
    """The cases cut into calls: one per (plan, clamp flag, noise mask or none), and per frame
    count when asked."""
    g = {}
    for k in cases:
        g.setdefault((k.center, k.clamp, k.mn is not None, k.T if by_frames else 0), []).append(k)
    return g


_expect = {}


def expectation(case):
    """The float64 references and allowances of a fused case, computed once per module."""
    if case not in _expect:
        _expect[case] = cc.fused_expectation(case)
    return _expect[case]


def status_must_be_zero(case):
    """The solve may report a bin whose Rs or Rn is all zero, indefinite or short of rank.  The
    status is held to 0 where the case is built to have none (covar_cases.FusedCase.well_posed) and
    its float64 matrices confirm it: Rs non-zero and cond(Rn) < 1e4 in every bin, the project's
    measure of a well-posed bin (test_gpu_wide_fused.py).  A clamped `over` mask at a handful of
    frames is the case that needs the second look: a bin whose every value is >= 1 has no noise."""
    if not case.well_posed:
        return False
    (_, Rs, _), (_, Rn, _) = expectation(case)
    ev = np.linalg.eigvalsh(Rn)
    return bool((np.abs(Rs).max(axis=(1, 2)) > 0).all() and (ev[:, 0] * 1e4 > ev[:, -1]).all())


def fused_under_the_judge(tally, c, C, cases, tag, pcm=False, by_frames=False):
    """Every case through the fused call in a few ragged batches (by_frames: batches of one frame
    count each); Rs and Rn of each judged whatever the solve's status is; the status asserted 0 on
    the well-posed cases.  Returns the taps' bytes per case."""
    taps = {}
    for (center, _, _, _), group in groups_of(cases, by_frames).items():
        c.stft_plan(512, cc.HOP, 512, center)
        st, Rs, Rn, _ = run_fused(c, C, group, pcm=pcm)
        for i, k in enumerate(group):
            taps[k] = (Rs[i].tobytes(), Rn[i].tobytes())
            if pcm:
                continue
            for (name, ref, A), got in zip(expectation(k), (Rs[i], Rn[i])):
                check(tally, k.label, f"{k.name} {name} [{tag}]", got, ref, A)
            if status_must_be_zero(k) and st[i] != 0:
                tally.fail([f"{k.name} [{tag}]: status {st[i]} on a well-posed case"])
    c.stft_plan(512, cc.HOP, 512, True)
    if not pcm:
        print(f"[{tally.form}] [{tag}] status held to 0 on {sum(status_must_be_zero(k) for k in cases)} "
              f"of {len(cases)} cases")
    return taps


@pytest.mark.parametrize("C", range(1, 9))
def test_fused_fold(ctx, C):
    """pass 1's register fold: tiles of pass1_tile_frames(C) frames inside the slabs of the default
    handle, then of a handle under SETK_P1_ITEMS=1; PCM16 input on the same cases gives the float
    form's taps bit for bit.

    The slab cut (choose_target, capi_support.hip) weighs the whole batch.  On the default handle
    (one slot per CU) the ragged batch cuts its longest utterances, 16 TB + 1 frames, into slabs of
    9 TB and 7 TB + 1 frames: a second slab costs nothing while the items fit one wave of slots.
    With one slot every item costs its frames, and a batch of EQUAL frame counts is cheapest
    uncut (n (T + 8) against 2 n (T / 2 + 8)) -- in the ragged batch it would be cut all the same,
    so the second handle runs one batch per frame count.  The two cuts must show: the longest
    cases change bits, the others fold the same frames in the same order and do not."""
    tally = cc.Tally(f"fused fold C={C}")
    cases = cc.fused_cases(C)
    base = fused_under_the_judge(tally, ctx, C, cases, "default cuts")
    with fresh_handle("SETK_P1_ITEMS=1") as c1:
        one = fused_under_the_judge(tally, c1, C, cases, "one slab", by_frames=True)
    changed = [k for k in cases if one[k] != base[k]]
    longest = max(cc.fused_frames(C))
    print(f"[{tally.form}] {len(changed)} of {len(cases)} cases change bits with the slab cut: "
          f"T in {sorted({k.T for k in changed})}")
    assert changed and {k.T for k in changed} == {longest}, sorted({k.T for k in changed})
    pcm = fused_under_the_judge(tally, ctx, C, cases, "pcm16", pcm=True)
    differ = [k.name for k in cases if pcm[k] != base[k]]
    tally.fail(f"{name}: the taps of the PCM16 call differ from the float call's" for name in differ)
    print(f"[{tally.form}] {len(cases)} cases: PCM16 taps == float taps, bit for bit: {not differ}")
    tally.finish()


MPDR_AT = (13, 14)      # one odd and one even count run the instantiation that also folds Ry


@pytest.mark.parametrize("C", range(9, 17))
def test_wide_fused_fold(ctx, C):
    """wide.hip's matrix-core fold at every channel count: the pairs read out of the 32 x 32 tile
    through run-time C, chunks of 8 frames in two halves of 4, slabs of 128 frames."""
    from setk_amd import _ffi
    tally = cc.Tally(f"wide fold C={C}")
    fused_under_the_judge(tally, ctx, C, cc.fused_cases(C, itf=C in (11, 16)), "wide")
    if C in MPDR_AT:
        # MPDR: covar_wide_mfma_kernel<true>.  Ry has no tap: Rs and Rn of that instantiation are
        # judged like the others, and the weights against the oracle on the tapped Rs and the
        # oracle's Ry where Rn is well posed (test_gpu_wide_fused.py's selection and bar).
        T = 129
        mix, sp, nz = o.synth_utterance(300 + C, C, cc.samples_for(T), return_parts=True)
        mask = (0.05 + 0.9 * o.irm_mask(sp, nz)).astype(np.float32)
        assert mask.shape == (T, F)
        case = cc.FusedCase(C, T, "synth", "mpdr", "uniform", True, None)
        st, Rs, Rn, w = run_fused(ctx, C, [case], kind=_ffi.BF_MPDR, audio=[mix], masks=[(mask, None)])
        geo = sc.Geom()
        X, X32 = sc.ref_stft(mix, geo), sc.f32_stft(mix, geo)
        for name, got, m in (("Rs", Rs[0], mask.astype(np.float64)), ("Rn", Rn[0], 1.0 - mask.astype(np.float64))):
            ref = cc.reference(X, m)
            check(tally, "mpdr", f"mpdr C={C} T={T} {name}", got, ref,
                  cc.allowance(X, m, ref) + cc.forward_allowance(X, X32, m))
        Xo = np.transpose(X, (0, 2, 1))
        Ry = o.compute_covar(Xo, np.ones_like(mask)).astype(np.complex64).astype(np.complex128)
        ev = np.linalg.eigvalsh(cc.reference(X, 1.0 - mask.astype(np.float64)))
        good = ev[:, 0] * 1e4 > ev[:, -1]
        wref = o.mpdr_weight(Rs[0].astype(np.complex128), Ry, gauge=True)
        e_w = rel_rms(w[0][good], wref[good])
        print(f"[{tally.form}] mpdr: status {st}, well-posed bins {int(good.sum())}, weights {e_w:.2e}")
        assert st == [0] and good.all() and np.isfinite(w).all()
        assert e_w < 2e-4, e_w
    tally.finish()


# ---------------------------------------------------------------- block-online
@pytest.mark.parametrize("C", cc.ONLINE_CHANNELS)
def test_online_recursion(ctx, C):
    """setk_enhance_online_batch's tapped Rs_c / Rn_c: pass 1 on work items cut at chunk boundaries
    that are no tile multiples, the recursion R_c = alpha R_{c-1} + phi_c r_c; every chunk and bin
    under the allowance carried through the recursion (covar_cases.online_recursion)."""
    import torch
    from setk_amd import _ffi
    dev = torch.device("cuda:0")
    T = cc.ONLINE_T
    tally = cc.Tally(f"online C={C}")
    opts = _ffi.BfOpts(kind=_ffi.BF_MVDR, flags=_ffi.FLAG_CLAMP_MASK, pmwf_ref=-1)
    for chunk in cc.online_chunks(C):
        K = -(-T // chunk)
        edges = cc.online_edges(C, T, chunk)
        for alpha in cc.ONLINE_ALPHAS:
            for n, label in enumerate(cc.ONLINE_MASKS):
                fam = ("white", "coherent")[n % 2]
                pcm, X, X32 = cc.spectra(fam, C, T)
                x = cc.as_float(pcm)
                N = x.shape[1]
                assert ctx.num_frames(N) == T and ctx.online_num_chunks(N, chunk) == K
                raw = cc.mask({"over-clamped": "over", "itf": "uniform"}.get(label, label), T, F, seed=C, edges=edges)
                itf = cc.mask("itf", T, F, seed=C + 100) if label == "itf" else None
                es = np.minimum(raw, np.float32(1)).astype(np.float64)
                en = (1.0 - es) if itf is None else itf.astype(np.float64)
                a = torch.from_numpy(x).to(dev)
                m = torch.from_numpy(raw).to(dev)
                mi = torch.from_numpy(itf).to(dev) if itf is not None else None
                out = torch.zeros(ctx.istft_num_samples(T), dtype=torch.float32, device=dev)
                tp = dict(Rs=np.full((K, F, C, C), np.nan, np.complex64), Rn=np.full((K, F, C, C), np.nan, np.complex64))
                st = np.full(1, -1, np.int32)
                ctx.enhance_online_batch(opts, chunk, alpha, C, [a.data_ptr()], [N], [m.data_ptr()],
                                         [mi.data_ptr()] if mi is not None else None, [out.data_ptr()],
                                         status=st, taps=tp)
                torch.cuda.synchronize()
                want = cc.online_recursion((X, X32), es, en, chunk, alpha)
                for name in ("Rs", "Rn"):
                    R, A = want[name]
                    for k in range(K):
                        check(tally, f"chunk {chunk}", f"{fam}/{label} chunk size {chunk} alpha {alpha:.1f} {name}[{k}]",
                              tp[name][k], R[k], A[k])
    tally.finish()
