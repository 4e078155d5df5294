"""
Conformance of the per-bin solver (setk_amd/csrc/solve.hip) on constructed matrices, through
`_ffi.Context.pevd` / `.weights` only.  The families, the complex128 truth and the sensitivity s of
that truth come from tests/solve_cases.py (checked without a GPU in tests/test_solve_cases.py).

  (a) backward error per matrix (gauge free, gap free): unit norm, residual, Rayleigh quotient;
  (b) parity with the complex128 oracle per family of 256 matrices: bar = 8 eps32 + M * s;
  (c) both at every scale of the list for 3, 4, 7, 8, 9, 12, 15 and 16 channels;
  (d) launch geometry: the answer of a bin does not depend on its neighbours, bit for bit;
  (e) the status, per bin, for every channel count.

Margins M (tests/PARITY_NOTES.md, "Solver conformance", holds the measured error / s): 1 wherever
the eigenvalue gap of Rs is >= 0.5, M_SMALL_GAP below that for every kind that solves an
eigenproblem.  Each test prints its figures before it asserts.
"""
import numpy as np
import pytest

import solve_cases as sc
from oracle import np_oracle as o

pytestmark = pytest.mark.gpu

EPS32 = sc.EPS32
M_CLEAR_GAP = 1
M_SMALL_GAP = 2   # next power of two above the worst measured error / s (1.31)
OK, SINGULAR, NOCONV, NONFINITE = 0, 1, 2, 3

# (C, scale): every channel count at scale 1, the listed ones at every scale
C_SCALE = [(C, 1.0) for C in sc.CHANNELS] + [(C, s) for C in sc.SCALE_CHANNELS for s in sc.SCALES if s != 1.0]
C_SCALE_WIDE = C_SCALE + [(C, s) for C in sc.SCALE_CHANNELS for s in sc.SCALES_WIDE]


def _id(cs):
    return f"C{cs[0]}-x2e{int(np.log2(cs[1])):+d}"


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def pevd(ctx, Rs, Rn=None, flags=0):
    F, C = Rs.shape[0], Rs.shape[1]
    pv = np.full((F, C), np.nan, np.complex64)
    st = np.full(F, -1, np.int32)
    ctx.pevd(np.ascontiguousarray(Rs), None if Rn is None else np.ascontiguousarray(Rn), F, C, flags, pv, st)
    return pv, st


def weights(ctx, Rs, Rn, Ry, kind, flags=0, pmwf_ref=-1, pmwf_beta=0.0, rank1="NONE"):
    from setk_amd import _ffi
    F, C = Rs.shape[0], Rs.shape[1]
    opts = _ffi.BfOpts(kind=getattr(_ffi, "BF_" + kind), flags=flags, pmwf_beta=pmwf_beta,
                       pmwf_ref=pmwf_ref, rank1=getattr(_ffi, "RANK1_" + rank1))
    w = np.full((F, C), np.nan, np.complex64)
    st = np.full(F, -1, np.int32)
    ref = ctx.weights(opts, np.ascontiguousarray(Rs), None if Rn is None else np.ascontiguousarray(Rn),
                      None if Ry is None else np.ascontiguousarray(Ry), F, C, w, st)
    return w, st, ref


def norm2(M):
    return np.linalg.norm(M.astype(np.complex128), ord=2, axis=(1, 2))


def rs_families(C, scale):
    fams = {f"gap{g:g}_floor{fl:g}": sc.rs_gap(C, g, fl, scale) for g in sc.GAPS for fl in sc.FLOORS}
    fams["rank1"] = sc.rs_rank1(C, scale)
    fams["diagonal"] = sc.rs_diagonal(C, scale)
    fams["real"] = sc.rs_real(C, scale)
    fams["identity"] = sc.rs_identity(C, scale)
    return fams


# ---- (a) backward error ------------------------------------------------------------------------
@pytest.mark.parametrize("cs", C_SCALE_WIDE, ids=_id)
def test_pevd_backward_error(ctx, cs):
    """|v| = 1 to 4 eps32, |A v - (v^H A v) v| <= 8 eps32 |A|_2 and v^H A v >= lambda_max (1 -
    8 eps32) for EVERY matrix of every family; the diagonal family returns the unit vector of its
    largest entry exactly.  All arithmetic of the checks in float64."""
    C, scale = cs
    worst = {}
    for name, Rs in rs_families(C, scale).items():
        pv, st = pevd(ctx, Rs)
        assert not st.any(), (C, scale, name, np.flatnonzero(st)[:8], st[st != 0][:8])
        A = Rs.astype(np.complex128)
        v = pv.astype(np.complex128)
        nrm = np.linalg.norm(v, axis=1)
        Av = np.einsum("fab,fb->fa", A, v)
        rq = np.einsum("fa,fa->f", v.conj(), Av).real
        res = np.linalg.norm(Av - rq[:, None] * v, axis=1) / norm2(Rs)
        lam = np.linalg.eigvalsh(A)[:, -1]
        worst[name] = res.max() / EPS32
        print(f"[solve a] pevd C={C} scale=2^{int(np.log2(scale))} {name}: | |v|-1 | {np.abs(nrm - 1).max() / EPS32:.2f} eps32, "
              f"residual {res.max() / EPS32:.2f} eps32, 1 - rq/lambda_max {np.max(1 - rq / lam) / EPS32:.2f} eps32")
        assert np.abs(nrm - 1).max() <= 4 * EPS32, (C, scale, name)
        assert res.max() <= 8 * EPS32, (C, scale, name, int(res.argmax()), res.max() / EPS32)
        assert np.all(rq >= lam * (1 - 8 * EPS32)), (C, scale, name)
        if name == "diagonal":
            unit = np.zeros((sc.F, C), np.complex64)
            unit[np.arange(sc.F), np.arange(sc.F) % C] = 1
            assert np.array_equal(pv, unit), (C, scale, np.flatnonzero((pv != unit).any(axis=1))[:8])
    pv, st = pevd(ctx, sc.rs_zero(C))
    assert not st.any() and np.isfinite(pv).all()
    assert np.abs(np.linalg.norm(pv.astype(np.complex128), axis=1) - 1).max() <= 4 * EPS32
    print(f"[solve a] pevd C={C} scale=2^{int(np.log2(scale))} worst residual {max(worst.values()):.2f} eps32")


@pytest.mark.parametrize("cs", C_SCALE_WIDE, ids=_id)
def test_pencil_backward_error(ctx, cs):
    """|v^H Rn v - 1| <= 8 eps32 cond, |Rs v - rho Rn v| <= 8 eps32 cond |Rs|_2 |v|,
    rho >= rho_max (1 - 8 eps32 cond), per matrix; rho_max from scipy in complex128."""
    C, scale = cs
    for gap, floor, cond in sc.PAIRS:
        Rs, Rn = sc.rs_gap(C, gap, floor, scale), sc.rn_cond(C, cond, scale)
        pv, st = pevd(ctx, Rs, Rn)
        assert not st.any(), (C, scale, gap, cond, st[st != 0][:8])
        A, B, v = Rs.astype(np.complex128), Rn.astype(np.complex128), pv.astype(np.complex128)
        Av = np.einsum("fab,fb->fa", A, v)
        Bv = np.einsum("fab,fb->fa", B, v)
        vBv = np.einsum("fa,fa->f", v.conj(), Bv).real
        rho = np.einsum("fa,fa->f", v.conj(), Av).real / vBv
        res = np.linalg.norm(Av - rho[:, None] * Bv, axis=1) / (norm2(Rs) * np.linalg.norm(v, axis=1))
        rho_max = sc.pencil_rho(Rs, Rn)
        tol = 8 * EPS32 * cond
        print(f"[solve a] pencil C={C} scale=2^{int(np.log2(scale))} gap={gap:g} cond={cond:g}: |vBv-1| {np.abs(vBv - 1).max() / tol:.3f}, "
              f"residual {res.max() / tol:.3f}, 1 - rho/rho_max {np.max(1 - rho / rho_max) / tol:.3f} (units of 8 eps32 cond); "
              f"residual {res.max() / EPS32:.2f} eps32")
        assert np.abs(vBv - 1).max() <= tol, (C, scale, gap, cond)
        assert res.max() <= tol, (C, scale, gap, cond, res.max() / EPS32)
        assert np.all(rho >= rho_max * (1 - tol)), (C, scale, gap, cond)


def test_ill_conditioned_noise_goes_through(ctx):
    """cond(Rn) = 1e9 is outside what is compared (the floored / loaded Cholesky departs from the
    reference there on purpose): finite and status OK only"""
    for C in (4, 8, 12):
        Rs, Rn = sc.rs_gap(C, 0.5, 1e-1), sc.rn_cond(C, 1e9)
        w, st, _ = weights(ctx, Rs, Rn, None, "MVDR")
        assert not st.any() and np.isfinite(w).all(), C


# ---- (b) parity, (c) at every scale --------------------------------------------------------------
def _check(tag, got, truth, s, margin, name, gap, cond, cap, failures):
    err = sc.rel_rms(got, truth)
    b = sc.bar(s, margin, name, gap, cond, cap)
    print(f"[solve b] {tag}: err {err:.2e} s {s:.2e} err/s {err / max(s, 1e-300):.2f} bar {b:.2e} (M={margin})")
    if not err <= b:
        failures.append(f"{tag}: err {err:.3e} > bar {b:.3e} (s {s:.2e}, err/s {err / max(s, 1e-300):.1f}, M={margin})")


@pytest.mark.parametrize("cs", C_SCALE_WIDE, ids=_id)
def test_pevd_parity(ctx, cs):
    """setk_pevd(Rs) against o.solve_pevd in complex128, declared gauge, every gap family plus the
    rank-1, real symmetric and diagonal ones"""
    C, scale = cs
    failures = []
    fams = [(f"gap{g:g}_floor{fl:g}", sc.rs_gap(C, g, fl, scale), g) for g in sc.GAPS for fl in sc.FLOORS]
    fams += [("rank1", sc.rs_rank1(C, scale), 1.0), ("real", sc.rs_real(C, scale), 0.5),
             ("diagonal", sc.rs_diagonal(C, scale), 0.5)]
    for name, Rs, gap in fams:
        rng = np.random.default_rng(sc.seed_of("probe_pevd", C, name))
        s, truth = sc.sensitivity(sc.op_pevd, (Rs,), rng)
        pv, st = pevd(ctx, Rs)
        assert not st.any(), (C, scale, name)
        margin = M_CLEAR_GAP if gap >= 0.5 else M_SMALL_GAP
        _check(f"pevd C={C} scale=2^{int(np.log2(scale))} {name}", pv, truth, s, margin, "pevd", gap, 1.0,
               sc.CAP_VEC, failures)
    assert not failures, "\n".join(failures)


def _kinds_at(scale):
    wide = scale in sc.SCALES_WIDE
    return ("mvdr", "gevd") if wide else tuple(sc.weight_kinds(2))


@pytest.mark.parametrize("cs", C_SCALE_WIDE, ids=_id)
def test_pencil_and_weight_parity(ctx, cs):
    """setk_pevd(Rs, Rn) and every kind of setk_weights, with and without BAN where the C ABI
    allows it, against the complex128 oracle evaluated at this scale; all 256 bins, status OK."""
    from setk_amd import _ffi
    C, scale = cs
    wide = scale in sc.SCALES_WIDE
    kinds = sc.weight_kinds(C)
    failures, decided, ties = [], 0, 0
    for gap, floor, cond in sc.PAIRS:
        case = sc.Case(C, gap, floor, cond, scale)   # truth and sensitivity: once per family
        tagp = f"C={C} scale=2^{int(np.log2(scale))} gap={gap:g} cond={cond:g}"
        eig_margin = M_CLEAR_GAP if gap >= 0.5 else M_SMALL_GAP
        truth, s = case.truth_and_s("pencil", lambda Rs, Rn, Ry: sc.op_pencil(Rs, Rn))
        pv, st = pevd(ctx, case.Rs, case.Rn)
        assert not st.any(), (tagp, "pencil")
        _check(f"pencil {tagp}", pv, truth, s, eig_margin, "gevd", gap, cond, sc.CAP_VEC, failures)
        for name in _kinds_at(scale):
            _, fn, opt, _ = kinds[name]
            solves_eig = name not in ("pmwf_search", "pmwf_last_beta1")
            margin = eig_margin if solves_eig else M_CLEAR_GAP
            for ban in ((False,) if (wide or name == "mpdr") else (False, True)):
                truth, s = case.truth_and_s(name, fn, ban=ban)
                w, st, ref = weights(ctx, case.Rs, case.Rn, case.Ry, flags=_ffi.FLAG_BAN if ban else 0, **opt)
                assert not st.any(), (tagp, name, ban, st[st != 0][:8])
                _check(f"{name}{'+ban' if ban else ''} {tagp}", w, truth, s, margin, name, gap, cond,
                       sc.CAP_WEIGHT, failures)
                if name == "pmwf_search" and not ban:
                    snr = np.sort(sc.pmwf_snr(*case.inputs[0][:2]))
                    if C == 1 or snr[-1] - snr[-2] > 1e-6 * abs(snr[-1]):
                        decided += 1
                        want = int(np.argmax(sc.pmwf_snr(*case.inputs[0][:2])))
                        if ref != want:
                            failures.append(f"pmwf_search {tagp}: reference channel {ref}, oracle {want}")
                    else:
                        ties += 1
    if not wide:
        print(f"[solve b] pmwf_search C={C} scale=2^{int(np.log2(scale))}: {decided} families decided, {ties} near ties")
        assert ties * 10 <= decided + ties, (decided, ties)
    assert not failures, "\n".join(failures)


# ---- (d) launch geometry and independence --------------------------------------------------------
GEOM_F = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 1000)


def _geom_stack(C):
    Rs = np.concatenate([sc.rs_gap(C, g, 1e-1) for g in (0.9, 0.5, 1e-1, 1e-2)])[:1000]
    Rn = np.concatenate([sc.rn_cond(C, c) for c in (1e1, 1e2, 1e3, 1e2)])[:1000]
    return np.ascontiguousarray(Rs), np.ascontiguousarray(Rn)


def _geom_ops(ctx):
    return {
        "pevd": lambda Rs, Rn: pevd(ctx, Rs)[:2],
        "mvdr": lambda Rs, Rn: weights(ctx, Rs, Rn, None, "MVDR")[:2],
        "gevd": lambda Rs, Rn: weights(ctx, Rs, Rn, None, "GEVD")[:2],
    }


@pytest.mark.parametrize("C", [2, 4, 5, 8, 12])
def test_launch_geometry(ctx, C):
    """(i) F copies of one matrix give F bit-identical answers; (ii) bin f of an F-bin call on
    distinct matrices is bit-identical to the one-bin call on that matrix.  A shuffle of the wrong
    width, a wrong LDS slot or a store from the tail lanes of the last wavefront breaks this."""
    Rs, Rn = _geom_stack(C)
    for op, fn in _geom_ops(ctx).items():
        alone = np.empty((1000, C), np.complex64)
        for f in range(1000):
            alone[f], st = fn(Rs[f:f + 1], Rn[f:f + 1])
            assert st[0] == OK
        for F in GEOM_F:
            same, st = fn(np.repeat(Rs[7:8], F, axis=0), np.repeat(Rn[7:8], F, axis=0))
            assert not st.any()
            assert np.array_equal(same.view(np.uint32), np.repeat(alone[7:8], F, axis=0).view(np.uint32)), (op, C, F)
            got, st = fn(Rs[:F], Rn[:F])
            assert not st.any()
            diff = np.flatnonzero((got.view(np.uint32) != alone[:F].view(np.uint32)).any(axis=1))
            assert diff.size == 0, (op, C, F, diff[:8])


# ---- (e) status ----------------------------------------------------------------------------------------
def _spoil(kind, Rs, Rn, b):
    """a copy of (Rs, Rn) whose bin b is bad; the non-finite value sits in the lower triangle"""
    Rs, Rn = Rs.copy(), Rn.copy()
    C = Rs.shape[1]
    if kind == "zero_rn":
        Rn[b] = 0
    elif kind == "negative_rn":
        Rn[b] = -Rn[b]
    elif kind == "nan_rs":
        Rs[b, C - 1, 0] = np.nan
    elif kind == "inf_rs":
        Rs[b, C // 2, C // 2] = np.inf
    elif kind == "nan_rn":
        Rn[b, C - 1, 0] = np.nan
    elif kind == "inf_rn":
        Rn[b, C // 2, C // 2] = np.inf
    return Rs, Rn


@pytest.mark.parametrize("C", sc.CHANNELS)
def test_status_is_per_bin(ctx, C):
    """One bad bin -- first, middle and last problem of a wavefront -- reports its own status; every
    other bin is OK and bit-identical to the call without it."""
    from setk_amd import _ffi
    pw = 64 // (16 if C > 8 else 8 if C > 4 else 4)    # problems per wavefront
    F = 3 * pw + 1
    Rs = sc.rs_gap(C, 0.5, 1e-1)[:F]
    Rn = sc.rn_cond(C, 1e2)[:F]
    clean, st, _ = weights(ctx, Rs, Rn, None, "MVDR")
    assert not st.any()
    expect = {"zero_rn": SINGULAR, "negative_rn": SINGULAR, "nan_rs": NONFINITE, "inf_rs": NONFINITE,
              "nan_rn": NONFINITE, "inf_rn": NONFINITE}
    for kind, code in expect.items():
        for b in (pw, pw + pw // 2, 2 * pw - 1, 0, F - 1):
            A, B = _spoil(kind, Rs, Rn, b)
            w, st, _ = weights(ctx, A, B, None, "MVDR")
            others = np.arange(F) != b
            assert st[b] == code, (C, kind, b, st[b])
            assert not st[others].any(), (C, kind, b, np.flatnonzero(st * others))
            assert np.array_equal(w[others].view(np.uint32), clean[others].view(np.uint32)), (C, kind, b)
    # the plain eigenvector has a status too
    cleanv, st = pevd(ctx, Rs)
    for kind in ("nan_rs", "inf_rs"):
        A, _ = _spoil(kind, Rs, Rn, pw + 1 if F > pw + 1 else 0)
        b = pw + 1 if F > pw + 1 else 0
        v, st = pevd(ctx, A)
        others = np.arange(F) != b
        assert st[b] == NONFINITE and not st[others].any(), (C, kind, st)
        assert np.array_equal(v[others].view(np.uint32), cleanv[others].view(np.uint32))
    # SETK_FLAG_STRICT_REFERENCE, GEVD: an all-zero Rn goes through as the pencil (Rs, I)
    b = pw + pw // 2
    A, B = _spoil("zero_rn", Rs, Rn, b)
    w, st, _ = weights(ctx, A, B, None, "GEVD", flags=_ffi.FLAG_STRICT_REFERENCE)
    assert not st.any(), (C, st)
    plain, _ = pevd(ctx, A[b:b + 1])
    assert np.isfinite(w).all() and sc.rel_rms(w[b], plain[0]) < 1e-6
    w, st, _ = weights(ctx, A, B, None, "GEVD")
    assert st[b] == SINGULAR and not st[np.arange(F) != b].any(), (C, st)
