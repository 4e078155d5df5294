"""
Conformance of the geometry-driven spatial features on the MI355X (setk_amd/csrc/spatial.hip with
the observation tiles of ssl.hip): IPD / cosIPD / sinIPD, the directional features and the SRP-PHAT
angular spectrum through libs.spatial and the batch entry, on the constructed cases of
spatial_cases.py.  Every cell is judged against the float64 reference there, at min(A, 1e-4) with A
the derived allowance of that cell; where the reference is not finite the device must be non-finite
in exactly the same cells.  test_spatial_cases.py shows on the CPU that this bar fails nine seeded
faults, three of which the flat 1e-4 bar of test_gpu_spatial.py cannot see.  Every test prints its
worst error / allowance and where it occurred before it asserts.  Figures: PARITY_NOTES_SPATIAL.md.
"""
import functools

import numpy as np
import pytest

import spatial_cases as sc

pytestmark = pytest.mark.gpu
T0, F0, D0 = 33, 33, 65
NUM_SV = 7


@pytest.fixture(scope="module")
def sp():
    from setk_amd.libs import spatial
    return spatial


def ipd_pairs(C):
    """a forward pair, a reversed pair, a repeated pair and a pair (l, l)"""
    return [(0, 1), (C - 1, 0), (0, 1), (C // 2, C // 2)]


def short_pairs(C):
    """shorter than all pairs wherever there is more than one"""
    return [(0, 1), (C - 1, 1), (C // 2, C - 1)] if C > 2 else [(1, 0)]


@functools.lru_cache(maxsize=None)
def srp_case(family, C, T, F, D, samp_doa=True):
    """(S, pairs, table, weights, SrpRef) over the full pair list of the linear topology topo(C): the
    table is the product's own (libs.spatial.linear_srp_tables), the reference takes it as packed."""
    from setk_amd.libs import spatial
    S = sc.spectrogram(family, C, T, F)
    pairs, table, w = spatial.linear_srp_tables(sc.topo(C), num_bins=F, num_doa=D, samp_doa=samp_doa)
    assert table.shape == (len(pairs), F, sc.dpad(D)) and table.dtype == np.complex64
    assert np.array_equal(table, sc.linear_tables(C, F, D, samp_doa)[1]) and not table[:, :, D:].any()
    for a in (S, table):
        a.setflags(write=False)
    return S, pairs, table, w, sc.ref_srp(S, pairs, table, D)


def judge_srp(tally, sp, family, name, case, D, weights=None):
    S, pairs, table, w, ref = case
    w = w if weights is None else weights
    got = sp.srp_feats(S, pairs, table, w, D)
    return tally.add(family, sc.judge(name, got, *ref.combined(w)))


# ---------------------------------------------------------------- SRP
@pytest.mark.parametrize("C", range(2, 17))
def test_srp_all_pairs(sp, C):
    """Every channel count with its full pair list: P = 1 .. 120."""
    T, F, D = (T0, 65, D0) if C <= 8 else (T0, 33, D0)
    tally = sc.Tally(f"srp C={C} P={C * (C - 1) // 2}")
    for family in ("white", "coherent"):
        judge_srp(tally, sp, family, f"{family} C={C} T={T} F={F} D={D}", srp_case(family, C, T, F, D), D)
    tally.finish()


EDGES = [("T", v) for v in (1, 31, 32, 33, 64, 65)] + [("D", v) for v in (1, 63, 64, 65, 181)] + \
        [("F", v) for v in (2, 31, 32, 33, 65, 257)]


@pytest.mark.parametrize("axis,value", EDGES)
def test_srp_edges(sp, axis, value):
    """The tile of 32 frames and 64 directions, the patches of 32 bins: on, below and above each."""
    shape = dict(T=T0, F=F0, D=D0)
    shape[axis] = value
    T, F, D = shape["T"], shape["F"], shape["D"]
    tally = sc.Tally(f"srp C=4 {axis}={value}")
    for family in ("white", "coherent", "lattice"):
        case = srp_case(family, 4, T, F, D)
        judge_srp(tally, sp, family, f"{family} T={T} F={F} D={D}", case, D)
        hot = np.eye(6)[5]
        judge_srp(tally, sp, family, f"{family} T={T} F={F} D={D} pair 5 alone", case, D, weights=hot)
    tally.finish()


@pytest.mark.parametrize("p", [0, 1, 63, 64, 119])
def test_srp_one_pair_of_120(sp, p):
    """pair_weight is an input: a one-hot weight over the full 120-pair table shows g_p alone."""
    tally = sc.Tally(f"srp C=16 pair {p} alone")
    for family in ("white", "coherent"):
        judge_srp(tally, sp, family, f"{family} g_{p}", srp_case(family, 16, T0, F0, D0), D0,
                  weights=np.eye(120)[p])
    tally.finish()


def test_srp_circular_form(sp):
    diag, n, d, D = [(0, 3), (1, 4), (2, 5)], 6, 0.07, 121
    tally = sc.Tally("srp circular C=6")
    for family in ("white", "lattice"):
        S = sc.spectrogram(family, 6, T0, F0)
        pairs, table, w = sp.circular_srp_tables(diag, n, d, num_bins=F0, num_doas=D)
        ref = sc.ref_srp(S, pairs, table, D)
        for name, wt in [("mean", w)] + [(f"pair {p} alone", np.eye(3)[p]) for p in range(3)]:
            tally.add(family, sc.judge(f"{family} circular {name}", sp.srp_feats(S, pairs, table, wt, D),
                                       *ref.combined(wt)))
    tally.finish()


def test_srp_tdoa_sampling(sp):
    tally = sc.Tally("srp C=4 samp_doa=False")
    for family in ("white", "coherent"):
        case = srp_case(family, 4, T0, F0, D0, False)
        judge_srp(tally, sp, family, f"{family} tdoa", case, D0)
        judge_srp(tally, sp, family, f"{family} tdoa pair 2 alone", case, D0, weights=np.eye(6)[2])
    tally.finish()


# ---------------------------------------------------------------- IPD and DF
def judge_ipd(tally, family, name, kind, got, S, pairs):
    tally.add(family, sc.judge(f"{name} {kind}", got, sc.ref_ipd(S, pairs, kind), sc.ipd_allowance(kind),
                               circle=kind == "ipd"))
    if kind == "ipd":
        tally.fail(sc.ipd_range(name, got, S, pairs))


@pytest.mark.parametrize("C", [2, 5, 16])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_ipd(sp, kind, C):
    tally = sc.Tally(f"{kind} C={C}")
    pairs = ipd_pairs(C)
    for T in (1, 33):
        for F in (2, 33, 257):
            for family in ("white", "lattice"):
                S = sc.spectrogram(family, C, T, F)
                got = sp.ipd_feats(S, pairs, cos=kind != "ipd", sin=kind == "cos_sin_ipd")
                judge_ipd(tally, family, f"{family} C={C} T={T} F={F}", kind, got, S, pairs)
    tally.finish()


DF_INDEX = ([3], [2, 0, 5], list(range(NUM_SV)), [6, 1, 6])        # n_index 1, 3, num_sv; a repeated index


@pytest.mark.parametrize("C", [2, 5, 16])
def test_geometry_df(sp, C):
    tally = sc.Tally(f"df C={C}")
    for T in (1, 33):
        for F in (2, 33, 257):
            S = sc.spectrogram("white", C, T, F)
            sv = sc.steer(NUM_SV, C, F)
            for k, idx in enumerate(DF_INDEX):
                pairs = short_pairs(C) if k % 2 else sc.all_pairs(C)
                ref, A = sc.ref_df(S, sv, idx, pairs)
                got = sp.geometry_df(S, sv, idx, pairs)
                tally.add(f"n_index {len(idx)}", sc.judge(f"C={C} T={T} F={F} idx {idx} P={len(pairs)}", got, ref, A))
    tally.finish()


# ---------------------------------------------------------------- ragged batches through setk_spatial_batch
BATCH_KINDS = sc.KINDS + ("df", "srp")


def run_batch(kind, C, F, specs, D=D0, sv=None, idx=None, pairs=None, table=None, weight=None):
    """One setk_spatial_batch call, then a second: (the maps of the first, whether both gave the same bytes)."""
    import torch
    from setk_amd import _ffi
    ctx = _ffi.default_context()
    if kind == "srp":
        opts = _ffi.spatial_opts("srp", pairs, table=table, num_doas=D, pair_weight=weight)
    elif kind == "df":
        opts = _ffi.spatial_opts("df", pairs, steer_vector=sv, num_sv=sv.shape[0], doa_index=idx)
    else:
        opts = _ffi.spatial_opts(kind, pairs)
    dev = [torch.from_numpy(np.array(s)).cuda() for s in specs]
    runs = []
    for _ in range(2):
        outs = [torch.full((s.shape[1], _ffi.spatial_width(opts, F)), float("nan"), dtype=torch.float32, device="cuda")
                for s in specs]
        ctx.spatial_batch(opts, C, [d.data_ptr() for d in dev], [s.shape[1] for s in specs], F,
                          [o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        runs.append([o.cpu().numpy() for o in outs])
    return runs[0], all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


def judge_batch(sp, tally, kind, C, frames, families):
    """Every utterance against the float64 reference of that utterance alone."""
    specs = [sc.spectrogram(fam, C, T, F0) for fam, T in zip(families, frames)]
    names = [f"utterance {k} ({fam}, T={T})" for k, (fam, T) in enumerate(zip(families, frames))]
    if kind == "srp":
        pairs, table, w = sp.linear_srp_tables(sc.topo(C), num_bins=F0, num_doa=D0)
        got, same = run_batch(kind, C, F0, specs, pairs=pairs, table=table, weight=w)
        for name, fam, S, g in zip(names, families, specs, got):
            tally.add(fam, sc.judge(name, g, *sc.ref_srp(S, pairs, table, D0).combined(w)))
    elif kind == "df":
        sv, pairs = sc.steer(NUM_SV, C, F0), short_pairs(C)
        idx = [[2, 0, 5], [1, 1, 6], [0, 3, 4], [6, 2, 2]][:len(specs)]
        got, same = run_batch(kind, C, F0, specs, sv=sv, idx=idx, pairs=pairs)
        for name, fam, S, g, ix in zip(names, families, specs, got, idx):
            tally.add(fam, sc.judge(name, g, *sc.ref_df(S, sv, ix, pairs)))
    else:
        pairs = ipd_pairs(C)
        got, same = run_batch(kind, C, F0, specs, pairs=pairs)
        for name, fam, S, g in zip(names, families, specs, got):
            judge_ipd(tally, fam, name, kind, g, S, pairs)
    if not same:
        tally.fail([f"{kind}: a second run of the batch gave other bytes"])


@pytest.mark.parametrize("kind", BATCH_KINDS)
def test_ragged_batch_against_the_reference(sp, kind):
    """A coherent utterance (m_p close to F) beside white ones (m_p a fraction of it) and a lattice:
    a normaliser leaked between utterances, or direction indices of the wrong utterance, show."""
    tally = sc.Tally(f"batch {kind}")
    judge_batch(sp, tally, kind, 4, (1, 33, 64, 5), ("coherent", "white", "lattice", "white"))
    tally.finish()


@pytest.mark.parametrize("kind", BATCH_KINDS)
def test_a_nan_stays_in_its_utterance(sp, kind):
    tally = sc.Tally(f"batch {kind} with a NaN")
    judge_batch(sp, tally, kind, 4, (33, 33, 5), ("white", "nan", "coherent"))
    tally.finish()


def test_every_modulus_of_complex64(sp):
    """From the smallest subnormal to the largest float32, both sides of every threshold of phasor()."""
    S = sc.moduli_grid()
    pairs = [(0, 1), (1, 0)]
    tally = sc.Tally("moduli")
    for kind in sc.KINDS:
        got = sp.ipd_feats(S, pairs, cos=kind != "ipd", sin=kind == "cos_sin_ipd")
        judge_ipd(tally, kind, "moduli grid", kind, got, S, pairs)
    sv = np.ascontiguousarray(np.stack([S[:, 3], S[::-1, 20]]))     # [2][2][N]: a subnormal row, a large one
    ref, A = sc.ref_df(S, sv, [1, 0], pairs)
    tally.add("df", sc.judge("moduli grid df", sp.geometry_df(S, sv, [1, 0], pairs), ref, A))
    tally.finish()


# ---------------------------------------------------------------- every family, one small shape per kind
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_families(sp, family):
    """`extreme` holds phasor() to every finite non-zero modulus of complex64; `nan` is judged by its
    non-finite pattern, and the pairs the NaN does not touch stay inside their allowance."""
    tally = sc.Tally(f"family {family}")
    C = 5
    S = sc.spectrogram(family, C, T0, F0)
    pairs = ipd_pairs(C)
    for kind in sc.KINDS:
        got = sp.ipd_feats(S, pairs, cos=kind != "ipd", sin=kind == "cos_sin_ipd")
        judge_ipd(tally, kind, f"{family} C={C}", kind, got, S, pairs)
        if family == "nan":
            assert int((~np.isfinite(got)).sum()) == (2 if kind == "cos_sin_ipd" else 1)   # pair (4, 0), one cell
    sv = sc.steer(NUM_SV, C, F0)
    for idx, prs in (([2, 0, 5], sc.all_pairs(C)), ([6, 6], short_pairs(C))):
        ref, A = sc.ref_df(S, sv, idx, prs)
        tally.add("df", sc.judge(f"{family} df idx {idx} P={len(prs)}", sp.geometry_df(S, sv, idx, prs), ref, A))
    case = srp_case(family, 4, T0, F0, D0)
    S, prs, table, w, ref = case
    judge_srp(tally, sp, "srp", f"{family} srp", case, D0)
    judge_srp(tally, sp, "srp one pair", f"{family} srp pair 5 alone", case, D0, weights=np.eye(6)[5])
    if family == "nan":
        assert not np.isfinite(ref.combined(w)[0]).any()
        keep = [p for p, (l, r) in enumerate(prs) if 3 not in (l, r)]
        sub_pairs, sub_table, sub_w = [prs[p] for p in keep], np.ascontiguousarray(table[keep]), [1 / 3] * 3
        want, A = sc.ref_srp(S, sub_pairs, sub_table, D0).combined(sub_w)
        assert np.isfinite(want).all()
        tally.add("srp", sc.judge("nan srp, the pairs without the NaN's channel",
                                  sp.srp_feats(S, sub_pairs, sub_table, sub_w, D0), want, A))
    tally.finish()
