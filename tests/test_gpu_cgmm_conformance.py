"""
Conformance of the three device forms of the two-class CGMM -- the bin-resident EM (cgmm_bin.hip:
8 channel counts x 6 configurations), the streaming kernels (cgmm.hip) and the general fp64 EM
(cgmm_k.hip) -- against the float64 oracle on the constructed spectrograms of cgmm_cases.py.

Every case is tiny (F = 6 bins, 33 where a 32-bin tile edge matters) and runs 0, 1 or 2 EM
iterations from a fixed start: there the oracle itself moves by less than 5e-5 per cell under
input rounding (test_cgmm_cases.py), so EVERY cell of a bin with more than 4 C frames is held
to the bar the older tests apply to decided cells, and every bin on its own to the bar they
apply to the whole-mask mean; bins with fewer frames have measured bars (BARS).  Which
instantiation a case ran, and where the frame-count edges are, comes from the library
(setk_cgmm_bin_config), not from a copy of its table.  Measured figures, the bars' reasons and
what the file found: PARITY_NOTES_CGMM.md.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cgmm_cases as cc

pytestmark = pytest.mark.gpu

# max |gamma - gamma_ref| over all cells, mean |d| of each bin on its own, and gamma_0 + gamma_1
# against the oracle's sum (1 wherever its denominator floor is off).  "long" is the project's
# own bars, undiluted; the others are for bins that hold fewer than 4 C non-zero frames n, where
# float32 frame passes cannot follow the float64 reference (PARITY_NOTES_CGMM.md: an eigenvalue
# of a class covariance below 1e-3 of the largest is lost in float32 sums, and with so few
# frames the EM's own weights put one there): the worst error measured against the oracle over
# both float32 forms, times 4.
BARS = {
    "long": (1e-3, 1e-4, 1e-5),                      # n > 4 C
    "short": (4 * 6.46e-3, 4 * 7.68e-4, 1e-5),       # C + 1 < n <= 4 C
    "square": (4 * 8.27e-2, 4 * 1.30e-2, 1e-5),      # C <= n <= C + 1
    "deficient": (4 * 1.64e-2, 4 * 2.39e-3, 4 * 1.44e-3),   # n < C
}


def regime(n, C):
    return "deficient" if n < C else "square" if n <= C + 1 else "short" if n <= 4 * C else "long"


HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def config(C, T):
    from setk_amd import _ffi
    return _ffi.cgmm_bin_config(C, T)


@pytest.fixture(scope="module")
def ctx():
    from setk_amd import _ffi
    return _ffi.default_context()


def device_gamma(ctx, obs, iters, init=None, update_alpha=False):
    """setk_cgmm_masks on obs [C][F][T]: posteriors [2][F][T] float32 (and mask == class 0)."""
    C, F, T = obs.shape
    spec = np.ascontiguousarray(np.transpose(obs, (0, 2, 1)))
    gamma = np.full((2, T, F), np.nan, np.float32)
    mask = np.full((T, F), np.nan, np.float32)
    ctx.cgmm_masks(spec, C, T, F, iters, None if init is None else np.ascontiguousarray(init.T),
                   gamma, mask, update_alpha=update_alpha)
    assert np.array_equal(mask, gamma[0]), "mask_out is not class 0 of gamma_out"
    return np.transpose(gamma, (0, 2, 1))


class Tally:
    """Failures with everything a log needs, and the worst figures per (configuration, kind)."""

    def __init__(self):
        self.failures, self.worst = [], {}

    def check(self, where, idx, nt, got, ref, obs):
        """got [2][F][T] or [F][T] (class 0 only) against the oracle's ref [2][F][T] for the case
        obs [C][F][T]; returns the worst per-cell error of the run."""
        both = got.ndim == 3
        g0 = got[0] if both else got
        where = f"{where} cfg={idx}"
        if not np.isfinite(got).all():
            self.failures.append(f"{where}: non-finite posteriors")
            return float("inf")
        C = obs.shape[0]
        nonzero = ((np.abs(obs.astype(np.complex128)) ** 2).sum(0) > 0).sum(-1)      # per bin
        rows = cc.bin_report(g0, ref[0], nt)
        ds = np.abs(got.astype(np.float64).sum(0) - ref.sum(0)).max(-1) if both else np.zeros(len(rows))
        d1 = np.abs(got[1].astype(np.float64) - ref[1]).max(-1) if both else np.zeros(len(rows))
        bad = []
        for r, n, dsum, dk1 in zip(rows, nonzero, ds, d1):
            r["regime"] = regime(n, C)
            r["max"] = max(r["max"], float(dk1))            # class 1's plane counts like class 0's
            cell, mean, total = BARS[r["regime"]]
            w = self.worst.setdefault((idx, r["regime"], r["kind"]), [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], r["max"]), max(w[1], r["mean"]), max(w[2], float(dsum))
            if not (r["max"] < cell and r["mean"] < mean):
                bad.append(r)
            if not dsum < total:
                self.failures.append(f"{where}: gamma_0 + gamma_1 off by {dsum:.2e} in bin {r['bin']} "
                                     f"({r['kind']}, {n} non-zero frames: {r['regime']})")
        if bad:
            self.failures.append(f"{where}: " + "; ".join(
                f"{cc.describe([r])} [{r['regime']}]" for r in bad))
        return max(r["max"] for r in rows)

    def run(self, ctx, C, T, obs, seed, start, iters, tag=""):
        idx, nt = config(C, T)[:2]
        F = obs.shape[1]
        init, ua = cc.start_args(start, F, T, seed)
        ref = cc.oracle_gamma(obs, iters, init, ua)
        got = device_gamma(ctx, obs, iters, init, ua)
        err = self.check(f"{tag}C={C} T={T} seed={seed} start={start} iters={iters}", idx, nt, got, ref, obs)
        return idx, got, ref, err

    def report(self, tag):
        for (idx, reg, kind), (mx, mean, dsum) in sorted(self.worst.items(), key=str):
            print(f"[cgmm conformance] {tag} cfg {idx!s:>2} {reg:9s} {kind:10s} max |d| {mx:.2e}  "
                  f"worst bin mean {mean:.2e}  sum {dsum:.1e}")

    def finish(self, tag):
        self.report(tag)
        assert not self.failures, f"{len(self.failures)} failing runs:\n" + "\n".join(self.failures[:40])


def run_edges(ctx, tally, C, frame_counts, tag=""):
    """Every start x 1 and 2 iterations at each frame count; the configurations they ran."""
    ran = set()
    for T in frame_counts:
        obs, seed = cc.sound_case(C, T)
        for start in cc.STARTS:
            for iters in (1, 2):
                ran.add(tally.run(ctx, C, T, obs, seed, start, iters, tag)[0])
    return ran


@pytest.mark.parametrize("C", range(1, 9))
def test_matrix_every_reachable_configuration_at_every_frame_count_edge(ctx, C):
    """Every T at which the dispatcher changes configuration (the change to the streaming kernels
    included), every nt * rf (all frames in registers / the first frame in LDS), each +- 1, and
    1, 2, 3, C - 1, C, C + 1, 31, 32, 33, 63, 65: three starts x 1 and 2 iterations; num_iters = 0
    once per start.  The configurations exercised are the ones the scan finds reachable."""
    scan = cc.scan_configs(C, config)
    reachable = {cfg[0] for _, cfg in scan}
    assert -1 in reachable and len(reachable) >= 4, scan
    tally = Tally()
    ran = run_edges(ctx, tally, C, cc.t_edges(C, config))
    obs, seed = cc.sound_case(C, 65)
    for start in cc.STARTS:
        tally.run(ctx, C, 65, obs, seed, start, 0)
    tally.finish(f"matrix C={C}")
    assert ran == reachable, (C, sorted(ran), sorted(reachable))


# ---- child processes: the dispatcher reads SETK_CGMM_CFG / SETK_CGMM_STREAMING once ----------
def child_main(mode, value):
    """Runs in a fresh process with the variable set; prints one JSON line."""
    from setk_amd import _ffi
    ctx = _ffi.default_context()
    tally = Tally()
    out = dict(ran={}, refused={})
    for C in range(1, 9):
        if mode == "cfg":
            edges = cc.t_edges(C, config)
            mine = [T for T in edges if config(C, T)[0] == value]
            # the dispatcher keeps its own choice where the forced configuration cannot hold the
            # utterance; those frame counts are reported, not run
            out["refused"][C] = [T for T in edges if T <= max(mine, default=0) and T not in mine]
        else:
            mine = sorted({1, 2, 3, max(C - 1, 1), C, C + 1, 31, 32, 33})
        ran = run_edges(ctx, tally, C, mine, tag=f"[{mode}={value}] ")
        out["ran"][C] = dict(frame_counts=mine, configs=sorted(ran), info=config(C, mine[0])[1:] if mine else None)
    tally.report(f"{mode}={value}")
    out["failures"] = tally.failures
    print("RESULT " + json.dumps(out))


def run_child(mode, value, env):
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_cgmm_conformance as m; "
            "m.child_main(%r, %r)" % (HERE, ROOT, mode, value))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **env))
    if r.returncode != 0:     # a crash is not a parity failure
        raise RuntimeError(f"child process ({mode}={value}) ended with {r.returncode}:\n{r.stderr[-3000:]}")
    lines = r.stdout.strip().splitlines()
    print("\n".join(l for l in lines if l.startswith("[cgmm conformance]")))
    return json.loads([l for l in lines if l.startswith("RESULT ")][-1][7:])


def unreachable_configs():
    reachable = {cfg[0] for C in range(1, 9) for _, cfg in cc.scan_configs(C, config)}
    # the table's length is not exported: a forced index the dispatcher does not know is refused
    # for every shape, which the child reports as "ran nothing"
    return [i for i in range(max(reachable) + 1) if i not in reachable]


@pytest.mark.parametrize("idx", [1, 4])
def test_forced_configurations_that_no_shape_reaches(idx):
    """The configurations the dispatcher never picks on its own (SETK_CGMM_CFG, A/B measurements):
    one child process each, C = 1 .. 8, at that configuration's own frame-count edges."""
    # a table change that makes one of them reachable moves it to the matrix, a new unreachable
    # one has to be added here
    assert unreachable_configs() == [1, 4]
    out = run_child("cfg", idx, {"SETK_CGMM_CFG": str(idx)})
    for C in range(1, 9):
        ran = out["ran"][str(C)]
        # the force took: every short count, the all-in-registers edge and the last count of the
        # configuration ran it and nothing else did; no shape it can hold was refused
        assert ran["configs"] == [idx], (idx, C, ran, out["refused"][str(C)])
        nt, u, rf = ran["info"]
        assert {1, 2, 3, C, 33, 65, nt * rf - 1, nt * rf, nt * rf + 1, nt * u} <= set(ran["frame_counts"]), \
            (idx, C, ran["frame_counts"])
        assert max(ran["frame_counts"]) == nt * u
        assert out["refused"][str(C)] == [], (idx, C, out["refused"][str(C)])
    assert not out["failures"], "\n".join(out["failures"][:40])


def test_streaming_kernels_on_the_short_frame_counts():
    """SETK_CGMM_STREAMING=1: T < C, 1, 2, 3, 31 .. 33 through cgmm.hip for C = 1 .. 8."""
    out = run_child("streaming", 1, {"SETK_CGMM_STREAMING": "1"})
    for C in range(1, 9):
        assert out["ran"][str(C)]["configs"] == [-1], (C, out["ran"][str(C)])
    assert not out["failures"], "\n".join(out["failures"][:40])


@pytest.mark.parametrize("C", range(1, 9))
def test_natural_fallback_boundary(ctx, C):
    """The first frame count the entry sends to the streaming kernels, and the one before it (the
    same utterance without its last frame): each side meets the bars, and on the frames they
    share the two device masks differ by no more than the oracle's two masks do plus the two
    errors against the oracle."""
    scan = cc.scan_configs(C, config)
    Tf = scan[-1][0]
    assert scan[-1][1][0] == -1 and config(C, Tf - 1)[0] >= 0
    full, seed = cc.sound_case(C, Tf)
    tally = Tally()
    for start in cc.STARTS:
        ia, ga, ra, ea = tally.run(ctx, C, Tf, full, seed, start, 2)
        init, ua = cc.start_args(start, 6, Tf, seed)
        cut = np.ascontiguousarray(full[:, :, :Tf - 1])
        init_cut = None if init is None else np.ascontiguousarray(init[:, :Tf - 1])
        rb = cc.oracle_gamma(cut, 2, init_cut, ua)
        # the shortened case is a new construction: the oracle must be sound on it too
        moved = np.abs(cc.oracle_gamma(cc.perturbed(cut, seed), 2, init_cut, ua) - rb).max()
        assert moved < cc.SENSITIVITY_BAR, (C, Tf - 1, start, moved)
        ib, nt = config(C, Tf - 1)[:2]
        gb = device_gamma(ctx, cut, 2, init_cut, ua)
        eb = tally.check(f"C={C} T={Tf - 1} (first {Tf - 1} frames of seed {seed}) start={start} iters=2",
                         ib, nt, gb, rb, cut)
        assert ia == -1 and ib >= 0
        between = np.abs(ga[:, :, :Tf - 1].astype(np.float64) - gb)
        bound = np.abs(ra[:, :, :Tf - 1] - rb) + ea + eb + 1e-7
        assert (between <= bound).all(), (C, Tf, start, float((between - bound).max()))
    tally.finish(f"fallback C={C} T={Tf - 1}|{Tf}")


@pytest.mark.parametrize("C", [1, 4, 8])
def test_three_device_forms_agree(ctx, C):
    """The general fp64 EM (setk_cgmm_masks_k, K = 2) with the deterministic start and with an
    initial mask against the bin-resident EM on the edge-bin case; each is held to the oracle."""
    T, F = 300, 6
    obs, seed = cc.sound_case(C, T)
    spec = np.ascontiguousarray(np.transpose(obs, (0, 2, 1)))
    tally = Tally()
    for start in ("identity", "mask"):
        idx, gbin, ref, ebin = tally.run(ctx, C, T, obs, seed, start, 2)
        assert idx >= 0
        init, _ = cc.start_args(start, F, T, seed)
        gk = np.full((2, T, F), np.nan, np.float32)
        ctx.cgmm_masks_k(spec, C, T, F, 2, 2, None, None if init is None else np.ascontiguousarray(init.T), gk)
        gk = np.transpose(gk, (0, 2, 1))
        ek = tally.check(f"general EM C={C} T={T} seed={seed} start={start} iters=2", "k", 0, gk, ref, obs)
        print(f"[cgmm conformance] forms C={C} start={start}: bin-resident {ebin:.2e}, general fp64 {ek:.2e}")
        assert np.abs(gk.astype(np.float64) - gbin).max() <= ebin + ek + 1e-7
    tally.finish(f"forms C={C}")


@pytest.mark.parametrize("C,T", [(3, 700), (3, 1500), (8, 700), (8, 1500)])
def test_frame_order_does_not_matter(ctx, C, T):
    """CGMM is a function of the SET of frames.  Reversing them (with the initial mask) swaps
    which frames sit in registers and which in LDS and which thread owns the ragged tail of the
    last, partly filled chunk; a fixed random permutation scatters them.  T = 700 runs 256 x 4,
    T = 1500 runs 256 x 8."""
    idx, nt, u, rf = config(C, T)
    assert idx >= 0 and T % nt != 0 and T > nt * rf
    obs, seed = cc.sound_case(C, T)
    init = cc.init_mask(6, T, seed)
    tally = Tally()
    _, g, ref, e = tally.run(ctx, C, T, obs, seed, "mask", 2)
    orders = dict(reversed=np.arange(T)[::-1], permuted=np.random.default_rng(T + C).permutation(T))
    for name, order in orders.items():
        obs_p = np.ascontiguousarray(obs[:, :, order])
        init_p = np.ascontiguousarray(init[:, order])
        ref_p = cc.oracle_gamma(obs_p, 2, init_p, False)
        # the oracle agrees with itself: float64 summation order (1e-16) over the eigenvalue floor
        # eps comes to 5e-9 on the exactly rank-1 bin, 1e-13 elsewhere
        assert np.abs(ref_p - ref[:, :, order]).max() < 1e-7
        g_p = device_gamma(ctx, obs_p, 2, init_p)
        e_p = tally.check(f"{name} C={C} T={T} seed={seed} start=mask iters=2", idx, nt, g_p, ref_p, obs_p)
        diff = np.abs(g_p.astype(np.float64) - g[:, :, order])
        f, t = np.unravel_index(int(np.argmax(diff.max(0))), diff.shape[1:])
        assert diff.max() <= e + e_p + 1e-7, \
            f"{name} C={C} T={T} cfg={idx}: {diff.max():.2e} > {e:.2e} + {e_p:.2e} at bin {f} " \
            f"({cc.kind_of_bin(f)}) frame {t} (frame % nt = {t % nt}; source frame {order[t]}, % nt = {order[t] % nt})"
    tally.finish(f"order C={C} T={T}")


@pytest.mark.parametrize("C", [2, 6, 8])
def test_ragged_batch_across_frame_count_classes(ctx, C):
    """One setk_cgmm_masks_batch launch with T = 1, 7, 513, 2049 and the longest bin-resident
    count: the configuration is the longest utterance's, so most threads of the short ones own
    nothing.  Once with initial masks and the natural pitch, once from the deterministic start
    with --update-alpha and spec_pitch = F + 3.  Every utterance meets the oracle bars and equals
    its single-utterance call: bit for bit where that call runs the same configuration."""
    import torch
    F = 6
    Tmax = cc.scan_configs(C, config)[-1][0] - 1
    frames = [1, 7, 513, 2049, Tmax]
    idx, nt = config(C, Tmax)[:2]
    assert idx >= 0
    dev = torch.device("cuda", ctx.device)
    cases = [cc.sound_case(C, T) for T in frames]
    tally = Tally()
    for start, pitch in (("mask", 0), ("alpha", F + 3)):
        specs, inits, outs = [], [], []
        for (obs, seed), T in zip(cases, frames):
            P = pitch or F
            spec = np.zeros((C, T, P), np.complex64)
            spec[:, :, :F] = np.transpose(obs, (0, 2, 1))
            if pitch:
                spec[:, :, F:] = 1e3 + 1e3j               # the padding is never read
            specs.append(torch.from_numpy(spec).to(dev))
            init, ua = cc.start_args(start, F, T, seed)
            inits.append(None if init is None else torch.from_numpy(np.ascontiguousarray(init.T)).to(dev))
            outs.append(torch.full((T, F), float("nan"), dtype=torch.float32, device=dev))
        ctx.cgmm_masks_batch(C, [s.data_ptr() for s in specs], frames, F, 2,
                             None if inits[0] is None else [i.data_ptr() for i in inits],
                             [t.data_ptr() for t in outs], update_alpha=ua, spec_pitch=pitch)
        torch.cuda.synchronize()
        for (obs, seed), T, out in zip(cases, frames, outs):
            got = out.cpu().numpy().T                         # F x T, class 0
            init, ua = cc.start_args(start, F, T, seed)
            ref = cc.oracle_gamma(obs, 2, init, ua)
            eb = tally.check(f"batch of {frames} pitch={pitch or F} utterance C={C} T={T} seed={seed} "
                             f"start={start} iters=2", idx, nt, got, ref, obs)
            single = device_gamma(ctx, obs, 2, init, ua)
            own = config(C, T)
            es = tally.check(f"single C={C} T={T} seed={seed} start={start} iters=2", own[0], own[1], single, ref, obs)
            diff = np.abs(got.astype(np.float64) - single[0])
            if own[0] == idx:
                assert np.array_equal(got, single[0]), (C, T, start, idx, float(diff.max()))
            else:
                assert diff.max() <= eb + es + 1e-7, (C, T, start, idx, own[0], float(diff.max()), eb, es)
    tally.finish(f"batch C={C}")


@pytest.mark.parametrize("C,T", [(3, 33), (3, 65), (8, 33), (8, 65)])
def test_layout_tiles_last_bin_and_last_frame(ctx, C, T):
    """F = 33: the second 32-bin tile of the two layout kernels holds one bin, T = 33 / 65 leave
    one frame in the last 32-frame tile.  Both classes' planes, last bin and last frame included."""
    F = 33
    obs, seed = cc.sound_case(C, T, F=F)
    tally = Tally()
    for start in cc.STARTS:
        idx, got, ref, _ = tally.run(ctx, C, T, obs, seed, start, 2)
        for k in (0, 1):
            for f, t in ((F - 1, T - 1), (F - 1, 0), (0, T - 1), (31, 31), (32, 32)):
                assert abs(float(got[k, f, t]) - ref[k, f, t]) < BARS["long"][0], (C, T, idx, start, k, f, t)
    tally.finish(f"tiles C={C} T={T}")
