"""
The float64 oracle on the constructed spectrograms of cgmm_cases.py (no GPU): it must be a sound
reference there before a device kernel is held to it cell by cell.  For every family the GPU file
test_gpu_cgmm_conformance.py runs (channel count x every frame count on an edge of the library's
dispatcher x start x iterations) the oracle raises nothing, returns finite posteriors, and
answers a float32-rounding-sized perturbation of its input with less than 5e-5 per cell -- the
figure that makes the GPU file's per-cell bar of 1e-3 meaningful after one or two iterations
from a fixed start.
"""
import numpy as np
import pytest

import cgmm_cases as cc


def library_config(C, T):
    """setk_cgmm_bin_config: host code of the library, no device."""
    from setk_amd import _ffi
    return _ffi.cgmm_bin_config(C, T)


@pytest.mark.parametrize("C", range(1, 9))
def test_oracle_is_finite_and_insensitive_to_input_rounding(C):
    worst, floored = {}, 0
    edges = cc.t_edges(C, library_config)
    assert {1, 2, 3, C, C + 1, 31, 32, 33, 63, 65, 640, 641, 1024, 1025, 2048, 2049} <= set(edges)
    for T in edges:
        obs, seed = cc.sound_case(C, T)
        assert obs.dtype == np.complex64 and obs.shape == (C, 6, T) and np.isfinite(obs).all()
        pert = cc.perturbed(obs, seed)
        for start in cc.STARTS:
            init, ua = cc.start_args(start, 6, T, seed)
            for iters in ((0, 1, 2) if T <= cc.SHORT_T else (1, 2)):
                with np.errstate(all="raise", under="ignore"):
                    g = cc.oracle_gamma(obs, iters, init, ua)
                gp = cc.oracle_gamma(pert, iters, init, ua)
                where = f"C={C} T={T} seed={seed} start={start} iters={iters}"
                assert g.shape == (2, 6, T) and np.isfinite(g).all() and g.min() >= 0.0, where
                # the posteriors sum to one except where the reference's own denominator floor
                # max(sum_k alpha_k N_k, eps) (cluster.py:261-287) is active: only with
                # --update-alpha, after a class's weight has collapsed on a rank-deficient bin
                s = g.sum(0)
                assert s.max() < 1.0 + 1e-12, where
                short = s < 1.0 - 1e-12
                assert not short.any() or (ua and iters > 0 and T <= 4 * C), where
                floored += int(short.sum())
                rows = cc.bin_report(gp[0], g[0])
                for r in rows:
                    worst[r["kind"]] = max(worst.get(r["kind"], 0.0), r["max"])
                bad = [r for r in rows if not r["max"] < cc.SENSITIVITY_BAR]
                assert not bad, where + ": " + cc.describe(bad)
    print(f"[oracle sensitivity C={C}, {len(edges)} frame counts] "
          + "  ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + f"  cells whose posteriors sum to less than one: {floored}")


def test_the_layout_tile_and_batch_cases():
    """F = 33 (a second 32-bin tile) and the frame counts of the ragged batch test."""
    for C, T, F in ((3, 33, 33), (3, 65, 33), (2, 7, 6), (6, 513, 6), (8, 3386, 6)):
        obs, seed = cc.sound_case(C, T, F=F)
        worst, rows = cc.sensitivity(obs, seed)
        assert worst < cc.SENSITIVITY_BAR, (C, T, F, cc.describe(rows))


def test_bin_kinds_are_what_they_say():
    obs = cc.make_case(5, 40, F=12, seed=3)
    p = (np.abs(obs.astype(np.complex128)) ** 2).sum(0)               # F x T
    for f in range(12):
        kind = cc.kind_of_bin(f)
        assert kind == cc.KINDS[f % 6]
        zero = np.flatnonzero(p[f] == 0.0)
        if kind == "zero_frame":
            assert list(zero) == [40 // 3]
        elif kind == "half_zero":
            assert list(zero) == list(range(20))
        else:
            assert zero.size == 0
        s = np.linalg.svd(obs[:, f, :].astype(np.complex128), compute_uv=False)
        if kind == "tiny":
            assert np.median(p[f]) < 1.1920929e-07 < p[f].max()       # phi's floor: on and off
        if kind == "big":
            assert p[f].min() > 1e4
        if kind == "rank1":
            assert s[1] <= 1e-15 * s[0]                               # exactly rank 1
        if kind == "ordinary":
            assert s[-1] > 0.05 * s[0]                                # full rank
    assert np.array_equal(obs, cc.make_case(5, 40, F=12, seed=3))     # seeded
    m = cc.init_mask(6, 9)
    assert m.dtype == np.float32 and m.shape == (6, 9) and 0.05 <= m.min() and m.max() <= 0.95


def test_t_edges_follow_the_supplied_dispatcher():
    """A made-up table: 64 threads x (2 frames, 1 in registers) up to T = 128, 64 x (4, 3) up to
    256, not resident beyond."""
    def config(C, T):
        if T <= 128:
            return (0, 64, 2, 1)
        if T <= 256:
            return (1, 64, 4, 3)
        return (-1, 0, 0, 0)
    assert [t for t, _ in cc.scan_configs(4, config, 400)] == [1, 129, 257]
    edges = cc.t_edges(4, config, 400)
    for t in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 128, 129, 130, 191, 192, 193, 256, 257, 258):
        assert t in edges
    assert edges == sorted(set(edges)) and edges[0] == 1 and edges[-1] <= 400
    rows = cc.bin_report(np.array([[0.0, 0.5, 0.0]]), np.zeros((1, 3)), nt=2)
    assert rows[0]["frame"] == 1 and rows[0]["lane"] == 1 and rows[0]["max"] == 0.5
    assert abs(rows[0]["mean"] - 0.5 / 3) < 1e-15
