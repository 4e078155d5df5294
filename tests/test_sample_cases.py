"""
The sample I/O cases of sample_cases.py judged on the CPU (no GPU): the exact integer reference
against the host writer's rule, the family's power to tell the two quantiser rules apart, the ingest
patterns and the numpy statement of the renorm.  Every test prints its figures before it asserts.
"""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import sample_cases as sm  # noqa: E402


def test_host_writer_is_the_exact_rule_on_the_whole_family():
    from setk_amd.libs.wavio import float_to_pcm16
    x, ref = sm.quantiser_family()
    got = float_to_pcm16(x)
    print(f"quantiser family: {x.size} members, wavio.float_to_pcm16 differs on {np.count_nonzero(got != ref)}")
    assert x.dtype == np.float32 and ref.dtype == np.int16 and got.dtype == np.int16
    assert x.size > 3 * 65535
    assert np.array_equal(got, ref)


def test_exact_reference_on_values_known_by_hand():
    one = np.float32(1.0)
    cases = [(0.0, 0), (-0.0, 0), (0.5, 16384), (-0.5, -16384),            # 16383.5: ties to even
             (1.0, 32767), (-1.0, -32767),
             (float(np.nextafter(one, np.float32(2))), 32767),             # 32767.0039: no wrap yet
             (2.0, -2), (-2.0, 2), (4.0, -4), (3.0, 32765),                # 65534, -65534, 131068, 98301 mod 2^16
             (float(np.finfo(np.float32).tiny), 0), (3e-45, 0)]
    for v, want in cases:
        got = int(sm.exact_pcm16(np.float32(v)).ravel()[0])
        assert got == want, (v, got, want)
    # the wrap itself: the first sample whose product rounds to 32768
    v = np.float32(32767.5 / 32767.0)
    v = np.nextafter(v, np.float32(2))
    assert int(sm.exact_pcm16(v).ravel()[0]) == -32768


def test_family_tells_the_two_rules_apart():
    x, ref = sm.quantiser_family()
    other = sm.f32_product_pcm16(x)
    differ = int(np.count_nonzero(other != ref))
    step = np.abs(other.astype(np.int32) - ref.astype(np.int32))
    inside = np.abs(x) < 1
    print(f"float32-product rule differs from the declared rule on {differ} of {x.size} members; "
          f"largest step inside (-1, 1): {int(step[inside].max())}")
    assert differ >= 30000
    assert int(step[inside].max()) == 1


def test_exactly_two_members_are_exact_ties():
    x, ref = sm.quantiser_family()
    ties = sm.exact_ties(x)
    print(f"exact ties in double: {x[ties].tolist()} -> {ref[ties].tolist()}")
    assert int(ties.sum()) == 2
    assert sorted(x[ties].tolist()) == [-0.5, 0.5]
    assert sorted(ref[ties].tolist()) == [-16384, 16384]


def test_family_rows_rotate_and_interleave():
    x, ref = sm.quantiser_family()
    for C, N in ((1, 1000), (3, 777), (8, x.size + 5)):
        audio, want = sm.family_rows(C, N)
        assert audio.shape == (C, N) and want.shape == (N, C)
        for c in range(C):
            assert audio[c, 0] == x[(7919 * c) % x.size] and want[0, c] == ref[(7919 * c) % x.size]
        assert np.array_equal(want, sm.exact_pcm16(audio).T)


def test_ingest_patterns_carry_both_extremes_in_every_channel():
    for C in range(1, 17):
        for n in (2, 3, 5, 257, 4099):
            pcm = sm.ingest_pattern(n, C)
            assert pcm.shape == (n, C) and pcm.dtype == np.int16
            assert (pcm.min(axis=0) == -32768).all() and (pcm.max(axis=0) == 32767).all(), (C, n)
        one = sm.ingest_pattern(1, C)
        assert set(np.unique(one)) <= {-32768, 32767}
    # neighbours in time and in channel are far apart: a misplaced sample is an error of order one
    pcm = sm.ingest_pattern(4099, 6).astype(np.int32)
    body = pcm[40:]           # (past the rows that hold the planted extremes)
    assert np.abs(np.diff(body, axis=0)).min() > 4000 and np.abs(np.diff(body, axis=1)).min() > 4000
    f = sm.ingest_float(sm.ingest_pattern(257, 3))
    assert f.shape == (3, 257) and f.dtype == np.float32 and f.min() == -1.0 and f.max() == np.float32(32767 / 32768)


def test_renorm_statement():
    w = np.random.default_rng(2).standard_normal(5000).astype(np.float32)
    omax = np.abs(w).max()
    assert np.array_equal(sm.renorm_f32(w, 0.0, omax), w) and np.array_equal(sm.renorm_f32(w, -1.0, omax), w)
    y = sm.renorm_f32(w, 0.9, omax)
    exact = w.astype(np.float64) * 0.9 / (float(omax) + 2.0 ** -23)
    ulp = np.spacing(np.abs(y))
    assert y.dtype == np.float32 and (np.abs(y - exact) <= 1.5 * ulp).all()     # two float32 roundings
    assert abs(float(np.abs(y).max()) - 0.9) < 1e-6
    lo, hi = sm.renorm_scale_neighbours(0.9, omax)[1:]
    assert lo < sm.renorm_scale(0.9, omax) < hi


def test_rules_disagree_on_plain_waveforms_too():
    """The figures of the issue: a Gaussian waveform of 400 000 samples renormed as the kernel does."""
    counts = {peak: sm.gaussian_disagreement(peak) for peak in (0.9, 0.3, 0.05)}
    print("Gaussian, 400000 samples, samples on which the float32-product rule differs:", counts)
    assert counts[0.9] > counts[0.05] and counts[0.9] >= 20
