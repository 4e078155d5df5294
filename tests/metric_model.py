"""
The float64 statement of SI-SNR scoring that the device is held to (tests/PARITY_NOTES_METRIC.md):
libs/metric.py:13-60 of the reference with every operation in float64 on the samples as given, the
residual n formed per sample, and a plain itertools walk over the orders.  Test infrastructure, not
product code: nothing under setk_amd imports it.
"""
from itertools import permutations

import numpy as np

EPS = 1e-8
FLOOR_DB = -160.0  # 20 log10(eps): silent or constant signals, one sample


def si_snr(x, s, eps=EPS, remove_dc=True):
    x = np.asarray(x, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    if remove_dc:
        x = x - np.mean(x)
        s = s - np.mean(s)
    a = np.dot(x, s) / (np.dot(s, s) + eps)
    t = a * s
    n = x - t
    return float(20 * np.log10(np.sqrt(np.dot(t, t)) / (np.sqrt(np.dot(n, n)) + eps) + eps))


def pair_table(xlist, slist, eps=EPS, remove_dc=True):
    """table[i, j] = si_snr(xlist[i], slist[j])"""
    return np.array([[si_snr(x, s, eps, remove_dc) for s in slist] for x in xlist], dtype=np.float64)


def best_order(table):
    """permute_si_snr(align=True) on a K x K table: the orders in itertools' own order, each
    valued sum(table[n, order[n]] for n) / K added left to right from 0, the first maximum."""
    K = table.shape[0]
    orders = list(permutations(range(K)))
    values = [sum([float(table[n, order[n]]) for n in range(K)]) / K for order in orders]
    idx = int(np.argmax(values))
    return values[idx], orders[idx]


def permute_si_snr(xlist, slist, align=False):
    if len(xlist) != len(slist):
        raise RuntimeError("size do not match between xlist " + f"and slist: {len(xlist)} vs {len(slist)}")
    best, order = best_order(pair_table(xlist, slist))
    return (best, order) if align else best


def planted(rng, L, db, scale=0.7, est_dc=-0.02, ref_dc=0.05, amp=0.1):
    """(estimate, reference) float32 of L samples whose SI-SNR is about `db`: reference Gaussian
    with an offset, estimate = scale x reference + noise + another offset."""
    s = amp * rng.standard_normal(L)
    noise = rng.standard_normal(L)
    noise *= scale * np.linalg.norm(s) / max(np.linalg.norm(noise), 1e-30) * 10.0 ** (-db / 20.0)
    return (scale * s + noise + est_dc).astype(np.float32), (s + ref_dc).astype(np.float32)
