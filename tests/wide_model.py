"""
numpy model of the 9-to-16-channel covariance of setk_amd/csrc/wide.hip as the kernels compute it:
the stacking z = [Re x ; Im x], the operand and result lane maps of v_mfma_f32_32x32x2_f32, the
chunks of 8 frames split between the two halves of a wave, the slabs of 128 frames summed in slab
order, the pairs j <= k read out of a result tile, and the embedding into the 16 x 16 problems of
the weight solve.  `dtype` is the arithmetic of the sums (the kernel's is float32).
tests/test_wide_model.py states what this construction has to give (no GPU needed); the GPU tests
check the kernels themselves.
"""
import numpy as np

CP, NP16, SLAB, BINS_PAD = 16, 136, 128, 264


def pair_index(i, j, c=CP):
    return i * c - i * (i - 1) // 2 + (j - i)


def operand_lanes(xb, mask, C, tb, t_end, dtype):
    """The A and B registers of the 64 lanes for the four instructions of one chunk.  xb: [C][Tp]
    complex of the bin (anything may stand in the frames >= t_end), mask: [T] weights.  Lane l
    carries row l & 31 of z for frame tb + 4 (l >> 5) + j in instruction j."""
    a = np.zeros((4, 64), dtype)
    b = np.zeros((4, 64), dtype)
    for lane in range(64):
        r, kh = lane & 31, lane >> 5
        if r >= 2 * C:
            continue  # rows 2C .. 31 are zero
        c, imag = (r, False) if r < C else (r - C, True)
        for j in range(4):
            t = tb + 4 * kh + j
            if t >= t_end:
                continue  # selected away, never multiplied
            z = dtype(xb[c, t].imag if imag else xb[c, t].real)
            a[j, lane] = dtype(mask[t]) * z
            b[j, lane] = z
    return a, b


def mfma_32x32x2(a, b, acc):
    """D = A B + C with lane l holding A[l & 31][l >> 5] and B[l >> 5][l & 31]; k ordered."""
    for k in range(2):
        acc = acc + np.outer(a[32 * k:32 * k + 32], b[32 * k:32 * k + 32]).astype(acc.dtype)
    return acc


def result_regs(tile):
    """The 32 x 32 result as the 16 registers of the 64 lanes: column = lane & 31,
    row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)."""
    regs = np.empty((16, 64), tile.dtype)
    for reg in range(16):
        for lane in range(64):
            regs[reg, lane] = tile[(reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31]
    return regs


def tile_of_regs(regs):
    """What store_pairs leaves in the wave's LDS image."""
    tile = np.full((32, 32), np.nan, regs.dtype)
    for reg in range(16):
        for lane in range(64):
            tile[(reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31] = regs[reg, lane]
    return tile


def pairs_of_tile(G, C):
    """[re 136 | im 136] of Phi = (A + D) + i (B^T - B), pairs j <= k < C; the rest zero."""
    out = np.zeros(2 * NP16, G.dtype)
    for j in range(C):
        for k in range(j, C):
            e = pair_index(j, k)
            out[e] = G[j, k] + G[C + j, C + k]
            out[NP16 + e] = G[k, C + j] - G[j, C + k]
    return out


def slab_tile(xb, mask, C, t0, t1, dtype):
    """G of one (bin, slab): chunks of 8 frames, four instructions each."""
    acc = np.zeros((32, 32), dtype)
    for tc in range(t0, t1, 8):
        a, b = operand_lanes(xb, mask, C, tc, t1, dtype)
        for j in range(4):
            acc = mfma_32x32x2(a[j], b[j], acc)
    return acc


def covar_planes(xb, mask, C, T, dtype=np.float32, den=None, pad_diag=0.0):
    """One covariance of one bin as the 272 plane values the solve reads.  den: the normaliser
    (default sum of the mask)."""
    num = np.zeros(2 * NP16, dtype)
    msum = dtype(0)
    for t0 in range(0, T, SLAB):
        t1 = min(T, t0 + SLAB)
        G = tile_of_regs(result_regs(slab_tile(xb, mask, C, t0, t1, dtype)))
        num = num + pairs_of_tile(G, C)
        msum = msum + np.sum(np.asarray(mask[t0:t1], dtype), dtype=dtype)
    d = dtype(msum if den is None else den)
    out = num * (dtype(1) / max(d, dtype(1e-6)))
    if C < CP and pad_diag:
        dmax = max(out[pair_index(i, i)] for i in range(C))
        for i in range(C, CP):
            out[pair_index(i, i)] = dtype(pad_diag) * dmax
    return out


def matrix_of_planes(planes, C=CP):
    """The leading C x C block (default: the whole 16 x 16 embedding) as a matrix."""
    M = np.zeros((C, C), np.complex128 if planes.dtype == np.float64 else np.complex64)
    for i in range(C):
        for j in range(i, C):
            e = pair_index(i, j)
            M[i, j] = complex(planes[e], 0.0 if i == j else planes[NP16 + e])
            if i != j:
                M[j, i] = complex(planes[e], -planes[NP16 + e])
    return M
