// wide.hip -- the batched path for 9 to 16 channels: masked spatial covariance on the fp32
// matrix cores and the beamformer, both on the bin-major spectra X[f][c][t] (frames contiguous,
// pitch Tp = (T + 3) & ~3) that stft_binmajor_kernel (pass1.hip) writes.
//
// Replaces (funcwj/setk): compute_covar x2 (x3 for MPDR) (libs/beamformer.py:87-103) and
// beamform (libs/beamformer.py:105-120) of apply_adaptive_beamformer.py:130-178 for a batch.
// Pass 1 for up to 8 channels keeps the accumulators of a bin in registers; 16 channels are
// 136 Hermitian pairs, and the natural form is one 32 x 32 real tile per covariance:
//
//   z_t = [Re x_t ; Im x_t]            2C <= 32 rows (the rest zero)
//   G   = sum_t m_t z_t z_t^T          = [[A, B], [B^T, D]]
//   Phi = sum_t m_t x_t x_t^H          = (A + D) + i (B^T - B)
//
// v_mfma_f32_32x32x2_f32 is exact fp32 (a k-ordered fmaf chain) and takes ONE register per
// operand: lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31], so the same lane carries
// z[row l & 31] of frame k = l >> 5 for both operands, A scaled by the mask.  Which frame
// plays k = 0 / 1 is free as long as both operands agree: of a chunk of 8 frames the lower
// half of the wave takes frames 0-3 and the upper half frames 4-7 (32 contiguous bytes per
// lane), four instructions per covariance and chunk.
//
// A wave owns (utterance, bin, slab of kWideSlab frames); slabs are summed in slab order by
// wide_finalize_kernel (no floating-point atomics: a result depends on the utterance alone).
// Only the pairs j <= k are read out of a tile -- Re from A + D, Im as B[k][j] - B[j][k] -- so
// the covariance is Hermitian bit for bit and its diagonal exactly real.
// Roofline: HBM.  The spectra are read twice (here and by the beamformer): 8 F C Tp bytes each.
#include "common.h"

namespace setk {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kCp = kMaxChannels16;            // the solve's 16-lane form
constexpr int kNP16 = npairs(kCp);             // 136
constexpr int kTileFloats = 2 * kNP16;         // [re NP | im NP] of one covariance
constexpr int kDenOff = 3 * kTileFloats;       // sum_t m_s, sum_t m_n behind the three tiles
constexpr int kTileLd = 33;                    // LDS pitch of a 32 x 32 result tile

// pair e of the upper triangle of a 16 x 16 matrix, row major: (j, k), j <= k
__device__ inline void pair_of(int e, int* j, int* k) {
    int i = 0;
    while (e >= kCp - i) {
        e -= kCp - i;
        ++i;
    }
    *j = i;
    *k = i + e;
}

// One result tile (C/D layout of the 32 x 32 forms: column = lane & 31, row = (reg & 3) +
// 8 (reg >> 2) + 4 (lane >> 5)) through the wave's LDS image to the pairs j <= k < C;
// every other pair of the 16 x 16 embedding is written as zero.
__device__ inline void store_pairs(const f32x16& acc, float* tile, float* dst, int C, int lane,
                                   const int (&pj)[3], const int (&pk)[3], bool store) {
    const int col = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[((i & 3) + 8 * (i >> 2) + 4 * hi) * kTileLd + col] = acc[i];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int e = lane + 64 * q;
        if (e < kNP16) {
            const int j = pj[q], k = pk[q];
            float re = 0.f, im = 0.f;
            if (k < C) {
                re = tile[j * kTileLd + k] + tile[(C + j) * kTileLd + (C + k)];
                im = tile[k * kTileLd + (C + j)] - tile[j * kTileLd + (C + k)];
            }
            if (store) {
                dst[e] = re;
                dst[kNP16 + e] = im;
            }
        }
    }
    __syncthreads();
}

template <bool YY>
__global__ __launch_bounds__(256) void covar_wide_mfma_kernel(WideArgs a) {
    __shared__ float tiles[4][32 * kTileLd];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, kh = lane >> 5;
    const WorkItem wi = a.items[blockIdx.x];
    const UttDesc ud = a.utts[wi.utt];
    const int C = a.num_channels;
    const int T = ud.num_frames, Tp = (T + 3) & ~3;
    const int fq = blockIdx.y * 4 + wave;
    const bool fvalid = fq < kBins;
    const int f = fvalid ? fq : kBins - 1;  // (the last workgroup's spare waves redo bin 256, unstored)
    const bool clamp = (a.flags & 0x2) != 0;
    const bool has_mn = ud.mask_n != nullptr;
    const bool active = r < 2 * C;          // rows 2C..31 of z are zero
    const int c = r < C ? r : r - C;
    const bool imag = r >= C;
    const float2* row = reinterpret_cast<const float2*>(ud.wave_out) + ((size_t)f * C + (active ? c : 0)) * Tp;

    f32x16 acc_s, acc_n, acc_y;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_s[i] = acc_n[i] = acc_y[i] = 0.f;
    float den_s = 0.f, den_n = 0.f;

#pragma unroll 1
    for (int t0 = wi.t0; t0 < wi.t1; t0 += 8) {
        const int tb = t0 + 4 * kh;  // a multiple of 4: tb < T implies tb + 4 <= Tp
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (active && tb < wi.t1) {
            const float4 v0 = *reinterpret_cast<const float4*>(row + tb);
            const float4 v1 = *reinterpret_cast<const float4*>(row + tb + 2);
            z[0] = imag ? v0.y : v0.x;
            z[1] = imag ? v0.w : v0.z;
            z[2] = imag ? v1.y : v1.x;
            z[3] = imag ? v1.w : v1.z;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = tb + j;
            // frames t >= T (the Tp padding, a short last chunk) hold whatever an earlier call
            // left in the arena: selected away, never multiplied
            const bool tv = t < wi.t1;
            const float zj = tv ? z[j] : 0.f;
            float ws = 0.f, wn = 0.f;
            if (tv) {
                ws = ud.mask_s[(size_t)t * kBins + f];
                if (clamp) ws = fminf(ws, 1.f);
                wn = has_mn ? ud.mask_n[(size_t)t * kBins + f] : 1.f - ws;
            }
            den_s += ws;
            den_n += wn;
            acc_s = __builtin_amdgcn_mfma_f32_32x32x2f32(ws * zj, zj, acc_s, 0, 0, 0);
            acc_n = __builtin_amdgcn_mfma_f32_32x32x2f32(wn * zj, zj, acc_n, 0, 0, 0);
            if (YY) acc_y = __builtin_amdgcn_mfma_f32_32x32x2f32(zj, zj, acc_y, 0, 0, 0);
        }
    }
    // the two halves of the wave summed different frames
    den_s += __shfl_xor(den_s, 32);
    den_n += __shfl_xor(den_n, 32);

    int pj[3], pk[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) pair_of(min(lane + 64 * q, kNP16 - 1), &pj[q], &pk[q]);
    float* P = a.partials + ((size_t)wi.part * kBins + f) * kWidePartFloats;
    store_pairs(acc_s, tiles[wave], P, C, lane, pj, pk, fvalid);
    store_pairs(acc_n, tiles[wave], P + kTileFloats, C, lane, pj, pk, fvalid);
    if (YY) store_pairs(acc_y, tiles[wave], P + 2 * kTileFloats, C, lane, pj, pk, fvalid);
    if (fvalid && lane == 0) {
        P[kDenOff + 0] = den_s;
        P[kDenOff + 1] = den_n;
    }
}

// Sum the slabs of every utterance in slab order, normalise by max(sum_t m, 1e-6)
// (libs/beamformer.py:99-102; Ry by the frame count) and lay the result out as the planes the
// solve reads: [Rs.re | Rs.im | Rn.re | Rn.im | (Ry.re | Ry.im)], 136 pairs each, the C x C
// matrix embedded as blkdiag(M, pad I) with pad = 0 for Rs and max_i Re M[i][i] for the
// matrices that get factored -- what pack_covar_kernel (solve.hip) does for the stand-alone
// operators.  A workgroup transposes 16 bins through LDS: contiguous reads of the slabs,
// 64-byte runs along the bins on the way out.
constexpr int kFinBins = 16;

__global__ __launch_bounds__(256) void wide_finalize_kernel(WideArgs a) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x;
    const int u = blockIdx.y, f0 = blockIdx.x * kFinBins;
    const UttDesc ud = a.utts[u];
    const int C = a.num_channels;
    const int ntile = a.with_ry ? 3 : 2;
    const int per_bin = ntile * kTileFloats;
    const int ld = per_bin + 1;
    for (int idx = tid; idx < kFinBins * per_bin; idx += 256) {
        const int fb = idx / per_bin, e = idx - fb * per_bin;
        const int tile = e / kTileFloats;
        const int f = f0 + fb;
        float v = 0.f;
        if (f < kBins) {
            float acc = 0.f, den = 0.f;
            for (int p = 0; p < ud.nparts; ++p) {
                const float* P = a.partials + ((size_t)(ud.part0 + p) * kBins + f) * kWidePartFloats;
                acc += P[e];
                if (tile < 2) den += P[kDenOff + tile];
            }
            if (tile == 2) den = (float)ud.num_frames;
            const float sc = 1.f / fmaxf(den, 1e-6f);
            v = acc * sc;
        }
        sm[fb * ld + e] = v;
    }
    __syncthreads();
    if (C < kCp) {
        // the padding's diagonal, tiles 1.. (Rn, Ry)
        for (int idx = tid; idx < kFinBins * (ntile - 1); idx += 256) {
            const int fb = idx / (ntile - 1), tile = 1 + idx % (ntile - 1);
            if (f0 + fb < kBins) {
                float* m = sm + fb * ld + tile * kTileFloats;
                float dmax = m[0];
                for (int i = 1; i < C; ++i) dmax = fmaxf(dmax, m[pair_index(i, i, kCp)]);
                for (int i = C; i < kCp; ++i) m[pair_index(i, i, kCp)] = dmax;
            }
        }
        __syncthreads();
    }
    float* out = a.covar + (size_t)u * per_bin * kBinsPad;
    for (int idx = tid; idx < kFinBins * per_bin; idx += 256) {
        const int e = idx / kFinBins, fb = idx - e * kFinBins;
        const int f = f0 + fb;
        if (f < kBinsPad) out[(size_t)e * kBinsPad + f] = sm[fb * ld + e];  // (bins 257..263: zeros)
    }
}

// y[t][f] = sum_c conj(w[f][c]) X[f][c][t] (times the speech mask with SETK_FLAG_POST_MASK): the
// [T][F] spectrogram beamform_istft_kernel<1, true> inverts.  A workgroup owns 16 bins x 64
// frames: a wave reads rows of 64 frames (512 contiguous bytes) for its 4 bins, the tile turns
// round in LDS, and a quarter wave writes 16 bins (128 contiguous bytes) of one frame.
constexpr int kBfBins = 16, kBfFrames = 64;

__global__ __launch_bounds__(256) void beamform_binmajor_kernel(WideArgs a) {
    __shared__ float2 tile[kBfFrames][kBfBins + 1];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int u = blockIdx.z;
    const UttDesc ud = a.utts[u];
    const int C = a.num_channels;
    const int T = ud.num_frames, Tp = (T + 3) & ~3;
    const int t0 = blockIdx.x * kBfFrames, f0 = blockIdx.y * kBfBins;
    if (t0 >= T) return;
    const float2* xb = reinterpret_cast<const float2*>(ud.wave_out);
    const float2* wts = reinterpret_cast<const float2*>(a.weight) + (size_t)u * kCp * kBinsPad;
    const int t = t0 + lane;
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
        const int fb = 4 * wave + bi, f = f0 + fb;
        float2 y = make_float2(0.f, 0.f);
        if (f < kBins && t < T) {
            const float2* xr = xb + (size_t)f * C * Tp + t;
            for (int c = 0; c < C; ++c) {
                const float2 w = wts[c * kBinsPad + f];
                const float2 x = xr[(size_t)c * Tp];
                // y + x conj(w), the two FMA chains of pass 2
                y = make_float2(fmaf(x.x, w.x, fmaf(x.y, w.y, y.x)), fmaf(x.y, w.x, fmaf(-x.x, w.y, y.y)));
            }
        }
        tile[lane][fb] = y;
    }
    __syncthreads();
    const bool post_mask = (a.flags & 0x4) != 0, clamp = (a.flags & 0x2) != 0;
    float2* out = reinterpret_cast<float2*>(ud.wave_f32);
    const int fb = tid & 15, f = f0 + fb;
    for (int tl = tid >> 4; tl < kBfFrames; tl += 16) {
        const int tt = t0 + tl;
        if (tt < T && f < kBins) {
            float2 y = tile[tl][fb];
            if (post_mask) {
                float m = ud.mask_s[(size_t)tt * kBins + f];
                if (clamp) m = fminf(m, 1.f);
                y.x *= m;
                y.y *= m;
            }
            out[(size_t)tt * kBins + f] = y;
        }
    }
}

// the taps: planes of the 16 x 16 embedding -> covar[u][F][C][C], weight planes [u][16][pitch]
// -> w[u][F][C]
__global__ void wide_unpack_covar_kernel(const float* planes, int n_planes, int plane0, int C, float2* out) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int u = blockIdx.y;
    if (f >= kBins) return;
    const float* base = planes + ((size_t)u * n_planes + plane0) * kBinsPad + f;
    float2* o = out + ((size_t)u * kBins + f) * C * C;
    for (int i = 0; i < C; ++i)
        for (int j = i; j < C; ++j) {
            const int e = pair_index(i, j, kCp);
            const float re = base[(size_t)e * kBinsPad], im = base[(size_t)(kNP16 + e) * kBinsPad];
            o[i * C + j] = make_float2(re, i == j ? 0.f : im);
            if (i != j) o[j * C + i] = make_float2(re, -im);
        }
}

__global__ void wide_unpack_weight_kernel(const float2* wp, int C, float2* w) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int u = blockIdx.y;
    if (f >= kBins) return;
    for (int c = 0; c < C; ++c) w[((size_t)u * kBins + f) * C + c] = wp[((size_t)u * kCp + c) * kBinsPad + f];
}

}  // namespace

static_assert(kWidePartFloats >= kDenOff + 2, "a slab holds three tiles and the two mask sums");

hipError_t launch_covar_wide(const WideArgs& a, int n_items, hipStream_t s) {
    const dim3 grid(n_items, (kBins + 3) / 4);
    if (a.with_ry) hipLaunchKernelGGL(covar_wide_mfma_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(covar_wide_mfma_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wide_finalize(const WideArgs& a, int n_utts, hipStream_t s) {
    const int per_bin = (a.with_ry ? 3 : 2) * kTileFloats;
    const size_t lds = (size_t)kFinBins * (per_bin + 1) * sizeof(float);
    hipLaunchKernelGGL(wide_finalize_kernel, dim3((kBinsPad + kFinBins - 1) / kFinBins, n_utts), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_beamform_binmajor(const WideArgs& a, int n_utts, int max_frames, hipStream_t s) {
    const dim3 grid((max_frames + kBfFrames - 1) / kBfFrames, (kBins + kBfBins - 1) / kBfBins, n_utts);
    hipLaunchKernelGGL(beamform_binmajor_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wide_unpack_covar(const float* planes, int n_utts, int n_planes, int plane0, int C, float* out,
                                    hipStream_t s) {
    hipLaunchKernelGGL(wide_unpack_covar_kernel, dim3((kBins + 255) / 256, n_utts), dim3(256), 0, s, planes,
                       n_planes, plane0, C, reinterpret_cast<float2*>(out));
    return hipGetLastError();
}

hipError_t launch_wide_unpack_weight(const float* wplanes, int n_utts, int C, float* w, hipStream_t s) {
    hipLaunchKernelGGL(wide_unpack_weight_kernel, dim3((kBins + 255) / 256, n_utts), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(wplanes), C, reinterpret_cast<float2*>(w));
    return hipGetLastError();
}

}  // namespace setk
