// online.hip -- block-online MVDR / GEV beamforming: the recursive covariance smoothing over the
// chunks of an utterance, blind analytic normalisation with the chunk's own noise covariance,
// and the per-utterance status.
//
// Replaces (funcwj/setk): OnlineSupervisedBeamformer.run (libs/beamformer.py:286-320) under
// do_online_beamform (apply_adaptive_beamformer.py:25-47), for every chunk of every utterance of
// a batch at once:
//   pass 1 (pass1.hip, unchanged) runs on work items cut at the chunk boundaries, so a partial
//       slab holds the masked sums of frames of ONE chunk;
//   online_smooth_kernel sums a chunk's slabs, normalises (compute_covar, :87-103) and applies
//       R_c = alpha R_{c-1} + phi_c r_c, phi_0 = 1, phi_c = 1 - alpha, writing R_c of every chunk
//       in the packed plane layout of the weight solve: a chunk is a virtual utterance there;
//   solve.hip (unchanged) computes the weights of all chunks;
//   online_ban_kernel scales them by do_ban (:14-28) with the chunk's UNSMOOTHED r_n;
//   online_status_kernel folds the chunks' status words into the utterance's by maximum;
//   pass 2 (pass2.hip, ONLINE) picks the weight set per frame.
// Nothing here accumulates across threads: every sum has one owner and a fixed order.
#include "common.h"

namespace setk {

// One workgroup = one (plane, utterance) row of 264 bins, as covar_finalize_kernel; the thread of
// bin f walks the utterance's chunks in order.  Per chunk the slabs are summed in slab order and
// scaled by one factor (covar_finalize_kernel's two expressions), then smoothed.
__global__ __launch_bounds__(320) void online_smooth_kernel(OnlineArgs a) {
    const int f = threadIdx.x;
    if (f >= kBinsPad) return;
    const int u = blockIdx.x;  // (x: the one grid dimension without a 65535 limit)
    const int e = blockIdx.y;  // plane of [Rs.re NP | Rs.im NP | Rn.re NP | Rn.im NP]
    const int NP = npairs(a.num_channels);
    const int planes_in = 4 * NP + 2;
    const size_t slab = (size_t)planes_in * kBinsPad;
    const int sel = e / (2 * NP);  // 0 speech, 1 noise
    const int c0 = a.chunk0[u], nc = a.chunk0[u + 1] - c0;
    const float phi_rest = 1.f - a.alpha;
    float R = 0.f;
    for (int c = 0; c < nc; ++c) {
        const int k = c0 + c;
        float r = 0.f;
        if (f < kBins) {
            const int2 pr = a.chunk_parts[k];  // (first slab, slabs)
            const float* P = a.partials + (size_t)pr.x * slab + f;
            float acc = 0.f, den = 0.f;
            for (int p = 0; p < pr.y; ++p) {
                acc += P[p * slab + (size_t)e * kBinsPad];
                den += P[p * slab + (size_t)(4 * NP + sel) * kBinsPad];
            }
            const float sc = 1.f / fmaxf(den, 1e-6f);
            r = acc * sc;
            R = a.alpha * R + (c == 0 ? 1.f : phi_rest) * r;
        }
        a.covar[((size_t)k * 4 * NP + e) * kBinsPad + f] = R;  // (the pad bins stay 0)
        if (a.rn_chunk && sel == 1) a.rn_chunk[((size_t)k * 2 * NP + (e - 2 * NP)) * kBinsPad + f] = r;
    }
}

hipError_t launch_online_smooth(const OnlineArgs& a, int n_utts, hipStream_t s) {
    hipLaunchKernelGGL(online_smooth_kernel, dim3(n_utts, 4 * npairs(a.num_channels)), dim3(320), 0, s, a);
    return hipGetLastError();
}

// do_ban per (chunk, bin), float64: w <- w sqrt(|Rn w|^2) / max(Re w^H Rn w, eps), Rn the chunk's
// own unsmoothed noise covariance from the packed planes [re NP | im NP] (pair (i, j), i <= j)
template <int C>
__global__ __launch_bounds__(256) void online_ban_kernel(float2* __restrict__ w, const float* __restrict__ rn,
                                                         int n_chunks) {
    constexpr int NP = npairs(C);
    const int f = blockIdx.y * 256 + threadIdx.x;
    const int k = blockIdx.x;  // (x: a batch may hold more than 65535 chunks)
    if (f >= kBins || k >= n_chunks) return;
    float2* wk = w + (size_t)k * C * kBinsPad + f;
    const float* re = rn + (size_t)k * 2 * NP * kBinsPad + f;
    const float* im = re + (size_t)NP * kBinsPad;
    double wx[C], wy[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float2 v = wk[(size_t)c * kBinsPad];
        wx[c] = v.x;
        wy[c] = v.y;
    }
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        double ux = 0.0, uy = 0.0;  // (Rn w)_i
#pragma unroll
        for (int m = 0; m < C; ++m) {
            const int lo = i < m ? i : m, hi = i < m ? m : i;
            const int e = pair_index(lo, hi, C);
            const double rr = re[(size_t)e * kBinsPad];
            // Rn[i][m]: stored for i <= m, its conjugate below the diagonal, real on it
            const double ri = (i == m) ? 0.0 : (i < m ? 1.0 : -1.0) * (double)im[(size_t)e * kBinsPad];
            ux += rr * wx[m] - ri * wy[m];
            uy += rr * wy[m] + ri * wx[m];
        }
        nom += ux * ux + uy * uy;
        den += wx[i] * ux + wy[i] * uy;
    }
    const double filt = sqrt(nom) / fmax(den, 1.1920928955078125e-07);
#pragma unroll
    for (int c = 0; c < C; ++c)
        wk[(size_t)c * kBinsPad] = make_float2((float)(wx[c] * filt), (float)(wy[c] * filt));
}

hipError_t launch_online_ban(int C, float* weight, const float* rn_chunk, int n_chunks, hipStream_t s) {
    const dim3 grid(n_chunks, (kBins + 255) / 256);
#define SETK_CASE(c)                                                                                   \
    case c:                                                                                            \
        hipLaunchKernelGGL(online_ban_kernel<c>, grid, dim3(256), 0, s, reinterpret_cast<float2*>(weight), \
                           rn_chunk, n_chunks);                                                        \
        break;
    switch (C) {
        SETK_CASE(1)
        SETK_CASE(2)
        SETK_CASE(3)
        SETK_CASE(4)
        SETK_CASE(5)
        SETK_CASE(6)
        SETK_CASE(7)
        SETK_CASE(8)
        default:
            return hipErrorInvalidValue;
    }
#undef SETK_CASE
    return hipGetLastError();
}

// status[u] = max over the utterance's chunks (the SETK_NUM_* values are ordered by severity as
// the solve's own atomicMax takes them)
__global__ __launch_bounds__(256) void online_status_kernel(const int* __restrict__ chunk_status,
                                                            const int* __restrict__ chunk0, int n_utts,
                                                            int* __restrict__ status) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n_utts) return;
    int st = 0;
    for (int k = chunk0[u]; k < chunk0[u + 1]; ++k) st = max(st, chunk_status[k]);
    status[u] = st;
}

hipError_t launch_online_status(const int* chunk_status, const int* chunk0, int n_utts, int* status,
                                hipStream_t s) {
    hipLaunchKernelGGL(online_status_kernel, dim3((n_utts + 255) / 256), dim3(256), 0, s, chunk_status, chunk0,
                       n_utts, status);
    return hipGetLastError();
}

}  // namespace setk
