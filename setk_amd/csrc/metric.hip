// metric.hip -- SI-SNR of every (estimate, reference) pair of an utterance and the best assignment
// of estimates to references (scripts/sptk/libs/metric.py:13-60), for ragged batches.
//
//   x' = x - mean(x), s' = s - mean(s);  a = <x', s'> / (|s'|^2 + eps);  n = x' - a s'
//   si_snr = 20 log10(|a| |s'| / (|n| + eps) + eps)
//
// Everything is float64 on the float32 (or 16-bit, v / 32768) samples as given.  Three phases, each
// ONE launch over all (utterance, tile) pairs of the batch, a tile being kMetricTile samples of
// every signal of the utterance:
//   means     sums of the 2 K signals                                  (skipped when DC is kept)
//   Gram      e_j = |s'_j|^2 and d_ij = <x'_i, s'_j> for all K^2 pairs
//   residual  |n_ij|^2 = sum_k (x'_ik - a_ij s'_jk)^2, formed per sample as the reference forms it
// A tile's workgroup loads each sample of each signal once and uses it for every pair; a thread
// keeps one accumulator per sum, the workgroup folds them (rows of 16 lanes through dpp.h, the 16
// row sums through LDS in a fixed order) and stores the tile's sums into its own row of the
// partial slab.  Behind each phase one workgroup per utterance adds the rows in tile order: one
// owner per sum, no floating-point atomics, the same bits for an utterance whatever batch it is in.
//
// Why the vector unit and not the float64 matrix instruction: per sample index a workgroup reads
// 2 K x 4 bytes and issues K^2 + K multiply-adds, 1.1 per byte at K = 8 and 0.4 at K = 2.  At the
// HBM rate that is 7 T multiply-adds a second against the 39 T of the vector unit, and measured
//  the Gram phase takes 1.1 to 1.2 times its bytes at the HBM rate at K = 2
// and at K = 8: it is bound by its loads.  The residual is no matrix product at all.
//
// Every multiply-add below is written as fma(): the instantiations (padded source count 2, 4, 8;
// the two sample forms) then perform the same operations, and an utterance has the same bits
// whichever of them its batch selects.
#include "common.h"
#include "dpp.h"

namespace setk {

namespace {

constexpr int kIters = kMetricTile / kMetricThreads;
constexpr int kP = kMetricMaxSrc;  // pitch of the per-utterance tables

// (the signals are device memory, which the front end has checked: global loads, not flat ones)
template <typename T>
using global_ptr = const T __attribute__((address_space(1)))*;

template <bool PCM>
SD double load_sample(const void* p, int stride, int k, bool& bad) {
    const size_t at = (size_t)k * (size_t)stride;
    if constexpr (PCM) {
        return (double)((global_ptr<int16_t>)p)[at] * (1.0 / 32768.0);
    } else {
        const float v = ((global_ptr<float>)p)[at];
        bad |= !isfinite(v);
        return (double)v;
    }
}

// The workgroup's sum of each of NQ per-thread accumulators into row[0 .. NQ): 16-lane rows by
// DPP, then the 16 row sums of the four waves in slot order by one owner each.
template <int NQ>
__device__ void block_fold(const double (&acc)[NQ], double* lds, double* row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double v = acc[q];
        v += dshfl_xor<1>(v);
        v += dshfl_xor<2>(v);
        v += dshfl_xor<4>(v);
        v += dshfl_xor<8>(v);
        if ((lane & 15) == 0) lds[q * 16 + wave * 4 + (lane >> 4)] = v;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < NQ; q += kMetricThreads) {
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += lds[q * 16 + r];
        row[q] = sum;
    }
}

// the signals of an utterance in the launch's compact order: estimates [0, KP), references [KP, 2 KP)
template <int KP>
SD int slot_of(int c) { return c < KP ? c : kP + c - KP; }

// The addresses of N signals of an utterance, fetched once in front of the sample loop.  A slot
// beyond the utterance's K sources aliases signal 0 (a valid address, the same length) and its
// sample is discarded: the loads of a step are then issued together, with no branch per source
// between them.
template <int N>
struct Signals {
    const void* p[N];
    int stride[N];
    bool on[N];
    SD void set(int c, const MetricUtt& u, int slot, bool live) {
        on[c] = live;
        p[c] = u.sig[live ? slot : 0];
        stride[c] = u.stride[live ? slot : 0];
    }
    // sample k of signal c less `mean`; 0 for a slot that is not live
    template <bool PCM>
    SD double get(int c, int k, double mean, bool& bad) const {
        const double v = load_sample<PCM>(p[c], stride[c], k, bad);
        return on[c] ? v - mean : 0.0;
    }
};

// ---- phase 1: sums of the signals ----
template <int KP, bool PCM>
__global__ __launch_bounds__(kMetricThreads) void metric_means_kernel(const MetricUtt* __restrict__ utts,
                                                                      const MetricItem* __restrict__ items,
                                                                      double* __restrict__ partial) {
    __shared__ double lds[2 * KP * 16];
    const MetricItem it = items[blockIdx.x];
    const MetricUtt& u = utts[it.utt];
    const int K = u.K, L = u.L, k0 = it.tile * kMetricTile + threadIdx.x;
    double acc[2 * KP];
    Signals<2 * KP> sig;
#pragma unroll
    for (int c = 0; c < 2 * KP; ++c) {
        acc[c] = 0.0;
        sig.set(c, u, slot_of<KP>(c), (c < KP ? c : c - KP) < K);
    }
    bool bad = false;
#pragma unroll 2
    for (int r = 0; r < kIters; ++r) {
        const int k = k0 + r * kMetricThreads;
        if (k < L) {
#pragma unroll
            for (int c = 0; c < 2 * KP; ++c) acc[c] += sig.template get<PCM>(c, k, 0.0, bad);
        }
    }
    block_fold<2 * KP>(acc, lds, partial + (size_t)(u.tile0 + it.tile) * metric_row(KP));
}

template <int KP>
__global__ __launch_bounds__(64) void metric_means_fold_kernel(const MetricUtt* __restrict__ utts,
                                                               const double* __restrict__ partial) {
    const MetricUtt& u = utts[blockIdx.x];
    const int q = threadIdx.x;
    if (q >= 2 * KP) return;
    const double* row = partial + (size_t)u.tile0 * metric_row(KP) + q;
    double sum = 0.0;
#pragma unroll 8
    for (int t = 0; t < u.ntiles; ++t) sum += row[(size_t)t * metric_row(KP)];
    u.mean[slot_of<KP>(q)] = sum / (double)u.L;
}

// the centred samples of index k: x[i] of the estimates, s[j] of the references (0 beyond K)
template <int KP, bool PCM>
SD void centred(const Signals<2 * KP>& sig, int k, const double (&mx)[KP], const double (&ms)[KP], double (&x)[KP],
                double (&s)[KP], bool& bad) {
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        x[i] = sig.template get<PCM>(i, k, mx[i], bad);
        s[i] = sig.template get<PCM>(KP + i, k, ms[i], bad);
    }
}

// ---- phase 2: the centred Gram block ----
template <int KP, bool PCM>
__global__ __launch_bounds__(kMetricThreads) void metric_gram_kernel(const MetricUtt* __restrict__ utts,
                                                                     const MetricItem* __restrict__ items,
                                                                     double* __restrict__ partial,
                                                                     int* __restrict__ flags) {
    constexpr int NQ = metric_row(KP);
    __shared__ double lds[NQ * 16];
    __shared__ int sm_bad;
    const MetricItem it = items[blockIdx.x];
    const MetricUtt& u = utts[it.utt];
    const int K = u.K, L = u.L, k0 = it.tile * kMetricTile + threadIdx.x;
    if (threadIdx.x == 0) sm_bad = 0;
    double mx[KP], ms[KP], acc[NQ];  // acc: e_j at [j], d_ij at [KP + i KP + j]
    Signals<2 * KP> sig;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        mx[i] = u.mean[i];
        ms[i] = u.mean[kP + i];
        sig.set(i, u, i, i < K);
        sig.set(KP + i, u, kP + i, i < K);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    bool bad = false;
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < kIters; ++r) {
        const int k = k0 + r * kMetricThreads;
        if (k < L) {
            double x[KP], s[KP];
            centred<KP, PCM>(sig, k, mx, ms, x, s, bad);
#pragma unroll
            for (int j = 0; j < KP; ++j) acc[j] = fma(s[j], s[j], acc[j]);
#pragma unroll
            for (int i = 0; i < KP; ++i)
#pragma unroll
                for (int j = 0; j < KP; ++j) acc[KP + i * KP + j] = fma(x[i], s[j], acc[KP + i * KP + j]);
        }
    }
    if (bad) sm_bad = 1;  // (every writer stores the same value)
    block_fold<NQ>(acc, lds, partial + (size_t)(u.tile0 + it.tile) * NQ);
    if (threadIdx.x == 0) flags[u.tile0 + it.tile] = sm_bad;  // (behind block_fold's barrier)
}

template <int KP>
__global__ __launch_bounds__(128) void metric_gram_fold_kernel(const MetricUtt* __restrict__ utts,
                                                               const double* __restrict__ partial,
                                                               const int* __restrict__ flags, double eps) {
    constexpr int NQ = metric_row(KP);
    __shared__ double sums[NQ];
    __shared__ int sm_bad;
    const MetricUtt& u = utts[blockIdx.x];
    const int q = threadIdx.x;
    if (q == 0) sm_bad = 0;
    __syncthreads();
    if (q < NQ) {
        const double* row = partial + (size_t)u.tile0 * NQ + q;
        double sum = 0.0;
#pragma unroll 8
        for (int t = 0; t < u.ntiles; ++t) sum += row[(size_t)t * NQ];
        sums[q] = sum;
    }
    int bad = 0;
    for (int t = q; t < u.ntiles; t += 128) bad = max(bad, flags[u.tile0 + t]);
    if (bad) sm_bad = 1;
    __syncthreads();
    if (q < KP) u.gram[q] = sums[q];
    if (q < KP * KP) {
        const int i = q / KP, j = q % KP;
        const double d = sums[KP + q];
        u.gram[kP + i * kP + j] = d;
        u.gram[kP + kP * kP + i * kP + j] = d / (sums[j] + eps);
    }
    if (q == 0) *u.status = sm_bad ? 3 /* SETK_NUM_NONFINITE */ : 0;
}

// ---- phase 3: the residual of every pair, per sample ----
// A thread keeps a_ij and the running sum of every pair it owns in registers: at eight sources all
// 64 pairs are 256 registers and one wave per SIMD.  There the estimates' rows are dealt over two
// neighbouring workgroups, four rows each (182 registers, two waves); both read the tile's
// references, the second one out of the cache.  A pair's operations are the same either way.
__host__ __device__ constexpr int residual_rows(int kp) { return kp == 8 ? 4 : kp; }

template <int KP, bool PCM>
__global__ __launch_bounds__(kMetricThreads) void metric_residual_kernel(const MetricUtt* __restrict__ utts,
                                                                         const MetricItem* __restrict__ items,
                                                                         double* __restrict__ partial) {
    constexpr int RB = residual_rows(KP), PARTS = KP / RB, NQ = RB * KP;
    __shared__ double lds[NQ * 16];
    const MetricItem it = items[blockIdx.x / PARTS];
    const int row0 = (blockIdx.x % PARTS) * RB;
    const MetricUtt& u = utts[it.utt];
    const int K = u.K, L = u.L, k0 = it.tile * kMetricTile + threadIdx.x;
    double mx[RB], ms[KP], a[NQ], acc[NQ];
    Signals<RB + KP> sig;  // this block's estimates, then the references
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        ms[j] = u.mean[kP + j];
        sig.set(RB + j, u, kP + j, j < K);
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        mx[i] = u.mean[row0 + i];
        sig.set(i, u, row0 + i, row0 + i < K);
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            a[i * KP + j] = u.gram[kP + kP * kP + (row0 + i) * kP + j];
            acc[i * KP + j] = 0.0;
        }
    }
    bool bad = false;
    if (row0 < K) {  // (rows beyond the utterance's sources: zeros, as the padded pairs elsewhere)
#pragma unroll 2
        for (int r = 0; r < kIters; ++r) {
            const int k = k0 + r * kMetricThreads;
            if (k < L) {
                double x[RB], s[KP];
#pragma unroll
                for (int j = 0; j < KP; ++j) s[j] = sig.template get<PCM>(RB + j, k, ms[j], bad);
#pragma unroll
                for (int i = 0; i < RB; ++i) x[i] = sig.template get<PCM>(i, k, mx[i], bad);
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = 0; j < KP; ++j) {
                        const double n = fma(-a[i * KP + j], s[j], x[i]);
                        acc[i * KP + j] = fma(n, n, acc[i * KP + j]);
                    }
            }
        }
    }
    block_fold<NQ>(acc, lds, partial + (size_t)(u.tile0 + it.tile) * metric_row(KP) + row0 * KP);
}

// order number `idx` of itertools.permutations(range(K)) (lexicographic: the factorial number
// system), as nibbles: order[n] = (result >> 4 n) & 15
SD unsigned long long unrank(int idx, int K) {
    unsigned long long rem = 0x76543210ull, out = 0;
    int fact = 1;
    for (int n = 2; n < K; ++n) fact *= n;  // (K - 1)!
    for (int n = 0; n < K; ++n) {
        const int q = idx / fact;
        idx -= q * fact;
        const int sh = 4 * q;
        out |= ((rem >> sh) & 15ull) << (4 * n);
        rem = (rem & ((1ull << sh) - 1ull)) | ((rem >> (sh + 4)) << sh);
        if (n + 1 < K) fact /= (K - 1 - n);
    }
    return out;
}

SD void take_better(double& bv, int& bi, double ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
    }
}

// ---- the residual's fold, the SI-SNR table, the search over the K! orders ----
template <int KP>
__global__ __launch_bounds__(kMetricThreads) void metric_search_kernel(const MetricUtt* __restrict__ utts,
                                                                       const double* __restrict__ partial,
                                                                       double eps) {
    __shared__ double tab[kP * kP];
    __shared__ double red_v[16];
    __shared__ int red_i[16];
    const MetricUtt& u = utts[blockIdx.x];
    const int K = u.K, tid = threadIdx.x;
    if (tid < KP * KP) {
        const int i = tid / KP, j = tid % KP;
        const double* row = partial + (size_t)u.tile0 * metric_row(KP) + tid;
        double nn = 0.0;
#pragma unroll 8
        for (int t = 0; t < u.ntiles; ++t) nn += row[(size_t)t * metric_row(KP)];
        if (i < K && j < K) {
            // |t| = |a| |s'|: a s' is one rounding per sample away from it, 1e-16 of |t|
            const double tn = fabs(u.gram[kP + kP * kP + i * kP + j]) * sqrt(u.gram[j]);
            const double v = 20.0 * log10(tn / (sqrt(nn) + eps) + eps);
            tab[i * kP + j] = v;
            u.pair[i * K + j] = v;
        }
    }
    if (!u.best && !u.perm) return;
    __syncthreads();
    int nperm = 1;
    for (int n = 2; n <= K; ++n) nperm *= n;
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int idx = tid; idx < nperm; idx += kMetricThreads) {
        const unsigned long long order = unrank(idx, K);
        double sum = 0.0;  // sum([...]) / len(xlist): left to right from 0, then the division
        for (int n = 0; n < K; ++n) sum += tab[n * kP + (int)((order >> (4 * n)) & 15ull)];
        take_better(bv, bi, sum / (double)K, idx);
    }
    take_better(bv, bi, dshfl_xor<1>(bv), dpp_xor<1>(bi));
    take_better(bv, bi, dshfl_xor<2>(bv), dpp_xor<2>(bi));
    take_better(bv, bi, dshfl_xor<4>(bv), dpp_xor<4>(bi));
    take_better(bv, bi, dshfl_xor<8>(bv), dpp_xor<8>(bi));
    if ((tid & 15) == 0) {
        red_v[tid >> 4] = bv;
        red_i[tid >> 4] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int r = 1; r < 16; ++r) take_better(bv, bi, red_v[r], red_i[r]);
        if (bi == 0x7fffffff) {  // every average NaN (the status word says so): the identity
            bi = 0;
            bv = NAN;
        }
        if (u.best) *u.best = bv;
        if (u.perm) {
            const unsigned long long order = unrank(bi, K);
            for (int n = 0; n < K; ++n) u.perm[n] = (int)((order >> (4 * n)) & 15ull);
        }
    }
}

}  // namespace

int metric_padded_sources(int max_k) { return max_k <= 2 ? 2 : max_k <= 4 ? 4 : 8; }

#define METRIC_DISPATCH(KERNEL, grid, block, ...)                                                    \
    do {                                                                                             \
        if (kp == 2)                                                                                 \
            hipLaunchKernelGGL(KERNEL(2), dim3(grid), dim3(block), 0, s, __VA_ARGS__);               \
        else if (kp == 4)                                                                            \
            hipLaunchKernelGGL(KERNEL(4), dim3(grid), dim3(block), 0, s, __VA_ARGS__);               \
        else                                                                                         \
            hipLaunchKernelGGL(KERNEL(8), dim3(grid), dim3(block), 0, s, __VA_ARGS__);               \
    } while (0)

hipError_t launch_metric_means(const MetricUtt* d_utts, const MetricItem* d_items, int n_items, int n_utts, int kp,
                               bool pcm16, double* d_partial, hipStream_t s) {
#define K_MEANS_PCM(KP) (metric_means_kernel<KP, true>)
#define K_MEANS_F32(KP) (metric_means_kernel<KP, false>)
#define K_MEANS_FOLD(KP) (metric_means_fold_kernel<KP>)
    if (pcm16)
        METRIC_DISPATCH(K_MEANS_PCM, n_items, kMetricThreads, d_utts, d_items, d_partial);
    else
        METRIC_DISPATCH(K_MEANS_F32, n_items, kMetricThreads, d_utts, d_items, d_partial);
    METRIC_DISPATCH(K_MEANS_FOLD, n_utts, 64, d_utts, (const double*)d_partial);
    return hipGetLastError();
}

hipError_t launch_metric_gram(const MetricUtt* d_utts, const MetricItem* d_items, int n_items, int n_utts, int kp,
                              bool pcm16, double eps, double* d_partial, int* d_flags, hipStream_t s) {
#define K_GRAM_PCM(KP) (metric_gram_kernel<KP, true>)
#define K_GRAM_F32(KP) (metric_gram_kernel<KP, false>)
#define K_GRAM_FOLD(KP) (metric_gram_fold_kernel<KP>)
    if (pcm16)
        METRIC_DISPATCH(K_GRAM_PCM, n_items, kMetricThreads, d_utts, d_items, d_partial, d_flags);
    else
        METRIC_DISPATCH(K_GRAM_F32, n_items, kMetricThreads, d_utts, d_items, d_partial, d_flags);
    METRIC_DISPATCH(K_GRAM_FOLD, n_utts, 128, d_utts, (const double*)d_partial, (const int*)d_flags, eps);
    return hipGetLastError();
}

hipError_t launch_metric_residual(const MetricUtt* d_utts, const MetricItem* d_items, int n_items, int kp,
                                  bool pcm16, double* d_partial, hipStream_t s) {
#define K_RES_PCM(KP) (metric_residual_kernel<KP, true>)
#define K_RES_F32(KP) (metric_residual_kernel<KP, false>)
    if (pcm16)
        METRIC_DISPATCH(K_RES_PCM, n_items * (kp / residual_rows(kp)), kMetricThreads, d_utts, d_items, d_partial);
    else
        METRIC_DISPATCH(K_RES_F32, n_items * (kp / residual_rows(kp)), kMetricThreads, d_utts, d_items, d_partial);
    return hipGetLastError();
}

hipError_t launch_metric_search(const MetricUtt* d_utts, int n_utts, int kp, double eps, const double* d_partial,
                                hipStream_t s) {
#define K_SEARCH(KP) (metric_search_kernel<KP>)
    METRIC_DISPATCH(K_SEARCH, n_utts, kMetricThreads, d_utts, d_partial, eps);
    return hipGetLastError();
}

}  // namespace setk
