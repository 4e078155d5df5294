// ns.hip -- single-channel OM-LSA noise suppression with MCRA / iMCRA noise tracking
// (scripts/sptk/libs/ns.py).
//
// The recursion is sequential over the frames and, across the bins, needs only short
// convolutions (np.convolve(..., mode="same") with 2 w + 1 taps) and, for MCRA, one mean per
// frame.  So an utterance is ONE workgroup: a lane owns a bin (two bins when F > 1024), the state
// of the bin lives in its registers for the whole utterance, and what the neighbours need goes
// through rows in LDS that carry kNsMaxHalf zeros on either side -- numpy's zero extension at
// both ends of the band.  A batch is one launch, grid = utterances.
//
// Everything is float64 as in the reference, the exponential integral E1 included (the reference
// integrates exp(-t) / t numerically per cell): the decisions compare smoothed ratios against
// thresholds, and the gain is exp(0.5 E1(v)).
//
// Barriers.  MCRA exchanges the power row and zeta in the same round, into rows that alternate
// with the frame's parity: one barrier per frame (a lane writes frame t + 2 into the rows of
// frame t only behind the barrier of frame t + 1, which every lane reaches after its reads of
// frame t).  iMCRA needs the indicator, which depends on the first round's convolution: two
// rounds, two barriers, single rows (round one of frame t + 1 is written behind barrier two of
// frame t, which every lane reaches after its round-one reads; likewise for round two).
//
// The spectrogram cell of frame t + 1 is loaded before frame t is computed.
#include "common.h"

namespace setk {

namespace {

constexpr int kRow = kNsMaxBins + 2 * kNsMaxHalf + 1;  // 1088 doubles
constexpr int kTaps = 2 * kNsMaxHalf + 1;

// E1(x) = int_x^inf exp(-t) / t dt for x > 0.
//   x <= 1: -gamma - ln x - sum_{k >= 1} (-x)^k / (k k!)   (22 terms: the last is below 1e-23)
//   x >  1: exp(-x) / (x + 1 - 1 / (x + 3 - 4 / (x + 5 - 9 / ...))), the convergent of
//           6 + ceil(96 / x) levels (measured against 40-digit arithmetic: 95 levels reach
//           3e-16 at x = 1, 50 at 2, 28 at 4, 9 at 20, 3 at 700).  It is evaluated by the forward
//           recurrence of its numerator and denominator, A_j = b_j A_{j-1} - j^2 A_{j-2} with
//           b_j = x + 2 j + 1: two independent multiply-add chains and ONE division, where the
//           evaluation from the tail costs a dependent division per level (a lane near x = 1 then
//           holds its wave for 100 of them).  The two terms of a step do not cancel (their ratio
//           tends to 2), rounding accumulates to 1.2e-14 at worst (x just above 1), and A stays
//           below 1e172.
// Beyond x = 746 exp(-x) has underflowed: 0 (x = +inf too).  x <= 0 is the caller's to avoid (the
// recursions floor their argument).
__device__ double expint_e1(double x) {
    if (x <= 1.0) {
        double term = 1.0, sum = 0.0;
#pragma unroll
        for (int k = 1; k <= 22; ++k) {
            term *= -x * (1.0 / k);
            sum -= term * (1.0 / k);
        }
        return (-0.57721566490153286061 - log(x)) + sum;
    }
    if (!(x <= 746.0)) return x != x ? x : 0.0;
    const int n = 6 + (int)ceil(96.0 / x);
    double a_prev = 1.0, a_cur = x + 1.0, b_prev = 0.0, b_cur = 1.0;
    for (int j = 1; j <= n; ++j) {
        const double b = x + (double)(2 * j + 1), a = -(double)(j * j);
        const double a_next = fma(b, a_cur, a * a_prev), b_next = fma(b, b_cur, a * b_prev);
        a_prev = a_cur;
        a_cur = a_next;
        b_prev = b_cur;
        b_cur = b_next;
    }
    return exp(-x) * b_cur / a_cur;
}

// g^p gmin^(1 - p) (ns.py:206, :383) for g > 0 through one logarithm and one exponential
__device__ __forceinline__ double om_lsa_gain(double g, double pr, double gmin, double log_gmin) {
    if (g > 0.0 && g < 1e300) return exp(pr * log(g) + (1.0 - pr) * log_gmin);
    return pow(g, pr) * pow(gmin, 1.0 - pr);
}

// np.convolve(row, w, mode="same")[f] for a row with zeros on both sides: sum_j row[f + half - j] w[j]
__device__ __forceinline__ double conv_same(const double* row, int f, const double* w, int half) {
    double acc = 0.0;
    for (int j = 0; j <= 2 * half; ++j) acc += row[f + half - j] * w[j];
    return acc;
}

struct NsShared {
    double rows[4][kRow];
    double taps[3][kTaps];
    int bad;
};

// zero the rows (the halos stay zero: only bins are written later), fetch the taps
__device__ void ns_prologue(NsShared& sm, const NsParams& p) {
    for (int i = threadIdx.x; i < 4 * kRow; i += blockDim.x) (&sm.rows[0][0])[i] = 0.0;
    for (int i = threadIdx.x; i < 3 * kTaps; i += blockDim.x) (&sm.taps[0][0])[i] = (&p.taps[0][0])[i];
    if (threadIdx.x == 0) sm.bad = 0;
    __syncthreads();
}

__device__ void ns_epilogue(NsShared& sm, const NsUtt& u, bool bad) {
    if (bad) sm.bad = 1;  // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0) *u.status = sm.bad ? 3 /* SETK_NUM_NONFINITE */ : 0;
}

__device__ __forceinline__ void ns_emit(const NsUtt& u, size_t cell, double gain, float2 x) {
    if (u.gain) u.gain[cell] = gain;
    if (u.out) reinterpret_cast<float2*>(u.out)[cell] = make_float2((float)(gain * (double)x.x), (float)(gain * (double)x.y));
}

__device__ __forceinline__ bool cell_bad(float2 x) { return !isfinite(x.x) || !isfinite(x.y); }

// eq.25 of Cohen & Berdugo 2001 as ns.py:150-169 writes it
__device__ __forceinline__ double prob_of(double z, double zmin, double zmax, double log_ratio) {
    if (z >= zmax) return 1.0;
    if (z > zmin) return log10(z / zmin) / log_ratio;
    return 0.0;
}

// ---- MCRA.run (ns.py:56-209) ----
template <int BPT>
__global__ __launch_bounds__(BPT == 1 ? 1024 : 576) void ns_mcra_kernel(const NsUtt* __restrict__ utts,
                                                                        const NsParams* __restrict__ params) {
    __shared__ NsShared sm;
    const NsParams& p = *params;
    const NsUtt u = utts[blockIdx.x];
    const int F = p.F, T = u.T;
    ns_prologue(sm, p);
    const float2* X = reinterpret_cast<const float2*>(u.spec);
    const double *wm = sm.taps[0], *wl = sm.taps[1], *wg = sm.taps[2];
    const double log_ratio = log10(p.zeta_max / p.zeta_min), log_gmin = log(p.gmin);

    int f[BPT];
    bool on[BPT];
    double lam[BPT], gh1[BPT], p_hat[BPT], zeta[BPT], var_s[BPT], s_min[BPT], s_tmp[BPT];
    float2 xn[BPT];
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
        f[k] = threadIdx.x + k * blockDim.x;
        on[k] = f[k] < F;
        gh1[k] = p_hat[k] = zeta[k] = 1.0;
        lam[k] = var_s[k] = s_min[k] = s_tmp[k] = 0.0;
        xn[k] = on[k] ? X[f[k]] : make_float2(0.f, 0.f);
    }
    double zeta_peak = 0.0, zf_pre = 0.0;
    bool bad = false;

    for (int t = 0; t < T; ++t) {
        double* rowP = sm.rows[(t & 1) * 2] + kNsMaxHalf;
        double* rowZ = sm.rows[(t & 1) * 2 + 1] + kNsMaxHalf;
        float2 x[BPT];
        double P[BPT], xi[BPT], v[BPT];
#pragma unroll
        for (int k = 0; k < BPT; ++k) {
            x[k] = xn[k];
            if (on[k] && t + 1 < T) xn[k] = X[(size_t)(t + 1) * F + f[k]];
            if (!on[k]) continue;
            bad |= cell_bad(x[k]);
            P[k] = (double)x[k].x * (double)x[k].x + (double)x[k].y * (double)x[k].y;
            if (t == 0) lam[k] = P[k];
            // eq.10, eq.18, eq.15
            const double gamma = fmax(P[k] / fmax(lam[k], p.eps), p.eps);
            xi[k] = fmax(p.alpha * gh1[k] * gh1[k] * gamma + (1.0 - p.alpha) * fmax(gamma - 1.0, 0.0), p.xi_min);
            v[k] = gamma * xi[k] / (1.0 + xi[k]);
            gh1[k] = xi[k] * exp(0.5 * expint_e1(v[k])) / (1.0 + xi[k]);
            // eq.23
            zeta[k] = p.beta * zeta[k] + (1.0 - p.beta) * xi[k];
            rowP[f[k]] = P[k];
            rowZ[f[k]] = zeta[k];
        }
        __syncthreads();
        // eq.26, eq.27: the same sum in the same order in every lane
        double zf = 0.0;
        for (int i = 0; i < p.mean_bins; ++i) zf += rowZ[i];
        zf /= (double)p.mean_bins;
        if (t == 0) zf_pre = zf;
        double p_frame = 0.0;
        if (zf > p.zeta_min) {
            if (zf > zf_pre) {
                zeta_peak = fmin(fmax(zf, p.zeta_p_min), p.zeta_p_max);
                p_frame = 1.0;
            } else if (zf <= p.zeta_min * zeta_peak)
                p_frame = 0.0;
            else if (zf >= p.zeta_max * zeta_peak)
                p_frame = 1.0;
            else
                p_frame = log10(zf / (p.zeta_min * zeta_peak)) / log_ratio;
        }
        zf_pre = zf;
#pragma unroll
        for (int k = 0; k < BPT; ++k) {
            if (!on[k]) continue;
            // eq.32 - eq.37
            const double var_sf = conv_same(rowP, f[k], wm, p.half_m);
            if (t == 0)
                var_s[k] = s_min[k] = s_tmp[k] = P[k];
            else
                var_s[k] = p.alpha_s * var_s[k] + (1.0 - p.alpha_s) * var_sf;
            if ((t + 1) % p.L == 10) {
                s_min[k] = fmin(s_tmp[k], var_s[k]);
                s_tmp[k] = var_s[k];
            } else {
                s_min[k] = fmin(s_min[k], var_s[k]);
                s_tmp[k] = fmin(s_tmp[k], var_s[k]);
            }
            // eq.39, eq.40, eq.31, eq.30
            const double var_sr = var_s[k] / fmax(p.eps, s_min[k]);
            p_hat[k] = p.alpha_p * p_hat[k] + (1.0 - p.alpha_p) * (var_sr > p.delta ? 1.0 : 0.0);
            const double a_d = p.alpha_d + (1.0 - p.alpha_d) * p_hat[k];
            lam[k] = a_d * lam[k] + (1.0 - a_d) * P[k];
            // eq.24, eq.25, eq.28
            const double pg = prob_of(conv_same(rowZ, f[k], wg, p.half_g), p.zeta_min, p.zeta_max, log_ratio);
            const double pl = prob_of(conv_same(rowZ, f[k], wl, p.half_l), p.zeta_min, p.zeta_max, log_ratio);
            const double q = fmin(p.q_max, 1.0 - pl * p_frame * pg);
            // eq.9, eq.16
            const double pr = 1.0 / (1.0 + q * (1.0 + xi[k]) * exp(-v[k]) / (1.0 - q));
            const double gain = om_lsa_gain(gh1[k], pr, p.gmin, log_gmin);
            bad |= !isfinite(gain);
            ns_emit(u, (size_t)t * F + f[k], gain, x[k]);
        }
    }
    ns_epilogue(sm, u, bad);
}

// ---- iMCRA.run (ns.py:247-387) ----
template <int BPT>
__global__ __launch_bounds__(BPT == 1 ? 1024 : 576) void ns_imcra_kernel(const NsUtt* __restrict__ utts,
                                                                         const NsParams* __restrict__ params) {
    __shared__ NsShared sm;
    const NsParams& p = *params;
    const NsUtt u = utts[blockIdx.x];
    const int F = p.F, T = u.T, U = p.U;
    ns_prologue(sm, p);
    const float2* X = reinterpret_cast<const float2*>(u.spec);
    const double* wm = sm.taps[0];
    double* rowP = sm.rows[0] + kNsMaxHalf;
    double* rowI = sm.rows[1] + kNsMaxHalf;
    double* rowIP = sm.rows[2] + kNsMaxHalf;
    const double log_gmin = log(p.gmin);

    int f[BPT];
    bool on[BPT];
    double lam[BPT], gh1[BPT], var_s[BPT], var_s_hat[BPT], s_min[BPT], s_min_sw[BPT], s_min_hat[BPT],
        s_min_sw_hat[BPT];
    // s_min_sw[-U:] / s_min_sw_hat[-U:] (ns.py:370-378): one entry per FRAME, as the reference
    // appends them
    double ring[BPT][kNsMaxRing], ring_hat[BPT][kNsMaxRing];
    float2 xn[BPT];
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
        f[k] = threadIdx.x + k * blockDim.x;
        on[k] = f[k] < F;
        gh1[k] = 1.0;
        lam[k] = var_s[k] = var_s_hat[k] = s_min[k] = s_min_sw[k] = s_min_hat[k] = s_min_sw_hat[k] = 0.0;
        xn[k] = on[k] ? X[f[k]] : make_float2(0.f, 0.f);
    }
    bool bad = false;
    int slot = 0;  // t % U

    for (int t = 0; t < T; ++t) {
        float2 x[BPT];
        double P[BPT], xi[BPT], v[BPT];
#pragma unroll
        for (int k = 0; k < BPT; ++k) {
            x[k] = xn[k];
            if (on[k] && t + 1 < T) xn[k] = X[(size_t)(t + 1) * F + f[k]];
            if (!on[k]) continue;
            bad |= cell_bad(x[k]);
            P[k] = (double)x[k].x * (double)x[k].x + (double)x[k].y * (double)x[k].y;
            if (t == 0) lam[k] = P[k];
            // eq.3, eq.32, eq.33
            const double gamma = P[k] / fmax(lam[k] * p.beta, p.eps);
            xi[k] = fmax(p.alpha * (gh1[k] * gh1[k] * gamma) + (1.0 - p.alpha) * fmax(gamma - 1.0, 0.0), p.xi_min);
            v[k] = gamma * xi[k] / (1.0 + xi[k]);
            // The reference has no floor under gamma here: a cell of digital silence gives v = 0,
            // E1 = inf and, a frame later, inf x 0 = NaN for the rest of the utterance.  E1 alone
            // sees gamma floored at eps, the floor MCRA.run applies (ns.py:84).
            const double v_e1 = fmax(gamma, p.eps) * xi[k] / (1.0 + xi[k]);
            gh1[k] = xi[k] / (1.0 + xi[k]) * exp(0.5 * expint_e1(v_e1));
            rowP[f[k]] = P[k];
        }
        __syncthreads();
        double var_sf[BPT];
#pragma unroll
        for (int k = 0; k < BPT; ++k) {
            if (!on[k]) continue;
            // eq.14, eq.15
            var_sf[k] = conv_same(rowP, f[k], wm, p.half_m);
            if (t == 0)
                var_s[k] = var_s_hat[k] = s_min[k] = s_min_sw[k] = var_sf[k];
            else {
                var_s[k] = p.alpha_s * var_s[k] + (1.0 - p.alpha_s) * var_sf[k];
                s_min[k] = fmin(s_min[k], var_s[k]);
                s_min_sw[k] = fmin(s_min_sw[k], var_s[k]);
            }
            // eq.21
            const double den = fmax(s_min[k], p.eps);
            const double gamma_min = P[k] * p.inv_b_min / den;
            const double zeta = var_sf[k] * p.inv_b_min / den;
            const double ind = (gamma_min < p.gamma0 && zeta < p.zeta0) ? 1.0 : 0.0;
            rowI[f[k]] = ind;
            rowIP[f[k]] = P[k] * ind;
        }
        __syncthreads();
        const int n_ring = t + 1 < U ? t + 1 : U;
        const bool block_end = (t + 1) % p.V == 0;
#pragma unroll
        for (int k = 0; k < BPT; ++k) {
            if (!on[k]) continue;
            // eq.26, eq.27
            const double ind_conv = conv_same(rowI, f[k], wm, p.half_m);
            const double obs_conv = conv_same(rowIP, f[k], wm, p.half_m);
            const double var_sf_hat = ind_conv > 0.0 ? obs_conv / ind_conv : var_s_hat[k];
            if (t == 0) {
                s_min_hat[k] = var_s[k];
                s_min_sw_hat[k] = var_sf[k];
            } else {
                var_s_hat[k] = p.alpha_s * var_s_hat[k] + (1.0 - p.alpha_s) * var_sf_hat;
                s_min_hat[k] = fmin(s_min_hat[k], var_s_hat[k]);
                s_min_sw_hat[k] = fmin(s_min_sw_hat[k], var_s_hat[k]);
            }
            // eq.28, eq.29, eq.7
            const double den = fmax(s_min_hat[k], p.eps);
            const double gmh = P[k] * p.inv_b_min / den;
            const double zh = var_s[k] * p.inv_b_min / den;
            double pr = 0.0;
            if (gmh > 1.0 && gmh < p.gamma1 && zh < p.zeta0) {
                const double q = (p.gamma1 - gmh) / (p.gamma1 - 1.0);
                pr = 1.0 / (1.0 + q * (1.0 + xi[k]) / (1.0 - q) * exp(-v[k]));
            }
            if (gmh >= p.gamma1 && zh >= p.zeta0) pr = 1.0;
            // eq.11, eq.10
            const double a_d = p.alpha_d + (1.0 - p.alpha_d) * pr;
            lam[k] = a_d * lam[k] + (1.0 - a_d) * P[k];
            ring[k][slot] = s_min_sw[k];
            ring_hat[k][slot] = s_min_sw_hat[k];
            if (block_end) {
                double m = ring[k][0], mh = ring_hat[k][0];
                for (int i = 1; i < n_ring; ++i) {
                    m = fmin(m, ring[k][i]);
                    mh = fmin(mh, ring_hat[k][i]);
                }
                s_min[k] = m;
                s_min_hat[k] = mh;
                s_min_sw[k] = var_s[k];
                s_min_sw_hat[k] = var_s_hat[k];
            }
            const double gain = om_lsa_gain(gh1[k], pr, p.gmin, log_gmin);
            bad |= !isfinite(gain);
            ns_emit(u, (size_t)t * F + f[k], gain, x[k]);
        }
        slot = slot + 1 == U ? 0 : slot + 1;
    }
    ns_epilogue(sm, u, bad);
}

__global__ __launch_bounds__(256) void expint_e1_kernel(const double* __restrict__ x, double* __restrict__ y, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = expint_e1(x[i]);
}

}  // namespace

bool ns_supported(int F) { return F >= 1 && F <= kNsMaxBins; }

hipError_t launch_ns(const NsUtt* d_utts, const NsParams* d_params, int kind, int n_utts, int F, hipStream_t s) {
    const int bpt = F > 1024 ? 2 : 1;
    const int threads = (((F + bpt - 1) / bpt) + 63) & ~63;
    if (kind == kNsMcra) {
        if (bpt == 1)
            hipLaunchKernelGGL(ns_mcra_kernel<1>, dim3(n_utts), dim3(threads), 0, s, d_utts, d_params);
        else
            hipLaunchKernelGGL(ns_mcra_kernel<2>, dim3(n_utts), dim3(threads), 0, s, d_utts, d_params);
    } else {
        if (bpt == 1)
            hipLaunchKernelGGL(ns_imcra_kernel<1>, dim3(n_utts), dim3(threads), 0, s, d_utts, d_params);
        else
            hipLaunchKernelGGL(ns_imcra_kernel<2>, dim3(n_utts), dim3(threads), 0, s, d_utts, d_params);
    }
    return hipGetLastError();
}

hipError_t launch_expint_e1(const double* x, double* y, int n, hipStream_t s) {
    hipLaunchKernelGGL(expint_e1_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, n);
    return hipGetLastError();
}

}  // namespace setk
