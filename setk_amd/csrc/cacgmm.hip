// cacgmm.hip -- CACGMM mask estimation: the complex angular central Gaussian mixture model of
// Ito, Araki, Nakatani (EUSIPCO 2016), the whole EM of one frequency bin in one launch, fp64.
//
// Replaces (funcwj/setk scripts/sptk/libs/cluster.py): norm_observation (:39-45), CacgmmTrainer
// (:468-535), Cacgmm.update / predict (:352-393), CacgDistribution.update_parameters / log_pdf
// (:298-337), Covariance (:94-135).  With eps = np.finfo(np.float32).eps and M channels:
//
//     z(f, t) = x(f, t) / max(||x(f, t)||_2, eps)                                     (:39-45, :489)
//     start (a)  gamma0 [K][F][T] from the caller, alpha = 1 / K, q = 1               (:509-518)
//     start (b)  K = 2: B_0 = sum_t z z^H / T, B_1 = I, alpha = 1 / 2, one E-step     (:496-507)
//     M-step     B_k = M sum_t (gamma_k / q_k) z z^H / max(sum_t gamma_k, eps)        (:302-309)
//                (B + B^H) / 2, eigh, w <- max(w / max(w_max, eps), eps)              (:99-113)
//                alpha_k = mean_t gamma_k   (update_alpha)                            (:364-365)
//     E-step     q_k = max(|z^H B_k^-1 z|, eps),  log p_k = -M log q_k - sum log w    (:325-332)
//                gamma_k = alpha_k e^(log p_k - max) / max(sum_k, eps)                (:383-389)
//
// The reference normalises in complex64; here z is float64 (the one deliberate deviation,
// measured in tests/PARITY_NOTES_CACGMM.md).  The per-iteration Q value the reference logs is
// not computed.
//
// One 256-thread workgroup owns one (utterance, bin) for the start, every iteration and the
// closing posterior: the bins of the model are independent, nothing crosses workgroups, no
// floating-point atomics, every sum has one fixed order -- the same input gives the same bits,
// alone or in a batch, resident or streaming.
//
//   load     x [C][Tp] complex64 of the bin (the bin-major layout of stft_binmajor_kernel /
//            auxiva_transpose_kernel) goes to LDS when it fits; thread = frame computes
//            r(t) = 1 / max(||x||, eps) in float64.  z = (double)x * r wherever it is used.
//   M-step   128-frame chunks of z are staged as float64 re / im rows with the K weights
//            gamma_k / q_k; the K covariances run on the fp64 matrix cores as in
//            auxiva_epoch_kernel: v_mfma_f64_16x16x4, A operand = B operand x weight, complex
//            C x C as a real 16 x 16 tile (result layout: tools/ubench/mfma_f64_layout.hip); the
//            four wavefronts take a quarter of a chunk each, their tiles are summed in
//            wavefront order.
//   eigh     wavefront k takes class k (K <= 4 wavefronts, in parallel): jacobi_herm of
//            jacobi_herm.h, the routine and stopping rule of cgmm_k.hip, called as it is.
//   E-step   thread = frame: q_k = sum_j |v_j^H z|^2 / w_j in the eigenbasis (all terms
//            positive), posteriors, the next weights.
//
// LDS budget (160 KiB per CU, one workgroup): fixed 38.6 KiB -- chunk rows 16 x 130 x 8 =
// 16.3 KiB, chunk weights 4 x 128 x 8 = 4 KiB, tiles 4 x 256 x 8 = 8 KiB, A and V
// 2 x 4 x 64 x 16 = 8 KiB, reductions 2 KiB, scalars -- plus the resident bin: x stays complex64
// there, 8 C T bytes (exact: float64 z is this times r(t), and 16 C T bytes of float64 would
// halve the length that fits): C = 8 holds 1940 frames, 31 s at hop 256.  A longer utterance
// streams x from global memory (L2 / Infinity Cache after the first pass) through the same
// staging, in the same order: the same bits.  SETK_CACGMM_STREAMING=1 forces that form.
//
// Per-frame state: r(t), gamma_k(t) and gamma_k(t) / q_k(t) are float64 in a global work area
// of the handle's arena, [F][2 K + 1][Tp]: 8 (2 K + 1) T bytes per bin (103 KiB at K = 3, 30 s)
// do not fit LDS beside the bin, a thread's frames (T / 256 of them) times 2 K + 1 doubles do
// not fit registers for any T.  Each word is written and read by its own workgroup only
// (ordered by the workgroup barrier): nothing there crosses workgroups.
#include <cstring>
#include "common.h"
#include "jacobi_herm.h"
#include "../../include/setk_hip.h"

namespace setk {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kCaK = 4;                // classes at most (one wavefront each in the eigh stage)
constexpr int kCaTC = 128;             // frames staged per chunk (32 per wavefront)
constexpr int kCaPitch = kCaTC + 2;    // row pitch in doubles (= 2 mod 32, as auxiva.hip)
constexpr double kCaEps = 1.1920928955078125e-07;  // np.finfo(np.float32).eps (libs/utils.py:16)

// the fixed part of the dynamic LDS, in bytes (every piece a multiple of 16)
constexpr size_t kCaXs = 16 * kCaPitch * sizeof(double);
constexpr size_t kCaWs = kCaK * kCaTC * sizeof(double);
constexpr size_t kCaS = kCaK * 256 * sizeof(double);
constexpr size_t kCaAV = 2 * kCaK * 64 * sizeof(zc);
constexpr size_t kCaScr = 256 * sizeof(double);
constexpr size_t kCaSmall = (kCaK * 8 + 4 * kCaK) * sizeof(double);  // w [K][8] | logdet, alpha, sumg, pad [K]
constexpr size_t kCaFixed = kCaXs + kCaWs + kCaS + kCaAV + kCaScr + kCaSmall;
constexpr size_t kCaLdsMax = 160 * 1024;

struct CacgArgs {
    const float2* x;       // [F][C][Tp] complex64
    const double* gamma0;  // [K][F][T] or null (cgmm_init)
    float* gamma_out;      // [K][T][F]
    double* work;          // [F][2 K + 1][Tp]: r | gamma [K] | gamma / q [K]
    int* status;           // [F], zeroed by the caller
    int T, Tp;
};

template <int C>
__global__ __launch_bounds__(256) void cacgmm_em_kernel(const CacgArgs* __restrict__ tbl, int F, int K,
                                                        int num_iters, int flags, int res_frames) {
    extern __shared__ __attribute__((aligned(16))) char cmem[];
    double* xs = reinterpret_cast<double*>(cmem);                      // [16][kCaPitch]
    double* ws = xs + 16 * kCaPitch;                                   // [kCaK][kCaTC]
    double* S = ws + kCaK * kCaTC;                                     // [kCaK][16][16]
    zc* Ak = reinterpret_cast<zc*>(S + kCaK * 256);                    // [kCaK][C][C]
    zc* Vk = Ak + kCaK * 64;                                           // [kCaK][C][C]
    double* scr = reinterpret_cast<double*>(Vk + kCaK * 64);           // [256]
    double* wk = scr + 256;                                            // [kCaK][8]
    double* logdet = wk + kCaK * 8;                                    // [kCaK]
    double* alpha = logdet + kCaK;                                     // [kCaK]
    double* sumg = alpha + kCaK;                                       // [kCaK]
    int* flag = reinterpret_cast<int*>(sumg + kCaK);                   // (pad [kCaK])
    float2* xres = reinterpret_cast<float2*>(cmem + kCaFixed);         // [C][Tp], resident form only

    const CacgArgs a = tbl[blockIdx.y];
    const int f = blockIdx.x, T = a.T, Tp = a.Tp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float2* xf = a.x + (size_t)f * C * Tp;
    double* rinv = a.work + (size_t)f * (2 * K + 1) * Tp;  // [Tp]
    double* gam = rinv + Tp;                               // [K][Tp]
    double* wgt = gam + (size_t)K * Tp;                    // [K][Tp]
    const bool resident = Tp <= res_frames;                // (uniform per workgroup)
    const bool cgmm_init = (flags & SETK_CACGMM_CGMM_INIT) != 0;
    const bool update_alpha = (flags & SETK_CACGMM_UPDATE_ALPHA) != 0;

    auto X = [&](int c, int t) { return resident ? xres[c * Tp + t] : xf[(size_t)c * Tp + t]; };
    auto block_sum = [&](double v) {
        scr[tid] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) scr[tid] += scr[tid + o];
            __syncthreads();
        }
        const double r = scr[0];
        __syncthreads();
        return r;
    };

    // ---- load: the bin into LDS, r(t), the start ----
    if (tid == 0) *flag = 0;
    if (tid < K) alpha[tid] = 1.0 / K;
    for (int i = tid; i < 16 * kCaPitch; i += 256) xs[i] = 0.0;  // rows of channels >= C stay 0
    __syncthreads();  // (the flag is cleared before any wave raises it)
    bool bad = false;
    for (int t = tid; t < T; t += 256) {
        double n2 = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float2 v = xf[(size_t)c * Tp + t];
            if (resident) xres[c * Tp + t] = v;
            n2 += (double)v.x * v.x + (double)v.y * v.y;
        }
        if (!isfinite(n2)) bad = true;
        rinv[t] = 1.0 / fmax(sqrt(n2), kCaEps);
        if (!cgmm_init)
            for (int k = 0; k < K; ++k) {
                const double g = a.gamma0[((size_t)k * F + f) * T + t];
                gam[(size_t)k * Tp + t] = g;
                wgt[(size_t)k * Tp + t] = g;  // q = 1 (cluster.py:516-518)
            }
    }
    if (bad) atomicMax(flag, SETK_NUM_NONFINITE);
    __syncthreads();

    const int row = lane & 15, kq = lane >> 4;  // the lane's place in the matrix-core operands
    const int mi = lane >> 3, mj = lane & 7;    // the lane's covariance entry

    // pass 0 is the start (b): B_0 = sum z z^H / T, B_1 = I, then the E-step
    for (int it = cgmm_init ? 0 : 1; it <= num_iters; ++it) {
        const bool start = it == 0;
        if (!start) {
            // sum_t gamma_k: the normaliser, and alpha of the posteriors this M-step uses
            for (int k = 0; k < K; ++k) {
                double s = 0.0;
                for (int t = tid; t < T; t += 256) s += gam[(size_t)k * Tp + t];
                s = block_sum(s);
                if (tid == 0) {
                    sumg[k] = s;
                    if (update_alpha) alpha[k] = s / T;
                }
            }
        }
        // ---- M-step: S_k[(i, p)][(j, q)] = sum_t w_k(t) z[(i, p)] z[(j, q)] ----
        v4d acc[kCaK];
#pragma unroll
        for (int k = 0; k < kCaK; ++k) acc[k] = (v4d){0.0, 0.0, 0.0, 0.0};
        for (int t0 = 0; t0 < T; t0 += kCaTC) {
            __syncthreads();
            for (int i = tid; i < C * kCaTC; i += 256) {
                const int c = i / kCaTC, tl = i % kCaTC, t = t0 + tl;
                double zr = 0.0, zi = 0.0;
                if (t < T) {
                    const float2 v = X(c, t);
                    const double r = rinv[t];
                    zr = (double)v.x * r;
                    zi = (double)v.y * r;
                }
                xs[(2 * c) * kCaPitch + tl] = zr;
                xs[(2 * c + 1) * kCaPitch + tl] = zi;
            }
            for (int i = tid; i < K * kCaTC; i += 256) {
                const int k = i / kCaTC, tl = i % kCaTC, t = t0 + tl;
                double w = 0.0;
                if (t < T) w = start ? (k == 0 ? 1.0 : 0.0) : wgt[(size_t)k * Tp + t];
                ws[i] = w;
            }
            __syncthreads();
            const int w0 = (kCaTC / 4) * wv;
            if (t0 + w0 < T) {  // (uniform per wavefront)
#pragma unroll 2
                for (int s = 0; s < kCaTC / 4; s += 4) {
                    const int tl = w0 + s + kq;
                    const double b = xs[row * kCaPitch + tl];
#pragma unroll
                    for (int k = 0; k < kCaK; ++k)
                        if (k < K)
                            acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(b * ws[k * kCaTC + tl], b, acc[k],
                                                                         0, 0, 0);
                }
            }
        }
        // lane holds column lane & 15 of rows lane / 16 + 4 v (tools/ubench/mfma_f64_layout.hip)
        for (int w = 0; w < 4; ++w) {
            __syncthreads();
            if (wv == w) {
#pragma unroll
                for (int k = 0; k < kCaK; ++k)
                    if (k < K) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int idx = k * 256 + (kq + 4 * v) * 16 + row;
                            S[idx] = (w == 0) ? acc[k][v] : S[idx] + acc[k][v];
                        }
                    }
            }
        }
        __syncthreads();
        // ---- B_k, Hermitian by (B + B^H) / 2; wavefront k, lane 8 i + j holds entry [i][j] ----
        if (wv < K && mi < C && mj < C) {
            const double* Sk = S + wv * 256;
            const double re_ij = Sk[(2 * mi) * 16 + 2 * mj] + Sk[(2 * mi + 1) * 16 + 2 * mj + 1];
            const double im_ij = Sk[(2 * mi + 1) * 16 + 2 * mj] - Sk[(2 * mi) * 16 + 2 * mj + 1];
            const double re_ji = Sk[(2 * mj) * 16 + 2 * mi] + Sk[(2 * mj + 1) * 16 + 2 * mi + 1];
            const double im_ji = Sk[(2 * mj + 1) * 16 + 2 * mi] - Sk[(2 * mj) * 16 + 2 * mi + 1];
            double br, bi;
            if (start) {
                br = wv == 0 ? re_ij / T : (mi == mj ? 1.0 : 0.0);
                bi = wv == 0 ? im_ij / T : 0.0;
                const double cr = wv == 0 ? re_ji / T : br, ci = wv == 0 ? im_ji / T : 0.0;
                br = (br + cr) / 2;
                bi = (bi - ci) / 2;
            } else {
                const double den = fmax(sumg[wv], kCaEps);
                br = ((double)C * re_ij / den + (double)C * re_ji / den) / 2;
                bi = ((double)C * im_ij / den - (double)C * im_ji / den) / 2;
            }
            Ak[wv * C * C + mi * C + mj] = zmk(br, bi);
        }
        __syncthreads();
        // ---- Covariance: eigh, scale by max(w_max, eps), floor eps ----
        if (wv < K && lane == 0) {
            zc* A = Ak + wv * C * C;
            zc* V = Vk + wv * C * C;
            const bool conv = jacobi_herm(A, V, C);
            double wmax = -1e300;
            bool finite = true;
            for (int i = 0; i < C; ++i) {
                wmax = fmax(wmax, A[i * C + i].x);
                finite = finite && isfinite(A[i * C + i].x);
            }
            // numpy.linalg.eigh raises on these (cluster.py:104-113); the posteriors go on being
            // computed, the status says what they are worth
            if (!(conv && finite)) atomicMax(flag, finite ? SETK_NUM_NOCONV : SETK_NUM_NONFINITE);
            const double sc = fmax(wmax, kCaEps);
            double ld = 0.0;
            for (int i = 0; i < C; ++i) {
                const double w = fmax(A[i * C + i].x / sc, kCaEps);
                wk[wv * 8 + i] = w;
                ld += log(w);
            }
            logdet[wv] = ld;
        }
        __syncthreads();
        // ---- E-step (Cacgmm.predict): q in the eigenbasis, posteriors, the next weights ----
        for (int t = tid; t < T; t += 256) {
            double zr[C], zi[C];
            const double r = rinv[t];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float2 v = X(c, t);
                zr[c] = (double)v.x * r;
                zi[c] = (double)v.y * r;
            }
            double lp[kCaK], qk[kCaK], lmax = -1e300;
#pragma unroll
            for (int k = 0; k < kCaK; ++k) {
                lp[k] = 0.0;
                qk[k] = 1.0;
                if (k < K) {
                    const zc* V = Vk + k * C * C;
                    double q = 0.0;
#pragma unroll 1
                    for (int j = 0; j < C; ++j) {
                        double pr = 0.0, pm = 0.0;  // v_j^H z
#pragma unroll
                        for (int i = 0; i < C; ++i) {
                            const zc v = V[i * C + j];
                            pr += v.x * zr[i] + v.y * zi[i];
                            pm += v.x * zi[i] - v.y * zr[i];
                        }
                        q += (pr * pr + pm * pm) / wk[k * 8 + j];
                    }
                    qk[k] = fmax(fabs(q), kCaEps);
                    lp[k] = -(double)C * log(qk[k]) - logdet[k];
                    lmax = fmax(lmax, lp[k]);
                }
            }
            double den = 0.0, nom[kCaK];
#pragma unroll
            for (int k = 0; k < kCaK; ++k) {
                nom[k] = 0.0;
                if (k < K) {
                    nom[k] = exp(lp[k] - lmax) * alpha[k];
                    den += nom[k];
                }
            }
            den = fmax(den, kCaEps);
#pragma unroll
            for (int k = 0; k < kCaK; ++k)
                if (k < K) {
                    const double g = nom[k] / den;
                    gam[(size_t)k * Tp + t] = g;
                    wgt[(size_t)k * Tp + t] = g / qk[k];
                }
        }
        __syncthreads();
    }
    for (int k = 0; k < K; ++k)
        for (int t = tid; t < T; t += 256)
            a.gamma_out[((size_t)k * T + t) * F + f] = (float)gam[(size_t)k * Tp + t];
    if (tid == 0 && *flag > a.status[f]) a.status[f] = *flag;
}

}  // namespace

bool cacgmm_supported(int C, int K) { return C >= 1 && C <= kMaxChannels && K >= 2 && K <= kCaK; }

const char* cacgmm_limit_message() {
    return "CACGMM on the device needs 1 <= num_channels <= 8 and 2 <= num_classes <= 4";
}

int cacgmm_pitch(int T) { return (T + 3) & ~3; }

size_t cacgmm_work_bytes(int K, int T, int F) {
    return (size_t)F * (2 * K + 1) * cacgmm_pitch(T) * sizeof(double);
}

// frames (of the padded pitch) of one bin that fit LDS beside the fixed part; 0: streaming
int cacgmm_resident_frames(int C, int max_frames, bool force_streaming) {
    const size_t need = (size_t)cacgmm_pitch(max_frames) * C * sizeof(float2);
    if (force_streaming || kCaFixed + need > kCaLdsMax) return 0;
    return cacgmm_pitch(max_frames);
}

size_t cacgmm_args_bytes() { return sizeof(CacgArgs); }

void cacgmm_fill_args(void* dst, const float* x_bin, const double* gamma0, float* gamma_out, double* work,
                      int* status, int T) {
    CacgArgs a;
    memset(&a, 0, sizeof(a));
    a.x = reinterpret_cast<const float2*>(x_bin);
    a.gamma0 = gamma0;
    a.gamma_out = gamma_out;
    a.work = work;
    a.status = status;
    a.T = T;
    a.Tp = cacgmm_pitch(T);
    memcpy(dst, &a, sizeof(a));
}

hipError_t launch_cacgmm(const void* d_tbl, int n_utts, int C, int F, int K, int num_iters, int flags,
                         int res_frames, hipStream_t s) {
    void (*kern)(const CacgArgs*, int, int, int, int, int) = nullptr;
    switch (C) {
        case 1: kern = cacgmm_em_kernel<1>; break;
        case 2: kern = cacgmm_em_kernel<2>; break;
        case 3: kern = cacgmm_em_kernel<3>; break;
        case 4: kern = cacgmm_em_kernel<4>; break;
        case 5: kern = cacgmm_em_kernel<5>; break;
        case 6: kern = cacgmm_em_kernel<6>; break;
        case 7: kern = cacgmm_em_kernel<7>; break;
        case 8: kern = cacgmm_em_kernel<8>; break;
    }
    if (!kern || K < 2 || K > kCaK) return hipErrorInvalidValue;
    const size_t lds = kCaFixed + (size_t)res_frames * C * sizeof(float2);
    if (lds > kCaLdsMax) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(F, n_utts), dim3(256), lds, s, static_cast<const CacgArgs*>(d_tbl), F, K,
                       num_iters, flags, res_frames);
    return hipGetLastError();
}

}  // namespace setk
