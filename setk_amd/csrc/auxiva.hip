// auxiva.hip -- AuxIVA blind source separation (N sources = N channels), fp64.
//
// Replaces (funcwj/setk) scripts/sptk/apply_auxiva.py: auxiva() (:24-57), the update rules
// of Ono, "Stable and fast update rules for independent vector analysis based on auxiliary
// function technique", WASPAA 2011:
//
//     W_f = I,  y_n(f, t) = w_n(f)^H x(f, t)
//     per epoch:  r_n(t) = sqrt(sum_f |y_n(f, t)|^2),  g_n(t) = 1 / (r_n(t) + eps_f32)   (:42-44)
//                 per bin, for n = 0 .. N-1 in order:                                     (:45-52)
//                     V_n = sum_t g_n(t) x x^H / T
//                     w = solve(W^H V_n, e_n);  W[:, n] = w / (w^H V_n w)
//                 y = W^H x                                                               (:54)
//
// The reference runs this in complex128 (its W is); with V, r and y in float32 the doc
// recording deviates by 5e-4, so only the observations are complex64 here.
//
// g is fixed for an epoch, so all N matrices V_n of a bin come from ONE pass over the bin's
// C x T observations; r needs every bin, so an epoch is two launches on the caller's stream
// (no grid-wide barrier inside a launch):
//   auxiva_norm_kernel    g_n(t) from the per-bin powers [F][N][Tp], summed over f in bin
//                         order by one thread (no floating-point atomics: the same input
//                         gives the same bits)
//   auxiva_epoch_kernel   one workgroup per (bin, utterance): the weighted covariances on the
//                         fp64 matrix cores, the N sequential updates (complex LU with partial
//                         pivoting, one wavefront, one matrix entry per lane), then the
//                         projection y = W^H x, which leaves |y_n(t)|^2 for the next epoch's
//                         norms or, after the last epoch, y itself.
// Layout: observations [F][C][Tp] complex64 (frames contiguous, Tp >= T: the layout
// stft_binmajor_kernel writes), powers [F][C][Tp] float64, weights 1 / r [C][Tp] float64,
// demixing matrices [F][C][C] complex128 (W[k][n] = entry k of w_n).
#include <cstring>
#include "common.h"
#include "../../include/setk_hip.h"

namespace setk {

namespace {

typedef double2 zd;
typedef double v4d __attribute__((ext_vector_type(4)));
#define AD __device__ __forceinline__
AD zd azmk(double a, double b) { return make_double2(a, b); }
AD zd azmul(zd a, zd b) { return azmk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
AD zd azsub(zd a, zd b) { return azmk(a.x - b.x, a.y - b.y); }
// conj(a) * b
AD zd azcmul(zd a, zd b) { return azmk(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }
AD zd azdiv(zd a, zd b) {
    const double d = b.x * b.x + b.y * b.y;
    return azmk((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
AD zd azshfl(zd v, int src) { return azmk(__shfl(v.x, src), __shfl(v.y, src)); }

constexpr int kAuxTC = 128;             // frames staged per chunk (32 per wavefront)
constexpr int kAuxPitch = kAuxTC + 2;   // row pitch in doubles, = 2 mod 32: the 16 rows x 2 frames
                                        // one half-wave reads land on 32 different bank pairs
constexpr double kAuxEps = 1.1920928955078125e-07;  // libs/utils.py:16 EPSILON (float32 eps)

struct AuxArgs {
    const float2* x;  // [F][C][Tp]
    double* pw;       // [F][C][Tp] |y_n(f, t)|^2; the last launch writes y there as float2
    double* g;        // [C][Tp] 1 / (r_n(t) + eps)
    double2* W;       // [F][C][C]
    int* status;      // [F], worst so far
    int T, Tp;
};

constexpr int kAuxUpdate = 1;  // run the update (else: W = I, projection only)
constexpr int kAuxWriteY = 2;  // the projection writes y (complex64) instead of |y|^2

// ---- g_n(t) = 1 / (sqrt(sum_f |y_n(f, t)|^2) + eps), f in order (apply_auxiva.py:42-44) ----
__global__ __launch_bounds__(256) void auxiva_norm_kernel(const AuxArgs* __restrict__ tbl, int C,
                                                          int F) {
    const AuxArgs a = tbl[blockIdx.z];
    const int n = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const double* p = a.pw + (size_t)n * a.Tp + t;
    const size_t step = (size_t)C * a.Tp;
    double s = 0.0;
    for (int f = 0; f < F; ++f) s += p[(size_t)f * step];
    a.g[(size_t)n * a.Tp + t] = 1.0 / (sqrt(s) + kAuxEps);
}

// ---- one epoch of one bin ----
// Covariances: with z[(c, p)] = Re / Im of x_c, row (c, p) = 2 c + p of a 16 x 16 real tile,
//     S_n[(i, p)][(j, q)] = sum_t g_n(t) z[(i, p)] z[(j, q)]       (v_mfma_f64_16x16x4_f64,
//     V_n[i][j] = ((S[i0][j0] + S[i1][j1]) + i (S[i1][j0] - S[i0][j1])) / T      one tile per n)
// The A operand of source n is the B operand times g_n: one LDS read per lane and step feeds
// all C tiles.  The four wavefronts take a quarter of every staged chunk each and their tiles
// are summed in wavefront order.
template <int C>
__global__ __launch_bounds__(256, 2) void auxiva_epoch_kernel(const AuxArgs* __restrict__ tbl, int mode) {
    __shared__ double xs[16 * kAuxPitch];  // [(c, p)][frame of the chunk]
    __shared__ double gs[C * kAuxTC];      // [n][frame of the chunk]
    __shared__ double S[C * 256];          // [n][row][col]
    __shared__ zd Wl[64];                  // [k][n], 8 x 8, identity beyond C
    __shared__ zd Vl[64];                  // V_n, 8 x 8, zero beyond C
    __shared__ int flag;

    const AuxArgs a = tbl[blockIdx.y];
    const int f = blockIdx.x, T = a.T, Tp = a.Tp;
    const float2* xf = a.x + (size_t)f * C * Tp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int mi = lane >> 3, mj = lane & 7;  // the lane's matrix entry (update stage)

    if (tid == 0) flag = 0;
    if (tid < 64) {
        zd w = azmk(mi == mj ? 1.0 : 0.0, 0.0);
        if ((mode & kAuxUpdate) && mi < C && mj < C) w = a.W[((size_t)f * C + mi) * C + mj];
        Wl[tid] = w;
        // (the first launch leaves W = I for the first update)
        if (!(mode & kAuxUpdate) && mi < C && mj < C) a.W[((size_t)f * C + mi) * C + mj] = w;
    }

    if (mode & kAuxUpdate) {
        for (int i = tid; i < 16 * kAuxPitch; i += 256) xs[i] = 0.0;  // rows of channels >= C stay 0
        v4d acc[C];
#pragma unroll
        for (int n = 0; n < C; ++n) acc[n] = (v4d){0.0, 0.0, 0.0, 0.0};
        const int row = lane & 15, kq = lane >> 4;
        for (int t0 = 0; t0 < T; t0 += kAuxTC) {
            __syncthreads();
            for (int i = tid; i < C * kAuxTC; i += 256) {
                const int c = i / kAuxTC, tl = i % kAuxTC;
                float2 v = make_float2(0.f, 0.f);
                double gv = 0.0;
                if (t0 + tl < T) {
                    v = xf[(size_t)c * Tp + t0 + tl];
                    gv = a.g[(size_t)c * Tp + t0 + tl];
                }
                xs[(2 * c) * kAuxPitch + tl] = (double)v.x;
                xs[(2 * c + 1) * kAuxPitch + tl] = (double)v.y;
                gs[i] = gv;
            }
            __syncthreads();
            const int w0 = (kAuxTC / 4) * wv;
            if (t0 + w0 < T) {  // (uniform per wavefront)
#pragma unroll 2
                for (int s = 0; s < kAuxTC / 4; s += 4) {
                    const int tl = w0 + s + kq;
                    const double b = xs[row * kAuxPitch + tl];
#pragma unroll
                    for (int n = 0; n < C; ++n)
                        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(b * gs[n * kAuxTC + tl], b, acc[n],
                                                                     0, 0, 0);
                }
            }
        }
        // result layout: lane holds column lane & 15 of rows lane / 16 + 4 v
        // (tools/ubench/mfma_f64_layout.hip)
        for (int w = 0; w < 4; ++w) {
            __syncthreads();
            if (wv == w) {
#pragma unroll
                for (int n = 0; n < C; ++n)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int idx = n * 256 + (kq + 4 * v) * 16 + row;
                        S[idx] = (w == 0) ? acc[n][v] : S[idx] + acc[n][v];
                    }
            }
        }
        __syncthreads();

        // ---- the N updates, in order; wavefront 0, lane 8 i + j holds entry [i][j] ----
        const double dT = (double)T;
        for (int n = 0; n < C; ++n) {
            zd vij = azmk(0.0, 0.0);
            if (wv == 0) {
                if (mi < C && mj < C) {
                    const double* Sn = S + n * 256;
                    vij = azmk((Sn[(2 * mi) * 16 + 2 * mj] + Sn[(2 * mi + 1) * 16 + 2 * mj + 1]) / dT,
                               (Sn[(2 * mi + 1) * 16 + 2 * mj] - Sn[(2 * mi) * 16 + 2 * mj + 1]) / dT);
                }
                Vl[lane] = vij;
            }
            __syncthreads();
            if (wv == 0) {
                // M = W^H V_n (identity beyond C), right-hand side e_n replicated along the rows
                zd m = azmk(mi == mj ? 1.0 : 0.0, 0.0);
                if (mi < C && mj < C) {
                    m = azmk(0.0, 0.0);
#pragma unroll
                    for (int k = 0; k < C; ++k) {
                        const zd p = azcmul(Wl[8 * k + mi], Vl[8 * k + mj]);
                        m = azmk(m.x + p.x, m.y + p.y);
                    }
                }
                zd b = azmk(mi == n ? 1.0 : 0.0, 0.0);
                // NaN / inf in the covariance (the bin's input, or r of some frame) is reported
                // as such, not as a zero pivot
                const bool nonfinite = __any(!(isfinite(m.x) && isfinite(m.y))) != 0;
                bool sing = nonfinite;
                // LU with partial pivoting (numpy.linalg.solve: ?gesv; pivot = first largest
                // |re| + |im| of the column, an exactly zero pivot is "Singular matrix")
                for (int k = 0; k < C && !nonfinite; ++k) {
                    const double mag = fabs(m.x) + fabs(m.y);
                    double best = -1.0;
                    int p = k;
                    for (int ii = k; ii < C; ++ii) {
                        const double v = __shfl(mag, 8 * ii + k);
                        if (v > best) {
                            best = v;
                            p = ii;
                        }
                    }
                    if (!(best > 0.0)) {  // zero or NaN column: every lane sees the same values
                        sing = true;
                        break;
                    }
                    const int sr = (mi == k) ? p : (mi == p) ? k : mi;
                    m = azshfl(m, 8 * sr + mj);
                    b = azshfl(b, 8 * sr + mj);
                    const zd piv = azshfl(m, 9 * k), lik = azshfl(m, 8 * mi + k);
                    const zd mkj = azshfl(m, 8 * k + mj), bk = azshfl(b, 8 * k);
                    if (mi > k) {
                        const zd l = azdiv(lik, piv);
                        m = azsub(m, azmul(l, mkj));
                        b = azsub(b, azmul(l, bk));
                    }
                }
                if (sing) {
                    if (lane == 0) flag = max(flag, nonfinite ? SETK_NUM_NONFINITE : SETK_NUM_SINGULAR);
                } else {
                    zd wi = azmk(0.0, 0.0), wj = azmk(0.0, 0.0);
                    for (int k = C - 1; k >= 0; --k) {
                        const zd xk = azdiv(azshfl(b, 8 * k), azshfl(m, 9 * k));
                        const zd mik = azshfl(m, 8 * mi + k);
                        if (mi < k) b = azsub(b, azmul(mik, xk));
                        if (mi == k) wi = xk;
                        if (mj == k) wj = xk;
                    }
                    // d = w^H V_n w, summed over the 64 entries in butterfly order
                    zd d = azcmul(wi, azmul(vij, wj));
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        d.x += __shfl_xor(d.x, o);
                        d.y += __shfl_xor(d.y, o);
                    }
                    if (mj == 0 && mi < C) Wl[8 * mi + n] = azdiv(wi, d);
                }
            }
            __syncthreads();
        }
        if (tid < 64 && mi < C && mj < C) a.W[((size_t)f * C + mi) * C + mj] = Wl[tid];
    }
    __syncthreads();

    // ---- y_n(t) = sum_c conj(W[c][n]) x_c(t), one frame per thread and trip; the loop over the
    // sources stays rolled: unrolled, the compiler keeps all C x C entries of W in registers (256
    // VGPRs at C = 8, one workgroup per CU) ----
    double* pw = a.pw + (size_t)f * C * Tp;
    float2* yo = reinterpret_cast<float2*>(pw);
    bool bad = false;
    for (int t = tid; t < T; t += 256) {
        double xr[C], xi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float2 v0 = xf[(size_t)c * Tp + t];
            xr[c] = v0.x;
            xi[c] = v0.y;
        }
#pragma unroll 1
        for (int n = 0; n < C; ++n) {
            double yr0 = 0.0, yi0 = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const zd w = Wl[8 * c + n];
                yr0 += w.x * xr[c] + w.y * xi[c];
                yi0 += w.x * xi[c] - w.y * xr[c];
            }
            const double p0 = yr0 * yr0 + yi0 * yi0;
            if (!isfinite(p0)) bad = true;
            if (mode & kAuxWriteY)
                yo[(size_t)n * Tp + t] = make_float2((float)yr0, (float)yi0);
            else
                pw[(size_t)n * Tp + t] = p0;
        }
    }
    if (bad) atomicMax(&flag, SETK_NUM_NONFINITE);
    __syncthreads();
    if (tid == 0 && flag > a.status[f]) a.status[f] = flag;
}

// [C][T][F] (the library's spectrogram layout, row pitch F) <-> [F][C][Tp]
template <bool TO_BIN>
__global__ __launch_bounds__(256) void auxiva_transpose_kernel(const float2* __restrict__ in, int C,
                                                               int T, int F, int Tp,
                                                               float2* __restrict__ out) {
    __shared__ float2 tile[32][33];
    const int c = blockIdx.z;
    const int f0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        if (TO_BIN) {
            const int t = t0 + i, f = f0 + tx;
            if (t < T && f < F) tile[i][tx] = in[((size_t)c * T + t) * F + f];
        } else {
            const int f = f0 + i, t = t0 + tx;
            if (t < T && f < F) tile[i][tx] = in[((size_t)f * C + c) * Tp + t];
        }
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        if (TO_BIN) {
            const int f = f0 + i, t = t0 + tx;
            if (t < T && f < F) out[((size_t)f * C + c) * Tp + t] = tile[tx][i];
        } else {
            const int t = t0 + i, f = f0 + tx;
            if (t < T && f < F) out[((size_t)c * T + t) * F + f] = tile[tx][i];
        }
    }
}

// the renorm target of every source of an utterance is the utterance's max |audio|
__global__ __launch_bounds__(256) void auxiva_spread_norm_kernel(const unsigned* __restrict__ norm_bits,
                                                                 int C, int n, unsigned* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = norm_bits[i / C];
}

}  // namespace

bool auxiva_supported(int C) { return C >= 1 && C <= kMaxChannels; }

const char* auxiva_limit_message() {
    return "AuxIVA on the device needs 1 <= channels <= 8 (sources = channels)";
}

size_t auxiva_args_bytes() { return sizeof(AuxArgs); }

void auxiva_fill_args(void* dst, const float* x_bin, double* power, double* g, void* W, int* status,
                      int T, int Tp) {
    AuxArgs a;
    a.x = reinterpret_cast<const float2*>(x_bin);
    a.pw = power;
    a.g = g;
    a.W = static_cast<double2*>(W);
    a.status = status;
    a.T = T;
    a.Tp = Tp;
    memcpy(dst, &a, sizeof(a));
}

hipError_t launch_auxiva_norm(const void* d_tbl, int n_utts, int C, int F, int max_frames,
                              hipStream_t s) {
    hipLaunchKernelGGL(auxiva_norm_kernel, dim3((max_frames + 255) / 256, C, n_utts), dim3(256), 0, s,
                       static_cast<const AuxArgs*>(d_tbl), C, F);
    return hipGetLastError();
}

// update: run the epoch's update (false: W = I, projection only -- the epoch-0 powers, or
// y = x for zero epochs); write_y: the projection leaves y (complex64, [F][C][Tp], in the
// power buffer) instead of |y|^2
hipError_t launch_auxiva_epoch(const void* d_tbl, int n_utts, int C, int F, bool update, bool write_y,
                               hipStream_t s) {
    void (*kern)(const AuxArgs*, int) = nullptr;
    switch (C) {
        case 1: kern = auxiva_epoch_kernel<1>; break;
        case 2: kern = auxiva_epoch_kernel<2>; break;
        case 3: kern = auxiva_epoch_kernel<3>; break;
        case 4: kern = auxiva_epoch_kernel<4>; break;
        case 5: kern = auxiva_epoch_kernel<5>; break;
        case 6: kern = auxiva_epoch_kernel<6>; break;
        case 7: kern = auxiva_epoch_kernel<7>; break;
        case 8: kern = auxiva_epoch_kernel<8>; break;
    }
    if (!kern) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(F, n_utts), dim3(256), 0, s, static_cast<const AuxArgs*>(d_tbl),
                       (update ? kAuxUpdate : 0) | (write_y ? kAuxWriteY : 0));
    return hipGetLastError();
}

hipError_t launch_auxiva_transpose(const float* in, int C, int T, int F, int Tp, float* out,
                                   bool to_bin, hipStream_t s) {
    dim3 grid((F + 31) / 32, (T + 31) / 32, C);
    if (to_bin)
        hipLaunchKernelGGL(auxiva_transpose_kernel<true>, grid, dim3(256), 0, s,
                           reinterpret_cast<const float2*>(in), C, T, F, Tp,
                           reinterpret_cast<float2*>(out));
    else
        hipLaunchKernelGGL(auxiva_transpose_kernel<false>, grid, dim3(256), 0, s,
                           reinterpret_cast<const float2*>(in), C, T, F, Tp,
                           reinterpret_cast<float2*>(out));
    return hipGetLastError();
}

hipError_t launch_auxiva_spread_norm(const unsigned* norm_bits, int C, int n, unsigned* out,
                                     hipStream_t s) {
    hipLaunchKernelGGL(auxiva_spread_norm_kernel, dim3((n + 255) / 256), dim3(256), 0, s, norm_bits, C,
                       n, out);
    return hipGetLastError();
}

}  // namespace setk
