// ssl.hip -- mask-based sound source localisation (scripts/sptk/libs/ssl.py): frame scores of the
// maximum-likelihood and SRP-PHAT backends, the MUSIC score on a principal eigenvector, and the
// window reduction + arg-extremum that turns frame scores into one direction per window.
//
// Frame scores.  S[t][a] = sum_f g(a, t, f) is a short inner product (K = channels or microphone
// pairs, <= 16 / a few dozen) per cell followed by a logarithm (ML) or nothing (SRP): plain fp32
// VALU on a directions x frames register tile.  A wave owns 64 directions (one per lane) and a
// tile of kSslTile = 32 frames and walks all bins in order, so every S[t][a] is produced by one
// lane in a fixed order -- no atomics, two runs give the same bits.  The steer-vector operand
// is stored direction-fastest ([F][K][Apad], ssl_sv_prep_kernel), so a wave reads 64 consecutive
// values and uses each for all 32 frames of its tile.  The observation operand is the same for
// all directions: ssl_obs_prep_kernel lays it out as [tile][F][K][32 frames], 64 consecutive
// floats per (bin, k) at a wave-uniform address, which the compiler turns into scalar loads --
// the multiply-adds then take x from scalar registers and no LDS is involved.
#include "common.h"
#include "../../include/setk_hip.h"

namespace setk {

namespace {

constexpr int kTile = kSslTile;
constexpr int kFoldChunk = 64;

// ---- steer vectors [A][C][F] -> [F][K][Apad], direction fastest, zero beyond A ----
//   kSslMl:    sv / ||sv||_2 over the microphones (ssl.py:27), K = C
//   kSslSrp:   exp(i (angle sv_l - angle sv_r)) per pair (ssl.py:66-70), K = P
//   kSslMusic: sv as given, K = C
__global__ __launch_bounds__(256) void ssl_sv_prep_kernel(const float2* __restrict__ sv, const int2* __restrict__ pairs,
                                                          int mode, int A, int Apad, int C, int F, int K,
                                                          float2* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)F * Apad) return;
    const int a = (int)(i % Apad), f = (int)(i / Apad);
    float2* o = out + (size_t)f * K * Apad + a;
    if (a >= A) {
        for (int k = 0; k < K; ++k) o[(size_t)k * Apad] = make_float2(0.f, 0.f);
        return;
    }
    const float2* s = sv + (size_t)a * C * F + f;
    if (mode == kSslSrp) {
        for (int p = 0; p < K; ++p) {
            const float2 l = phasor(s[(size_t)pairs[p].x * F]), r = phasor(s[(size_t)pairs[p].y * F]);
            o[(size_t)p * Apad] = make_float2(l.x * r.x + l.y * r.y, l.y * r.x - l.x * r.y);
        }
        return;
    }
    float scale = 1.f;
    if (mode == kSslMl) {
        float n2 = 0.f;
        for (int m = 0; m < C; ++m) n2 += s[(size_t)m * F].x * s[(size_t)m * F].x + s[(size_t)m * F].y * s[(size_t)m * F].y;
        scale = 1.f / sqrtf(n2);
    }
    for (int m = 0; m < C; ++m) o[(size_t)m * Apad] = make_float2(s[(size_t)m * F].x * scale, s[(size_t)m * F].y * scale);
}

// ---- observations -> the tile layout.  grid (frame tiles, ceil(F / 32), utterances), 256 threads:
// a 32 frames x 32 bins patch per k is read bin-fastest and written frame-fastest through LDS ----
template <int MODE>
__global__ __launch_bounds__(256) void ssl_obs_prep_kernel(const SslUtt* __restrict__ utts, const int2* __restrict__ pairs,
                                                           int C, int F, int K, int norm, float eps) {
    __shared__ float2 patch[32][33];
    const SslUtt u = utts[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile * kTile >= u.T) return;
    const int col = threadIdx.x & 31, row = threadIdx.x >> 5;
    const int f0 = blockIdx.y * 32;
    const size_t chan = (size_t)u.T * u.pitch;
    const float2* spec = reinterpret_cast<const float2*>(u.spec);
    float2* xt = reinterpret_cast<float2*>(u.xt) + (size_t)tile * F * K * kTile;
    float ssh[4] = {0.f, 0.f, 0.f, 0.f}, mk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = tile * kTile + row + 8 * i, f = f0 + col;
        mk[i] = (t < u.T && f < F) ? (u.mask ? u.mask[(size_t)t * F + f] : 1.f) : 0.f;
    }
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = tile * kTile + row + 8 * i, f = f0 + col;
            float2 v = make_float2(0.f, 0.f);
            if (t < u.T && f < F) {
                const size_t at = (size_t)t * u.pitch + f;
                if (MODE == kSslMl) {
                    v = spec[(size_t)k * chan + at];
                    if (norm) {  // stft / np.maximum(|stft|, eps)  (ssl.py:29)
                        const float n2 = v.x * v.x + v.y * v.y;
                        if (n2 > 0x1p124f && eps <= 0x1p62f) {
                            // the squares overflow above |v| = 2^64: |v| > eps here, so v / |v|
                            // through phasor()'s exact rescaling
                            v = phasor(v);
                        } else {
                            const float r = 1.f / fmaxf(sqrtf(n2), eps);
                            v.x *= r;
                            v.y *= r;
                        }
                    }
                    ssh[i] += v.x * v.x + v.y * v.y;
                } else {  // mask x exp(i (angle x_l - angle x_r))  (ssl.py:64-68)
                    const float2 l = phasor(spec[(size_t)pairs[k].x * chan + at]);
                    const float2 r = phasor(spec[(size_t)pairs[k].y * chan + at]);
                    v = make_float2(mk[i] * (l.x * r.x + l.y * r.y), mk[i] * (l.y * r.x - l.x * r.y));
                }
            }
            patch[row + 8 * i][col] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = f0 + row + 8 * i;
            if (f < F) xt[((size_t)f * K + k) * kTile + col] = patch[col][row + 8 * i];
        }
        __syncthreads();
    }
    if (MODE == kSslMl) {
#pragma unroll
        for (int i = 0; i < 4; ++i) patch[row + 8 * i][col] = make_float2(ssh[i], mk[i]);
        __syncthreads();
        float* pm = u.pm + (size_t)tile * F * 2 * kTile;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = f0 + row + 8 * i;
            if (f < F) {
                const float2 v = patch[col][row + 8 * i];
                pm[((size_t)f * 2 + 0) * kTile + col] = v.x;
                pm[((size_t)f * 2 + 1) * kTile + col] = v.y;
            }
        }
    }
}

// ---- SRP offline: U[p][f] = sum_t mask u_p over the frames [t0, t1): partial sums over chunks
// of 64 frames, then the chunks in order (float64 throughout, fixed order), written as frame 0
// of a one-tile layout (the other 31 frames zero).  The contraction with the steer-vector
// phasors is then the frame-score kernel on one pseudo-frame: T times less work.
// grid (ceil(P F / 256), chunks of the longest utterance, utterances) ----
__global__ __launch_bounds__(256) void ssl_srp_fold_kernel(const SslUtt* __restrict__ utts, const int2* __restrict__ pairs,
                                                           int F, int P) {
    const SslUtt u = utts[blockIdx.z];
    const int ta = u.t0 + blockIdx.y * kFoldChunk;
    if (ta >= u.t1) return;
    const int tb = min(u.t1, ta + kFoldChunk);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P * F) return;
    const int f = i % F, p = i / F;
    const size_t chan = (size_t)u.T * u.pitch;
    const float2* xl = reinterpret_cast<const float2*>(u.spec) + (size_t)pairs[p].x * chan + f;
    const float2* xr = reinterpret_cast<const float2*>(u.spec) + (size_t)pairs[p].y * chan + f;
    double re = 0.0, im = 0.0;
    for (int t = ta; t < tb; ++t) {
        const float2 l = phasor(xl[(size_t)t * u.pitch]), r = phasor(xr[(size_t)t * u.pitch]);
        const float m = u.mask ? u.mask[(size_t)t * F + f] : 1.f;
        re += (double)(m * (l.x * r.x + l.y * r.y));
        im += (double)(m * (l.y * r.x - l.x * r.y));
    }
    reinterpret_cast<double2*>(u.pm)[(size_t)blockIdx.y * P * F + i] = make_double2(re, im);
}

__global__ __launch_bounds__(256) void ssl_srp_fold_sum_kernel(const SslUtt* __restrict__ utts, int F, int P) {
    const SslUtt u = utts[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P * F) return;
    const int f = i % F, p = i / F;
    const int chunks = (u.t1 - u.t0 + kFoldChunk - 1) / kFoldChunk;
    const double2* part = reinterpret_cast<const double2*>(u.pm);
    double re = 0.0, im = 0.0;
    for (int c = 0; c < chunks; ++c) {
        re += part[(size_t)c * P * F + i].x;
        im += part[(size_t)c * P * F + i].y;
    }
    float2* o = reinterpret_cast<float2*>(u.xt) + ((size_t)f * P + p) * kTile;
    o[0] = make_float2((float)re, (float)im);
    for (int t = 1; t < kTile; ++t) o[t] = make_float2(0.f, 0.f);
}

// ---- the frame scores.  grid (frame tiles, Apad / 64, utterances), one wave per workgroup.
// The observation tiles are read through the constant address space: written by the launch
// before, never by this one, and addressed wave-uniformly, so they arrive as scalar loads ----
typedef const __attribute__((address_space(4))) float* ssl_const_f32;
constexpr int kMlLog = 0, kSrp = 1, kMlPow = 2;  // MODE below

template <int MODE>
__global__ __launch_bounds__(64) void ssl_frame_score_kernel(const SslUtt* __restrict__ utts, const float2* __restrict__ svt,
                                                             int A, int Apad, int F, int K, float inv1pe, float eps,
                                                             float compression, float out_scale) {
    const SslUtt u = utts[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile * kTile >= u.T) return;
    const int a = blockIdx.y * 64 + threadIdx.x;
    const ssl_const_f32 xt = (ssl_const_f32)(u.xt + (size_t)tile * F * K * kTile * 2);
    const ssl_const_f32 pm = (ssl_const_f32)(u.pm + (size_t)tile * F * 2 * kTile);
    const float2* __restrict__ sp = svt + a;
    float S[kTile];
#pragma unroll
    for (int t = 0; t < kTile; ++t) S[t] = 0.f;
    for (int f = 0; f < F; ++f) {
        if (MODE != kSrp) {
            float ar[kTile], ai[kTile];
#pragma unroll
            for (int t = 0; t < kTile; ++t) ar[t] = ai[t] = 0.f;
            for (int m = 0; m < K; ++m) {
                const float2 s = sp[((size_t)f * K + m) * Apad];
                const ssl_const_f32 x = xt + ((size_t)f * K + m) * kTile * 2;
#pragma unroll
                for (int t = 0; t < kTile; ++t) {  // sv conj(x)  (ssl.py:31)
                    ar[t] = fmaf(s.x, x[2 * t], fmaf(s.y, x[2 * t + 1], ar[t]));
                    ai[t] = fmaf(s.y, x[2 * t], fmaf(-s.x, x[2 * t + 1], ai[t]));
                }
            }
            const ssl_const_f32 q = pm + (size_t)f * 2 * kTile;
#pragma unroll
            for (int t = 0; t < kTile; ++t) {
                const float delta = q[t] - (ar[t] * ar[t] + ai[t] * ai[t]) * inv1pe;  // ssl.py:33
                float ll;
                if (MODE == kMlLog)
                    ll = -__logf(delta < eps ? eps : delta);  // (a NaN stays one, as np.maximum has it)
                else
                    ll = -__expf(compression * __logf(delta));  // -delta^compression (NaN below 0, like numpy)
                S[t] = fmaf(q[kTile + t], ll, S[t]);
            }
        } else {
            for (int p = 0; p < K; ++p) {
                const float2 d = sp[((size_t)f * K + p) * Apad];
                const ssl_const_f32 x = xt + ((size_t)f * K + p) * kTile * 2;
#pragma unroll
                for (int t = 0; t < kTile; ++t)  // Re(conj(d) u) = cos(obs ipd - oracle ipd)  (ssl.py:72)
                    S[t] = fmaf(d.x, x[2 * t], fmaf(d.y, x[2 * t + 1], S[t]));
            }
        }
    }
    if (a >= A) return;
    const int n = min(kTile, u.T - tile * kTile);
    float* out = u.S + (size_t)tile * kTile * A + a;
#pragma unroll
    for (int t = 0; t < kTile; ++t)
        if (t < n) out[(size_t)t * A] = S[t] * out_scale;
}

// ---- MUSIC: score[w][a] = sum_f | ||sv||^2 - |v_f^H sv|^2 |, v the principal eigenvector of
// window w's covariance (I - v v^H is the noise-subspace projector of ssl.py:98-107).  A bin whose
// covariance [C][C] is zero has no principal eigenvector, which the eigen-solve does not say:
// the first workgroup reports it beside that solve's status ----
__global__ __launch_bounds__(64) void ssl_music_score_kernel(const float2* __restrict__ svt, const float* __restrict__ v,
                                                             const float2* __restrict__ cov, int A, int Apad, int F,
                                                             int C, double* __restrict__ score, int* __restrict__ status) {
    if (blockIdx.x == 0)
        for (int f = threadIdx.x; f < F; f += 64) {
            bool zero = true;
            for (int e = 0; e < C * C; ++e) {
                const float2 r = cov[(size_t)f * C * C + e];
                zero = zero && r.x == 0.f && r.y == 0.f;
            }
            if (zero && status[f] == SETK_NUM_OK) status[f] = SETK_NUM_SINGULAR;
        }
    const int a = blockIdx.x * 64 + threadIdx.x;
    const float2* __restrict__ sp = svt + a;
    double acc = 0.0;
    for (int f = 0; f < F; ++f) {
        const float* __restrict__ vf = v + (size_t)f * C * 2;
        float n2 = 0.f, re = 0.f, im = 0.f;
        for (int m = 0; m < C; ++m) {
            const float2 s = sp[((size_t)f * C + m) * Apad];
            n2 = fmaf(s.x, s.x, fmaf(s.y, s.y, n2));
            re = fmaf(vf[2 * m], s.x, fmaf(vf[2 * m + 1], s.y, re));   // conj(v) s
            im = fmaf(vf[2 * m], s.y, fmaf(-vf[2 * m + 1], s.x, im));
        }
        acc += (double)fabsf(n2 - (re * re + im * im));
    }
    if (a < A) score[a] = acc;
}

// ---- frames [t0, t1) of spec -> [C][t1 - t0][F] contiguous, and the squared mask (the
// covariance of stft * mask is setk_covar's with mask^2, ssl.py:94-96) ----
__global__ __launch_bounds__(256) void ssl_music_prep_kernel(const float2* __restrict__ spec, const float* __restrict__ mask,
                                                             int C, int T, int F, int pitch, int t0, int t1,
                                                             float2* __restrict__ xo, float* __restrict__ m2) {
    const int Tw = t1 - t0;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Tw * F) return;
    const int f = (int)(i % F), t = (int)(i / F);
    const float m = mask ? mask[(size_t)(t0 + t) * F + f] : 1.f;
    m2[i] = m * m;
    for (int c = 0; c < C; ++c) xo[((size_t)c * Tw + t) * F + f] = spec[((size_t)c * T + t0 + t) * pitch + f];
}

// ---- window reduce + arg-extremum.  One workgroup per window: score[w][a] = sum of S[t][a]
// over [t0, t1) in frame order (float64), index[w] = the lowest index attaining the maximum
// (minimum: MUSIC), a NaN counting as the extremum, as np.argmax / np.argmin do ----
__device__ __forceinline__ bool ssl_better(double v, int i, double bv, int bi, bool take_min) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    if (v == bv) return i < bi;
    return take_min ? v < bv : v > bv;
}

__global__ __launch_bounds__(256) void ssl_window_kernel(const SslWin* __restrict__ wins, int A, int take_min,
                                                         double* __restrict__ score, int* __restrict__ index) {
    __shared__ double sv_[256];
    __shared__ int si_[256];
    const SslWin w = wins[blockIdx.x];
    double* sc = score + (size_t)blockIdx.x * A;
    double bv = 0.0;
    int bi = -1;
    for (int a = threadIdx.x; a < A; a += 256) {
        double v;
        if (w.S) {
            v = 0.0;
            for (int t = w.t0; t < w.t1; ++t) v += (double)w.S[(size_t)t * A + a];
            sc[a] = v;
        } else
            v = sc[a];
        if (bi < 0 || ssl_better(v, a, bv, bi, take_min)) {
            bv = v;
            bi = a;
        }
    }
    sv_[threadIdx.x] = bv;
    si_[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const double ov = sv_[threadIdx.x + s];
            const int oi = si_[threadIdx.x + s];
            if (oi >= 0 && (si_[threadIdx.x] < 0 || ssl_better(ov, oi, sv_[threadIdx.x], si_[threadIdx.x], take_min))) {
                sv_[threadIdx.x] = ov;
                si_[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) index[blockIdx.x] = si_[0];
}

}  // namespace

int ssl_apad(int A) { return (A + 63) & ~63; }
int ssl_tiles(int T) { return (T + kTile - 1) / kTile; }
size_t ssl_xt_bytes(int T, int F, int K) { return (size_t)ssl_tiles(T) * F * K * kTile * sizeof(float2); }
size_t ssl_pm_bytes(int T, int F) { return (size_t)ssl_tiles(T) * F * 2 * kTile * sizeof(float); }

size_t ssl_fold_bytes(int frames, int F, int P) {
    return (size_t)((frames + kFoldChunk - 1) / kFoldChunk) * P * F * sizeof(double2);
}

hipError_t launch_ssl_sv_prep(const float* sv, const int* d_pairs, int mode, int A, int C, int F, int K,
                              float* out, hipStream_t s) {
    const int Apad = ssl_apad(A);
    const long n = (long)F * Apad;
    hipLaunchKernelGGL(ssl_sv_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(sv), reinterpret_cast<const int2*>(d_pairs), mode, A, Apad, C,
                       F, K, reinterpret_cast<float2*>(out));
    return hipGetLastError();
}

hipError_t launch_ssl_obs_prep(const SslUtt* u, const int* d_pairs, int mode, int n_utts, int max_frames, int C,
                               int F, int K, int norm, float eps, hipStream_t s) {
    const dim3 grid(ssl_tiles(max_frames), (F + 31) / 32, n_utts);
    const int2* p = reinterpret_cast<const int2*>(d_pairs);
    if (mode == kSslMl)
        hipLaunchKernelGGL(ssl_obs_prep_kernel<kSslMl>, grid, dim3(256), 0, s, u, p, C, F, K, norm, eps);
    else
        hipLaunchKernelGGL(ssl_obs_prep_kernel<kSslSrp>, grid, dim3(256), 0, s, u, p, C, F, K, norm, eps);
    return hipGetLastError();
}

hipError_t launch_ssl_srp_fold(const SslUtt* u, const int* d_pairs, int n_utts, int max_frames, int F, int P,
                               hipStream_t s) {
    const int bx = (P * F + 255) / 256;
    hipLaunchKernelGGL(ssl_srp_fold_kernel, dim3(bx, (max_frames + kFoldChunk - 1) / kFoldChunk, n_utts), dim3(256),
                       0, s, u, reinterpret_cast<const int2*>(d_pairs), F, P);
    hipLaunchKernelGGL(ssl_srp_fold_sum_kernel, dim3(bx, 1, n_utts), dim3(256), 0, s, u, F, P);
    return hipGetLastError();
}

hipError_t launch_ssl_frame_scores(const SslUtt* u, const float* svt, int mode, int n_utts, int max_frames, int A,
                                   int F, int K, float inv1pe, float eps, float compression, hipStream_t s) {
    const int Apad = ssl_apad(A);
    const dim3 grid(ssl_tiles(max_frames), Apad / 64, n_utts);
    const float2* v = reinterpret_cast<const float2*>(svt);
    if (mode == kSslMl && compression <= 0.f)
        hipLaunchKernelGGL(ssl_frame_score_kernel<kMlLog>, grid, dim3(64), 0, s, u, v, A, Apad, F, K, inv1pe, eps,
                           compression, 1.f);
    else if (mode == kSslMl)
        hipLaunchKernelGGL(ssl_frame_score_kernel<kMlPow>, grid, dim3(64), 0, s, u, v, A, Apad, F, K, inv1pe, eps,
                           compression, 1.f);
    else
        hipLaunchKernelGGL(ssl_frame_score_kernel<kSrp>, grid, dim3(64), 0, s, u, v, A, Apad, F, K, inv1pe, eps,
                           compression, 1.f / (float)K);
    return hipGetLastError();
}

hipError_t launch_ssl_music_prep(const float* spec, const float* mask, int C, int T, int F, int pitch, int t0, int t1,
                                 float* xo, float* m2, hipStream_t s) {
    const long n = (long)(t1 - t0) * F;
    hipLaunchKernelGGL(ssl_music_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(spec), mask, C, T, F, pitch, t0, t1,
                       reinterpret_cast<float2*>(xo), m2);
    return hipGetLastError();
}

hipError_t launch_ssl_music_score(const float* svt, const float* v, const float* cov, int A, int F, int C,
                                  double* score, int* status, hipStream_t s) {
    const int Apad = ssl_apad(A);
    hipLaunchKernelGGL(ssl_music_score_kernel, dim3(Apad / 64), dim3(64), 0, s, reinterpret_cast<const float2*>(svt),
                       v, reinterpret_cast<const float2*>(cov), A, Apad, F, C, score, status);
    return hipGetLastError();
}

hipError_t launch_ssl_windows(const SslWin* d_wins, int n_wins, int A, bool take_min, double* score, int* index,
                              hipStream_t s) {
    hipLaunchKernelGGL(ssl_window_kernel, dim3(n_wins), dim3(256), 0, s, d_wins, A,
                       take_min ? 1 : 0, score, index);
    return hipGetLastError();
}

}  // namespace setk
