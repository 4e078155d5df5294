// spatial.hip -- geometry-driven spatial features (scripts/sptk/libs/spatial.py): IPD maps,
// directional features over several directions of a steer-vector set, and the SRP-PHAT angular
// spectrum of linear and circular arrays.
//
// All three start from the pair coherence u_p[t][f] = exp(i (arg X_l - arg X_r)), the product of
// two unit phasors (arg 0 = 0, as np.angle has it): no atan2 but for the raw IPD, no cos / sin.
//
// IPD and DF are elementwise and memory-bound: one thread per (frame, bin), coalesced along the
// bins, one launch for all utterances (and all chosen directions) of a batch.
//
// SRP.  s_p[t][d] = Re sum_f u_p[t][f] W_p[f][d] is the frame-score contraction of ssl.hip per
// pair: a wave owns 64 directions (one per lane) and a tile of 32 frames, walks the bins in
// order, takes the observations of ssl_obs_prep_kernel<kSslSrp>'s tile layout through scalar
// loads and the table W [P][F][Dpad] direction-fastest.  Every pair has its own normaliser
// max_{t,d} |s_p|, so the pairs are contracted separately (grid z = utterance x pair) and the
// spectrum is finished in a second launch: phase 1 stores s_p and folds max |s_p| into one word
// per pair as an INTEGER maximum on the bits of the non-negative floats (order-free, so two runs
// give the same bits; no floating-point atomics), phase 2 divides, floors and sums the pairs in
// order with their weights.
#include "common.h"

namespace setk {

namespace {

constexpr int kTile = kSslTile;
constexpr float kPi = 3.14159265358979323846f;
constexpr float kEps = 1.1920929e-07f;  // np.finfo(np.float32).eps, the reference's EPSILON

// l conj(r) of two unit phasors (phasor(): common.h): (cos, sin) of the phase difference
__device__ __forceinline__ float2 coherence(float2 l, float2 r) {
    return make_float2(l.x * r.x + l.y * r.y, l.y * r.x - l.x * r.y);
}

// ---- IPD (spatial.py:163-181), the pairs side by side along the bins (np.hstack).
// grid (ceil(max T F / 256), 1, utterances) ----
template <int KIND>
__global__ __launch_bounds__(256) void spatial_ipd_kernel(const SpatialUtt* __restrict__ utts,
                                                          const int2* __restrict__ pairs, int F, int P) {
    const SpatialUtt u = utts[blockIdx.z];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)u.T * F) return;
    const int f = (int)(i % F);
    const long t = i / F;
    const size_t chan = (size_t)u.T * F;
    const float2* x = reinterpret_cast<const float2*>(u.spec) + (size_t)t * F + f;
    const int per = KIND == kSpatialCosSinIpd ? 2 * F : F;
    float* o = u.out + (size_t)t * P * per + f;
    for (int p = 0; p < P; ++p) {
        const float2 c = coherence(phasor(x[(size_t)pairs[p].x * chan]), phasor(x[(size_t)pairs[p].y * chan]));
        if (KIND == kSpatialIpd) {  // wrapped into [-pi, pi)
            float v = atan2f(c.y, c.x);
            if (v >= kPi) v -= 2.f * kPi;
            o[(size_t)p * per] = v;
        } else {
            o[(size_t)p * per] = c.x;
            if (KIND == kSpatialCosSinIpd) o[(size_t)p * per + F] = c.y;
        }
    }
}

// ---- DF over several directions (spatial.py:184-208, compute_df_on_geometry.py:49-60):
// out[t][k F + f] = mean_p cos((arg X_l - arg X_r) - (arg v_l - arg v_r)), v the steer vector of
// the utterance's k-th direction index.  grid (ceil(max T F / 256), directions, utterances) ----
__global__ __launch_bounds__(256) void spatial_df_kernel(const SpatialUtt* __restrict__ utts,
                                                         const int2* __restrict__ pairs,
                                                         const float2* __restrict__ sv,
                                                         const int* __restrict__ idx, int n_idx, int C, int F,
                                                         int P) {
    const SpatialUtt u = utts[blockIdx.z];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)u.T * F) return;
    const int f = (int)(i % F);
    const long t = i / F;
    const int k = blockIdx.y;
    const size_t chan = (size_t)u.T * F;
    const float2* x = reinterpret_cast<const float2*>(u.spec) + (size_t)t * F + f;
    const float2* v = sv + (size_t)idx[u.idx0 + k] * C * F + f;
    float acc = 0.f;
    for (int p = 0; p < P; ++p) {
        const float2 c = coherence(phasor(x[(size_t)pairs[p].x * chan]), phasor(x[(size_t)pairs[p].y * chan]));
        const float2 d = coherence(phasor(v[(size_t)pairs[p].x * F]), phasor(v[(size_t)pairs[p].y * F]));
        acc += c.x * d.x + c.y * d.y;
    }
    u.out[(size_t)t * n_idx * F + (size_t)k * F + f] = acc / (float)P;
}

// ---- SRP phase 1.  grid (frame tiles, Dpad / 64, utterances x pairs), one wave per workgroup.
// The observation tiles arrive as scalar loads (constant address space, wave-uniform address:
// written by the launch before, never by this one) ----
typedef const __attribute__((address_space(4))) float* spatial_const_f32;

__global__ __launch_bounds__(64) void spatial_srp_pair_kernel(const SslUtt* __restrict__ obs,
                                                              const SpatialUtt* __restrict__ utts,
                                                              const float2* __restrict__ table, int D, int Dpad,
                                                              int F, int P) {
    const int ui = blockIdx.z / P, p = blockIdx.z % P;
    const SpatialUtt u = utts[ui];
    const int tile = blockIdx.x;
    if (tile * kTile >= u.T) return;
    const int d = blockIdx.y * 64 + threadIdx.x;
    const spatial_const_f32 xt = (spatial_const_f32)(obs[ui].xt + (size_t)tile * F * P * kTile * 2);
    const float2* __restrict__ w = table + (size_t)p * F * Dpad + d;
    float S[kTile];
#pragma unroll
    for (int t = 0; t < kTile; ++t) S[t] = 0.f;
    for (int f = 0; f < F; ++f) {
        const float2 c = w[(size_t)f * Dpad];
        const spatial_const_f32 x = xt + ((size_t)f * P + p) * kTile * 2;
#pragma unroll
        for (int t = 0; t < kTile; ++t)  // Re(u W)  (spatial.py:52)
            S[t] = fmaf(c.x, x[2 * t], fmaf(-c.y, x[2 * t + 1], S[t]));
    }
    const int n = min(kTile, u.T - tile * kTile);
    float* sp = u.sp + ((size_t)p * u.T + (size_t)tile * kTile) * Dpad + d;
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < kTile; ++t)
        if (t < n) {
            sp[(size_t)t * Dpad] = S[t];  // (d < Dpad always; columns beyond D are zero: W is)
            // a NaN sticks and reaches the normaliser, as np.max passes it on: its bits exceed every float's
            const float a = fabsf(S[t]);
            if (d < D && (a > m || a != a)) m = a;
        }
    unsigned bits = __float_as_uint(m) & 0x7fffffffu;
    for (int s = 32; s > 0; s >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, s, 64));
    if (threadIdx.x == 0) atomicMax(u.pmax + p, bits);
}

// ---- SRP phase 2: out[t][d] = sum_p weight_p max(s_p / max(max |s_p|, eps), 0), the pairs in
// order (spatial.py:53-57, :118-123; compute_circular_srp.py:51).
// grid (ceil(max T D / 256), 1, utterances) ----
__global__ __launch_bounds__(256) void spatial_srp_combine_kernel(const SpatialUtt* __restrict__ utts,
                                                                  const float* __restrict__ weight, int D, int Dpad,
                                                                  int P) {
    const SpatialUtt u = utts[blockIdx.z];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)u.T * D) return;
    const int d = (int)(i % D);
    const long t = i / D;
    const float* sp = u.sp + (size_t)t * Dpad + d;
    float acc = 0.f;
    for (int p = 0; p < P; ++p) {
        const float m = __uint_as_float(u.pmax[p]);
        const float g = sp[(size_t)p * u.T * Dpad] / (m != m ? m : fmaxf(m, kEps));
        acc = fmaf(weight[p], g != g ? g : fmaxf(g, 0.f), acc);
    }
    u.out[i] = acc;
}

}  // namespace

hipError_t launch_spatial_ipd(const SpatialUtt* u, const int* d_pairs, int kind, int n_utts, int max_frames, int F,
                              int P, hipStream_t s) {
    const dim3 grid((unsigned)(((long)max_frames * F + 255) / 256), 1, n_utts);
    const int2* p = reinterpret_cast<const int2*>(d_pairs);
    if (kind == kSpatialIpd)
        hipLaunchKernelGGL(spatial_ipd_kernel<kSpatialIpd>, grid, dim3(256), 0, s, u, p, F, P);
    else if (kind == kSpatialCosIpd)
        hipLaunchKernelGGL(spatial_ipd_kernel<kSpatialCosIpd>, grid, dim3(256), 0, s, u, p, F, P);
    else
        hipLaunchKernelGGL(spatial_ipd_kernel<kSpatialCosSinIpd>, grid, dim3(256), 0, s, u, p, F, P);
    return hipGetLastError();
}

hipError_t launch_spatial_df(const SpatialUtt* u, const int* d_pairs, const float* sv, const int* d_idx, int n_idx,
                             int n_utts, int max_frames, int C, int F, int P, hipStream_t s) {
    const dim3 grid((unsigned)(((long)max_frames * F + 255) / 256), n_idx, n_utts);
    hipLaunchKernelGGL(spatial_df_kernel, grid, dim3(256), 0, s, u, reinterpret_cast<const int2*>(d_pairs),
                       reinterpret_cast<const float2*>(sv), d_idx, n_idx, C, F, P);
    return hipGetLastError();
}

hipError_t launch_spatial_srp_pairs(const SslUtt* d_obs, const SpatialUtt* u, const float* table, int n_utts,
                                    int max_frames, int D, int F, int P, hipStream_t s) {
    const int Dpad = ssl_apad(D);
    hipLaunchKernelGGL(spatial_srp_pair_kernel, dim3(ssl_tiles(max_frames), Dpad / 64, n_utts * P), dim3(64), 0, s,
                       d_obs, u, reinterpret_cast<const float2*>(table), D, Dpad, F, P);
    return hipGetLastError();
}

hipError_t launch_spatial_srp_combine(const SpatialUtt* u, const float* d_weight, int n_utts, int max_frames, int D,
                                      int P, hipStream_t s) {
    hipLaunchKernelGGL(spatial_srp_combine_kernel, dim3((unsigned)(((long)max_frames * D + 255) / 256), 1, n_utts),
                       dim3(256), 0, s, u, d_weight, D, ssl_apad(D), P);
    return hipGetLastError();
}

}  // namespace setk
