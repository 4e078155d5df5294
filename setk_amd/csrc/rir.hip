// rir.hip -- room impulse responses by the image method: RirGenerator::GenerateRir and MicrophoneSim
// of the reference (include/rir-generator.cc:108-223) for a ragged batch of (RIR, microphone) pairs.
//
// Per pair ("channel") the reference walks the images (x, y, z, q, j, k) of the source, |x| <= nx =
// ceil(ns / (2 T.x)) and so on, and every image that passes the order test and floor(dist) < ns adds
// Tw taps of a Hann-windowed sinc at pos = floor(dist) - Tw / 2 + 1:
//     rir[pos + n] += gain * 0.5 (1 - cos(2 pi (n + 1 - d) / Tw)) * sinc(pi (n + 1 - d - Tw / 2))
// with d = dist - floor(dist) and gain = mic(p) Refl / (4 pi dist cts).  About 157 000 images of 128
// taps for a 7 x 8 x 3 m room at 8000 taps: 20 M tap contributions per channel.
//
// Arithmetic.  The inputs are the reference's float32 values; everything from there is float64,
// rounded to float32 once at the end (the reference: float32 distances and sums).
//
// One sine per image.  With m = n + 1 - Tw / 2 an integer, sin(pi (m - d)) = -(-1)^m sin(pi d): the
// sinc over the taps of an image is  -(-1)^m sin(pi d) / (pi (m - d)),  one sinpi per image and one
// reciprocal per tap.  The window follows by angle addition from a table of cos / sin(2 pi (n + 1) /
// Tw) (LDS, Tw entries) and one sincospi(2 d / Tw) per image.  d == 0 (an image at a whole number of
// samples): the sinc is 1 at m = 0 and 0 elsewhere (Sinc, rir-generator.h:156), where the window is
// 1: the image adds its gain to tap floor(dist) alone.
//
// Order of the sums.  A workgroup owns a run of images of one channel (RirItem) and keeps the
// channel's taps in LDS as 64-bit FIXED POINT, multiples of 2^-40: each contribution is rounded to
// that grid once (to nearest, ties to even) and added with an integer LDS add.  Integer adds commute, so the sum does
// not depend on which wave comes first, nor on how the images are cut into parts: the parts go to
// global memory as integers and rir_finish_kernel adds them as integers.  The same input gives the
// same bits run to run, alone or in a batch, split or not; there is no floating-point atomic.
//   Scale and headroom: a contribution is gain x (window x sinc), |window x sinc| <= 1, and an image
// whose |gain| is not below 2^10 (a source within 1e-4 m of a microphone, or coefficients far
// above 1) is left out and flagged SETK_NUM_NONFINITE, so every contribution is below 2^11, where the
// rounding is one addition (kFixMagic); 2^63 / 2^40 = 2^23 is left for the sum.  With
// |beta| <= 1 the taps of a room of 1 m^3 at 16384 taps sum to below 1e3 (128 d / (V_samples cts)
// bounds the images overlapping a tap at distance d).  Rounding to the grid: 2^-41 per
// contribution, below 3e-9 of the direct path at 3 m for the few thousand images that meet in a tap
// -- four orders under the reference's own float32 noise (tests/PARITY_NOTES_RIR.md).
//
// Shape.  512 threads; per step every lane sets up one image (geometry, reflection product,
// pattern, gain, sin(pi d), the window's phase) in its registers; then each wave walks the images of
// its own 64 lanes that passed (a ballot), the image's values broadcast as scalars (v_readlane),
// lanes = taps, two taps a lane at Tw = 128.  The waves never wait for each other inside the walk.
// LDS: 8 bytes a tap and the window table, 66 KB at 8000 taps: two workgroups, four waves per SIMD.
// rir_finish_kernel: one workgroup per channel, 2048 taps at a time: the parts are added, one lane
// runs the 3-state high-pass recursion of :180-190 over LDS, all lanes round and store.
#include "common.h"

namespace setk {

namespace {

constexpr int kFinishChunk = 2048;

constexpr int kFinishThreads = 256;
// v + kFixMagic has an ulp of 2^-40 for |v| < 2^11: the low mantissa bits of the sum ARE rint(v 2^40) in
// two's complement, one add and one 64-bit subtract instead of a conversion sequence
constexpr double kFixMagic = 0x1.8p12;

// lane `src` (wave-uniform) of a per-lane double, as a scalar
__device__ __forceinline__ double bcast(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ unsigned long long to_fixed(double v) {
    return (unsigned long long)(__double_as_longlong(v + kFixMagic) - __double_as_longlong(kFixMagic));
}

// b^n for a small non-negative integer n; b^0 = 1 also for b = 0 (pow(0, 0), the anechoic room)
__device__ __forceinline__ double ipow(double b, int n) {
    double r = 1.0;
    while (n) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

__global__ __launch_bounds__(kRirThreads) void rir_images_kernel(const RirChan* __restrict__ chans,
                                                                 const RirItem* __restrict__ items) {
    extern __shared__ __attribute__((aligned(16))) char rmem[];
    const RirItem it = items[blockIdx.x];
    const RirChan& c = chans[it.chan];
    const int ns = c.ns, Tw = c.Tw, half = Tw / 2, order = c.order;
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(rmem);     // [ns]
    double* wtab = reinterpret_cast<double*>(acc + ns);                         // [Tw][2]

    for (int t = tid; t < ns; t += kRirThreads) acc[t] = 0ull;
    for (int n = tid; n < Tw; n += kRirThreads) {
        double sn, cn;
        sincospi(2.0 * (double)(n + 1) / (double)Tw, &sn, &cn);
        wtab[2 * n] = cn;
        wtab[2 * n + 1] = sn;
    }
    const int ny1 = 2 * c.n[1] + 1, nz1 = 2 * c.n[2] + 1;
    const double rho = c.rho, inv_tw2 = 2.0 / (double)Tw;
    const double kInvPi = 0.31830988618379067154, kPi = 3.14159265358979323846;
    bool flagged = false;
    __syncthreads();

    for (long long base = it.img0; base < it.img1; base += kRirThreads) {
        const long long i = base + tid;
        bool take = false;
        // the image of this lane: a = gain * 0.5 * sin(pi d) / pi (d == 0: the gain), cos / sin(2 pi d / Tw)
        double r_a = 0.0, r_d = 0.0, r_cb = 0.0, r_sb = 0.0;
        int r_pos = 0;
        if (i < it.img1) {
            const int k = (int)(i & 1), j = (int)((i >> 1) & 1), q = (int)((i >> 2) & 1);
            long long cell = i >> 3;
            const int z = (int)(cell % nz1) - c.n[2];
            cell /= nz1;
            const int y = (int)(cell % ny1) - c.n[1];
            const int x = (int)(cell / ny1) - c.n[0];
            if (order == -1 || abs(2 * x - q) + abs(2 * y - j) + abs(2 * z - k) <= order) {
                const double px = (double)(1 - 2 * q) * c.S[0] - c.R[0] + (double)(2 * x) * c.T[0];
                const double py = (double)(1 - 2 * j) * c.S[1] - c.R[1] + (double)(2 * y) * c.T[1];
                const double pz = (double)(1 - 2 * k) * c.S[2] - c.R[2] + (double)(2 * z) * c.T[2];
                const double dist = sqrt(px * px + py * py + pz * pz);
                const double fd = floor(dist);
                if (fd < (double)ns) {
                    const double refl = ipow(c.beta[0], abs(x - q)) * ipow(c.beta[1], abs(x)) *
                                        ipow(c.beta[2], abs(y - j)) * ipow(c.beta[3], abs(y)) *
                                        ipow(c.beta[4], abs(z - k)) * ipow(c.beta[5], abs(z));
                    double pat = 1.0;
                    if (rho != 1.0) pat = rho + (1.0 - rho) * ((c.u[0] * px + c.u[1] * py + c.u[2] * pz) / dist);
                    const double gain = pat * refl / (4.0 * kPi * dist * c.cts);
                    if (!(fabs(gain) < 0x1p10)) {
                        flagged = true;  // a source on the microphone, or NaN / inf: left out
                    } else {
                        r_d = dist - fd;
                        r_a = r_d == 0.0 ? gain : gain * 0.5 * kInvPi * sinpi(r_d);
                        sincospi(r_d * inv_tw2, &r_sb, &r_cb);
                        r_pos = (int)fd - half + 1;
                        take = true;
                    }
                }
            }
        }
        // the wave walks the images of its own lanes that passed; their values come over as scalars
        unsigned long long todo = __ballot(take);
        while (todo) {
            const int t = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const double a = bcast(r_a, t), d = bcast(r_d, t);
            const int pos = __builtin_amdgcn_readlane(r_pos, t);
            if (d == 0.0) {
                // pos + half - 1 = floor(dist) < ns; it is >= 0 as dist >= 0
                const int idx = pos + half - 1;
                if (lane == 0 && Tw > 0 && idx >= 0 && idx < ns) atomicAdd(&acc[idx], to_fixed(a));
                continue;
            }
            const double cb = bcast(r_cb, t), sb = bcast(r_sb, t);
            for (int n = lane; n < Tw; n += 64) {
                const int idx = pos + n;
                if (idx >= 0 && idx < ns) {
                    const int m = n + 1 - half;
                    const double x = (double)m - d;  // never 0: 0 < d < 1
                    double rc = __builtin_amdgcn_rcp(x);  // a seed: two Newton steps to float64
                    rc = fma(fma(-x, rc, 1.0), rc, rc);
                    rc = fma(fma(-x, rc, 1.0), rc, rc);
                    const double w = 1.0 - fma(wtab[2 * n], cb, wtab[2 * n + 1] * sb);
                    const double v = ((m & 1) ? a : -a) * w * rc;
                    atomicAdd(&acc[idx], to_fixed(v));
                }
            }
        }
    }
    if (flagged) atomicMax(c.status, 3 /* SETK_NUM_NONFINITE */);
    __syncthreads();
    long long* part = c.part + (size_t)it.part * ns;
    for (int t = tid; t < ns; t += kRirThreads) part[t] = (long long)acc[t];
}

__global__ __launch_bounds__(kFinishThreads) void rir_finish_kernel(const RirChan* __restrict__ chans) {
    __shared__ double buf[kFinishChunk];
    const RirChan& c = chans[blockIdx.x];
    const int ns = c.ns, np = c.nparts, tid = threadIdx.x;
    if (tid == 0 && c.bad) atomicMax(c.status, 3 /* SETK_NUM_NONFINITE */);
    const double B1 = c.hp[0], B2 = c.hp[1], A1 = c.hp[2], R1 = c.hp[3];
    double y1 = 0.0, y2 = 0.0;  // Y.y, Y.z of :185-188 (thread 0)
    for (int base = 0; base < ns; base += kFinishChunk) {
        const int len = min(kFinishChunk, ns - base);
        for (int t = tid; t < len; t += kFinishThreads) {
            long long sum = 0;
            for (int p = 0; p < np; ++p) sum += c.part[(size_t)p * ns + base + t];
            buf[t] = (double)sum * 0x1p-40;
        }
        __syncthreads();
        if (c.hp_on && tid == 0) {
            for (int t = 0; t < len; ++t) {
                const double y0 = B1 * y1 + B2 * y2 + buf[t];
                buf[t] = y0 + A1 * y1 + R1 * y2;
                y2 = y1;
                y1 = y0;
            }
        }
        __syncthreads();
        for (int t = tid; t < len; t += kFinishThreads) c.out[base + t] = (float)buf[t];
        __syncthreads();
    }
}

}  // namespace

size_t rir_lds_bytes(int ns, int Tw) {
    return (size_t)ns * sizeof(unsigned long long) + (size_t)Tw * 2 * sizeof(double);
}

hipError_t launch_rir_images(const RirChan* d_chans, const RirItem* d_items, int n_items, int max_ns, int max_tw,
                             hipStream_t s) {
    if (max_ns < 1 || max_ns > kRirMaxTaps || max_tw < 0 || max_tw > kRirMaxWindow) return hipErrorInvalidValue;
    const size_t lds = rir_lds_bytes(max_ns, max_tw);  // at most 139 264 of the 163 840 bytes
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rir_images_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rir_images_kernel, dim3(n_items), dim3(kRirThreads), lds, s, d_chans, d_items);
    return hipGetLastError();
}

hipError_t launch_rir_finish(const RirChan* d_chans, int n_chans, hipStream_t s) {
    hipLaunchKernelGGL(rir_finish_kernel, dim3(n_chans), dim3(kFinishThreads), 0, s, d_chans);
    return hipGetLastError();
}

}  // namespace setk
