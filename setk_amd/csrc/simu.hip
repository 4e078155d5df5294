// simu.hip -- data simulation (scripts/sptk/wav_simulate.py): reverberation of a source with a
// multi-channel RIR as a uniformly partitioned overlap-save convolution on the 512-point real
// transform of fft512.h, and the mixing of the images at an SDR / SNR with peak normalisation.
//
// Reverberation (add_room_response, :29-54), block B = 256.  The RIR of channel c is cut into
// P = ceil(R / 256) blocks, each zero-padded to 512 and transformed once (H[c][p]); source frame k
// is samples [(k-1) B, (k+1) B) with zeros in front of sample 0 (X[k]); then
//     Y[c][k] = sum_{p <= min(P-1, k)} X[k-p] H[c][p]
// and output block k is the last 256 samples of the inverse transform of Y[c][k].  Exact up to
// rounding: no convolutive-transfer-function approximation.
//
// A transform lives on a quad-row of 16 lanes (fft512.h): after the Hermitian split lane la
// owns bins k = la + 16 m and 256 - k, m < 8; lane 0 carries (Re X[0], Re X[256]) in its entry 0
// and bin 128 in its entry 8.  X and H are STORED in that order ("lane layout": 256 complex per
// transform, row r = 16 consecutive lanes = 128 contiguous bytes), so the product-accumulate
// reads both with coalesced 8-byte loads straight into the registers that the inverse transform
// starts from: Y lives in the accumulator registers and never goes to memory.
//
// simu_conv_kernel: a workgroup of 16 quad-rows takes 16 consecutive frames of one source, a
// quad-row one frame and NC channels of the RIR per pass over X (NC = 2, or 1 for an odd channel
// count): X[k-p] is loaded once per step and used for NC channels.  The 16 quad-rows need the
// SAME H[c][p] in the same step: the workgroup fetches it once (a thread one entry per channel),
// one step ahead, into a double-buffered 2 x NC x 2 KB of LDS, and every quad-row reads it from
// there (the four quad-rows of a wave read the same addresses: a broadcast).  All of H (P x 2 KB
// per channel, 66 KB at P = 32) would fit LDS for one or two channels only; a step's worth always
// does.  The X[k-p] windows of the 16 quad-rows overlap by 15 of 16 frames and come through the
// CU's vector cache.  Measured at the bench workload (profiles/simu/ab_channels.txt): two channels
// per pass beat four (256 registers, one wave per SIMD) and one.
//
// Mixing (add_speaker, add_point_noise, the tail of run_simu, :57-143, :244-312).  Mean squares
// are float64 sums in a fixed two-stage order (a workgroup per 8192 samples with a fixed LDS
// tree, then the partials in index order by one thread): bit-reproducible, no floating-point
// atomics.  A mixture sample is recomputed from the images in float64 wherever it is needed
// (speaker power, peak, output) rather than stored unscaled; the peak max |mix| is an INTEGER
// maximum on the bits of the float64 magnitudes (order-free).
#include "common.h"
#include "fft512.h"

namespace setk {

namespace {

constexpr int ROW = 18;
constexpr int SL = slot_entries(ROW);
constexpr int kB = kSimuBlock;
constexpr double kEps = 1.1920928955078125e-07;  // np.finfo(np.float32).eps, the reference's EPSILON

// the twiddle rows of fft512.h's per-lane tables, computed here (float64 sincospi, rounded once)
// so that the convolution needs no STFT plan on the handle
__device__ __forceinline__ void fill_twiddles(cf* tw_l, cf* tw5_l, int tid, int nthreads) {
    for (int i = tid; i < 256; i += nthreads) {
        const int la = i & 15, q = i >> 4;
        double s, c;
        sincospi(-(double)(la * q) / 128.0, &s, &c);
        tw_l[la * ROW + q] = make_float2((float)c, (float)s);
    }
    for (int i = tid; i < 128; i += nthreads) {
        const int la = i & 15, m = i >> 4;
        double s, c;
        sincospi(-(double)(la + 16 * m) / 256.0, &s, &c);
        tw5_l[la * kRow5 + m] = make_float2((float)c, (float)s);
    }
}

__device__ __forceinline__ float sample_at(const void* p, int fmt, size_t i) {
    return fmt ? (float)static_cast<const short*>(p)[i] * (1.f / 32768.f) : static_cast<const float*>(p)[i];
}

// ---- forward transforms of source frames and RIR blocks into the lane layout.
// grid: work items of 16 transforms, a quad-row each ----
__global__ __launch_bounds__(256) void simu_fwd_kernel(const SimuFwd* __restrict__ jobs,
                                                       const SimuItem* __restrict__ items) {
    __shared__ __attribute__((aligned(16))) cf slots[16 * SL];
    __shared__ __attribute__((aligned(16))) cf tw_l[16 * ROW];
    __shared__ __attribute__((aligned(16))) cf tw5_l[16 * kRow5];
    const int tid = threadIdx.x, la = tid & 15, g = tid >> 4;
    fill_twiddles(tw_l, tw5_l, tid, 256);
    __syncthreads();
    const SimuItem it = items[blockIdx.x];
    const SimuFwd j = jobs[it.job];
    const int f = it.f0 + g;
    const bool valid = f < j.frames;
    // RIR block p: samples [p B, (p + 1) B) in front of 256 zeros; source frame k: [(k-1) B, (k+1) B)
    const int s = j.rir ? f * kB : (f - 1) * kB;
    const int lo = j.rir ? s : 0;
    const int hi = j.rir ? min(s + kB, j.n) : j.n;
    cf v[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        const int i0 = s + 2 * (la + 16 * jj);
        float a = 0.f, b = 0.f;
        // (the 1/2 the Hermitian split omits, exact)
        if (valid && i0 >= lo && i0 < hi) a = 0.5f * sample_at(j.src, j.fmt, j.wrap ? i0 % j.len : i0);
        if (valid && i0 + 1 >= lo && i0 + 1 < hi) b = 0.5f * sample_at(j.src, j.fmt, j.wrap ? (i0 + 1) % j.len : i0 + 1);
        v[jj] = make_float2(a, b);
    }
    cf* slot = slots + g * SL;
    fft256_stage_a_pad<-1, ROW>(v, slot, tw_l + la * ROW, la);
    __builtin_amdgcn_wave_barrier();
    fft256_stage_b_pad<-1, ROW>(v, slot, la);  // v[pos(kb)] = Z[la + 16 kb]
    cf t5[8];
    lds_row<8, true>(tw5_l + la * kRow5, t5);
    const bool lane0 = la == 0;
    cf* out = j.X + (size_t)f * 256 + la;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const cf Zk = v[dft16_pos(m)];
        const cf oth = v[dft16_pos(15 - m)];
        const cf own = v[dft16_pos((16 - m) & 15)];
        cf Zm = make_float2(qr_partner(oth.x), qr_partner(oth.y));
        Zm = make_float2(lane0 ? own.x : Zm.x, lane0 ? own.y : Zm.y);
        cf Xk, Xm;
        rfft_split(Zk, Zm, t5[m], Xk, Xm);
        if (m == 0 && lane0) {
            const cf Z128 = v[dft16_pos(8)];
            const cf x0 = make_float2(Xk.x, Xm.x);  // (Re X[0], Re X[256])
            Xm = make_float2(2.f * Z128.x, -2.f * Z128.y);
            Xk = x0;
        }
        if (valid) {
            out[16 * m] = Xk;
            out[16 * (8 + m)] = Xm;
        }
    }
}

// ---- product-accumulate and inverse transform.  grid: work items (job, 16 frames, NC channels) ----
template <int NC>
__global__ __launch_bounds__(256) void simu_conv_kernel(const SimuConv* __restrict__ jobs,
                                                        const SimuConvItem* __restrict__ items) {
    __shared__ __attribute__((aligned(16))) cf slots[16 * SL];
    __shared__ __attribute__((aligned(16))) cf tw_l[16 * ROW];
    __shared__ __attribute__((aligned(16))) cf tw5_l[16 * kRow5];
    __shared__ __attribute__((aligned(16))) cf hbuf[2 * NC * 256];  // H[c][p] of this step | of the next
    const int tid = threadIdx.x, la = tid & 15, g = tid >> 4;
    fill_twiddles(tw_l, tw5_l, tid, 256);
    const SimuConvItem it = items[blockIdx.x];
    const SimuConv j = jobs[it.job];
    const int k = it.k0 + g;
    const bool valid = k < j.K;
    const bool lane0 = la == 0;
    cf acc[NC][16];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = make_float2(0.f, 0.f);
    const int pmax = valid ? min(j.P - 1, k) : -1;
    const int pend = min(j.P - 1, it.k0 + 15);  // the workgroup's last step (its last frame's)
    const gcfloat2_p X = (gcfloat2_p)j.X + la;
    // H[c][p] of the pass's channels goes through LDS, fetched by the whole workgroup one step
    // ahead (a thread one entry per channel) into the buffer the step before last has left
    const gcfloat2_p Hc = (gcfloat2_p)j.H + (size_t)it.c0 * j.P * 256 + tid;
    v2f hnext[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) hbuf[c * 256 + tid] = make_float2(Hc[(size_t)c * j.P * 256].x, Hc[(size_t)c * j.P * 256].y);
    __syncthreads();
    for (int p = 0; p <= pend; ++p) {
        const cf* hb = hbuf + (p & 1) * NC * 256 + la;
        if (p < pend) {
#pragma unroll
            for (int c = 0; c < NC; ++c) hnext[c] = Hc[((size_t)c * j.P + p + 1) * 256];
        }
        if (p <= pmax) {
            const gcfloat2_p xr = X + (size_t)(k - p) * 256;
            cf x[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const v2f d = xr[16 * r];
                x[r] = make_float2(d.x, d.y);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const cf d = hb[c * 256 + 16 * r];
                    const cf a = acc[c][r];
                    const cf full = make_float2(fmaf(x[r].x, d.x, fmaf(-x[r].y, d.y, a.x)),
                                                fmaf(x[r].x, d.y, fmaf(x[r].y, d.x, a.y)));
                    if (r == 0) {
                        // lane 0: the two real bins 0 and 256 ride in one entry
                        const cf packed = make_float2(fmaf(x[r].x, d.x, a.x), fmaf(x[r].y, d.y, a.y));
                        acc[c][r] = make_float2(lane0 ? packed.x : full.x, lane0 ? packed.y : full.y);
                    } else
                        acc[c][r] = full;
                }
            }
        }
        if (p < pend) {
            cf* hn = hbuf + ((p + 1) & 1) * NC * 256 + tid;
#pragma unroll
            for (int c = 0; c < NC; ++c) hn[c * 256] = make_float2(hnext[c].x, hnext[c].y);
        }
        __syncthreads();  // the next step's H is there; this step's buffer is free
    }
    cf* slot = slots + g * SL;
    const cf* tw_row = tw_l + la * ROW;
    cf t5[8];
    lds_row<8, true>(tw5_l + la * kRow5, t5);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        cf Zlo[8], Zhi[8];  // 2 Z'[la + 16 m] and 2 Z'[256 - (la + 16 m)]
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const cf yk = acc[c][m], ym = acc[c][8 + m];
            cf zk, zm;
            irfft_merge(yk, ym, t5[m], zk, zm);
            if (m == 0) {
                const cf z0 = make_float2(yk.x + yk.y, yk.x - yk.y);
                const cf z128 = make_float2(2.f * ym.x, -2.f * ym.y);
                Zlo[m] = lane0 ? z0 : zk;
                Zhi[m] = lane0 ? z128 : zm;  // lane 0: Zhi[0] holds 2 Z'[128]
            } else {
                Zlo[m] = zk;
                Zhi[m] = zm;
            }
        }
        // v[j] = 2 Z'[la + 16 j]: j < 8 own; j >= 8 the mirror value of the partner lane (lane 0:
        // its own Zhi[16 - j], Zhi[0] for j = 8)
        cf v[16];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) v[jj] = Zlo[jj];
#pragma unroll
        for (int jj = 8; jj < 16; ++jj) {
            const cf src = Zhi[15 - jj];
            const cf own = Zhi[(16 - jj) & 7];
            const cf pv = make_float2(qr_partner(src.x), qr_partner(src.y));
            v[jj] = make_float2(lane0 ? own.x : pv.x, lane0 ? own.y : pv.y);
        }
        __builtin_amdgcn_wave_barrier();  // the slot is free (the channel before has read it)
        fft256_stage_a_pad<+1, ROW>(v, slot, tw_row, la);
        __builtin_amdgcn_wave_barrier();
        fft256_stage_b_pad<+1, ROW>(v, slot, la);
        // time samples (2 n, 2 n + 1) of n = la + 16 kb; the last 256 are output block k
        if (valid) {
            float* o = j.out + (size_t)(it.c0 + c) * j.S;
#pragma unroll
            for (int kb = 8; kb < 16; ++kb) {
                const cf z = v[dft16_pos(kb)];
                const int i = k * kB + 2 * (la + 16 * (kb - 8));
                if (i < j.S) o[i] = z.x * (1.f / 512.f);
                if (i + 1 < j.S) o[i + 1] = z.y * (1.f / 512.f);
            }
        }
    }
}

// ---- sum of squares: stage one of the fixed two-stage order.  A workgroup takes
// kSimuPowChunk samples: a thread sums every 256th in order, then a fixed LDS tree ----
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// one image's contribution to channel c, sample n of its mixture.  The load is unconditional (of
// sample 0 where n lies outside the image), so that the loads of a thread's several samples can be
// in flight together
__device__ __forceinline__ double img_term(const SimuImage& im, double coeff, int c, int n) {
    const int i = n - im.beg;
    const bool in = i >= 0 && i < im.dur;
    int k = in ? i : 0;
    if (k >= im.len) k %= im.len;  // (a repeated close-talk noise)
    const float v = sample_at(im.data, im.fmt, (size_t)(im.nch == 1 ? 0 : c) * im.pitch + k);
    return in ? coeff * (double)v : 0.0;
}

// grid (chunks of the longest image, images)
__global__ __launch_bounds__(256) void simu_power_kernel(const SimuImage* __restrict__ imgs,
                                                         double* __restrict__ partial) {
    __shared__ double red[256];
    const SimuImage im = imgs[blockIdx.y];
    const int n0 = blockIdx.x * kSimuPowChunk;
    if (n0 >= im.pw_n) return;
    const int n1 = min(n0 + kSimuPowChunk, im.pw_n);
    double s = 0.0;
#pragma unroll 4
    for (int i = n0 + threadIdx.x; i < n1; i += 256) {
        const double v = (double)sample_at(im.data, im.fmt, i >= im.len ? i % im.len : i);
        s += v * v;
    }
    s = block_sum(s, red, threadIdx.x);
    if (threadIdx.x == 0) partial[im.part0 + blockIdx.x] = s;
}

__device__ __forceinline__ double spk_value(const SimuMix& m, int c, int n) {
    double v = 0.0;
    for (int i = 0; i < m.n_spk; ++i) v += img_term(m.img[i], m.coeff[i], c, n);
    return v;
}

__device__ __forceinline__ double noise_value(const SimuMix& m, int c, int n) {
    double v = 0.0;
    for (int i = m.n_spk; i < m.n_img; ++i) v += img_term(m.img[i], m.coeff[i], c, n);
    return v;
}

// channel 0 of the speaker-only mixture (run_simu :255).  grid (chunks of the longest, mixtures)
__global__ __launch_bounds__(256) void simu_spkpow_kernel(const SimuMix* __restrict__ mixes) {
    __shared__ double red[256];
    const SimuMix m = mixes[blockIdx.y];
    const int n0 = blockIdx.x * kSimuPowChunk;
    if (n0 >= m.L) return;
    const int n1 = min(n0 + kSimuPowChunk, m.L);
    double s = 0.0;
#pragma unroll 4
    for (int n = n0 + threadIdx.x; n < n1; n += 256) {
        const double v = spk_value(m, 0, n);
        s += v * v;
    }
    s = block_sum(s, red, threadIdx.x);
    if (threadIdx.x == 0) m.spk_partial[blockIdx.x] = s;
}

__device__ __forceinline__ double coeff_snr(double sig_pow, double ref_pow, double snr) {
    return sqrt(ref_pow / (sig_pow * pow(10.0, snr / 10.0) + kEps));
}

// stage two of the sums and the coefficients, a thread per mixture.  STAGE 0: image powers and the
// speakers' coefficients (:87-91); STAGE 1: the speaker-only power and the noises' (:141, :296)
template <int STAGE>
__global__ __launch_bounds__(64) void simu_coeff_kernel(const SimuMix* __restrict__ mixes, int n_mix,
                                                        const double* __restrict__ partial) {
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= n_mix) return;
    const SimuMix m = mixes[u];
    if (STAGE == 0) {
        for (int i = 0; i < m.n_img; ++i) {
            const SimuImage im = m.img[i];
            double s = 0.0;
            for (int q = 0; q < im.nparts; ++q) s += partial[im.part0 + q];
            m.power[i] = s / (double)im.pw_n;
        }
        for (int i = 0; i < m.n_spk; ++i) m.coeff[i] = i == 0 ? 1.0 : coeff_snr(m.power[i], m.power[0], m.img[i].snr);
    } else {
        double s = 0.0;
        const int nparts = (m.L + kSimuPowChunk - 1) / kSimuPowChunk;
        for (int q = 0; q < nparts; ++q) s += m.spk_partial[q];
        const double spk_power = s / (double)m.L;
        m.power[m.n_img] = spk_power;
        for (int i = m.n_spk; i < m.n_img; ++i) m.coeff[i] = coeff_snr(m.power[i], spk_power, m.img[i].snr);
    }
}

// max |mix| over channels and samples, as an integer maximum on the bits of the non-negative
// float64 magnitudes.  grid (ceil(max L / 2048), channels, mixtures)
__global__ __launch_bounds__(256) void simu_peak_kernel(const SimuMix* __restrict__ mixes) {
    const SimuMix m = mixes[blockIdx.z];
    const int c = blockIdx.y;
    if (c >= m.N || (int)blockIdx.x * 2048 >= m.L) return;
    unsigned long long bits = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = (blockIdx.x * 8 + q) * 256 + threadIdx.x;
        const int nn = min(n, m.L - 1);
        const double a = fabs(spk_value(m, c, nn) + noise_value(m, c, nn));
        // (a NaN sticks: its bits exceed every number's)
        const unsigned long long b = (unsigned long long)__double_as_longlong(a) & 0x7fffffffffffffffull;
        bits = n < m.L ? max(bits, b) : bits;
    }
    for (int s = 32; s > 0; s >>= 1) bits = max(bits, (unsigned long long)__shfl_xor((long long)bits, s, 64));
    // one atomic per workgroup, and none where the word already holds as much (thousands of
    // workgroups share a mixture's word: the atomics, not the loads, set this kernel's time otherwise)
    __shared__ unsigned long long red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        bits = max(max(red[0], red[1]), max(red[2], red[3]));
        if (bits > __hip_atomic_load(m.peak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(m.peak, bits);
    }
}

__device__ __forceinline__ void put(void* dst, size_t i, float v, bool pcm16) {
    // libsndfile's float -> PCM_16 as launch_float_to_pcm16 has it
    if (pcm16)
        static_cast<int16_t*>(dst)[i] = (int16_t)(long long)rint((double)v * 32767.0);
    else
        static_cast<float*>(dst)[i] = v;
}

// the scaled mixture and its channel-0 references (:304-312).  grid (ceil(max L / 1024), channels,
// mixtures)
__global__ __launch_bounds__(256) void simu_out_kernel(const SimuMix* __restrict__ mixes, int pcm16) {
    const SimuMix m = mixes[blockIdx.z];
    const int c = blockIdx.y;
    const unsigned long long pb = *m.peak;
    if (c == 0 && blockIdx.x == 0 && threadIdx.x == 0)
        *m.status = pb >= 0x7ff0000000000000ull ? 3 /* SETK_NUM_NONFINITE */ : 0;
    if (c >= m.N || (int)blockIdx.x * 1024 >= m.L) return;
    const double factor = m.norm_factor / (__longlong_as_double((long long)pb) + kEps);
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // four samples a thread, their loads in flight together
        const int n = (blockIdx.x * 4 + q) * 256 + threadIdx.x;
        const int nn = min(n, m.L - 1);
        const bool live = n < m.L;
        const double nz = noise_value(m, c, nn);
        double spk = 0.0;
        for (int s = 0; s < m.n_spk; ++s) {
            const double v = img_term(m.img[s], m.coeff[s], c, nn);
            spk += v;
            if (live && c == 0 && m.spk_ref[s]) put(m.spk_ref[s], n, (float)(v * factor), pcm16 != 0);
        }
        if (live && c == 0 && m.noise_ref) put(m.noise_ref, n, (float)(nz * factor), pcm16 != 0);
        // float32 planar [N][L]; 16-bit frames as a wave file stores them, [L][N]
        if (live) put(m.mix, pcm16 ? (size_t)n * m.N + c : (size_t)c * m.L + n, (float)((spk + nz) * factor), pcm16 != 0);
    }
}

template <int NC>
hipError_t launch_conv_t(const SimuConv* jobs, const SimuConvItem* items, int n_items, hipStream_t s) {
    if (n_items > 0) hipLaunchKernelGGL(simu_conv_kernel<NC>, dim3(n_items), dim3(256), 0, s, jobs, items);
    return hipGetLastError();
}

}  // namespace

int simu_conv_channels(int N) { return N % 2 == 0 ? 2 : 1; }

hipError_t launch_simu_fwd(const SimuFwd* d_jobs, const SimuItem* d_items, int n_items, hipStream_t s) {
    if (n_items > 0) hipLaunchKernelGGL(simu_fwd_kernel, dim3(n_items), dim3(256), 0, s, d_jobs, d_items);
    return hipGetLastError();
}

hipError_t launch_simu_conv(const SimuConv* d_jobs, const SimuConvItem* d_items, int nc, int n_items,
                            hipStream_t s) {
    if (nc == 2) return launch_conv_t<2>(d_jobs, d_items, n_items, s);
    return launch_conv_t<1>(d_jobs, d_items, n_items, s);
}

hipError_t launch_simu_power(const SimuImage* d_imgs, int n_imgs, int max_n, double* d_partial, hipStream_t s) {
    if (n_imgs > 0)
        hipLaunchKernelGGL(simu_power_kernel, dim3((max_n + kSimuPowChunk - 1) / kSimuPowChunk, n_imgs), dim3(256), 0,
                           s, d_imgs, d_partial);
    return hipGetLastError();
}

hipError_t launch_simu_coeff(const SimuMix* d_mixes, int n_mix, int stage, const double* d_partial, hipStream_t s) {
    const dim3 grid((n_mix + 63) / 64);
    if (stage == 0)
        hipLaunchKernelGGL(simu_coeff_kernel<0>, grid, dim3(64), 0, s, d_mixes, n_mix, d_partial);
    else
        hipLaunchKernelGGL(simu_coeff_kernel<1>, grid, dim3(64), 0, s, d_mixes, n_mix, d_partial);
    return hipGetLastError();
}

hipError_t launch_simu_spkpow(const SimuMix* d_mixes, int n_mix, int max_len, hipStream_t s) {
    hipLaunchKernelGGL(simu_spkpow_kernel, dim3((max_len + kSimuPowChunk - 1) / kSimuPowChunk, n_mix), dim3(256), 0, s,
                       d_mixes);
    return hipGetLastError();
}

hipError_t launch_simu_peak(const SimuMix* d_mixes, int n_mix, int max_channels, int max_len, hipStream_t s) {
    hipLaunchKernelGGL(simu_peak_kernel, dim3((max_len + 2047) / 2048, max_channels, n_mix), dim3(256), 0, s, d_mixes);
    return hipGetLastError();
}

hipError_t launch_simu_out(const SimuMix* d_mixes, int n_mix, int max_channels, int max_len, bool pcm16,
                           hipStream_t s) {
    hipLaunchKernelGGL(simu_out_kernel, dim3((max_len + 1023) / 1024, max_channels, n_mix), dim3(256), 0, s, d_mixes,
                       pcm16 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace setk
