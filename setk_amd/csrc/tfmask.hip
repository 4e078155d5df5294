// tfmask.hip -- oracle TF masks (scripts/sptk/compute_mask.py), mask-based separation
// (wav_separate.py) and oracle separation (oracle_separate.py).
//
// Cell arithmetic.  Everything is float32, as the reference is once its spectra are complex64.
// |z| is cmat_abs (libs/utils.py:30-42): sqrt(re^2 + im^2), not hypot.  The cosine of the phase
// difference needs no trigonometry: cos(arg mix - arg tgt) = <mix / |mix|, tgt / |tgt|> as vectors of
// the plane; an operand that is exactly zero has phase 0 (np.angle), i.e. the unit vector (1, 0).
// Divisions are left to IEEE: 0 / 0 is NaN and x / 0 is +-inf as in numpy.  The clips follow
// np.minimum / np.maximum, which hand a NaN on (fminf / fmaxf drop it).
//
// Stored spectra (any T, F): tf_mask_kernel<kind>, tf_apply_kernel -- a thread per cell.
//
// Fused forward (n_fft = 512): tf_forward_kernel<mode, kind>.  A workgroup of 16 quad-rows
// (fft512.h) walks a frame range of one utterance, a quad-row one frame per step.  It transforms
// the signals the mode needs one after the other -- lane la ends up with bins k = la + 16 m and
// 256 - k, m < 8, lane 0 with bins 0, 256 (both real) and 128 -- evaluates the cells on those
// registers and stores the result alone: the mask, the masked spectrum, or the K masked spectra of
// oracle separation.  A target leaves ONE real number per cell behind (|tgt| or |tgt| cos), so
// K + 1 transforms per frame serve K targets.  The input spectra never reach memory.
//
// The statistics compute_mask.py logs (cells over the cutoff, cells below zero, the sum of those):
// the counts are integer atomics; the sum is float64, a lane's cells in their order, the lanes by a
// fixed tree, the waves in their order, ONE slot per workgroup, and tf_fold_kernel adds an
// utterance's slots in slot order.  No floating-point atomics: the same bits in any batch.
#include "common.h"
#include "fft512.h"

namespace setk {

namespace {

constexpr int ROW = 18;
constexpr int SL = slot_entries(ROW);
constexpr float kEps = 1.1920928955078125e-07f;  // np.finfo(np.float32).eps, the reference's EPSILON

// ---------------------------------------------------------------- cell arithmetic
SETK_DEV float cabs32(cf z) { return sqrtf(z.x * z.x + z.y * z.y); }
// np.minimum / np.maximum
SETK_DEV float np_min(float a, float b) { return (a < b || a != a) ? a : b; }
SETK_DEV float np_max(float a, float b) { return (a > b || a != a) ? a : b; }
SETK_DEV bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// cos(np.angle(mix) - np.angle(tgt)), ma = |mix|, ta = |tgt|
SETK_DEV float cos_between(cf mix, float ma, cf tgt, float ta) {
    const cf um = ma == 0.f ? make_float2(1.f, 0.f) : make_float2(mix.x / ma, mix.y / ma);
    const cf ut = ta == 0.f ? make_float2(1.f, 0.f) : make_float2(tgt.x / ta, tgt.y / ta);
    return um.x * ut.x + um.y * ut.y;
}

// compute_mask.py:77-107 but crm
template <int KIND>
SETK_DEV float mask_cell(cf tgt, cf mix) {
    const float ta = cabs32(tgt);
    if constexpr (KIND == kTfIbm || KIND == kTfIrm) {
        const float ia = cabs32(csub(mix, tgt));
        if constexpr (KIND == kTfIbm) return ta > ia ? 1.f : 0.f;
        return ta / sqrtf(ta * ta + ia * ia + kEps);
    } else {
        const float ma = cabs32(mix);
        if constexpr (KIND == kTfIam) return ta / ma;
        const float c = cos_between(mix, ma, tgt, ta);
        if constexpr (KIND == kTfPsm) return ta * c / ma;
        return ta * np_max(0.f, c);  // psa
    }
}

// K (1 - e^{-C x}) / (1 + e^{-C x}), K = 10, C = 0.1, by the branch of the sign as :40-56 has it;
// 1 - e through expm1f, which keeps the small arguments' digits
SETK_DEV float crm_squash(float x) {
    if (x >= 0.f) {
        const float d = expm1f(-0.1f * x);  // e - 1
        return 10.f * -d / (2.f + d);
    }
    const float d = expm1f(0.1f * x);  // (a NaN comes this way, as in the reference)
    return 10.f * d / (2.f + d);
}

// tgt / (mix + eps) as numpy divides complex64 (Smith's form), both parts squashed
SETK_DEV cf crm_cell(cf tgt, cf mix) {
    const cf b = make_float2(mix.x + kEps, mix.y);
    cf q;
    if (fabsf(b.x) >= fabsf(b.y)) {
        if (b.x == 0.f && b.y == 0.f) {
            q = make_float2(tgt.x / fabsf(b.x), tgt.y / fabsf(b.y));
        } else {
            const float rat = b.y / b.x, scl = 1.f / (b.x + b.y * rat);
            q = make_float2((tgt.x + tgt.y * rat) * scl, (tgt.y - tgt.x * rat) * scl);
        }
    } else {
        const float rat = b.x / b.y, scl = 1.f / (b.y + b.x * rat);
        q = make_float2((tgt.x * rat + tgt.y) * scl, (tgt.y * rat - tgt.x) * scl);
    }
    return make_float2(crm_squash(q.x), crm_squash(q.y));
}

// run() :136-152: min(mask, cutoff) when cutoff > 0, then max(mask, 0), and what it logs
struct ClipAcc {
    unsigned over = 0, below = 0;
    double sum = 0.0;
    bool bad = false;
};
SETK_DEV float clip_cell(float m, float cutoff, ClipAcc& acc) {
    if (cutoff != cutoff) {  // NaN: the mask as compute_mask() returns it, no clip, nothing counted
        acc.bad |= nonfinite(m);
        return m;
    }
    if (cutoff > 0.f) {
        if (m > cutoff) ++acc.over;
        m = np_min(m, cutoff);
    }
    if (m < 0.f) {
        ++acc.below;
        acc.sum += (double)m;
    }
    m = np_max(m, 0.f);
    acc.bad |= nonfinite(m);
    return m;
}

// the workgroup's statistics: lanes by a fixed tree, waves in their order, one slot
SETK_DEV void fold_stats(ClipAcc acc, unsigned long long* counts, double* slot, int* status, double* red_sum,
                         unsigned* red_cnt, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc.over += __shfl_xor(acc.over, o);
        acc.below += __shfl_xor(acc.below, o);
        acc.sum += __shfl_xor(acc.sum, o);
    }
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        red_sum[wave] = acc.sum;
        red_cnt[2 * wave] = acc.over;
        red_cnt[2 * wave + 1] = acc.below;
    }
    if (acc.bad && status) atomicMax(status, 3);  // SETK_NUM_NONFINITE
    __syncthreads();
    if (tid == 0) {
        double s = red_sum[0];
        unsigned long long ov = red_cnt[0], be = red_cnt[1];
        for (int w = 1; w < 4; ++w) {
            s += red_sum[w];
            ov += red_cnt[2 * w];
            be += red_cnt[2 * w + 1];
        }
        *slot = s;
        if (ov) atomicAdd(counts, ov);
        if (be) atomicAdd(counts + 1, be);
    }
}

// ---------------------------------------------------------------- stored spectra
template <int KIND>
__global__ __launch_bounds__(256) void tf_mask_kernel(const float2* __restrict__ tgt, const float2* __restrict__ mix,
                                                      size_t cells, int F, float cutoff, float* __restrict__ mask,
                                                      unsigned long long* counts, double* slots, int* status) {
    __shared__ double red_sum[4];
    __shared__ unsigned red_cnt[8];
    const int tid = threadIdx.x;
    ClipAcc acc;
    const size_t base = (size_t)blockIdx.x * kTfChunk;
#pragma unroll 1
    for (int i = 0; i < kTfChunk / 256; ++i) {
        const size_t idx = base + (size_t)i * 256 + tid;
        if (idx >= cells) break;
        const cf a = tgt[idx], b = mix[idx];
        if constexpr (KIND == kTfCrm) {
            const cf m = crm_cell(a, b);
            const size_t t = idx / (size_t)F, f = idx - t * (size_t)F;
            mask[t * 2 * F + f] = clip_cell(m.x, cutoff, acc);
            mask[t * 2 * F + F + f] = clip_cell(m.y, cutoff, acc);
        } else {
            mask[idx] = clip_cell(mask_cell<KIND>(a, b), cutoff, acc);
        }
    }
    fold_stats(acc, counts, slots + blockIdx.x, status, red_sum, red_cnt, tid);
}

__global__ __launch_bounds__(64) void tf_fold_kernel(const TfFold* __restrict__ jobs, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const TfFold j = jobs[i];
    double s = 0.0;
    for (int k = 0; k < j.nslots; ++k) s += j.slots[k];
    TfStats st;
    st.over = (long long)j.counts[0];
    st.below = (long long)j.counts[1];
    st.below_sum = s;
    *j.out = st;
}

// wav_separate.py:63-74: spec x mask, or |spec| x mask x exp(i angle(ref))
__global__ __launch_bounds__(256) void tf_apply_kernel(const float2* __restrict__ spec, const float* __restrict__ mask,
                                                       const float2* __restrict__ ref, size_t cells,
                                                       float2* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= cells) return;
    const cf x = spec[idx];
    const float m = mask[idx];
    if (ref) {
        const float am = cabs32(x) * m;
        const cf p = phasor(ref[idx]);
        out[idx] = make_float2(am * p.x, am * p.y);
    } else {
        out[idx] = make_float2(x.x * m, x.y * m);
    }
}

// ---------------------------------------------------------------- fused forward
// One real 512-point transform on a quad-row, the spectrum left in registers: X[m] = bin
// la + 16 m, X[8 + m] = bin 256 - (la + 16 m); lane 0: X[0] = (Re bin 0, Re bin 256), X[8] = bin 128.
template <bool PCM>
SETK_DEV void qr_spectrum(cf (&X)[16], const void* audio, int n_samp, int s, bool valid, cf* slot, const cf* win_row,
                          const cf* tw_row, const cf* tw5_row, int la) {
    cf v[16];
    if constexpr (PCM) {
        int raw[16];
        load_raw_pcm(raw, (gcshort_p) static_cast<const short*>(audio), n_samp, s, la, valid);
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = unpack_pcm(raw[j]);  // (integers as floats; the window carries 2^-15)
    } else {
        load_raw(v, (gcfloat_p) static_cast<const float*>(audio), n_samp, s, la, valid);
    }
    apply_window<ROW>(v, win_row);
    fft256_stage_a_pad<-1, ROW>(v, slot, tw_row, la);
    __builtin_amdgcn_wave_barrier();
    fft256_stage_b_pad<-1, ROW>(v, slot, la);  // v[pos(kb)] = Z[la + 16 kb]
    __builtin_amdgcn_wave_barrier();           // (the next signal's stage one writes this slot)
    cf t5[8];
    lds_row<8, true>(tw5_row, t5);
    const bool lane0 = la == 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const cf Zk = v[dft16_pos(m)];
        const cf oth = v[dft16_pos(15 - m)];
        const cf own = v[dft16_pos((16 - m) & 15)];
        cf Zm = make_float2(qr_partner(oth.x), qr_partner(oth.y));
        Zm = make_float2(lane0 ? own.x : Zm.x, lane0 ? own.y : Zm.y);
        cf Xk, Xm;
        rfft_split(Zk, Zm, t5[m], Xk, Xm);
        if (m == 0) {
            const cf Z128 = v[dft16_pos(8)];
            const cf x0 = make_float2(Xk.x, Xm.x);
            const cf x128 = make_float2(2.f * Z128.x, -2.f * Z128.y);
            Xk = make_float2(lane0 ? x0.x : Xk.x, lane0 ? x0.y : Xk.y);
            Xm = make_float2(lane0 ? x128.x : Xm.x, lane0 ? x128.y : Xm.y);
        }
        X[m] = Xk;
        X[8 + m] = Xm;
    }
}

// The 17 cells of a lane: c < 16 its registers, c = 16 bin 256 (lane 0 alone).
SETK_DEV int cell_bin(int la, int c) {
    if (c == 16) return 256;
    if (c < 8) return la + 16 * c;
    const int k = la + 16 * (c - 8);
    return k == 0 ? 128 : 256 - k;
}
SETK_DEV cf cell_value(const cf (&X)[16], int la, int c) {
    if (c == 16) return make_float2(X[0].y, 0.f);
    if (c == 0) return make_float2(X[0].x, la == 0 ? 0.f : X[0].y);
    return X[c];
}

struct TfShared {
    __attribute__((aligned(16))) cf slots[16 * SL];
    __attribute__((aligned(16))) cf tabs[table_entries(ROW)];
    double red_sum[4];
    unsigned red_cnt[8];
};

template <int MODE, int KIND, bool PCM>
SETK_DEV void tf_forward_body(const TfFwdArgs& a, TfShared& sh) {
    constexpr int F = kBins;
    constexpr int NC = 17;
    cf* slots = sh.slots;
    cf* tabs = sh.tabs;
    double* red_sum = sh.red_sum;
    unsigned* red_cnt = sh.red_cnt;
    const int tid = threadIdx.x, la = tid & 15, g = tid >> 4;
    cf* win_l = tabs;
    cf* tw_l = win_l + LaneTab<ROW>::size;
    cf* tw5_l = tw_l + LaneTab<ROW>::size;
    fill_lane_tables<ROW>(win_l, tw_l, tw5_l, a.window, a.tw256, a.tw512, tid, 256);
    __syncthreads();
    const WorkItem wi = a.items[blockIdx.x];
    const TfUtt* ud = a.utts + wi.utt;
    const int n_samp = ud->num_samples;
    const void* mix_p = ud->mix;
    cf* slot = slots + g * SL;
    const cf* win_row = win_l + la * LaneTab<ROW>::lstride;
    const cf* tw_row = tw_l + la * LaneTab<ROW>::lstride;
    const cf* tw5_row = tw5_l + la * LaneTab<ROW>::lstride5;
    const int K = MODE == kTfModeOracle ? a.num_targets : 1;
    ClipAcc acc;
    bool bad = false;

#pragma unroll 1
    for (int tb = wi.t0; tb < wi.t1; tb += 16) {
        const int t = tb + g;
        const bool valid = t < wi.t1;
        const int s = t * a.g.hop - a.g.pad;
        cf M[16];
        qr_spectrum<PCM>(M, mix_p, n_samp, s, valid, slot, win_row, tw_row, tw5_row, la);

        if constexpr (MODE == kTfModeMask) {
            cf T[16];
            qr_spectrum<PCM>(T, ud->aux[0], n_samp, s, valid, slot, win_row, tw_row, tw5_row, la);
            float* out = static_cast<float*>(ud->out[0]);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bool live = valid && (c < 16 || la == 0);
                if (!live) continue;
                const int k = cell_bin(la, c);
                const cf tg = cell_value(T, la, c), mx = cell_value(M, la, c);
                if constexpr (KIND == kTfCrm) {
                    const cf m = crm_cell(tg, mx);
                    out[(size_t)t * 2 * F + k] = clip_cell(m.x, a.cutoff, acc);
                    out[(size_t)t * 2 * F + F + k] = clip_cell(m.y, a.cutoff, acc);
                } else {
                    out[(size_t)t * F + k] = clip_cell(mask_cell<KIND>(tg, mx), a.cutoff, acc);
                }
            }
        } else if constexpr (MODE == kTfModeSeparate) {
            const void* ref_p = ud->aux[0];  // (uniform over the workgroup)
            cf R[16];
            if (ref_p) qr_spectrum<PCM>(R, ref_p, n_samp, s, valid, slot, win_row, tw_row, tw5_row, la);
            float2* out = static_cast<float2*>(ud->out[0]);
            const float* mask = ud->mask;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bool live = valid && (c < 16 || la == 0);
                if (!live) continue;
                const int k = cell_bin(la, c);
                const cf mx = cell_value(M, la, c);
                const float m = mask[(size_t)t * F + k];
                cf y;
                if (ref_p) {
                    const float am = cabs32(mx) * m;
                    const cf p = phasor(cell_value(R, la, c));
                    y = make_float2(am * p.x, am * p.y);
                } else {
                    y = make_float2(mx.x * m, mx.y * m);
                }
                bad |= nonfinite(y.x) | nonfinite(y.y);
                out[(size_t)t * F + k] = y;
            }
        } else {
            // oracle_separate.py:19-45: one real number per target and cell
            float r[kTfMaxTargets][NC];
            float ma[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) ma[c] = cabs32(cell_value(M, la, c));
#pragma unroll
            for (int j = 0; j < kTfMaxTargets; ++j) {
                if (j < K) {
                    cf T[16];
                    qr_spectrum<PCM>(T, ud->aux[j], n_samp, s, valid, slot, win_row, tw_row, tw5_row, la);
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const cf tg = cell_value(T, la, c);
                        const float ta = cabs32(tg);
                        r[j][c] = KIND == kTfPsm ? ta * cos_between(cell_value(M, la, c), ma[c], tg, ta) : ta;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < NC; ++c) r[j][c] = 0.f;
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bool live = valid && (c < 16 || la == 0);
                if (!live) continue;
                const int k = cell_bin(la, c);
                const cf mx = cell_value(M, la, c);
                float den = ma[c] + kEps;
                int best = 0;
                if constexpr (KIND == kTfIrm) {
                    float sum = r[0][c];
#pragma unroll
                    for (int j = 1; j < kTfMaxTargets; ++j)
                        if (j < K) sum += r[j][c];
                    den = sum + kEps;
                }
                if constexpr (KIND == kTfIbm) {
                    // np.argmax: the first of equal maxima, a NaN counts as the maximum
                    float bv = r[0][c];
#pragma unroll
                    for (int j = 1; j < kTfMaxTargets; ++j)
                        if (j < K && !(bv != bv) && (r[j][c] > bv || r[j][c] != r[j][c])) {
                            bv = r[j][c];
                            best = j;
                        }
                }
#pragma unroll
                for (int j = 0; j < kTfMaxTargets; ++j) {
                    if (j < K) {
                        const float m = KIND == kTfIbm ? (best == j ? 1.f : 0.f) : r[j][c] / den;
                        const cf y = make_float2(mx.x * m, mx.y * m);
                        bad |= nonfinite(y.x) | nonfinite(y.y);
                        static_cast<float2*>(ud->out[j])[(size_t)t * F + k] = y;
                    }
                }
            }
        }
    }

    if constexpr (MODE == kTfModeMask) {
        fold_stats(acc, ud->counts, a.slots + wi.part, ud->status, red_sum, red_cnt, tid);
    } else {
        if (bad) atomicMax(ud->status, 3);  // SETK_NUM_NONFINITE
    }
}

// Two entry points so that each form takes the registers it needs and no scratch: the mask and
// separation forms hold two spectra while the second is transformed (under 200 registers, two
// waves per SIMD; a three-wave budget was tried and spills 28 of them), the oracle form keeps one
// real number per target and cell (8 x 17) next to the mixture's spectrum (one wave per SIMD).
template <int MODE, int KIND, bool PCM>
__global__ __launch_bounds__(256) void tf_forward_kernel(TfFwdArgs a) {
    __shared__ TfShared sh;
    tf_forward_body<MODE, KIND, PCM>(a, sh);
}
template <int KIND, bool PCM>
__global__ __launch_bounds__(256) void tf_oracle_kernel(TfFwdArgs a) {
    __shared__ TfShared sh;
    tf_forward_body<kTfModeOracle, KIND, PCM>(a, sh);
}

template <int MODE, int KIND>
hipError_t launch_fwd_t(bool pcm16, const TfFwdArgs& a, int n_items, hipStream_t s) {
    if constexpr (MODE == kTfModeOracle) {
        if (pcm16)
            hipLaunchKernelGGL((tf_oracle_kernel<KIND, true>), dim3(n_items), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((tf_oracle_kernel<KIND, false>), dim3(n_items), dim3(256), 0, s, a);
    } else {
        if (pcm16)
            hipLaunchKernelGGL((tf_forward_kernel<MODE, KIND, true>), dim3(n_items), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((tf_forward_kernel<MODE, KIND, false>), dim3(n_items), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tf_mask(int kind, const float* tgt, const float* mix, size_t cells, int F, float cutoff, float* mask,
                          unsigned long long* counts, double* slots, int* status, hipStream_t s) {
    const dim3 grid((unsigned)((cells + kTfChunk - 1) / kTfChunk));
    const float2* t2 = reinterpret_cast<const float2*>(tgt);
    const float2* m2 = reinterpret_cast<const float2*>(mix);
#define SETK_TF_MASK(KIND)                                                                                        \
    case KIND:                                                                                                    \
        hipLaunchKernelGGL((tf_mask_kernel<KIND>), grid, dim3(256), 0, s, t2, m2, cells, F, cutoff, mask, counts, \
                           slots, status);                                                                        \
        break;
    switch (kind) {
        SETK_TF_MASK(kTfIbm)
        SETK_TF_MASK(kTfIrm)
        SETK_TF_MASK(kTfIam)
        SETK_TF_MASK(kTfPsm)
        SETK_TF_MASK(kTfPsa)
        SETK_TF_MASK(kTfCrm)
        default:
            return hipErrorInvalidValue;
    }
#undef SETK_TF_MASK
    return hipGetLastError();
}

hipError_t launch_tf_fold(const TfFold* d_jobs, int n, hipStream_t s) {
    hipLaunchKernelGGL(tf_fold_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_jobs, n);
    return hipGetLastError();
}

hipError_t launch_tf_apply(const float* spec, const float* mask, const float* phase_ref, size_t cells, float* out,
                           hipStream_t s) {
    hipLaunchKernelGGL(tf_apply_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(spec), mask, reinterpret_cast<const float2*>(phase_ref), cells,
                       reinterpret_cast<float2*>(out));
    return hipGetLastError();
}

hipError_t launch_tf_forward(int mode, int kind, bool pcm16, const TfFwdArgs& a, int n_items, hipStream_t s) {
    if (mode == kTfModeSeparate) return launch_fwd_t<kTfModeSeparate, 0>(pcm16, a, n_items, s);
    if (mode == kTfModeMask) {
        switch (kind) {
            case kTfIbm: return launch_fwd_t<kTfModeMask, kTfIbm>(pcm16, a, n_items, s);
            case kTfIrm: return launch_fwd_t<kTfModeMask, kTfIrm>(pcm16, a, n_items, s);
            case kTfIam: return launch_fwd_t<kTfModeMask, kTfIam>(pcm16, a, n_items, s);
            case kTfPsm: return launch_fwd_t<kTfModeMask, kTfPsm>(pcm16, a, n_items, s);
            case kTfPsa: return launch_fwd_t<kTfModeMask, kTfPsa>(pcm16, a, n_items, s);
            case kTfCrm: return launch_fwd_t<kTfModeMask, kTfCrm>(pcm16, a, n_items, s);
        }
    }
    if (mode == kTfModeOracle) {
        switch (kind) {
            case kTfIbm: return launch_fwd_t<kTfModeOracle, kTfIbm>(pcm16, a, n_items, s);
            case kTfIrm: return launch_fwd_t<kTfModeOracle, kTfIrm>(pcm16, a, n_items, s);
            case kTfIam: return launch_fwd_t<kTfModeOracle, kTfIam>(pcm16, a, n_items, s);
            case kTfPsm: return launch_fwd_t<kTfModeOracle, kTfPsm>(pcm16, a, n_items, s);
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace setk
