// capi_cgmm.hip -- front end (include/setk_hip.h): CGMM mask estimation.  Two classes on the
// bin-resident EM (cgmm_bin.hip) or the streaming kernels (cgmm.hip); K classes on cgmm_k.hip.
#include "capi.h"

using namespace setk;

namespace {
// The bin-resident EM (cgmm_bin.hip) when one bin of the longest utterance fits a CU,
// otherwise (or with SETK_CGMM_STREAMING=1) the streaming kernels of cgmm.hip.
bool cgmm_use_bin(int C, int max_frames) {
    static const bool forced_off = [] {
        const char* e = getenv("SETK_CGMM_STREAMING");
        return e && *e && *e != '0';
    }();
    return !forced_off && cgmm_bin_threads(C, max_frames) != 0;
}

// spec / init / mask / gamma: device pointers per utterance (gamma entries may be null)
// spec == NULL: `audio` / `num_samples` are given instead and the spectrograms are computed
// straight into the bin-major layout (stft_binmajor_kernel, n_fft = 512 plan)
int run_cgmm_bin(setk_handle_t h, int C, int n_utts, const float* const* spec, const int* frames,
                 int F, int num_iters, const float* const* init, float* const* mask,
                 float* const* gamma, int flags, int spec_pitch, hipStream_t s,
                 const float* const* audio = nullptr, const int* num_samples = nullptr) {
    const size_t ab = cgmm_bin_args_bytes();
    std::vector<char> tbl((size_t)n_utts * ab);
    std::vector<const float*> sp(n_utts);
    std::vector<float*> mp(n_utts), gp(n_utts), xbs;
    int max_frames = 0;
    const int nout = gamma ? 2 : 1;
    // diagnostic: SETK_CGMM_TIMING=<file> dumps the per-bin cycle counters of utterance 0
    // (best effort: without arena for them the run goes on undiagnosed)
    const char* timing_path = getenv("SETK_CGMM_TIMING");
    void* d_timing = nullptr;
    if (timing_path && *timing_path) {
        d_timing = arena_alloc(h, (size_t)F * cgmm_bin_timing_slots() * sizeof(long long));
        if (d_timing) HIP_TRY(h, hipMemsetAsync(d_timing, 0, (size_t)F * cgmm_bin_timing_slots() * sizeof(long long), s));
    }
    for (int u = 0; u < n_utts; ++u) {
        const int T = frames[u], Tp = cgmm_bin_pitch(T);
        max_frames = std::max(max_frames, T);
        float *xb, *gb;
        SETK_TRY(arena_get(h, (size_t)F * C * Tp * sizeof(float2), &xb));
        SETK_TRY(arena_get(h, (size_t)nout * F * Tp * sizeof(float), &gb));
        cgmm_bin_fill_args(tbl.data() + (size_t)u * ab, xb, init ? init[u] : nullptr, gb, T, F,
                           (flags & SETK_CGMM_UPDATE_ALPHA) ? 1 : 0, nout, u == 0 ? d_timing : nullptr);
        sp[u] = spec ? spec[u] : nullptr;
        xbs.push_back(xb);
        mp[u] = mask[u];
        gp[u] = gamma ? gamma[u] : nullptr;
    }
    const char* d_tbl;
    const float* const* d_sp = nullptr;
    float* const* d_mp;
    float* const* d_gp = nullptr;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    if (spec) {
        SETK_TRY(upload(h, sp, s, &d_sp));
    } else {
        Pass1Args a;
        int n_items;
        SETK_TRY(prepare_stft_binmajor(h, n_utts, audio, num_samples, frames, xbs.data(), s, &a, &n_items));
        HIP_TRY(h, launch_stft_binmajor(C, a, n_items, s));
    }
    SETK_TRY(upload(h, mp, s, &d_mp));
    if (gamma) SETK_TRY(upload(h, gp, s, &d_gp));
    HIP_TRY(h, launch_cgmm_bin(C, d_tbl, d_sp, spec_pitch > 0 ? spec_pitch : F, d_mp, d_gp, n_utts, F,
                               max_frames, num_iters, nout, s));
    if (d_timing) {
        const int ns = cgmm_bin_timing_slots();
        std::vector<long long> tm((size_t)F * ns);
        HIP_TRY(h, hipMemcpyAsync(tm.data(), d_timing, tm.size() * sizeof(long long),
                                  hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        if (FILE* fp = fopen(timing_path, "w")) {
            fprintf(fp, "# bin | 0 frames 1 - 2 barrier 3 solve 4 tail 5 passes 6 nfast0 7 nfast1 | -DSETK_CGMM_PHASES: 8 E0 9 E1 10 P "
                        "11 R-acc 12 R-sum 13 I-acc 14 I-sum | 16 solve:sums 17 scale 18 chol 19 bound 20 logdet 21 exact-path "
                        "(shader cycles of wave 0, summed over passes)\n");
            for (int f = 0; f < F; ++f) {
                fprintf(fp, "%d", f);
                for (int k = 0; k < ns; ++k) fprintf(fp, " %lld", tm[(size_t)f * ns + k]);
                fprintf(fp, "\n");
            }
            fclose(fp);
        }
    }
    return SETK_OK;
}
}  // namespace

extern "C" {

int setk_cgmm_bin_config(int num_channels, int max_frames, int info[3]) {
    if (max_frames <= 0 || !cgmm_use_bin(num_channels, max_frames)) return -1;
    const int cfg = cgmm_bin_config(num_channels, max_frames);
    if (cfg >= 0 && info) cgmm_bin_config_info(cfg, info);
    return cfg;
}

int setk_cgmm_masks_batch(setk_handle_t h, int n_utts, int num_channels,
                          const float* const* spec, const int* num_frames, int num_bins,
                          int num_iters, const float* const* init_mask, float* const* mask_out,
                          int flags, int spec_pitch, void* stream) {
    if (spec_pitch != 0 && spec_pitch < num_bins) return fail(h, SETK_ERR_INVALID, "spec_pitch < F");
    if (!h || n_utts <= 0 || !spec || !num_frames || !mask_out || num_bins <= 0 || num_iters < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    if (num_channels < 1 || num_channels > kMaxChannels)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 8");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const int C = num_channels, F = num_bins;
    const size_t ab = cgmm_args_bytes();
    std::vector<char> tbl((size_t)n_utts * ab);
    int max_frames = 0;
    for (int u = 0; u < n_utts; ++u) {
        if (!spec[u] || !mask_out[u] || num_frames[u] <= 0)
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(spec[u]) || !is_device_ptr(mask_out[u]) ||
            (init_mask && init_mask[u] && !is_device_ptr(init_mask[u])))
            return fail(h, SETK_ERR_INVALID, "setk_cgmm_masks_batch takes device pointers");
        max_frames = std::max(max_frames, num_frames[u]);
    }
    if (cgmm_use_bin(C, max_frames))
        return run_cgmm_bin(h, C, n_utts, spec, num_frames, F, num_iters, init_mask, mask_out,
                            nullptr, flags, spec_pitch, s);
    for (int u = 0; u < n_utts; ++u) {
        const int T = num_frames[u];
        char* scr;
        SETK_TRY(arena_get(h, cgmm_scratch_bytes(C, T, F), &scr));
        cgmm_fill_args(tbl.data() + (size_t)u * ab, C, spec[u], T, F,
                       init_mask ? init_mask[u] : nullptr, nullptr, mask_out[u], scr,
                       (flags & SETK_CGMM_UPDATE_ALPHA) ? 1 : 0, spec_pitch);
    }
    const char* d_tbl;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    HIP_TRY(h, launch_cgmm_batch(C, d_tbl, n_utts, F, max_frames, num_iters, s));
    return SETK_OK;
}

int setk_cgmm_estimate_batch(setk_handle_t h, int n_utts, int num_channels,
                             const float* const* audio, const int* num_samples, int num_iters,
                             const float* const* init_mask, float* const* mask_out, int flags,
                             void* stream) {
    if (!h || n_utts <= 0 || !audio || !num_samples || !mask_out || num_iters < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int C = num_channels;
    if (C < 1 || C > kMaxChannels) return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 8");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    std::vector<int> frames(n_utts);
    int max_frames = 0;
    for (int u = 0; u < n_utts; ++u) {
        if (!audio[u] || !mask_out[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(audio[u]) || !is_device_ptr(mask_out[u]) ||
            (init_mask && init_mask[u] && !is_device_ptr(init_mask[u])))
            return fail(h, SETK_ERR_INVALID, "setk_cgmm_estimate_batch takes device pointers");
        frames[u] = setk_stft_num_frames(h, num_samples[u]);
        if (frames[u] < 0) return frames[u];
        max_frames = std::max(max_frames, frames[u]);
    }
    if (!cgmm_use_bin(C, max_frames))
        return fail(h, SETK_ERR_UNSUPPORTED,
                    "one bin of the longest utterance does not fit a CU: use setk_stft_batch + "
                    "setk_cgmm_masks_batch (streaming kernels)");
    return run_cgmm_bin(h, C, n_utts, nullptr, frames.data(), kBins, num_iters, init_mask, mask_out,
                        nullptr, flags, 0, s, audio, num_samples);
}

int setk_cgmm_masks(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                    int num_bins, int num_iters, const float* init_mask, float* gamma_out,
                    float* mask_out, int flags, void* stream) {
    if (!h || !spec || !mask_out || num_frames <= 0 || num_bins <= 0 || num_iters < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    if (num_channels < 1 || num_channels > kMaxChannels)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 8");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const int C = num_channels, T = num_frames, F = num_bins;
    const float *d_spec, *d_init = nullptr;
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &d_spec));
    if (init_mask) SETK_TRY(stage_in(h, init_mask, (size_t)T * F, s, &d_init));
    OutBuf om, og;
    SETK_TRY(stage_out(h, mask_out, (size_t)T * F * 4, &om));
    float* d_gamma = nullptr;
    if (gamma_out) {
        SETK_TRY(stage_out(h, gamma_out, (size_t)2 * T * F * 4, &og));
        d_gamma = static_cast<float*>(og.dev);
    }
    if (cgmm_use_bin(C, T)) {
        float* mo = static_cast<float*>(om.dev);
        SETK_TRY(run_cgmm_bin(h, C, 1, &d_spec, &T, F, num_iters, d_init ? &d_init : nullptr, &mo,
                              d_gamma ? &d_gamma : nullptr, flags, 0, s));
    } else {
        char* d_scr;
        SETK_TRY(arena_get(h, cgmm_scratch_bytes(C, T, F), &d_scr));
        std::vector<char> tbl(cgmm_args_bytes());
        cgmm_fill_args(tbl.data(), C, d_spec, T, F, d_init, d_gamma, static_cast<float*>(om.dev),
                       d_scr, (flags & SETK_CGMM_UPDATE_ALPHA) ? 1 : 0, 0);
        const char* d_tbl;
        SETK_TRY(upload(h, tbl, s, &d_tbl));
        HIP_TRY(h, launch_cgmm_batch(C, d_tbl, 1, F, T, num_iters, s));
    }
    SETK_TRY(copy_back(h, om, s));
    if (gamma_out) SETK_TRY(copy_back(h, og, s));
    if (om.host || (gamma_out && og.host)) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_cgmm_masks_k(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                      int num_bins, int num_classes, int num_iters, const double* gamma0,
                      const float* init_mask, float* gamma_out, int flags, void* stream) {
    return setk_cgmm_masks_k_status(h, spec, num_channels, num_frames, num_bins, num_classes, num_iters,
                                    gamma0, init_mask, gamma_out, flags, nullptr, stream);
}

int setk_cgmm_masks_k_status(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                             int num_bins, int num_classes, int num_iters, const double* gamma0,
                             const float* init_mask, float* gamma_out, int flags, int* status,
                             void* stream) {
    if (!h || !spec || !gamma_out || num_frames <= 0 || num_bins <= 0 || num_iters < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    const int C = num_channels, T = num_frames, F = num_bins, K = num_classes;
    if (!cgmm_k_supported(C, K))
        return fail(h, SETK_ERR_UNSUPPORTED, "general CGMM: 1 <= num_channels <= 16, 2 <= num_classes <= 4");
    if (K != 2 && !gamma0) return fail(h, SETK_ERR_INVALID, "num_classes > 2 needs the start gamma0");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const float *d_spec, *d_init = nullptr, *d_g0f = nullptr;
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &d_spec));
    if (gamma0)  // (stage_in counts floats: a double is two)
        SETK_TRY(stage_in(h, reinterpret_cast<const float*>(gamma0), (size_t)K * F * T * 2, s, &d_g0f));
    else if (init_mask)
        SETK_TRY(stage_in(h, init_mask, (size_t)T * F, s, &d_init));
    OutBuf og;
    SETK_TRY(stage_out(h, gamma_out, (size_t)K * T * F * 4, &og));
    double* d_work;
    SETK_TRY(arena_get(h, cgmm_k_work_bytes(K, T, F), &d_work));
    OutBuf os;
    if (status) {
        SETK_TRY(stage_out(h, status, (size_t)F * sizeof(int), &os));
        HIP_TRY(h, hipMemsetAsync(os.dev, 0, (size_t)F * sizeof(int), s));
    }
    HIP_TRY(h, launch_cgmm_k(d_spec, reinterpret_cast<const double*>(d_g0f), d_init, static_cast<float*>(og.dev),
                             d_work, status ? static_cast<int*>(os.dev) : nullptr, C, T, F, K, num_iters,
                             (flags & SETK_CGMM_UPDATE_ALPHA) ? 1 : 0, s));
    SETK_TRY(copy_back(h, og, s));
    if (status) SETK_TRY(copy_back(h, os, s));
    if (og.host || (status && os.host)) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
