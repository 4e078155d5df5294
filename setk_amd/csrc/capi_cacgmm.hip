// capi_cacgmm.hip -- front end (include/setk_hip.h): CACGMM mask estimation (cacgmm.hip) on a
// spectrogram, and on batches of waveforms with the STFT in front.
#include "capi.h"

using namespace setk;

namespace {
struct CacgUtt {
    const float* x_bin;    // [F][C][Tp] complex64 (device)
    const double* gamma0;  // [K][F][T] (device) or null
    float* gamma_out;      // [K][T][F] (device)
    int T;
};

// read at call time, so that one process can compare the two forms
bool cacgmm_force_streaming() {
    const char* e = getenv("SETK_CACGMM_STREAMING");
    return e && *e && *e != '0';
}

int check_cacgmm(setk_handle_t h, int C, int K, int flags, bool have_gamma0) {
    if (!cacgmm_supported(C, K)) return fail(h, SETK_ERR_UNSUPPORTED, cacgmm_limit_message());
    if (flags & ~(SETK_CACGMM_UPDATE_ALPHA | SETK_CACGMM_CGMM_INIT))
        return fail(h, SETK_ERR_INVALID, "unknown CACGMM flag");
    if (flags & SETK_CACGMM_CGMM_INIT) {
        if (K != 2 || have_gamma0)
            return fail(h, SETK_ERR_INVALID, "SETK_CACGMM_CGMM_INIT needs num_classes = 2 and gamma0 = NULL");
    } else if (!have_gamma0) {
        return fail(h, SETK_ERR_INVALID, "gamma0 is NULL: the caller draws the start (or SETK_CACGMM_CGMM_INIT)");
    }
    return SETK_OK;
}

// The EM of every (bin, utterance) in one launch; leaves the per-bin status in d_st [n_utts][F].
int cacgmm_run(setk_handle_t h, int C, int F, int K, int num_iters, int flags,
               const std::vector<CacgUtt>& us, int** d_st_out, hipStream_t s) {
    const int n_utts = (int)us.size();
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_utts * F * sizeof(int), &d_st));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, (size_t)n_utts * F * sizeof(int), s));
    const size_t ab = cacgmm_args_bytes();
    std::vector<char> tbl((size_t)n_utts * ab);
    int max_frames = 0;
    for (int u = 0; u < n_utts; ++u) {
        const CacgUtt& q = us[u];
        max_frames = std::max(max_frames, q.T);
        double* work;
        SETK_TRY(arena_get(h, cacgmm_work_bytes(K, q.T, F), &work));
        cacgmm_fill_args(tbl.data() + (size_t)u * ab, q.x_bin, q.gamma0, q.gamma_out, work,
                         d_st + (size_t)u * F, q.T);
    }
    const char* d_tbl;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    HIP_TRY(h, launch_cacgmm(d_tbl, n_utts, C, F, K, num_iters, flags,
                             cacgmm_resident_frames(C, max_frames, cacgmm_force_streaming()), s));
    *d_st_out = d_st;
    return SETK_OK;
}
}  // namespace

extern "C" {

int setk_cacgmm_masks(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                      int num_bins, int num_classes, int num_iters, const double* gamma0, int flags,
                      float* gamma_out, int* status, void* stream) {
    if (!h || !spec || !gamma_out || num_frames <= 0 || num_bins <= 0 || num_iters < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    const int C = num_channels, T = num_frames, F = num_bins, K = num_classes;
    SETK_TRY(check_cacgmm(h, C, K, flags, gamma0 != nullptr));
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const float *d_spec, *d_g0f = nullptr;
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &d_spec));
    if (gamma0)  // (stage_in counts floats: a double is two)
        SETK_TRY(stage_in(h, reinterpret_cast<const float*>(gamma0), (size_t)K * F * T * 2, s, &d_g0f));
    OutBuf og;
    SETK_TRY(stage_out(h, gamma_out, (size_t)K * T * F * sizeof(float), &og));
    float* xb;
    SETK_TRY(arena_get(h, (size_t)F * C * cacgmm_pitch(T) * sizeof(float2), &xb));
    HIP_TRY(h, launch_auxiva_transpose(d_spec, C, T, F, cacgmm_pitch(T), xb, true, s));
    std::vector<CacgUtt> us(1);
    us[0].x_bin = xb;
    us[0].gamma0 = reinterpret_cast<const double*>(d_g0f);
    us[0].gamma_out = static_cast<float*>(og.dev);
    us[0].T = T;
    int* d_st = nullptr;
    SETK_TRY(cacgmm_run(h, C, F, K, num_iters, flags, us, &d_st, s));
    SETK_TRY(copy_back(h, og, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)F * sizeof(int), s, nullptr));
    // staged buffers and the work area live in the arena: drained before the next call reuses it
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_cacgmm_estimate_batch(setk_handle_t h, int n_utts, int num_channels,
                               const float* const* audio, const int* num_samples, int num_classes,
                               int num_iters, const double* const* gamma0, int flags,
                               float* const* gamma_out, int* status, void* stream) {
    if (!h || n_utts <= 0 || !audio || !num_samples || !gamma_out || num_iters < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int C = num_channels, F = kBins, K = num_classes;
    SETK_TRY(check_cacgmm(h, C, K, flags, gamma0 != nullptr));
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    std::vector<CacgUtt> us(n_utts);
    std::vector<int> frames(n_utts);
    std::vector<float*> xbs(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        if (!audio[u] || !gamma_out[u] || (gamma0 && !gamma0[u]))
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(audio[u]) || !is_device_ptr(gamma_out[u]) || (gamma0 && !is_device_ptr(gamma0[u])))
            return fail(h, SETK_ERR_INVALID, "setk_cacgmm_estimate_batch takes device pointers");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T <= 0) return T < 0 ? T : fail(h, SETK_ERR_INVALID, "utterance shorter than a frame");
        frames[u] = us[u].T = T;
        SETK_TRY(arena_get(h, (size_t)F * C * cacgmm_pitch(T) * sizeof(float2), &xbs[u]));
        us[u].x_bin = xbs[u];
        us[u].gamma0 = gamma0 ? gamma0[u] : nullptr;
        us[u].gamma_out = gamma_out[u];
    }
    SETK_TRY(profile_begin(h, s));
    Pass1Args a;
    int n_items;
    SETK_TRY(prepare_stft_binmajor(h, n_utts, audio, num_samples, frames.data(), xbs.data(), s, &a, &n_items));
    HIP_TRY(h, launch_stft_binmajor(C, a, n_items, s));
    SETK_TRY(profile_mark(h, 1, s));
    int* d_st = nullptr;
    SETK_TRY(cacgmm_run(h, C, F, K, num_iters, flags, us, &d_st, s));
    for (int i = 2; i <= 4; ++i) SETK_TRY(profile_mark(h, i, s));  // (stages: STFT, EM, -, -)
    // worst bin of every utterance (host memory: the call drains)
    if (status) {
        std::vector<int> st((size_t)n_utts * F), worst(n_utts, 0);
        HIP_TRY(h, hipMemcpyAsync(st.data(), d_st, st.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        for (int u = 0; u < n_utts; ++u)
            for (int f = 0; f < F; ++f) worst[u] = std::max(worst[u], st[(size_t)u * F + f]);
        SETK_TRY(put_result(h, status, worst.data(), (size_t)n_utts * sizeof(int)));
    }
    return SETK_OK;
}

}  // extern "C"
