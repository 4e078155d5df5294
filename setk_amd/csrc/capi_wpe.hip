// capi_wpe.hip -- front end (include/setk_hip.h): WPE dereverberation (wpe.hip).
// wpe_step (libs/wpe.py:58-81) `num_iters` times.  lambda of iteration 0 comes from
// `lambda_enh` (facted_wpd: |previous enhanced|^2) when given, else from
// compute_lambda(spec); later iterations use compute_lambda(dereverb).
#include "capi.h"

using namespace setk;

namespace {
// n_utts utterances of the same channel count per call: one wpe_step launch per
// iteration covers every (bin, utterance).  lambda_enh / inv_lambda_out: per-utterance arrays
// (facted_wpd) or NULL; lambda_ft only with n_utts == 1 (wpe_step).  status: [n_utts][F] (host
// or device) or NULL.
// fnt: spec / out are in the reference's own layout, F x N x T (libs/wpe.py:84-110) -- which is
// the layout the step kernel works in, so the two transposes fall away
int wpe_batch_impl(setk_handle_t h, int n_utts, const float* const* spec, int num_channels,
                   const int* num_frames, int num_bins, int taps, int delay, int context,
                   int num_iters, const float* const* lambda_enh, const double* lambda_ft,
                   float* const* out, float* const* inv_lambda_out, int* status, void* stream,
                   bool fnt = false) {
    if (!h || n_utts <= 0 || !spec || !out || !num_frames || num_bins <= 0 || num_iters <= 0 ||
        delay < 0 || context < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    if (lambda_ft && n_utts != 1)
        return fail(h, SETK_ERR_INVALID, "caller-supplied variances (wpe_step) need n_utts == 1");
    const int C = num_channels, F = num_bins;
    if (!wpe_supported(C, taps))
        return fail(h, SETK_ERR_UNSUPPORTED, wpe_limit_message(C, taps));
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    struct Utt {
        const float* d_spec;
        OutBuf ob;
        float *x_fct, *bufs[2];
        double* lam;
        const float* d_enh;
        OutBuf ob_il;
        int T;
    };
    std::vector<Utt> us(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        Utt& q = us[u];
        q.T = num_frames[u];
        if (!spec[u] || !out[u] || q.T <= 0) return fail(h, SETK_ERR_INVALID, "null utterance");
        const size_t n = (size_t)C * q.T * F;
        SETK_TRY(stage_in(h, spec[u], n * 2, s, &q.d_spec));
        SETK_TRY(stage_out(h, out[u], n * sizeof(float2), &q.ob));
        if (fnt)
            q.x_fct = const_cast<float*>(q.d_spec);
        else
            SETK_TRY(arena_get(h, n * sizeof(float2), &q.x_fct));
        SETK_TRY(arena_get(h, n * sizeof(float2), &q.bufs[0]));
        SETK_TRY(arena_get(h, n * sizeof(float2), &q.bufs[1]));
        SETK_TRY(arena_get(h, (size_t)q.T * F * sizeof(double), &q.lam));
        // F x N x T in and out: the last iteration writes the caller's (or its staged) output
        if (fnt) q.bufs[(num_iters - 1) & 1] = static_cast<float*>(q.ob.dev);
        q.d_enh = nullptr;
        if (lambda_enh && lambda_enh[u])
            SETK_TRY(stage_in(h, lambda_enh[u], (size_t)q.T * F * 2, s, &q.d_enh));
        if (inv_lambda_out) {
            if (!inv_lambda_out[u]) return fail(h, SETK_ERR_INVALID, "null inv_lambda_out entry");
            SETK_TRY(stage_out(h, inv_lambda_out[u], (size_t)q.T * F * sizeof(float), &q.ob_il));
        }
    }
    const double* d_lam_in = nullptr;
    if (lambda_ft) SETK_TRY(stage_in(h, lambda_ft, (size_t)us[0].T * F, s, &d_lam_in));
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_utts * F * sizeof(int) * (size_t)num_iters, &d_st));
    if (!fnt)
        for (int u = 0; u < n_utts; ++u)
            HIP_TRY(h, launch_wpe_transpose(us[u].d_spec, C, us[u].T, F, us[u].x_fct, true, s));
    const size_t ab = wpe_args_bytes();
    std::vector<char> tbl((size_t)n_utts * ab);
    // SETK_WPE_TIMING=<file>: in-kernel cycle counters of the LAST iteration, [n_utts][F][4]
    // int64 (correlation, factorisation, back substitution, filter)
    const char* timing_path = getenv("SETK_WPE_TIMING");
    long long* d_timing = nullptr;
    if (timing_path && *timing_path)
        SETK_TRY(arena_get(h, (size_t)n_utts * F * 4 * sizeof(long long), &d_timing));
    // channels x taps beyond LDS: R in global scratch, [F][NK][NK] complex128 per utterance of a
    // launch; the launches of an iteration then cover as many utterances as ~2 GB of it hold
    const size_t wide_utt = wpe_wide_bytes_per_bin(C, taps) * (size_t)F;
    int per_launch = n_utts;
    char* d_rwork = nullptr;
    if (wide_utt) {
        per_launch = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_utts, ((size_t)2 << 30) / wide_utt));
        SETK_TRY(arena_get(h, wide_utt * per_launch, &d_rwork));
    }
    for (int it = 0; it < num_iters; ++it) {
        for (int u = 0; u < n_utts; ++u) {
            Utt& q = us[u];
            const float* cur = it == 0 ? q.x_fct : q.bufs[(it - 1) & 1];
            if (it == 0 && d_lam_in)
                // wpe_step (libs/wpe.py:58-81): the caller's variances as given, F x T float64
                HIP_TRY(h, hipMemcpyAsync(q.lam, d_lam_in, (size_t)q.T * F * sizeof(double),
                                          hipMemcpyDeviceToDevice, s));
            else if (it == 0 && q.d_enh)
                HIP_TRY(h, launch_wpe_lambda_from_enh(q.d_enh, q.T, F, q.lam, s));
            else
                HIP_TRY(h, launch_wpe_lambda(cur, C, q.T, F, context, q.lam, s));
            wpe_fill_args(tbl.data() + (size_t)u * ab, q.x_fct, q.lam, q.bufs[it & 1],
                          d_st + ((size_t)it * n_utts + u) * F, C, q.T, taps, delay,
                          d_timing ? d_timing + (size_t)u * F * 4 : nullptr,
                          d_rwork ? d_rwork + wide_utt * (size_t)(u % per_launch) : nullptr);
        }
        const char* d_tbl;
        SETK_TRY(upload(h, tbl, s, &d_tbl));
        for (int u0 = 0; u0 < n_utts; u0 += per_launch)
            HIP_TRY(h, launch_wpe_step_batch(d_tbl + (size_t)u0 * ab, std::min(per_launch, n_utts - u0), C, F,
                                             taps, s));
    }
    for (int u = 0; u < n_utts; ++u) {
        Utt& q = us[u];
        if (!fnt)
            HIP_TRY(h, launch_wpe_transpose(q.bufs[(num_iters - 1) & 1], C, q.T, F,
                                            static_cast<float*>(q.ob.dev), false, s));
        SETK_TRY(copy_back(h, q.ob, s));
        if (inv_lambda_out) {
            HIP_TRY(h, launch_wpe_inv_lambda(q.lam, q.T, F, static_cast<float*>(q.ob_il.dev), s));
            SETK_TRY(copy_back(h, q.ob_il, s));
        }
    }
    if (status) {
        // worst status over the iterations, per utterance and bin: an error code (1..3) wins
        // over the SETK_NUM_RANKDEF note (4)
        std::vector<int> st((size_t)n_utts * F * num_iters);
        HIP_TRY(h, hipMemcpyAsync(st.data(), d_st, st.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        std::vector<int> worst((size_t)n_utts * F, 0);
        for (int it = 0; it < num_iters; ++it)
            for (size_t i = 0; i < worst.size(); ++i) {
                const int v = st[(size_t)it * n_utts * F + i], w0 = worst[i];
                const bool ev = v > 0 && v != SETK_NUM_RANKDEF, ew = w0 > 0 && w0 != SETK_NUM_RANKDEF;
                worst[i] = (ev && ew) ? std::max(v, w0) : ev ? v : ew ? w0 : std::max(v, w0);
            }
        SETK_TRY(put_result(h, status, worst.data(), worst.size() * sizeof(int)));
    }
    // descriptors and staged buffers live in the arena: drained before the next call reuses it
    HIP_TRY(h, hipStreamSynchronize(s));
    if (d_timing) {
        std::vector<long long> tm((size_t)n_utts * F * 4);
        HIP_TRY(h, hipMemcpy(tm.data(), d_timing, tm.size() * sizeof(long long), hipMemcpyDeviceToHost));
        if (FILE* fp = fopen(timing_path, "wb")) {
            fwrite(tm.data(), sizeof(long long), tm.size(), fp);
            fclose(fp);
        }
    }
    return SETK_OK;
}
}  // namespace

extern "C" {

int setk_wpe_form(int num_channels, int taps, int* wide, int* tiles_per_wave, int* chunk_frames) {
    if (!wpe_supported(num_channels, taps)) return SETK_ERR_UNSUPPORTED;
    wpe_form(num_channels, taps, wide, tiles_per_wave, chunk_frames);
    return SETK_OK;
}

int setk_wpe(setk_handle_t h, const float* spec, int num_channels, int num_frames, int num_bins,
             int taps, int delay, int context, int num_iters, const float* lambda_enh,
             float* out, float* inv_lambda_out, int* status, void* stream) {
    return wpe_batch_impl(h, 1, &spec, num_channels, &num_frames, num_bins, taps, delay, context,
                          num_iters, lambda_enh ? &lambda_enh : nullptr, nullptr, &out,
                          inv_lambda_out ? &inv_lambda_out : nullptr, status, stream);
}

int setk_wpe_batch_var(setk_handle_t h, int n_utts, const float* const* spec, int num_channels,
                       const int* num_frames, int num_bins, int taps, int delay, int context,
                       int num_iters, const float* const* lambda_enh, float* const* out,
                       float* const* inv_lambda_out, int* status, void* stream) {
    return wpe_batch_impl(h, n_utts, spec, num_channels, num_frames, num_bins, taps, delay, context,
                          num_iters, lambda_enh, nullptr, out, inv_lambda_out, status, stream);
}

int setk_wpe_step(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                  int num_bins, int taps, int delay, const double* lambda_ft, float* out,
                  int* status, void* stream) {
    if (!lambda_ft) return fail(h, SETK_ERR_INVALID, "setk_wpe_step needs lambda");
    return wpe_batch_impl(h, 1, &spec, num_channels, &num_frames, num_bins, taps, delay, 0, 1,
                          nullptr, lambda_ft, &out, nullptr, status, stream);
}

int setk_wpe_batch(setk_handle_t h, int n_utts, const float* const* spec, int num_channels,
                   const int* num_frames, int num_bins, int taps, int delay, int context,
                   int num_iters, float* const* out, int* status, void* stream) {
    return wpe_batch_impl(h, n_utts, spec, num_channels, num_frames, num_bins, taps, delay, context,
                          num_iters, nullptr, nullptr, out, nullptr, status, stream);
}

int setk_wpe_batch_fnt(setk_handle_t h, int n_utts, const float* const* spec, int num_channels,
                       const int* num_frames, int num_bins, int taps, int delay, int context,
                       int num_iters, float* const* out, int* status, void* stream) {
    return wpe_batch_impl(h, n_utts, spec, num_channels, num_frames, num_bins, taps, delay, context,
                          num_iters, nullptr, nullptr, out, nullptr, status, stream, true);
}

}  // extern "C"
