// capi_metric.hip -- front end (include/setk_hip.h): SI-SNR of every (estimate, reference) pair
// and the best assignment (metric.hip) for ragged batches of utterances, and for one pair.
#include <cmath>

#include "capi.h"

using namespace setk;

namespace {

constexpr int kMetricFlags = SETK_FLAG_IN_PCM16 | SETK_FLAG_KEEP_DC;

// The launches of a batch whose signals and results are device memory (results of the running
// call's arena or the caller's).  est / ref: sum(num_src) pointers, utterance-major.
int run_metric(setk_handle_t h, hipStream_t s, int n_utts, const int* num_src, const void* const* est,
               const int* est_stride, const void* const* ref, const int* ref_stride, const int* num_samples,
               double eps, int flags, double* d_pair, double* d_best, int* d_perm, int* d_status) {
    const bool pcm16 = (flags & SETK_FLAG_IN_PCM16) != 0, keep_dc = (flags & SETK_FLAG_KEEP_DC) != 0;
    constexpr int kGram = kMetricMaxSrc + 2 * kMetricMaxSrc * kMetricMaxSrc, kMean = 2 * kMetricMaxSrc;
    std::vector<MetricUtt> tbl(n_utts);
    memset(tbl.data(), 0, tbl.size() * sizeof(MetricUtt));
    std::vector<MetricItem> items;
    double *d_mean, *d_gram;
    SETK_TRY(arena_get(h, (size_t)n_utts * kMean * sizeof(double), &d_mean));
    SETK_TRY(arena_get(h, (size_t)n_utts * kGram * sizeof(double), &d_gram));
    int max_k = 1;
    size_t sig = 0, cell = 0, tiles = 0;
    for (int u = 0; u < n_utts; ++u) {
        MetricUtt& m = tbl[u];
        const int K = num_src[u];
        max_k = std::max(max_k, K);
        for (int i = 0; i < K; ++i) {
            m.sig[i] = est[sig + i];
            m.stride[i] = est_stride[sig + i];
            m.sig[kMetricMaxSrc + i] = ref[sig + i];
            m.stride[kMetricMaxSrc + i] = ref_stride[sig + i];
        }
        m.K = K;
        m.L = num_samples[u];
        m.tile0 = (int)tiles;
        m.ntiles = (m.L + kMetricTile - 1) / kMetricTile;
        m.mean = d_mean + (size_t)u * kMean;
        m.gram = d_gram + (size_t)u * kGram;
        m.pair = d_pair + cell;
        m.best = d_best ? d_best + u : nullptr;
        m.perm = d_perm ? d_perm + sig : nullptr;
        m.status = d_status + u;
        for (int t = 0; t < m.ntiles; ++t) items.push_back(MetricItem{u, t});
        sig += K;
        cell += (size_t)K * K;
        tiles += m.ntiles;
    }
    if (tiles > 0x7fffffffu) return fail(h, SETK_ERR_UNSUPPORTED, "at most 2^31 - 1 tiles of 8192 samples per batch");
    const int kp = metric_padded_sources(max_k), n_items = (int)items.size();
    double* d_partial;
    int* d_flags;
    SETK_TRY(arena_get(h, tiles * metric_row(kp) * sizeof(double), &d_partial));
    SETK_TRY(arena_get(h, tiles * sizeof(int), &d_flags));
    const MetricUtt* d_tbl;
    const MetricItem* d_items;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    SETK_TRY(upload(h, items, s, &d_items));
    // ---- the means, or none (remove_dc=False) ----
    if (keep_dc)
        HIP_TRY(h, hipMemsetAsync(d_mean, 0, (size_t)n_utts * kMean * sizeof(double), s));
    else
        HIP_TRY(h, launch_metric_means(d_tbl, d_items, n_items, n_utts, kp, pcm16, d_partial, s));
    SETK_TRY(profile_mark(h, 1, s));
    HIP_TRY(h, launch_metric_gram(d_tbl, d_items, n_items, n_utts, kp, pcm16, eps, d_partial, d_flags, s));
    SETK_TRY(profile_mark(h, 2, s));
    HIP_TRY(h, launch_metric_residual(d_tbl, d_items, n_items, kp, pcm16, d_partial, s));
    SETK_TRY(profile_mark(h, 3, s));
    HIP_TRY(h, launch_metric_search(d_tbl, n_utts, kp, eps, d_partial, s));
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_si_snr_batch(setk_handle_t h, int n_utts, const int* num_src, const void* const* est,
                      const int* est_stride, const void* const* ref, const int* ref_stride,
                      const int* num_samples, double eps, int flags, double* pair, double* best, int* perm,
                      int* status, void* stream) {
    if (!h || n_utts <= 0 || !num_src || !est || !est_stride || !ref || !ref_stride || !num_samples || !pair)
        return fail(h, SETK_ERR_INVALID, "bad args");
    if (flags & ~kMetricFlags) return fail(h, SETK_ERR_INVALID, "flags: SETK_FLAG_IN_PCM16 | SETK_FLAG_KEEP_DC");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(h, SETK_ERR_INVALID, "eps >= 0");
    size_t n_sig = 0, n_cell = 0;
    for (int u = 0; u < n_utts; ++u) {
        const int K = num_src[u];
        if (K < 1) return fail(h, SETK_ERR_INVALID, "num_sources >= 1");
        if (K > kMetricMaxSrc)
            return fail(h, SETK_ERR_UNSUPPORTED, "num_sources <= 8 (the search walks num_sources! orders)");
        if (num_samples[u] < 1) return fail(h, SETK_ERR_INVALID, "num_samples >= 1");
        for (int i = 0; i < K; ++i) {
            if (!est[n_sig + i] || !ref[n_sig + i]) return fail(h, SETK_ERR_INVALID, "null signal pointer");
            if (!is_device_ptr(est[n_sig + i]) || !is_device_ptr(ref[n_sig + i]))
                return fail(h, SETK_ERR_INVALID, "setk_si_snr_batch takes device pointers");
            if (est_stride[n_sig + i] < 1 || ref_stride[n_sig + i] < 1)
                return fail(h, SETK_ERR_INVALID, "sample stride >= 1");
        }
        n_sig += K;
        n_cell += (size_t)K * K;
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    OutBuf op, ob, oo;
    SETK_TRY(stage_out(h, pair, n_cell * sizeof(double), &op));
    if (best) SETK_TRY(stage_out(h, best, (size_t)n_utts * sizeof(double), &ob));
    if (perm) SETK_TRY(stage_out(h, perm, n_sig * sizeof(int), &oo));
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_utts * sizeof(int), &d_st));
    SETK_TRY(run_metric(h, s, n_utts, num_src, est, est_stride, ref, ref_stride, num_samples, eps, flags,
                        static_cast<double*>(op.dev), best ? static_cast<double*>(ob.dev) : nullptr,
                        perm ? static_cast<int*>(oo.dev) : nullptr, d_st));
    SETK_TRY(copy_back(h, op, s));
    if (best) SETK_TRY(copy_back(h, ob, s));
    if (perm) SETK_TRY(copy_back(h, oo, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)n_utts * sizeof(int), s, nullptr));
    SETK_TRY(profile_mark(h, 4, s));
    // the tables, the partial slab and staged results live in the arena: the call drains
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_si_snr(setk_handle_t h, const float* x, const float* s, int num_samples, double eps, int flags,
                double* out, void* stream) {
    if (!h || !x || !s || !out || num_samples < 1) return fail(h, SETK_ERR_INVALID, "bad args");
    if (flags & ~kMetricFlags) return fail(h, SETK_ERR_INVALID, "flags: SETK_FLAG_IN_PCM16 | SETK_FLAG_KEEP_DC");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(h, SETK_ERR_INVALID, "eps >= 0");
    hipStream_t st;
    SETK_TRY(begin_call(h, stream, &st));
    SETK_TRY(profile_begin(h, st));
    const void *d_x, *d_s;
    if (flags & SETK_FLAG_IN_PCM16) {
        const int16_t *px, *ps;
        SETK_TRY(stage_in(h, reinterpret_cast<const int16_t*>(x), (size_t)num_samples, st, &px));
        SETK_TRY(stage_in(h, reinterpret_cast<const int16_t*>(s), (size_t)num_samples, st, &ps));
        d_x = px;
        d_s = ps;
    } else {
        const float *px, *ps;
        SETK_TRY(stage_in(h, x, (size_t)num_samples, st, &px));
        SETK_TRY(stage_in(h, s, (size_t)num_samples, st, &ps));
        d_x = px;
        d_s = ps;
    }
    OutBuf ob;
    SETK_TRY(stage_out(h, out, sizeof(double), &ob));
    int* d_st;
    SETK_TRY(arena_get(h, sizeof(int), &d_st));
    const int one = 1;
    SETK_TRY(run_metric(h, st, 1, &one, &d_x, &one, &d_s, &one, &num_samples, eps, flags,
                        static_cast<double*>(ob.dev), nullptr, nullptr, d_st));
    SETK_TRY(copy_back(h, ob, st));
    SETK_TRY(profile_mark(h, 4, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return SETK_OK;
}

}  // extern "C"
