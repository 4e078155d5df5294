// capi_spatial.hip -- front end (include/setk_hip.h): the geometry-driven spatial features of
// spatial.hip on one stored spectrogram and on a batch of device spectrograms.
#include "capi.h"

using namespace setk;

namespace {

struct SpatialJob {
    const float* spec;  // [C][T][F] complex64 (device)
    float* out;         // [T][width] (device)
    int T;
};

int check_opts(setk_handle_t h, const setk_spatial_opts* o, int n_utts, int C, int F) {
    if (!o) return fail(h, SETK_ERR_INVALID, "bad args");
    if (o->kind < SETK_SPATIAL_IPD || o->kind > SETK_SPATIAL_SRP)
        return fail(h, SETK_ERR_INVALID, "kind must be one of SETK_SPATIAL_*");
    if (C < 2 || C > kMaxChannels16) return fail(h, SETK_ERR_UNSUPPORTED, "2 <= num_channels <= 16");
    if (F < 2) return fail(h, SETK_ERR_UNSUPPORTED, "num_bins >= 2");
    if (o->n_pairs <= 0 || !o->pairs) return fail(h, SETK_ERR_INVALID, "spatial features need microphone pairs");
    if (o->n_pairs > kSpatialMaxPairs) return fail(h, SETK_ERR_UNSUPPORTED, "at most 120 microphone pairs");
    for (int i = 0; i < 2 * o->n_pairs; ++i)
        if (o->pairs[i] < 0 || o->pairs[i] >= C)
            return fail(h, SETK_ERR_INVALID, "microphone pair out of range");
    if (o->kind == SETK_SPATIAL_SRP) {
        if (o->num_doas <= 0 || !o->table || !o->pair_weight)
            return fail(h, SETK_ERR_INVALID, "SRP needs its table, the pair weights and num_doas >= 1");
        if ((long)n_utts * o->n_pairs > 65535)
            return fail(h, SETK_ERR_UNSUPPORTED, "utterances x pairs of one SRP batch <= 65535");
    }
    if (o->kind == SETK_SPATIAL_DF) {
        if (o->num_sv <= 0 || !o->steer_vector || o->n_index <= 0 || !o->doa_index)
            return fail(h, SETK_ERR_INVALID, "DF needs steer vectors and direction indices");
        if (o->n_index > 65535) return fail(h, SETK_ERR_UNSUPPORTED, "at most 65535 directions per utterance");
        for (long i = 0; i < (long)n_utts * o->n_index; ++i)
            if (o->doa_index[i] < 0 || o->doa_index[i] >= o->num_sv)
                return fail(h, SETK_ERR_INVALID, "direction index outside the steer-vector set");
    }
    if (n_utts > 65535) return fail(h, SETK_ERR_UNSUPPORTED, "at most 65535 utterances per batch");
    return SETK_OK;
}

size_t spatial_width(const setk_spatial_opts& o, int F) {
    switch (o.kind) {
        case SETK_SPATIAL_COS_SIN_IPD: return (size_t)2 * o.n_pairs * F;
        case SETK_SPATIAL_DF: return (size_t)o.n_index * F;
        case SETK_SPATIAL_SRP: return (size_t)o.num_doas;
        default: return (size_t)o.n_pairs * F;
    }
}

// Every job's features, enqueued on s (the entry points have checked the options)
int spatial_run(setk_handle_t h, const setk_spatial_opts& o, int C, int F, const std::vector<SpatialJob>& jobs,
                hipStream_t s) {
    const int n = (int)jobs.size(), P = o.n_pairs;
    int max_frames = 0;
    for (const SpatialJob& j : jobs) max_frames = std::max(max_frames, j.T);
    const int* d_pairs;
    SETK_TRY(upload(h, o.pairs, (size_t)2 * P, s, &d_pairs));
    std::vector<SpatialUtt> tbl(n);  // (value-initialised; neither struct has padding)
    for (int u = 0; u < n; ++u) {
        tbl[u].spec = jobs[u].spec;
        tbl[u].out = jobs[u].out;
        tbl[u].T = jobs[u].T;
        tbl[u].idx0 = u * o.n_index;
    }
    const SpatialUtt* d_tbl;
    if (o.kind == SETK_SPATIAL_DF) {
        const float* d_sv;
        SETK_TRY(stage_in(h, o.steer_vector, (size_t)o.num_sv * C * F * 2, s, &d_sv));
        const int* d_idx;
        SETK_TRY(upload(h, o.doa_index, (size_t)n * o.n_index, s, &d_idx));
        SETK_TRY(upload(h, tbl, s, &d_tbl));
        HIP_TRY(h, launch_spatial_df(d_tbl, d_pairs, d_sv, d_idx, o.n_index, n, max_frames, C, F, P, s));
        SETK_TRY(profile_mark(h, 1, s));
        SETK_TRY(profile_mark(h, 2, s));
        SETK_TRY(profile_mark(h, 3, s));
        return SETK_OK;
    }
    if (o.kind != SETK_SPATIAL_SRP) {
        SETK_TRY(upload(h, tbl, s, &d_tbl));
        HIP_TRY(h, launch_spatial_ipd(d_tbl, d_pairs, o.kind, n, max_frames, F, P, s));
        SETK_TRY(profile_mark(h, 1, s));
        SETK_TRY(profile_mark(h, 2, s));
        SETK_TRY(profile_mark(h, 3, s));
        return SETK_OK;
    }
    // SRP: the observation tiles, the contraction per pair with its maximum, the combination
    const int D = o.num_doas, Dpad = ssl_apad(D);
    const float *d_table, *d_weight;
    SETK_TRY(stage_in(h, o.table, (size_t)P * F * Dpad * 2, s, &d_table));
    SETK_TRY(upload(h, o.pair_weight, (size_t)P, s, &d_weight));
    unsigned* pmax;
    SETK_TRY(arena_get(h, (size_t)n * P * sizeof(unsigned), &pmax));
    HIP_TRY(h, hipMemsetAsync(pmax, 0, (size_t)n * P * sizeof(unsigned), s));
    std::vector<SslUtt> obs(n);
    for (int u = 0; u < n; ++u) {
        float* xt;
        SETK_TRY(arena_get(h, ssl_xt_bytes(jobs[u].T, F, P), &xt));
        SETK_TRY(arena_get(h, (size_t)P * jobs[u].T * Dpad * sizeof(float), &tbl[u].sp));
        tbl[u].pmax = pmax + (size_t)u * P;
        obs[u].spec = jobs[u].spec;
        obs[u].xt = xt;
        obs[u].T = jobs[u].T;
        obs[u].pitch = F;
        obs[u].t1 = jobs[u].T;
    }
    const SslUtt* d_obs;
    SETK_TRY(upload(h, obs, s, &d_obs));
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    HIP_TRY(h, launch_ssl_obs_prep(d_obs, d_pairs, kSslSrp, n, max_frames, C, F, P, 0, 0.f, s));
    SETK_TRY(profile_mark(h, 1, s));
    HIP_TRY(h, launch_spatial_srp_pairs(d_obs, d_tbl, d_table, n, max_frames, D, F, P, s));
    SETK_TRY(profile_mark(h, 2, s));
    HIP_TRY(h, launch_spatial_srp_combine(d_tbl, d_weight, n, max_frames, D, P, s));
    SETK_TRY(profile_mark(h, 3, s));
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_spatial_feats(setk_handle_t h, const setk_spatial_opts* opts, const float* spec, int num_channels,
                       int num_frames, int num_bins, float* out, void* stream) {
    if (!h || !spec || !out || num_frames <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    const int C = num_channels, T = num_frames, F = num_bins;
    SETK_TRY(check_opts(h, opts, 1, C, F));
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    std::vector<SpatialJob> jobs(1);
    jobs[0].T = T;
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &jobs[0].spec));
    OutBuf ob;
    SETK_TRY(stage_out(h, out, (size_t)T * spatial_width(*opts, F) * sizeof(float), &ob));
    jobs[0].out = static_cast<float*>(ob.dev);
    SETK_TRY(spatial_run(h, *opts, C, F, jobs, s));
    SETK_TRY(copy_back(h, ob, s));
    SETK_TRY(profile_mark(h, 4, s));
    // host operands are pageable copies queued on the stream: drained before they may be
    // released; with device operands the call is asynchronous like the other operators
    const bool staged = jobs[0].spec != spec ||
                        (opts->kind == SETK_SPATIAL_SRP && !is_device_ptr(opts->table)) ||
                        (opts->kind == SETK_SPATIAL_DF && !is_device_ptr(opts->steer_vector));
    if (ob.host || staged) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_spatial_batch(setk_handle_t h, const setk_spatial_opts* opts, int n_utts, int num_channels,
                       const float* const* spec, const int* num_frames, int num_bins, float* const* out,
                       void* stream) {
    if (!h || n_utts <= 0 || !spec || !num_frames || !out) return fail(h, SETK_ERR_INVALID, "bad args");
    const int C = num_channels, F = num_bins;
    SETK_TRY(check_opts(h, opts, n_utts, C, F));
    std::vector<SpatialJob> jobs(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        if (!spec[u] || !out[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (num_frames[u] <= 0) return fail(h, SETK_ERR_INVALID, "utterance without a frame");
        if (!is_device_ptr(spec[u]) || !is_device_ptr(out[u]))
            return fail(h, SETK_ERR_INVALID, "setk_spatial_batch takes device pointers");
        jobs[u].spec = spec[u];
        jobs[u].out = out[u];
        jobs[u].T = num_frames[u];
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    SETK_TRY(spatial_run(h, *opts, C, F, jobs, s));
    SETK_TRY(profile_mark(h, 4, s));
    // a table or steer-vector set in host memory was staged from a pageable copy
    if ((opts->kind == SETK_SPATIAL_SRP && !is_device_ptr(opts->table)) ||
        (opts->kind == SETK_SPATIAL_DF && !is_device_ptr(opts->steer_vector)))
        HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
