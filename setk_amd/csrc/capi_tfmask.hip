// capi_tfmask.hip -- front end (include/setk_hip.h): oracle TF masks, mask application and
// oracle separation (tfmask.hip) on stored spectra and, behind the n_fft = 512 plan, on batches of
// waveforms with the forward transform fused in front and the batched inverse STFT behind.
#include "capi.h"

using namespace setk;

namespace {

bool mask_kind_ok(int kind) { return kind >= kTfIbm && kind <= kTfCrm; }

// frames that contribute to `nsamps` output samples (all T of them when nsamps < 0), as setk_istft
int frames_for(setk_handle_t h, int T, int nsamps) {
    if (nsamps < 0) return T;
    const long padded = (long)nsamps + (h->center ? h->n_fft : 0);
    return (int)std::max<long>(1, std::min<long>(T, (padded + h->hop - 1) / h->hop));
}

// what every batch entry checks first: the plan, the table sizes, the flags it takes
int check_batch(setk_handle_t h, int n_utts, const void* a, const void* b, const void* c, int flags) {
    if (!h || n_utts <= 0 || !a || !b || !c) return fail(h, SETK_ERR_INVALID, "bad args");
    if (flags & ~(SETK_FLAG_IN_PCM16 | SETK_FLAG_OUT_PCM16))
        return fail(h, SETK_ERR_INVALID, "flags: SETK_FLAG_IN_PCM16 | SETK_FLAG_OUT_PCM16");
    SETK_TRY(require_plan512(h));
    return SETK_OK;
}

TfFwdArgs fwd_args(setk_handle_t h, const TfUtt* utts, const WorkItem* items, bool pcm16) {
    TfFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.utts = utts;
    a.items = items;
    a.window = pcm16 ? h->d_window_pcm : h->d_window;
    a.tw256 = h->d_tw256;
    a.tw512 = h->d_tw512;
    a.g = geom_of(h);
    a.cutoff = -1.f;
    a.num_targets = 1;
    return a;
}

// The masked spectra spec[v] ([T_v][257] complex64, device) of `nv` virtual utterances through the
// batched inverse STFT and the scale kernel: norm[v] > 0 renorms to that max-abs (null: none),
// nsamps[v] >= 0 keeps that length (null: the natural one); 16-bit output is rounded there too.
int inverse_batch(setk_handle_t h, int nv, const std::vector<float*>& spec, const std::vector<int>& frames,
                  const std::vector<float>* norm, const std::vector<int>* nsamps, void* const* wave, bool out16,
                  hipStream_t s) {
    std::vector<UttDesc> sds = zeroed_utts(nv);
    std::vector<WorkItem> sitems;
    int max_len = 0;
    for (int v = 0; v < nv; ++v) {
        const int keep = nsamps ? (*nsamps)[v] : -1;
        const int T = frames_for(h, frames[v], keep), L = setk_istft_num_samples(h, frames[v], keep);
        float* w32 = static_cast<float*>(wave[v]);
        if (out16) SETK_TRY(arena_get(h, (size_t)std::max(L, 1) * sizeof(float), &w32));
        if (L > 0) HIP_TRY(h, hipMemsetAsync(w32, 0, (size_t)L * sizeof(float), s));
        sds[v].audio = spec[v];  // ISTFT mode: per-item spectrogram
        sds[v].num_frames = T;
        sds[v].out_len = L;
        sds[v].wave_f32 = w32;
        sds[v].wave_out = wave[v];
        push_items(&sitems, v, T, 128, kSuperTile);
        max_len = std::max(max_len, L);
    }
    DescTables st;
    SETK_TRY(upload_tables(h, sds, sitems, s, &st));
    unsigned* d_omax;
    SETK_TRY(arena_get(h, (size_t)nv * sizeof(unsigned), &d_omax));
    HIP_TRY(h, hipMemsetAsync(d_omax, 0, (size_t)nv * sizeof(unsigned), s));
    const Pass2Args pa = pass2_args(h, st.utts, st.items, d_omax);
    HIP_TRY(h, launch_pass2(1, true, pa, st.n_items, s));
    SETK_TRY(profile_mark(h, 2, s));
    if (norm || out16) {
        std::vector<float> hn(nv, -1.f);
        if (norm) hn = *norm;
        const float* d_norm;
        SETK_TRY(upload(h, hn, s, &d_norm));
        ScaleArgs sa = scale_args(pa.utts, nullptr, pa.outmax_bits, out16);
        sa.norm_override = d_norm;
        HIP_TRY(h, launch_scale(sa, nv, max_len, s));
    }
    SETK_TRY(profile_mark(h, 3, s));
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_tf_mask(setk_handle_t h, int kind, const float* tgt, const float* mix, int num_frames, int num_bins,
                 float cutoff, float* mask, setk_tfmask_stats* stats, void* stream) {
    if (!h || !tgt || !mix || !mask || num_frames <= 0 || num_bins <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    if (!mask_kind_ok(kind)) return fail(h, SETK_ERR_INVALID, "kind must be one of SETK_TFMASK_*");
    static_assert(sizeof(TfStats) == sizeof(setk_tfmask_stats), "setk_tfmask_stats");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const size_t cells = (size_t)num_frames * num_bins;
    const float *d_tgt, *d_mix;
    SETK_TRY(stage_in(h, tgt, cells * 2, s, &d_tgt));
    SETK_TRY(stage_in(h, mix, cells * 2, s, &d_mix));
    OutBuf ob;
    SETK_TRY(stage_out(h, mask, cells * (kind == kTfCrm ? 2 : 1) * sizeof(float), &ob));
    const int nslots = (int)((cells + kTfChunk - 1) / kTfChunk);
    unsigned long long* d_counts;
    double* d_slots;
    TfStats* d_stats;
    SETK_TRY(arena_get(h, 2 * sizeof(unsigned long long), &d_counts));
    SETK_TRY(arena_get(h, (size_t)nslots * sizeof(double), &d_slots));
    SETK_TRY(arena_get(h, sizeof(TfStats), &d_stats));
    HIP_TRY(h, hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), s));
    HIP_TRY(h, launch_tf_mask(kind, d_tgt, d_mix, cells, num_bins, cutoff, static_cast<float*>(ob.dev), d_counts,
                              d_slots, nullptr, s));
    if (stats) {
        TfFold job;
        memset(&job, 0, sizeof(job));
        job.counts = d_counts;
        job.slots = d_slots;
        job.out = d_stats;
        job.nslots = nslots;
        const TfFold* d_job;
        SETK_TRY(upload(h, &job, 1, s, &d_job));
        HIP_TRY(h, launch_tf_fold(d_job, 1, s));
        SETK_TRY(copy_out(h, stats, d_stats, sizeof(TfStats), s, nullptr));
    }
    SETK_TRY(copy_back(h, ob, s));
    // the counters, the slots and staged operands live in the arena: the call drains
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_tf_apply(setk_handle_t h, const float* spec, const float* mask, const float* phase_ref, int num_frames,
                  int num_bins, float* out, void* stream) {
    if (!h || !spec || !mask || !out || num_frames <= 0 || num_bins <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const size_t cells = (size_t)num_frames * num_bins;
    const float *d_spec, *d_mask, *d_ref = nullptr;
    SETK_TRY(stage_in(h, spec, cells * 2, s, &d_spec));
    SETK_TRY(stage_in(h, mask, cells, s, &d_mask));
    if (phase_ref) SETK_TRY(stage_in(h, phase_ref, cells * 2, s, &d_ref));
    OutBuf ob;
    SETK_TRY(stage_out(h, out, cells * sizeof(float2), &ob));
    HIP_TRY(h, launch_tf_apply(d_spec, d_mask, d_ref, cells, static_cast<float*>(ob.dev), s));
    return finish_out(h, ob, s);
}

int setk_tf_mask_batch(setk_handle_t h, int kind, int n_utts, const void* const* tgt, const void* const* mix,
                       const int* num_samples, float cutoff, float* const* mask, setk_tfmask_stats* stats,
                       int* status, int flags, void* stream) {
    SETK_TRY(check_batch(h, n_utts, tgt, mix, num_samples, flags));
    if (!mask) return fail(h, SETK_ERR_INVALID, "bad args");
    if (flags & SETK_FLAG_OUT_PCM16) return fail(h, SETK_ERR_INVALID, "a mask has no 16-bit form");
    if (!mask_kind_ok(kind)) return fail(h, SETK_ERR_INVALID, "kind must be one of SETK_TFMASK_*");
    const bool in16 = (flags & SETK_FLAG_IN_PCM16) != 0;
    std::vector<int> frames(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        if (!tgt[u] || !mix[u] || !mask[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(tgt[u]) || !is_device_ptr(mix[u]) || !is_device_ptr(mask[u]))
            return fail(h, SETK_ERR_INVALID, "setk_tf_mask_batch takes device pointers");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T <= 0) return T < 0 ? T : fail(h, SETK_ERR_INVALID, "utterance shorter than a frame");
        frames[u] = T;
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    std::vector<TfUtt> tbl(n_utts);
    memset(tbl.data(), 0, tbl.size() * sizeof(TfUtt));
    std::vector<WorkItem> items;
    std::vector<int> slot0(n_utts + 1);
    int* d_st;
    unsigned long long* d_counts;
    TfStats* d_stats;
    SETK_TRY(arena_get(h, (size_t)n_utts * sizeof(int), &d_st));
    SETK_TRY(arena_get(h, (size_t)n_utts * 2 * sizeof(unsigned long long), &d_counts));
    SETK_TRY(arena_get(h, (size_t)n_utts * sizeof(TfStats), &d_stats));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, (size_t)n_utts * sizeof(int), s));
    HIP_TRY(h, hipMemsetAsync(d_counts, 0, (size_t)n_utts * 2 * sizeof(unsigned long long), s));
    int next = 0;
    for (int u = 0; u < n_utts; ++u) {
        tbl[u].mix = mix[u];
        tbl[u].aux[0] = tgt[u];
        tbl[u].out[0] = mask[u];
        tbl[u].status = d_st + u;
        tbl[u].counts = d_counts + 2 * u;
        tbl[u].num_samples = num_samples[u];
        tbl[u].num_frames = frames[u];
        slot0[u] = next;
        push_items(&items, u, frames[u], 128, 16, &next);
    }
    slot0[n_utts] = next;
    double* d_slots;
    SETK_TRY(arena_get(h, (size_t)next * sizeof(double), &d_slots));
    const TfUtt* d_tbl;
    const WorkItem* d_items;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    SETK_TRY(upload(h, items, s, &d_items));
    TfFwdArgs a = fwd_args(h, d_tbl, d_items, in16);
    a.slots = d_slots;
    a.cutoff = cutoff;
    HIP_TRY(h, launch_tf_forward(kTfModeMask, kind, in16, a, (int)items.size(), s));
    SETK_TRY(profile_mark(h, 1, s));
    if (stats) {
        std::vector<TfFold> jobs(n_utts);
        memset(jobs.data(), 0, jobs.size() * sizeof(TfFold));
        for (int u = 0; u < n_utts; ++u) {
            jobs[u].counts = d_counts + 2 * u;
            jobs[u].slots = d_slots + slot0[u];
            jobs[u].out = d_stats + u;
            jobs[u].nslots = slot0[u + 1] - slot0[u];
        }
        const TfFold* d_jobs;
        SETK_TRY(upload(h, jobs, s, &d_jobs));
        HIP_TRY(h, launch_tf_fold(d_jobs, n_utts, s));
        SETK_TRY(copy_out(h, stats, d_stats, (size_t)n_utts * sizeof(TfStats), s, nullptr));
    }
    SETK_TRY(profile_mark(h, 2, s));
    SETK_TRY(profile_mark(h, 3, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)n_utts * sizeof(int), s, nullptr));
    SETK_TRY(profile_mark(h, 4, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // the tables and counters live in the arena: the call drains
    return SETK_OK;
}

int setk_tf_separate_batch(setk_handle_t h, int n_utts, const void* const* mix, const void* const* phase_ref,
                           const int* num_samples, const float* const* mask, const float* norm, const int* nsamps,
                           void* const* wave, int* status, int flags, void* stream) {
    SETK_TRY(check_batch(h, n_utts, mix, num_samples, mask, flags));
    if (!wave) return fail(h, SETK_ERR_INVALID, "bad args");
    if (n_utts > 65535) return fail(h, SETK_ERR_UNSUPPORTED, "at most 65535 utterances per batch");
    const bool in16 = (flags & SETK_FLAG_IN_PCM16) != 0, out16 = (flags & SETK_FLAG_OUT_PCM16) != 0;
    std::vector<int> frames(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        if (!mix[u] || !mask[u] || !wave[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(mix[u]) || !is_device_ptr(mask[u]) || !is_device_ptr(wave[u]) ||
            (phase_ref && phase_ref[u] && !is_device_ptr(phase_ref[u])))
            return fail(h, SETK_ERR_INVALID, "setk_tf_separate_batch takes device pointers");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T <= 0) return T < 0 ? T : fail(h, SETK_ERR_INVALID, "utterance shorter than a frame");
        frames[u] = T;
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    std::vector<TfUtt> tbl(n_utts);
    memset(tbl.data(), 0, tbl.size() * sizeof(TfUtt));
    std::vector<WorkItem> items;
    std::vector<float*> spec(n_utts);
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_utts * sizeof(int), &d_st));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, (size_t)n_utts * sizeof(int), s));
    for (int u = 0; u < n_utts; ++u) {
        SETK_TRY(arena_get(h, (size_t)frames[u] * kBins * sizeof(float2), &spec[u]));
        tbl[u].mix = mix[u];
        tbl[u].aux[0] = phase_ref ? phase_ref[u] : nullptr;
        tbl[u].out[0] = spec[u];
        tbl[u].mask = mask[u];
        tbl[u].status = d_st + u;
        tbl[u].num_samples = num_samples[u];
        tbl[u].num_frames = frames[u];
        push_items(&items, u, frames[u], 128, 16);
    }
    const TfUtt* d_tbl;
    const WorkItem* d_items;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    SETK_TRY(upload(h, items, s, &d_items));
    const TfFwdArgs a = fwd_args(h, d_tbl, d_items, in16);
    HIP_TRY(h, launch_tf_forward(kTfModeSeparate, 0, in16, a, (int)items.size(), s));
    SETK_TRY(profile_mark(h, 1, s));
    std::vector<float> hn;
    std::vector<int> hk;
    if (norm) hn.assign(norm, norm + n_utts);
    if (nsamps) hk.assign(nsamps, nsamps + n_utts);
    SETK_TRY(inverse_batch(h, n_utts, spec, frames, norm ? &hn : nullptr, nsamps ? &hk : nullptr, wave, out16, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)n_utts * sizeof(int), s, nullptr));
    SETK_TRY(profile_mark(h, 4, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // the spectra and tables live in the arena: the call drains
    return SETK_OK;
}

int setk_oracle_separate_batch(setk_handle_t h, int kind, int n_utts, int num_targets, const void* const* mix,
                               const void* const* targets, const int* num_samples, const int* nsamps,
                               void* const* wave, int* status, int flags, void* stream) {
    SETK_TRY(check_batch(h, n_utts, mix, targets, num_samples, flags));
    if (!wave || num_targets < 1) return fail(h, SETK_ERR_INVALID, "bad args");
    if (num_targets > kTfMaxTargets) return fail(h, SETK_ERR_UNSUPPORTED, "at most 8 targets");
    if (kind != kTfIbm && kind != kTfIrm && kind != kTfIam && kind != kTfPsm)
        return fail(h, SETK_ERR_INVALID, "oracle separation takes ibm, irm, iam or psm");
    const int K = num_targets;
    if ((long)n_utts * K > 65535) return fail(h, SETK_ERR_UNSUPPORTED, "at most 65535 waves per batch");
    const bool in16 = (flags & SETK_FLAG_IN_PCM16) != 0, out16 = (flags & SETK_FLAG_OUT_PCM16) != 0;
    std::vector<int> frames(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        if (!mix[u] || !is_device_ptr(mix[u])) return fail(h, SETK_ERR_INVALID, "mix: device pointers");
        for (int k = 0; k < K; ++k)
            if (!targets[u * K + k] || !wave[u * K + k] || !is_device_ptr(targets[u * K + k]) ||
                !is_device_ptr(wave[u * K + k]))
                return fail(h, SETK_ERR_INVALID, "targets, wave: device pointers");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T <= 0) return T < 0 ? T : fail(h, SETK_ERR_INVALID, "utterance shorter than a frame");
        frames[u] = T;
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    std::vector<TfUtt> tbl(n_utts);
    memset(tbl.data(), 0, tbl.size() * sizeof(TfUtt));
    std::vector<WorkItem> items;
    std::vector<float*> spec((size_t)n_utts * K);
    std::vector<int> vframes((size_t)n_utts * K), vkeep((size_t)n_utts * K, -1);
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_utts * sizeof(int), &d_st));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, (size_t)n_utts * sizeof(int), s));
    for (int u = 0; u < n_utts; ++u) {
        tbl[u].mix = mix[u];
        for (int k = 0; k < K; ++k) {
            SETK_TRY(arena_get(h, (size_t)frames[u] * kBins * sizeof(float2), &spec[u * K + k]));
            tbl[u].aux[k] = targets[u * K + k];
            tbl[u].out[k] = spec[u * K + k];
            vframes[u * K + k] = frames[u];
            if (nsamps) vkeep[u * K + k] = nsamps[u];
        }
        tbl[u].status = d_st + u;
        tbl[u].num_samples = num_samples[u];
        tbl[u].num_frames = frames[u];
        push_items(&items, u, frames[u], 128, 16);
    }
    const TfUtt* d_tbl;
    const WorkItem* d_items;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    SETK_TRY(upload(h, items, s, &d_items));
    TfFwdArgs a = fwd_args(h, d_tbl, d_items, in16);
    a.num_targets = K;
    HIP_TRY(h, launch_tf_forward(kTfModeOracle, kind, in16, a, (int)items.size(), s));
    SETK_TRY(profile_mark(h, 1, s));
    SETK_TRY(inverse_batch(h, n_utts * K, spec, vframes, nullptr, nsamps ? &vkeep : nullptr, wave, out16, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)n_utts * sizeof(int), s, nullptr));
    SETK_TRY(profile_mark(h, 4, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // the spectra and tables live in the arena: the call drains
    return SETK_OK;
}

}  // extern "C"
