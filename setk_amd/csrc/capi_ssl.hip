// capi_ssl.hip -- front end (include/setk_hip.h): mask-based sound source localisation
// (ssl.hip) on a stored spectrogram, and on batches of waveforms with the STFT in front.
#include "capi.h"

using namespace setk;

namespace {

struct SslJob {
    const float* spec;  // [C][T][pitch] complex64 (device)
    const float* mask;  // [T][F] (device) or null
    int T, pitch;
    const int* win;     // host [W][2]
    int W;
};

int check_opts(setk_handle_t h, const setk_ssl_opts* o, int C, int A, int F) {
    if (!o) return fail(h, SETK_ERR_INVALID, "bad args");
    if (o->backend != SETK_SSL_ML && o->backend != SETK_SSL_SRP && o->backend != SETK_SSL_MUSIC)
        return fail(h, SETK_ERR_INVALID, "backend must be SETK_SSL_ML, SETK_SSL_SRP or SETK_SSL_MUSIC");
    if (A <= 0 || F <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    if (C < 1 || C > kMaxChannels16) return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 16");
    if (o->backend == SETK_SSL_SRP) {
        if (o->n_pairs <= 0 || !o->pairs) return fail(h, SETK_ERR_INVALID, "SRP needs microphone pairs");
        for (int i = 0; i < 2 * o->n_pairs; ++i)
            if (o->pairs[i] < 0 || o->pairs[i] >= C)
                return fail(h, SETK_ERR_INVALID, "SRP pair index outside the channels");
    }
    return SETK_OK;
}

int check_windows(setk_handle_t h, const SslJob& j) {
    if (j.T <= 0 || j.W <= 0 || !j.win) return fail(h, SETK_ERR_INVALID, "bad args");
    for (int w = 0; w < j.W; ++w)
        if (j.win[2 * w] < 0 || j.win[2 * w] >= j.win[2 * w + 1] || j.win[2 * w + 1] > j.T)
            return fail(h, SETK_ERR_INVALID, "window outside [0, num_frames) or empty");
    return SETK_OK;
}

// The scores of every window of every job into d_score [sum W][A] and the arg-extrema into
// d_index [sum W]; worst[j] receives the worst per-bin status of job j (MUSIC: setk_pevd's).
// The entry points have checked every job's windows.  MUSIC has drained when this returns (its
// statuses are read back); otherwise work may be in flight.
int ssl_run(setk_handle_t h, const setk_ssl_opts& o, int C, int F, int A, const float* d_sv,
            const std::vector<SslJob>& jobs, double* d_score, int* d_index, std::vector<int>* worst,
            hipStream_t s) {
    const int n = (int)jobs.size();
    const int mode = o.backend;
    const int K = mode == SETK_SSL_SRP ? o.n_pairs : C;
    int n_wins = 0, max_frames = 0;
    bool single = true;
    for (const SslJob& j : jobs) {
        n_wins += j.W;
        max_frames = std::max(max_frames, j.T);
        single = single && j.W == 1;
    }
    worst->assign(n, SETK_NUM_OK);
    const int* d_pairs = nullptr;
    if (mode == SETK_SSL_SRP) SETK_TRY(upload(h, o.pairs, (size_t)2 * K, s, &d_pairs));
    float* svt;
    SETK_TRY(arena_get(h, (size_t)F * K * ssl_apad(A) * sizeof(float2), &svt));
    HIP_TRY(h, launch_ssl_sv_prep(d_sv, d_pairs, mode, A, C, F, K, svt, s));
    std::vector<SslWin> wins(n_wins);  // (value-initialised; neither struct has padding)
    const SslWin* d_wins;

    if (mode == SETK_SSL_MUSIC) {
        int* d_st;
        SETK_TRY(arena_get(h, (size_t)n_wins * F * sizeof(int), &d_st));
        const int pitch = ((F + 7) / 8) * 8;
        int w0 = 0;
        for (const SslJob& j : jobs)
            for (int w = 0; w < j.W; ++w, ++w0) {
                const int t0 = j.win[2 * w], Tw = j.win[2 * w + 1] - t0;
                // (one window's scratch, handed back before the next window)
                const std::vector<size_t> mark = arena_mark(h);
                float *xo, *m2, *part, *cov, *pv;
                SETK_TRY(arena_get(h, (size_t)C * Tw * F * sizeof(float2), &xo));
                SETK_TRY(arena_get(h, (size_t)Tw * F * sizeof(float), &m2));
                // (setk_covar's own split of the frames)
                const int split = std::max(1, std::min(64, (Tw + 31) / 32));
                const int per = (Tw + split - 1) / split, used = (Tw + per - 1) / per;
                SETK_TRY(arena_get(h, (size_t)split * (2 * npairs(C) + 1) * pitch * 4, &part));
                SETK_TRY(arena_get(h, (size_t)F * C * C * sizeof(float2), &cov));
                SETK_TRY(arena_get(h, (size_t)F * C * sizeof(float2), &pv));
                HIP_TRY(h, launch_ssl_music_prep(j.spec, j.mask, C, j.T, F, j.pitch, t0, t0 + Tw, xo, m2, s));
                HIP_TRY(h, launch_covar_spec(C, xo, m2, Tw, F, part, split, s));
                HIP_TRY(h, launch_covar_spec_finalize(C, part, used, F, cov, s));
                SETK_TRY(pevd_in_arena(h, cov, F, C, pv, d_st + (size_t)w0 * F, s));
                HIP_TRY(h, launch_ssl_music_score(svt, pv, cov, A, F, C, d_score + (size_t)w0 * A,
                                                  d_st + (size_t)w0 * F, s));
                arena_rewind(h, mark);
            }
        SETK_TRY(profile_mark(h, 2, s));
        SETK_TRY(upload(h, wins, s, &d_wins));
        HIP_TRY(h, launch_ssl_windows(d_wins, n_wins, A, true, d_score, d_index, s));
        SETK_TRY(profile_mark(h, 3, s));
        std::vector<int> st((size_t)n_wins * F);
        HIP_TRY(h, hipMemcpyAsync(st.data(), d_st, st.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        w0 = 0;
        for (int u = 0; u < n; ++u)
            for (int w = 0; w < jobs[u].W; ++w, ++w0)
                for (int f = 0; f < F; ++f) (*worst)[u] = std::max((*worst)[u], st[(size_t)w0 * F + f]);
        return SETK_OK;
    }

    // ML, SRP: frame scores, then the windows.  SRP with one window per utterance (offline)
    // folds the frames first and scores the one folded pseudo-frame.
    const bool fold = mode == SETK_SSL_SRP && single;
    std::vector<SslUtt> tbl(n), tbl_fold(fold ? n : 0);
    int w0 = 0;
    for (int u = 0; u < n; ++u) {
        const SslJob& j = jobs[u];
        const int Ts = fold ? 1 : j.T;
        float *xt, *pm = nullptr, *S;
        SETK_TRY(arena_get(h, ssl_xt_bytes(Ts, F, K), &xt));
        if (mode == SETK_SSL_ML) SETK_TRY(arena_get(h, ssl_pm_bytes(Ts, F), &pm));
        if (fold) SETK_TRY(arena_get(h, ssl_fold_bytes(j.win[1] - j.win[0], F, K), &pm));
        SETK_TRY(arena_get(h, (size_t)Ts * A * sizeof(float), &S));
        SslUtt& e = tbl[u];
        e.spec = j.spec;
        e.mask = j.mask;
        e.xt = xt;
        e.pm = pm;
        e.S = S;
        e.T = Ts;
        e.pitch = j.pitch;
        e.t1 = Ts;
        if (fold) {  // the same buffers, the utterance's own frames and the window to sum
            tbl_fold[u] = e;
            tbl_fold[u].T = j.T;
            tbl_fold[u].t0 = j.win[0];
            tbl_fold[u].t1 = j.win[1];
        }
        for (int w = 0; w < j.W; ++w, ++w0) {
            wins[w0].S = S;
            wins[w0].t0 = fold ? 0 : j.win[2 * w];
            wins[w0].t1 = fold ? 1 : j.win[2 * w + 1];
        }
    }
    const SslUtt* d_tbl;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    if (fold) {
        const SslUtt* d_fold;
        SETK_TRY(upload(h, tbl_fold, s, &d_fold));
        HIP_TRY(h, launch_ssl_srp_fold(d_fold, d_pairs, n, max_frames, F, K, s));
    } else {
        HIP_TRY(h, launch_ssl_obs_prep(d_tbl, d_pairs, mode, n, max_frames, C, F, K, o.norm, (float)o.eps, s));
    }
    HIP_TRY(h, launch_ssl_frame_scores(d_tbl, svt, mode, n, fold ? 1 : max_frames, A, F, K,
                                       (float)(1.0 / (1.0 + o.eps)), (float)o.eps, o.compression, s));
    SETK_TRY(profile_mark(h, 2, s));
    SETK_TRY(upload(h, wins, s, &d_wins));
    HIP_TRY(h, launch_ssl_windows(d_wins, n_wins, A, false, d_score, d_index, s));
    SETK_TRY(profile_mark(h, 3, s));
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_ssl_scores(setk_handle_t h, const setk_ssl_opts* opts, const float* spec, const float* mask,
                    const float* steer_vector, int num_doas, int num_channels, int num_frames, int num_bins,
                    const int* windows, int num_windows, double* score, int* index, int* status,
                    void* stream) {
    if (!h || !spec || !steer_vector || !index || num_frames <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    const int C = num_channels, T = num_frames, F = num_bins, A = num_doas;
    SETK_TRY(check_opts(h, opts, C, A, F));
    const int whole[2] = {0, T};
    std::vector<SslJob> jobs(1);
    jobs[0].win = windows ? windows : whole;
    jobs[0].W = windows ? num_windows : 1;
    jobs[0].T = T;
    jobs[0].pitch = F;
    SETK_TRY(check_windows(h, jobs[0]));
    const int W = jobs[0].W;
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    SETK_TRY(profile_mark(h, 1, s));
    const float* d_sv;
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &jobs[0].spec));
    if (mask) SETK_TRY(stage_in(h, mask, (size_t)T * F, s, &jobs[0].mask));
    SETK_TRY(stage_in(h, steer_vector, (size_t)A * C * F * 2, s, &d_sv));
    OutBuf os, oi;
    if (score)
        SETK_TRY(stage_out(h, score, (size_t)W * A * sizeof(double), &os));
    else
        SETK_TRY(arena_get(h, (size_t)W * A * sizeof(double), &os.dev));
    SETK_TRY(stage_out(h, index, (size_t)W * sizeof(int), &oi));
    std::vector<int> worst;
    SETK_TRY(ssl_run(h, *opts, C, F, A, d_sv, jobs, static_cast<double*>(os.dev), static_cast<int*>(oi.dev),
                     &worst, s));
    SETK_TRY(profile_mark(h, 4, s));
    SETK_TRY(copy_back(h, os, s));
    SETK_TRY(copy_back(h, oi, s));
    // staged buffers and scratch live in the arena: drained before the next call reuses it
    HIP_TRY(h, hipStreamSynchronize(s));
    if (status) SETK_TRY(put_result(h, status, worst.data(), sizeof(int)));
    return SETK_OK;
}

int setk_ssl_batch(setk_handle_t h, const setk_ssl_opts* opts, int n_utts, int num_channels,
                   const float* const* audio, const int* num_samples, const float* const* mask,
                   const float* steer_vector, int num_doas, const int* windows, const int* num_windows,
                   int* index, double* score, int* status, void* stream) {
    if (!h || n_utts <= 0 || !audio || !num_samples || !steer_vector || !windows || !num_windows || !index)
        return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int C = num_channels, F = kBins, A = num_doas;
    SETK_TRY(check_opts(h, opts, C, A, F));
    std::vector<SslJob> jobs(n_utts);
    int n_wins = 0;
    for (int u = 0; u < n_utts; ++u) {
        if (!audio[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(audio[u]) || (mask && mask[u] && !is_device_ptr(mask[u])))
            return fail(h, SETK_ERR_INVALID, "setk_ssl_batch takes device pointers");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T <= 0) return T < 0 ? T : fail(h, SETK_ERR_INVALID, "utterance shorter than a frame");
        jobs[u].T = T;
        jobs[u].pitch = F;
        jobs[u].mask = mask ? mask[u] : nullptr;
        jobs[u].win = windows + (size_t)2 * n_wins;
        jobs[u].W = num_windows[u];
        if (jobs[u].W <= 0) return fail(h, SETK_ERR_INVALID, "an utterance without a window");
        n_wins += jobs[u].W;
        SETK_TRY(check_windows(h, jobs[u]));
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));

    // ---- STFT into arena scratch: one launch for the batch up to 8 channels, beyond that the
    // stand-alone transform's channel groups per utterance ----
    std::vector<UttDesc> uds = zeroed_utts(n_utts);
    std::vector<WorkItem> items;
    for (int u = 0; u < n_utts; ++u) {
        float* sp;
        SETK_TRY(arena_get(h, (size_t)C * jobs[u].T * F * sizeof(float2), &sp));
        jobs[u].spec = sp;
        uds[u].audio = audio[u];
        uds[u].num_samples = num_samples[u];
        uds[u].num_frames = jobs[u].T;
        uds[u].wave_out = sp;
        push_items(&items, u, jobs[u].T, 128, 32);
    }
    if (C <= kMaxChannels) {
        DescTables t;
        SETK_TRY(upload_tables(h, uds, items, s, &t));
        Pass1Args a = pass1_args(h, t.utts, t.items);
        HIP_TRY(h, launch_pass1(C, true, a, t.n_items, s));
    } else {
        for (int u = 0; u < n_utts; ++u)
            for (int c0 = 0; c0 < C; c0 += kMaxChannels) {
                std::vector<UttDesc> one = zeroed_utts(1);
                one[0].audio = audio[u] + (size_t)c0 * num_samples[u];
                one[0].num_samples = num_samples[u];
                one[0].num_frames = jobs[u].T;
                std::vector<WorkItem> it;
                push_items(&it, 0, jobs[u].T, 64, 32);
                DescTables t;
                SETK_TRY(upload_tables(h, one, it, s, &t));
                Pass1Args a = pass1_args(h, t.utts, t.items);
                a.spec_dump = const_cast<float*>(jobs[u].spec) + (size_t)c0 * jobs[u].T * F * 2;
                HIP_TRY(h, launch_pass1(std::min(kMaxChannels, C - c0), true, a, t.n_items, s));
            }
    }
    SETK_TRY(profile_mark(h, 1, s));

    const float* d_sv;
    SETK_TRY(stage_in(h, steer_vector, (size_t)A * C * F * 2, s, &d_sv));
    OutBuf os, oi;
    if (score)
        SETK_TRY(stage_out(h, score, (size_t)n_wins * A * sizeof(double), &os));
    else
        SETK_TRY(arena_get(h, (size_t)n_wins * A * sizeof(double), &os.dev));
    SETK_TRY(stage_out(h, index, (size_t)n_wins * sizeof(int), &oi));
    std::vector<int> worst;
    SETK_TRY(ssl_run(h, *opts, C, F, A, d_sv, jobs, static_cast<double*>(os.dev), static_cast<int*>(oi.dev),
                     &worst, s));
    SETK_TRY(profile_mark(h, 4, s));
    SETK_TRY(copy_back(h, os, s));
    SETK_TRY(copy_back(h, oi, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (status) SETK_TRY(put_result(h, status, worst.data(), (size_t)n_utts * sizeof(int)));
    return SETK_OK;
}

}  // extern "C"
