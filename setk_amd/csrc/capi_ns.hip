// capi_ns.hip -- front end (include/setk_hip.h): OM-LSA noise suppression (ns.hip) on one stored
// spectrogram and on batches of single-channel waveforms with the STFT in front and the inverse
// STFT behind, and the exponential integral on its own.
#include <cmath>

#include "capi.h"

using namespace setk;

namespace {

// one smoothing window into its row of NsParams::taps
int take_window(setk_handle_t h, const double* w, int n, int F, const char* name, double* taps, int* half) {
    if (!w || n <= 0 || (n & 1) == 0)
        return fail(h, SETK_ERR_INVALID, std::string(name) + ": an odd number of taps (2 w + 1)");
    if (n > SETK_NS_MAX_TAPS)
        return fail(h, SETK_ERR_UNSUPPORTED, std::string(name) + ": at most 63 taps (w <= 31)");
    if (F < n)
        return fail(h, SETK_ERR_UNSUPPORTED, std::string(name) + ": more taps than bins (np.convolve's \"same\" "
                                             "then returns the window's length)");
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(w[i])) return fail(h, SETK_ERR_INVALID, std::string(name) + ": tap not finite");
        taps[i] = w[i];
    }
    *half = n / 2;
    return SETK_OK;
}

int make_params(setk_handle_t h, const setk_ns_opts* o, int F, NsParams* p) {
    if (!o) return fail(h, SETK_ERR_INVALID, "bad args");
    if (o->kind != SETK_NS_MCRA && o->kind != SETK_NS_IMCRA)
        return fail(h, SETK_ERR_INVALID, "kind must be one of SETK_NS_*");
    if (!(o->flags & (SETK_NS_OUT_GAIN | SETK_NS_OUT_SPEC)))
        return fail(h, SETK_ERR_INVALID, "no output selected (SETK_NS_OUT_*)");
    if (F < 1) return fail(h, SETK_ERR_INVALID, "bad args");
    if (!ns_supported(F)) return fail(h, SETK_ERR_UNSUPPORTED, "num_bins <= 1025 (n_fft <= 2048)");
    memset(p, 0, sizeof(*p));
    p->kind = o->kind;
    p->F = F;
    SETK_TRY(take_window(h, o->w_mcra, o->n_mcra, F, "w_mcra", p->taps[0], &p->half_m));
    if (o->kind == SETK_NS_MCRA) {
        SETK_TRY(take_window(h, o->w_local, o->n_local, F, "w_local", p->taps[1], &p->half_l));
        SETK_TRY(take_window(h, o->w_global, o->n_global, F, "w_global", p->taps[2], &p->half_g));
        if (o->L < 1 || o->M < 0) return fail(h, SETK_ERR_INVALID, "MCRA: L >= 1, M >= 0");
        if (!(o->zeta_min > 0.0) || !(o->zeta_max > o->zeta_min))
            return fail(h, SETK_ERR_INVALID, "MCRA: 0 < zeta_min < zeta_max");
        p->L = o->L;
        p->mean_bins = std::min(o->M / 2 + 1, F);
        p->V = p->U = 1;
    } else {
        if (o->V < 1 || o->U < 1) return fail(h, SETK_ERR_INVALID, "iMCRA: V >= 1, U >= 1");
        if (o->U > kNsMaxRing) return fail(h, SETK_ERR_UNSUPPORTED, "iMCRA: U <= 32");
        p->V = o->V;
        p->U = o->U;
        p->L = 1;
        p->mean_bins = 1;
    }
    p->alpha = o->alpha;
    p->alpha_s = o->alpha_s;
    p->alpha_d = o->alpha_d;
    p->alpha_p = o->alpha_p;
    p->beta = o->beta;
    p->delta = o->delta;
    p->gmin = o->gmin;
    p->xi_min = o->xi_min;
    p->q_max = o->q_max;
    p->zeta_min = o->zeta_min;
    p->zeta_max = o->zeta_max;
    p->zeta_p_min = o->zeta_p_min;
    p->zeta_p_max = o->zeta_p_max;
    p->inv_b_min = o->inv_b_min;
    p->gamma0 = o->gamma0;
    p->gamma1 = o->gamma1;
    p->zeta0 = o->zeta0;
    p->eps = o->eps;
    if (!(o->eps > 0.0)) return fail(h, SETK_ERR_INVALID, "eps > 0");
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_ns_gain(setk_handle_t h, const setk_ns_opts* opts, const float* spec, int num_frames, int num_bins,
                 double* gain, float* out, int* status, void* stream) {
    if (!h || !spec || num_frames <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    const int T = num_frames, F = num_bins;
    NsParams p;
    SETK_TRY(make_params(h, opts, F, &p));
    const bool want_gain = (opts->flags & SETK_NS_OUT_GAIN) != 0, want_spec = (opts->flags & SETK_NS_OUT_SPEC) != 0;
    if ((want_gain && !gain) || (want_spec && !out)) return fail(h, SETK_ERR_INVALID, "a selected output is NULL");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    const size_t cells = (size_t)T * F;
    std::vector<NsUtt> tbl(1);
    memset(tbl.data(), 0, sizeof(NsUtt));
    SETK_TRY(stage_in(h, spec, cells * 2, s, &tbl[0].spec));
    OutBuf og, os;
    if (want_gain) {
        SETK_TRY(stage_out(h, gain, cells * sizeof(double), &og));
        tbl[0].gain = static_cast<double*>(og.dev);
    }
    if (want_spec) {
        SETK_TRY(stage_out(h, out, cells * sizeof(float2), &os));
        tbl[0].out = static_cast<float*>(os.dev);
    }
    SETK_TRY(arena_get(h, sizeof(int), &tbl[0].status));
    HIP_TRY(h, hipMemsetAsync(tbl[0].status, 0, sizeof(int), s));
    tbl[0].T = T;
    const NsUtt* d_tbl;
    const NsParams* d_p;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    SETK_TRY(upload(h, &p, 1, s, &d_p));
    SETK_TRY(profile_mark(h, 1, s));
    HIP_TRY(h, launch_ns(d_tbl, d_p, p.kind, 1, F, s));
    SETK_TRY(profile_mark(h, 2, s));
    if (want_gain) SETK_TRY(copy_back(h, og, s));
    if (want_spec) SETK_TRY(copy_back(h, os, s));
    if (status) SETK_TRY(copy_out(h, status, tbl[0].status, sizeof(int), s, nullptr));
    SETK_TRY(profile_mark(h, 3, s));
    SETK_TRY(profile_mark(h, 4, s));
    // the tables, the status word and staged operands live in the arena: drained before the next
    // call reuses it
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_ns_batch(setk_handle_t h, const setk_ns_opts* opts, int n_utts, const void* const* audio,
                  const int* num_samples, void* const* wave, double* const* gain, int* status, int flags,
                  void* stream) {
    if (!h || n_utts <= 0 || !audio || !num_samples) return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int F = kBins;
    NsParams p;
    SETK_TRY(make_params(h, opts, F, &p));
    const bool want_gain = (opts->flags & SETK_NS_OUT_GAIN) != 0, want_wave = (opts->flags & SETK_NS_OUT_SPEC) != 0;
    const bool in16 = (flags & SETK_FLAG_IN_PCM16) != 0, out16 = (flags & SETK_FLAG_OUT_PCM16) != 0;
    if ((want_gain && !gain) || (want_wave && !wave)) return fail(h, SETK_ERR_INVALID, "a selected output is NULL");
    if (n_utts > 65535) return fail(h, SETK_ERR_UNSUPPORTED, "at most 65535 utterances per batch");
    std::vector<int> frames(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        if (!audio[u] || (want_gain && !gain[u]) || (want_wave && !wave[u]))
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(audio[u]) || (want_gain && !is_device_ptr(gain[u])) ||
            (want_wave && !is_device_ptr(wave[u])))
            return fail(h, SETK_ERR_INVALID, "setk_ns_batch takes device pointers");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T <= 0) return T < 0 ? T : fail(h, SETK_ERR_INVALID, "utterance shorter than a frame");
        frames[u] = T;
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));

    // ---- 16-bit samples to float32, the STFT of every utterance in one launch ----
    std::vector<const float*> a32(n_utts);
    if (in16) {
        std::vector<char> ptbl(pcm_item_bytes() * n_utts);
        int max_n = 0;
        for (int u = 0; u < n_utts; ++u) {
            float* d;
            SETK_TRY(arena_get(h, (size_t)num_samples[u] * sizeof(float), &d));
            pcm_item_fill(ptbl.data(), u, static_cast<const int16_t*>(audio[u]), d, num_samples[u]);
            a32[u] = d;
            max_n = std::max(max_n, num_samples[u]);
        }
        const char* d_ptbl;
        SETK_TRY(upload(h, ptbl, s, &d_ptbl));
        HIP_TRY(h, launch_pcm16_to_float_batch(d_ptbl, n_utts, 1, max_n, nullptr, s));
    } else
        for (int u = 0; u < n_utts; ++u) a32[u] = static_cast<const float*>(audio[u]);
    std::vector<UttDesc> uds = zeroed_utts(n_utts);
    std::vector<WorkItem> items;
    std::vector<NsUtt> tbl(n_utts);
    memset(tbl.data(), 0, tbl.size() * sizeof(NsUtt));
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_utts * sizeof(int), &d_st));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, (size_t)n_utts * sizeof(int), s));
    for (int u = 0; u < n_utts; ++u) {
        const size_t cells = (size_t)frames[u] * F;
        float *spec, *enh = nullptr;
        SETK_TRY(arena_get(h, cells * sizeof(float2), &spec));
        if (want_wave) SETK_TRY(arena_get(h, cells * sizeof(float2), &enh));
        uds[u].audio = a32[u];
        uds[u].num_samples = num_samples[u];
        uds[u].num_frames = frames[u];
        uds[u].wave_out = spec;
        push_items(&items, u, frames[u], 128, 32);
        tbl[u].spec = spec;
        tbl[u].gain = want_gain ? gain[u] : nullptr;
        tbl[u].out = enh;
        tbl[u].status = d_st + u;
        tbl[u].T = frames[u];
    }
    DescTables t;
    SETK_TRY(upload_tables(h, uds, items, s, &t));
    Pass1Args a = pass1_args(h, t.utts, t.items);
    a.spec_dump = nullptr;  // per-utterance outputs: UttDesc::wave_out
    a.dump_pitch = 0;
    HIP_TRY(h, launch_pass1(1, true, a, t.n_items, s));
    SETK_TRY(profile_mark(h, 1, s));

    // ---- the recursion: one workgroup per utterance ----
    const NsUtt* d_tbl;
    const NsParams* d_p;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    SETK_TRY(upload(h, &p, 1, s, &d_p));
    HIP_TRY(h, launch_ns(d_tbl, d_p, p.kind, n_utts, F, s));
    SETK_TRY(profile_mark(h, 2, s));

    // ---- inverse_stft(gain * stft), no norm (apply_ns.py:42) ----
    if (want_wave) {
        std::vector<UttDesc> sds = zeroed_utts(n_utts);
        std::vector<WorkItem> sitems;
        for (int u = 0; u < n_utts; ++u) {
            const int T = frames[u], L = setk_istft_num_samples(h, T, -1);
            float* w32 = static_cast<float*>(wave[u]);
            if (out16) SETK_TRY(arena_get(h, (size_t)std::max(L, 1) * sizeof(float), &w32));
            if (L > 0) HIP_TRY(h, hipMemsetAsync(w32, 0, (size_t)L * sizeof(float), s));
            sds[u].audio = tbl[u].out;  // ISTFT mode: per-item spectrogram
            sds[u].num_frames = T;
            sds[u].out_len = L;
            sds[u].wave_f32 = w32;
            sds[u].wave_out = w32;
            push_items(&sitems, u, T, 128, kSuperTile);
        }
        DescTables st;
        SETK_TRY(upload_tables(h, sds, sitems, s, &st));
        unsigned* d_omax;
        SETK_TRY(arena_get(h, (size_t)n_utts * sizeof(unsigned), &d_omax));
        HIP_TRY(h, hipMemsetAsync(d_omax, 0, (size_t)n_utts * sizeof(unsigned), s));
        HIP_TRY(h, launch_pass2(1, true, pass2_args(h, st.utts, st.items, d_omax), st.n_items, s));
        SETK_TRY(profile_mark(h, 3, s));
        // rounded as setk_float_to_pcm16 and the host writer round (rint(x * 32767) in double): the
        // renorm kernel of the beamformer paths multiplies in float32
        if (out16)
            for (int u = 0; u < n_utts; ++u)
                if (sds[u].out_len > 0)
                    HIP_TRY(h, launch_float_to_pcm16(sds[u].wave_f32, 1, sds[u].out_len,
                                                     static_cast<int16_t*>(wave[u]), s));
    } else
        SETK_TRY(profile_mark(h, 3, s));
    SETK_TRY(profile_mark(h, 4, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)n_utts * sizeof(int), s, nullptr));
    // the spectrograms and tables live in the arena: the call drains
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_expint_e1(setk_handle_t h, const double* x, double* y, int n, void* stream) {
    if (!h || !x || !y || n <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const double* d_x;
    SETK_TRY(stage_in(h, x, (size_t)n, s, &d_x));
    OutBuf ob;
    SETK_TRY(stage_out(h, y, (size_t)n * sizeof(double), &ob));
    HIP_TRY(h, launch_expint_e1(d_x, static_cast<double*>(ob.dev), n, s));
    SETK_TRY(copy_back(h, ob, s));
    if (ob.host || d_x != x) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
