// capi_auxiva.hip -- front end (include/setk_hip.h): AuxIVA blind source separation
// (auxiva.hip) on a spectrogram, and on batches of waveforms with the STFT in front and the
// inverse STFT of every source behind.
#include "capi.h"

using namespace setk;

namespace {
struct AuxUtt {
    const float* x_bin;  // [F][C][Tp] complex64 (device)
    int T, Tp;
    double* pw;          // [F][C][Tp] float64: |y|^2 between the epochs, y (complex64) at the end
};

// auxiva() (apply_auxiva.py:24-57) on observations that lie bin-major on the device: the epoch-0
// powers, then per epoch one norm launch and one epoch launch over every (bin, utterance).
// Leaves y as complex64 [F][C][Tp] in us[u].pw and the per-bin status in d_st [n_utts][F].
int auxiva_run(setk_handle_t h, int C, int F, int num_epochs, std::vector<AuxUtt>& us, int** d_st_out,
               hipStream_t s) {
    const int n_utts = (int)us.size();
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_utts * F * sizeof(int), &d_st));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, (size_t)n_utts * F * sizeof(int), s));
    const size_t ab = auxiva_args_bytes();
    std::vector<char> tbl((size_t)n_utts * ab);
    int max_frames = 0;
    for (int u = 0; u < n_utts; ++u) {
        AuxUtt& q = us[u];
        max_frames = std::max(max_frames, q.T);
        double* g;
        char* W;
        SETK_TRY(arena_get(h, (size_t)F * C * q.Tp * sizeof(double), &q.pw));
        SETK_TRY(arena_get(h, (size_t)C * q.Tp * sizeof(double), &g));
        SETK_TRY(arena_get(h, (size_t)F * C * C * 2 * sizeof(double), &W));
        auxiva_fill_args(tbl.data() + (size_t)u * ab, q.x_bin, q.pw, g, W, d_st + (size_t)u * F, q.T,
                         q.Tp);
    }
    const char* d_tbl;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    HIP_TRY(h, launch_auxiva_epoch(d_tbl, n_utts, C, F, false, num_epochs == 0, s));
    for (int e = 1; e <= num_epochs; ++e) {
        HIP_TRY(h, launch_auxiva_norm(d_tbl, n_utts, C, F, max_frames, s));
        HIP_TRY(h, launch_auxiva_epoch(d_tbl, n_utts, C, F, true, e == num_epochs, s));
    }
    *d_st_out = d_st;
    return SETK_OK;
}
}  // namespace

extern "C" {

int setk_auxiva(setk_handle_t h, const float* spec, int num_channels, int num_frames, int num_bins,
                int num_epochs, float* out, int* status, void* stream) {
    if (!h || !spec || !out || num_frames <= 0 || num_bins <= 0 || num_epochs < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    const int C = num_channels, T = num_frames, F = num_bins;
    if (!auxiva_supported(C)) return fail(h, SETK_ERR_UNSUPPORTED, auxiva_limit_message());
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const size_t n = (size_t)C * T * F;
    const float* d_spec;
    SETK_TRY(stage_in(h, spec, n * 2, s, &d_spec));
    OutBuf ob;
    SETK_TRY(stage_out(h, out, n * sizeof(float2), &ob));
    std::vector<AuxUtt> us(1);
    us[0].T = T;
    us[0].Tp = (T + 3) & ~3;
    float* xb;
    SETK_TRY(arena_get(h, (size_t)F * C * us[0].Tp * sizeof(float2), &xb));
    us[0].x_bin = xb;
    HIP_TRY(h, launch_auxiva_transpose(d_spec, C, T, F, us[0].Tp, xb, true, s));
    int* d_st = nullptr;
    SETK_TRY(auxiva_run(h, C, F, num_epochs, us, &d_st, s));
    HIP_TRY(h, launch_auxiva_transpose(reinterpret_cast<const float*>(us[0].pw), C, T, F, us[0].Tp,
                                       static_cast<float*>(ob.dev), false, s));
    SETK_TRY(copy_back(h, ob, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)F * sizeof(int), s, nullptr));
    // staged buffers and scratch live in the arena: drained before the next call reuses it
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_auxiva_batch(setk_handle_t h, int n_utts, int num_channels, const float* const* audio,
                      const int* num_samples, int num_epochs, void* const* wave, int* status,
                      int flags, void* stream) {
    if (!h || n_utts <= 0 || !audio || !num_samples || !wave || num_epochs < 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int C = num_channels, F = kBins;
    if (!auxiva_supported(C)) return fail(h, SETK_ERR_UNSUPPORTED, auxiva_limit_message());
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const bool pcm16 = (flags & SETK_FLAG_OUT_PCM16) != 0;
    SETK_TRY(profile_begin(h, s));

    // ---- STFT of every utterance straight into the bin-major layout; max |audio| ----
    std::vector<AuxUtt> us(n_utts);
    std::vector<int> frames(n_utts);
    std::vector<float*> xbs(n_utts);
    int max_samples = 0;
    for (int u = 0; u < n_utts; ++u) {
        if (!audio[u] || !wave[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (!is_device_ptr(audio[u]) || !is_device_ptr(wave[u]))
            return fail(h, SETK_ERR_INVALID, "setk_auxiva_batch takes device pointers");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T <= 0) return T < 0 ? T : fail(h, SETK_ERR_INVALID, "utterance shorter than a frame");
        frames[u] = us[u].T = T;
        us[u].Tp = (T + 3) & ~3;
        SETK_TRY(arena_get(h, (size_t)F * C * us[u].Tp * sizeof(float2), &xbs[u]));
        us[u].x_bin = xbs[u];
        max_samples = std::max(max_samples, num_samples[u]);
    }
    Pass1Args a;
    int n_items;
    SETK_TRY(prepare_stft_binmajor(h, n_utts, audio, num_samples, frames.data(), xbs.data(), s, &a, &n_items));
    const int n_src = n_utts * C;
    // [n_utts] max |audio| | [n_src] the same per source | [n_src] max |source wave|
    unsigned* d_norm;
    SETK_TRY(arena_get(h, (size_t)(n_utts + 2 * n_src) * sizeof(unsigned), &d_norm));
    unsigned* d_norm_src = d_norm + n_utts;
    unsigned* d_omax = d_norm_src + n_src;
    HIP_TRY(h, hipMemsetAsync(d_norm, 0, (size_t)(n_utts + 2 * n_src) * sizeof(unsigned), s));
    HIP_TRY(h, launch_stft_binmajor(C, a, n_items, s));
    // SpectrogramReader.maxabs(key), the norm of inverse_stft (apply_auxiva.py:74-76)
    HIP_TRY(h, launch_maxabs(a.utts, C, d_norm, n_utts, max_samples, s));
    HIP_TRY(h, launch_auxiva_spread_norm(d_norm, C, n_src, d_norm_src, s));
    SETK_TRY(profile_mark(h, 1, s));

    // ---- the epochs ----
    int* d_st = nullptr;
    SETK_TRY(auxiva_run(h, C, F, num_epochs, us, &d_st, s));
    SETK_TRY(profile_mark(h, 2, s));

    // ---- y -> [C][T][F], inverse STFT of every source (one item list for the batch) ----
    std::vector<UttDesc> sds = zeroed_utts(n_src);
    std::vector<WorkItem> sitems;
    int max_len = 0;
    for (int u = 0; u < n_utts; ++u) {
        const int T = us[u].T;
        const int L = setk_istft_num_samples(h, T, -1);
        max_len = std::max(max_len, L);
        float* y;
        float* w32 = static_cast<float*>(wave[u]);
        SETK_TRY(arena_get(h, (size_t)C * T * F * sizeof(float2), &y));
        if (pcm16) SETK_TRY(arena_get(h, (size_t)C * L * sizeof(float), &w32));
        HIP_TRY(h, launch_auxiva_transpose(reinterpret_cast<const float*>(us[u].pw), C, T, F, us[u].Tp, y,
                                           false, s));
        if (L > 0) HIP_TRY(h, hipMemsetAsync(w32, 0, (size_t)C * L * sizeof(float), s));
        for (int c = 0; c < C; ++c) {
            UttDesc& sd = sds[(size_t)u * C + c];
            sd.audio = y + (size_t)c * T * F * 2;  // ISTFT mode: per-item spectrogram
            sd.num_frames = T;
            sd.out_len = L;
            sd.wave_f32 = w32 + (size_t)c * L;
            sd.wave_out = pcm16 ? static_cast<void*>(static_cast<int16_t*>(wave[u]) + (size_t)c * L)
                                : static_cast<void*>(sd.wave_f32);
            push_items(&sitems, u * C + c, T, 128, kSuperTile);
        }
    }
    DescTables t;
    SETK_TRY(upload_tables(h, sds, sitems, s, &t));
    HIP_TRY(h, launch_pass2(1, true, pass2_args(h, t.utts, t.items, d_omax), t.n_items, s));
    SETK_TRY(profile_mark(h, 3, s));
    HIP_TRY(h, launch_scale(scale_args(t.utts, d_norm_src, d_omax, pcm16), n_src, max_len, s));
    SETK_TRY(profile_mark(h, 4, s));

    // worst bin of every utterance; the descriptors live in the arena, so the call drains
    if (status) {
        std::vector<int> st((size_t)n_utts * F), worst(n_utts, 0);
        HIP_TRY(h, hipMemcpyAsync(st.data(), d_st, st.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        for (int u = 0; u < n_utts; ++u)
            for (int f = 0; f < F; ++f) worst[u] = std::max(worst[u], st[(size_t)u * F + f]);
        SETK_TRY(put_result(h, status, worst.data(), (size_t)n_utts * sizeof(int)));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
