// capi_modular.hip -- front end (include/setk_hip.h): the stand-alone operators on caller
// arrays (covariance, principal vector, beamformer weights, BAN, rank-1 rebuild, beamform,
// directional features) and the PCM / Kaldi compressed-matrix conversions.
#include "capi.h"

using namespace setk;

namespace {

constexpr int kKindPevd = 100;

int pitch_of(int F) { return (F == kBins) ? kBinsPad : ((F + 7) / 8) * 8; }

// the caller has selected the device; the arena is recycled here
int run_weights(setk_handle_t h, const setk_bf_opts& o, int kind, const float* Rs, const float* Rn,
                const float* Ry, int F, int C_in, float* weight, int* status, int* ref_out,
                hipStream_t s, bool reset = true) {
    // 8 < C <= 16: embedded in 16 x 16 problems, blkdiag(Rs, 0) / blkdiag(Rn, max diag(Rn) I):
    // same solution in the first C components, 16 lanes per problem (solve.hip)
    const int C = C_in > kMaxChannels ? kMaxChannels16 : C_in;
    const int NP = npairs(C);
    const int pitch = pitch_of(F);
    const bool mpdr = (kind == SETK_BF_MPDR || kind == SETK_BF_MPDR_WHITEN);
    const int planes = mpdr ? 6 * NP : (Rn ? 4 * NP : 2 * NP);
    if (reset) arena_reset(h, s);
    const float *d_Rs, *d_Rn = nullptr, *d_Ry = nullptr;
    const size_t nmat = (size_t)F * C_in * C_in * 2;
    SETK_TRY(stage_in(h, Rs, nmat, s, &d_Rs));
    if (Rn) SETK_TRY(stage_in(h, Rn, nmat, s, &d_Rn));
    if (Ry) SETK_TRY(stage_in(h, Ry, nmat, s, &d_Ry));
    float *d_planes, *d_w;
    int* d_bin;
    SETK_TRY(arena_get(h, (size_t)planes * pitch * 4, &d_planes));
    SETK_TRY(arena_get(h, (size_t)C * pitch * 8, &d_w));
    SETK_TRY(arena_get(h, (size_t)F * 4, &d_bin));
    HIP_TRY(h, hipMemsetAsync(d_planes, 0, (size_t)planes * pitch * 4, s));
    HIP_TRY(h, launch_pack_covar(d_Rs, F, C_in, C, 0.f, d_planes, 0, s));
    if (d_Rn) HIP_TRY(h, launch_pack_covar(d_Rn, F, C_in, C, 1.f, d_planes, 2 * NP, s));
    if (d_Ry) HIP_TRY(h, launch_pack_covar(d_Ry, F, C_in, C, 1.f, d_planes, 4 * NP, s));
    OutBuf ob;
    SETK_TRY(stage_out(h, weight, (size_t)F * C_in * sizeof(float2), &ob));
    SolveArgs a;
    memset(&a, 0, sizeof(a));
    a.covar = d_planes;
    a.weight = d_w;
    a.bin_status = d_bin;
    a.n_utts = 1;
    a.num_bins = F;
    a.num_channels = C;
    a.planes = planes;
    a.kind = kind;
    a.flags = o.flags;
    a.rank1 = o.rank1;
    a.pmwf_ref = o.pmwf_ref;
    a.pmwf_beta = o.pmwf_beta;
    int* d_ref = nullptr;
    if (kind == SETK_BF_PMWF && o.pmwf_ref < 0) {
        SETK_TRY(arena_get(h, (size_t)F * C * 2 * sizeof(double), &a.snr_acc));
        SETK_TRY(arena_get(h, (size_t)F * C * C * 8, &a.wmat));
        SETK_TRY(arena_get(h, sizeof(int), &d_ref));
    }
    HIP_TRY(h, launch_solve(a, s));
    if (kind == SETK_BF_PMWF && o.pmwf_ref < 0) HIP_TRY(h, launch_pmwf_select(a, d_ref, s));
    HIP_TRY(h, launch_unpack_weight(d_w, F, C_in, static_cast<float*>(ob.dev), s));
    SETK_TRY(copy_back(h, ob, s));
    bool sync_owed = ob.host;
    if (status) SETK_TRY(copy_out(h, status, d_bin, F * 4, s, &sync_owed));
    if (ref_out) {
        // (host memory by contract: the fixed reference is stored through the pointer)
        if (d_ref)
            HIP_TRY(h, hipMemcpyAsync(ref_out, d_ref, 4, hipMemcpyDeviceToHost, s));
        else
            *ref_out = o.pmwf_ref;
        sync_owed = true;
    }
    if (sync_owed) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // namespace

namespace setk {
int pevd_in_arena(setk_handle_t h, const float* d_Rs, int F, int C, float* d_pvec, int* d_status,
                  hipStream_t s) {
    setk_bf_opts o;
    memset(&o, 0, sizeof(o));
    return run_weights(h, o, kKindPevd, d_Rs, nullptr, nullptr, F, C, d_pvec, d_status, nullptr, s, false);
}
}  // namespace setk

extern "C" {

int setk_covar(setk_handle_t h, const float* spec, const float* mask, int num_channels,
               int num_frames, int num_bins, float* covar, void* stream) {
    if (!h || !spec || !mask || !covar || num_frames <= 0 || num_bins <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    if (num_channels < 1 || num_channels > kMaxChannels16)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 16");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const int C = num_channels, T = num_frames, F = num_bins;
    const float *d_spec, *d_mask;
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &d_spec));
    SETK_TRY(stage_in(h, mask, (size_t)T * F, s, &d_mask));
    OutBuf ob;
    SETK_TRY(stage_out(h, covar, (size_t)F * C * C * sizeof(float2), &ob));
    const int split = std::max(1, std::min(64, (T + 31) / 32));
    const int pitch = ((F + 7) / 8) * 8;
    float* d_part;
    SETK_TRY(arena_get(h, (size_t)split * (2 * npairs(C) + 1) * pitch * 4, &d_part));
    const int per = (T + split - 1) / split;
    const int used = (T + per - 1) / per;
    HIP_TRY(h, launch_covar_spec(C, d_spec, d_mask, T, F, d_part, split, s));
    HIP_TRY(h, launch_covar_spec_finalize(C, d_part, used, F, static_cast<float*>(ob.dev), s));
    return finish_out(h, ob, s);
}

int setk_pevd(setk_handle_t h, const float* Rs, const float* Rn, int num_bins, int num_channels,
              int flags, float* pvec, int* status, void* stream) {
    if (!h || !Rs || !pvec || num_bins <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    if (num_channels < 1 || num_channels > kMaxChannels16)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 16");
    HIP_TRY(h, hipSetDevice(h->device));
    setk_bf_opts o;
    memset(&o, 0, sizeof(o));
    o.flags = flags & SETK_FLAG_NO_GAUGE;
    return run_weights(h, o, kKindPevd, Rs, Rn, nullptr, num_bins, num_channels, pvec, status,
                       nullptr, static_cast<hipStream_t>(stream));
}

int setk_weights(setk_handle_t h, const setk_bf_opts* opts, const float* Rs, const float* Rn,
                 const float* Ry, int num_bins, int num_channels, float* weight, int* status,
                 int* ref_out, void* stream) {
    if (!h || !opts || !Rs || !weight || num_bins <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    if (num_channels < 1 || num_channels > kMaxChannels16)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 16");
    const int kind = opts->kind;
    const bool mpdr = (kind == SETK_BF_MPDR || kind == SETK_BF_MPDR_WHITEN);
    const char* operands = (mpdr && !Ry)                      ? "MPDR needs Ry"
                           : (kind != SETK_BF_MPDR && !Rn) ? "Rn is required"
                                                              : nullptr;
    SETK_TRY(check_bf_opts(h, *opts, num_channels, SETK_ERR_INVALID, operands));
    HIP_TRY(h, hipSetDevice(h->device));
    return run_weights(h, *opts, kind, Rs, Rn, Ry, num_bins, num_channels, weight, status,
                       ref_out, static_cast<hipStream_t>(stream));
}

int setk_ban(setk_handle_t h, const float* weight, const float* Rn, int num_bins,
             int num_channels, float* out, void* stream) {
    if (!h || !weight || !Rn || !out || num_bins <= 0 || num_channels <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const int F = num_bins, C = num_channels;
    const float *d_w, *d_Rn;
    SETK_TRY(stage_in(h, weight, (size_t)F * C * 2, s, &d_w));
    SETK_TRY(stage_in(h, Rn, (size_t)F * C * C * 2, s, &d_Rn));
    OutBuf ob;
    SETK_TRY(stage_out(h, out, (size_t)F * C * sizeof(float2), &ob));
    HIP_TRY(h, launch_ban(d_w, d_Rn, F, C, static_cast<float*>(ob.dev), s));
    return finish_out(h, ob, s);
}

int setk_pcm16_to_float(setk_handle_t h, const int16_t* pcm, int num_channels, int num_samples,
                        float* audio, void* stream) {
    if (!h || !pcm || !audio || num_channels <= 0 || num_samples <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const size_t n16 = (size_t)num_channels * num_samples;
    const int16_t* d_pcm;
    SETK_TRY(stage_in(h, pcm, n16, s, &d_pcm));
    OutBuf ob;
    SETK_TRY(stage_out(h, audio, n16 * sizeof(float), &ob));
    HIP_TRY(h, launch_pcm16_to_float(d_pcm, num_channels, num_samples,
                                     static_cast<float*>(ob.dev), s));
    return finish_out(h, ob, s);
}

int setk_float_to_pcm16(setk_handle_t h, const float* audio, int num_channels, int num_samples,
                        int16_t* pcm, void* stream) {
    if (!h || !pcm || !audio || num_channels <= 0 || num_samples <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const size_t n = (size_t)num_channels * num_samples;
    const float* d_in;
    SETK_TRY(stage_in(h, audio, n, s, &d_in));
    OutBuf ob;
    SETK_TRY(stage_out(h, pcm, n * sizeof(int16_t), &ob));
    HIP_TRY(h, launch_float_to_pcm16(d_in, num_channels, num_samples, static_cast<int16_t*>(ob.dev), s));
    return finish_out(h, ob, s);
}

int setk_pcm16_to_float_batch(setk_handle_t h, int n_utts, int num_channels,
                              const int16_t* const* pcm, const int* num_samples,
                              float* const* audio, double* power0, void* stream) {
    if (!h || n_utts <= 0 || num_channels <= 0 || !pcm || !num_samples || !audio)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    std::vector<char> tbl(pcm_item_bytes() * n_utts);
    int max_n = 0;
    for (int u = 0; u < n_utts; ++u) {
        if (!pcm[u] || !audio[u] || num_samples[u] <= 0)
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        pcm_item_fill(tbl.data(), u, pcm[u], audio[u], num_samples[u]);
        max_n = std::max(max_n, num_samples[u]);
    }
    const char* d_tbl;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    if (power0) HIP_TRY(h, hipMemsetAsync(power0, 0, (size_t)n_utts * sizeof(double), s));
    HIP_TRY(h, launch_pcm16_to_float_batch(d_tbl, n_utts, num_channels, max_n, power0, s));
    return SETK_OK;
}

int setk_pcm16_channel_stride(int num_samples) { return num_samples <= 0 ? 0 : ((num_samples + 7) & ~7); }

int setk_pcm16_deinterleave_batch(setk_handle_t h, int n_utts, int num_channels,
                                  const int16_t* const* pcm, const int* num_samples,
                                  int16_t* const* out, double* power0, void* stream) {
    if (!h || n_utts <= 0 || num_channels <= 0 || !pcm || !num_samples || !out)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    std::vector<char> tbl(pcm_item_bytes() * n_utts);
    int max_n = 0;
    for (int u = 0; u < n_utts; ++u) {
        if (!pcm[u] || !out[u] || num_samples[u] <= 0)
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        pcm_item_fill_planar(tbl.data(), u, pcm[u], out[u], num_samples[u],
                             setk_pcm16_channel_stride(num_samples[u]));
        max_n = std::max(max_n, num_samples[u]);
    }
    const char* d_tbl;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    if (power0) HIP_TRY(h, hipMemsetAsync(power0, 0, (size_t)n_utts * sizeof(double), s));
    HIP_TRY(h, launch_pcm16_deinterleave_batch(d_tbl, n_utts, num_channels, max_n, power0, s));
    return SETK_OK;
}

int setk_kaldi_cm_decode_batch(setk_handle_t h, int n, const int* kinds, const float* vmin, const float* vrange,
                               const int* rows, const int* cols, const int* transpose,
                               const void* const* src, float* const* dst, void* stream) {
    if (!h || n <= 0 || !kinds || !vmin || !vrange || !rows || !cols || !src || !dst)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    std::vector<char> tbl(cm_item_bytes() * n);
    long max_elems = 0;
    for (int i = 0; i < n; ++i) {
        if (!src[i] || !dst[i] || rows[i] <= 0 || cols[i] <= 0) return fail(h, SETK_ERR_INVALID, "null or empty matrix");
        if (kinds[i] < SETK_KALDI_CM || kinds[i] > SETK_KALDI_CM3)
            return fail(h, SETK_ERR_UNSUPPORTED, "compressed matrix kind: 1 (CM), 2 (CM2) or 3 (CM3)");
        if (kinds[i] != SETK_KALDI_CM3 && (reinterpret_cast<uintptr_t>(src[i]) & 1))
            return fail(h, SETK_ERR_INVALID, "CM / CM2 bodies must be 2-byte aligned");
        cm_item_fill(tbl.data(), i, src[i], dst[i], vmin[i], vrange[i], rows[i], cols[i], kinds[i],
                     transpose ? transpose[i] : 0);
        max_elems = std::max(max_elems, (long)rows[i] * cols[i]);
    }
    const char* d_tbl;
    SETK_TRY(upload(h, tbl, s, &d_tbl));
    HIP_TRY(h, launch_kaldi_cm_decode_batch(d_tbl, n, max_elems, s));
    return SETK_OK;
}

int setk_rank1(setk_handle_t h, const float* Rs, const float* Rn, int num_bins,
               int num_channels, float* out, int* status, void* stream) {
    if (!h || !Rs || !out || num_bins <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    if (num_channels < 1 || num_channels > kMaxChannels16)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 16");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(h, hipSetDevice(h->device));
    const int F = num_bins, C = num_channels;
    // principal vectors first (device resident), then the rebuild kernel
    float* d_pv = nullptr;
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&d_pv), (size_t)F * C * sizeof(float2)));
    setk_bf_opts o;
    memset(&o, 0, sizeof(o));
    o.flags = SETK_FLAG_NO_GAUGE;
    int rc = run_weights(h, o, kKindPevd, Rs, Rn, nullptr, F, C, d_pv, status, nullptr, s);
    if (rc == SETK_OK) {
        arena_reset(h, s);
        const float *d_Rs, *d_Rn = nullptr;
        rc = stage_in(h, Rs, (size_t)F * C * C * 2, s, &d_Rs);
        if (rc == SETK_OK && Rn) rc = stage_in(h, Rn, (size_t)F * C * C * 2, s, &d_Rn);
        OutBuf ob;
        if (rc == SETK_OK) rc = stage_out(h, out, (size_t)F * C * C * sizeof(float2), &ob);
        if (rc == SETK_OK) {
            hipError_t e = launch_rank1(d_pv, d_Rs, d_Rn, F, C, static_cast<float*>(ob.dev), s);
            if (e != hipSuccess) rc = fail(h, SETK_ERR_HIP, hipGetErrorString(e));
        }
        if (rc == SETK_OK) rc = copy_back(h, ob, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_pv);
    return rc;
}

int setk_beamform(setk_handle_t h, const float* weight, const float* spec, int num_channels,
                  int num_frames, int num_bins, float* out, void* stream) {
    if (!h || !weight || !spec || !out || num_channels <= 0 || num_frames <= 0 || num_bins <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const int C = num_channels, T = num_frames, F = num_bins;
    const float *d_w, *d_spec;
    SETK_TRY(stage_in(h, weight, (size_t)F * C * 2, s, &d_w));
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &d_spec));
    OutBuf ob;
    SETK_TRY(stage_out(h, out, (size_t)T * F * sizeof(float2), &ob));
    HIP_TRY(h, launch_beamform_spec(d_w, d_spec, C, T, F, static_cast<float*>(ob.dev), s));
    return finish_out(h, ob, s);
}

int setk_directional_feats(setk_handle_t h, const float* spec, const float* steer_vector,
                           const int* pairs, int n_pairs, int num_channels, int num_frames,
                           int num_bins, float* out, void* stream) {
    if (!h || !spec || !steer_vector || !pairs || !out || n_pairs <= 0 || num_channels <= 0 ||
        num_frames <= 0 || num_bins <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    for (int p = 0; p < 2 * n_pairs; ++p)
        if (pairs[p] < 0 || pairs[p] >= num_channels)
            return fail(h, SETK_ERR_INVALID, "microphone pair out of range");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const int C = num_channels, T = num_frames, F = num_bins;
    const float *d_spec, *d_sv;
    SETK_TRY(stage_in(h, spec, (size_t)C * T * F * 2, s, &d_spec));
    SETK_TRY(stage_in(h, steer_vector, (size_t)F * C * 2, s, &d_sv));
    const int* d_pairs;
    SETK_TRY(upload(h, pairs, (size_t)2 * n_pairs, s, &d_pairs));
    OutBuf ob;
    SETK_TRY(stage_out(h, out, (size_t)T * F * sizeof(float), &ob));
    HIP_TRY(h, launch_directional_feats(d_spec, d_sv, d_pairs, n_pairs, C, T, F,
                                        static_cast<float*>(ob.dev), s));
    SETK_TRY(copy_back(h, ob, s));
    // (`pairs` went through the handle's page-locked buffer: upload() has copied it)  Host
    // operands are pageable copies queued on the stream: drained before they may be released;
    // with device operands the call is asynchronous like the other stand-alone operators
    // (a staged operand is one stage_in gave an arena twin)
    if (ob.host || d_spec != spec || d_sv != steer_vector) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
