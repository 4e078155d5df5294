// capi_fused.hip -- front end (include/setk_hip.h): the fused path on waveforms,
// setk_enhance_batch / setk_enhance_batch_taps (STFT + covariances, weights, beamform + iSTFT,
// renorm: four stream-ordered stages per batch) and setk_apply_weights_batch.
#include "capi.h"

using namespace setk;

namespace {

// setk_enhance_batch(_taps) for 9 to 16 channels (wide.hip): the spectra make one round trip
// through the arena in the bin-major layout -- STFT, covariances on the fp32 matrix cores,
// their reduction into the solve's 16-lane planes, the solve as it is, the beamformer on the
// spectra, the iSTFT-only pass 2, renorm.  Arguments and options have been checked.
int enhance_wide(setk_handle_t h, const setk_bf_opts* opts, int n_utts, int C, const float* const* audio,
                 const int* num_samples, const float* const* mask_s, const float* const* mask_n,
                 void* const* wave, int* status, const setk_batch_taps* taps, hipStream_t s) {
    const int kind = opts->kind;
    const bool mpdr = (kind == SETK_BF_MPDR || kind == SETK_BF_MPDR_WHITEN);
    const bool pcm16 = (opts->flags & SETK_FLAG_OUT_PCM16) != 0;
    constexpr int Cp = kMaxChannels16, NP = npairs(kMaxChannels16);
    const int planes_out = mpdr ? 6 * NP : 4 * NP;

    // ---- descriptors and work lists: [0] STFT, covariance, beamformer; [1] iSTFT ----
    std::vector<UttDesc> uds = zeroed_utts(n_utts), yds = zeroed_utts(n_utts);
    std::vector<WorkItem> items_stft, items_cov, items_istft;
    int max_len = 0, max_samples = 0, max_frames = 0, nparts_total = 0;
    for (int u = 0; u < n_utts; ++u) {
        UttDesc& ud = uds[u];
        if (!audio[u] || !mask_s[u] || !wave[u] || (mask_n && !mask_n[u]))
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T < 0) return T;
        ud.audio = audio[u];
        ud.mask_s = mask_s[u];
        ud.mask_n = mask_n ? mask_n[u] : nullptr;
        ud.num_samples = num_samples[u];
        ud.num_frames = T;
        ud.out_len = setk_istft_num_samples(h, T, -1);
        ud.part0 = nparts_total;
        ud.nparts = push_items(&items_cov, u, T, kWideSlab, kWideSlab, &nparts_total);
        push_items(&items_stft, u, T, 64, 64);
        push_items(&items_istft, u, T, 128, kSuperTile);
        max_len = std::max(max_len, ud.out_len);
        max_samples = std::max(max_samples, ud.num_samples);
        max_frames = std::max(max_frames, T);
        yds[u].mask_s = ud.mask_s;
        yds[u].num_frames = T;
        yds[u].out_len = ud.out_len;
        yds[u].wave_out = wave[u];
    }

    // ---- scratch: everything is taken before anything is launched ----
    SETK_TRY(carve_wave_f32(h, yds, wave, pcm16));
    for (int u = 0; u < n_utts; ++u) {
        const size_t T = (size_t)uds[u].num_frames, Tp = (T + 3) & ~(size_t)3;
        float *xb, *y;
        SETK_TRY(arena_get(h, std::max<size_t>((size_t)kBins * C * Tp * sizeof(float2), 256), &xb));
        SETK_TRY(arena_get(h, std::max<size_t>(T * kBins * sizeof(float2), 256), &y));
        uds[u].wave_out = xb;
        uds[u].wave_f32 = y;
        yds[u].audio = y;  // ISTFT mode: per-item spectrogram
    }
    float *d_part, *d_covar, *d_w;
    unsigned* d_small;
    SETK_TRY(arena_get(h, std::max<size_t>((size_t)nparts_total * kBins * kWidePartFloats * 4, 256), &d_part));
    SETK_TRY(arena_get(h, (size_t)n_utts * planes_out * kBinsPad * 4, &d_covar));
    SETK_TRY(arena_get(h, (size_t)n_utts * Cp * kBinsPad * 8, &d_w));
    SETK_TRY(arena_get(h, (size_t)n_utts * 3 * 4, &d_small));
    unsigned* d_norm = d_small;
    unsigned* d_omax = d_small + n_utts;
    int* d_status = reinterpret_cast<int*>(d_small + 2 * n_utts);
    SolveArgs sa;
    memset(&sa, 0, sizeof(sa));
    const bool snr_ref = kind == SETK_BF_PMWF && opts->pmwf_ref < 0;
    if (snr_ref) {
        SETK_TRY(arena_get(h, (size_t)n_utts * kBins * Cp * 2 * sizeof(double), &sa.snr_acc));
        SETK_TRY(arena_get(h, (size_t)n_utts * kBins * Cp * Cp * 8, &sa.wmat));
    }
    OutBuf tap_rs, tap_rn, tap_w;
    if (taps && taps->Rs) SETK_TRY(stage_out(h, taps->Rs, (size_t)n_utts * kBins * C * C * sizeof(float2), &tap_rs));
    if (taps && taps->Rn) SETK_TRY(stage_out(h, taps->Rn, (size_t)n_utts * kBins * C * C * sizeof(float2), &tap_rn));
    if (taps && taps->weight) SETK_TRY(stage_out(h, taps->weight, (size_t)n_utts * kBins * C * sizeof(float2), &tap_w));
    DescTables t_stft, t_istft;
    const WorkItem* d_items_cov;
    SETK_TRY(upload_tables(h, uds, items_stft, s, &t_stft));
    SETK_TRY(upload(h, items_cov, s, &d_items_cov));
    SETK_TRY(upload_tables(h, yds, items_istft, s, &t_istft));
    HIP_TRY(h, hipMemsetAsync(d_small, 0, (size_t)n_utts * 3 * 4, s));

    SETK_TRY(profile_begin(h, s));

    // ---- stage 1: STFT into the bin-major layout, max |audio|, covariances ----
    Pass1Args p1 = pass1_args(h, t_stft.utts, t_stft.items);
    HIP_TRY(h, launch_stft_binmajor(C, p1, t_stft.n_items, s));
    HIP_TRY(h, launch_maxabs(t_stft.utts, C, d_norm, n_utts, max_samples, s));
    WideArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.utts = t_stft.utts;
    wa.items = d_items_cov;
    wa.partials = d_part;
    wa.covar = d_covar;
    wa.weight = d_w;
    wa.num_channels = C;
    wa.with_ry = mpdr ? 1 : 0;
    wa.flags = opts->flags;
    HIP_TRY(h, launch_covar_wide(wa, (int)items_cov.size(), s));
    HIP_TRY(h, launch_wide_finalize(wa, n_utts, s));
    SETK_TRY(profile_mark(h, 1, s));
    if (tap_rs.dev) {
        HIP_TRY(h, launch_wide_unpack_covar(d_covar, n_utts, planes_out, 0, C, static_cast<float*>(tap_rs.dev), s));
        SETK_TRY(copy_back(h, tap_rs, s));
    }
    if (tap_rn.dev) {
        HIP_TRY(h, launch_wide_unpack_covar(d_covar, n_utts, planes_out, 2 * NP, C, static_cast<float*>(tap_rn.dev), s));
        SETK_TRY(copy_back(h, tap_rn, s));
    }

    // ---- stage 2: weights, the 16-lane form on the padded problems ----
    sa.covar = d_covar;
    sa.weight = d_w;
    sa.status = d_status;
    sa.n_utts = n_utts;
    sa.num_bins = kBins;
    sa.num_channels = Cp;
    sa.planes = planes_out;
    sa.kind = kind;
    sa.flags = opts->flags;
    sa.rank1 = opts->rank1;
    sa.pmwf_ref = opts->pmwf_ref;
    sa.pmwf_beta = opts->pmwf_beta;
    sa.num_scale = 1.f;
    HIP_TRY(h, launch_solve(sa, s));
    if (snr_ref) HIP_TRY(h, launch_pmwf_select(sa, nullptr, s));
    SETK_TRY(profile_mark(h, 2, s));
    if (tap_w.dev) {
        HIP_TRY(h, launch_wide_unpack_weight(d_w, n_utts, C, static_cast<float*>(tap_w.dev), s));
        SETK_TRY(copy_back(h, tap_w, s));
    }

    // ---- stage 3: beamform on the spectra, inverse STFT ----
    HIP_TRY(h, launch_beamform_binmajor(wa, n_utts, max_frames, s));
    HIP_TRY(h, launch_pass2(1, true, pass2_args(h, t_istft.utts, t_istft.items, d_omax), t_istft.n_items, s));
    SETK_TRY(profile_mark(h, 3, s));

    // ---- stage 4: renorm ----
    HIP_TRY(h, launch_scale(scale_args(t_istft.utts, d_norm, d_omax, pcm16), n_utts, max_len, s));
    SETK_TRY(profile_mark(h, 4, s));
    bool sync_owed = true;  // the descriptors live in the arena: the call drains
    if (taps && taps->maxabs) SETK_TRY(copy_out(h, taps->maxabs, d_norm, (size_t)n_utts * 4, s, &sync_owed));
    if (status) SETK_TRY(copy_out(h, status, d_status, (size_t)n_utts * 4, s, &sync_owed));
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_apply_weights_batch(setk_handle_t h, int n_utts, int num_channels,
                             const float* const* audio, const int* num_samples,
                             const float* weights, int n_sets, const int* weight_index,
                             void* const* wave, int flags, void* stream) {
    if (!h || n_utts <= 0 || !audio || !num_samples || !weights || n_sets <= 0 || !wave)
        return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int C = num_channels;
    if (C < 1 || C > kMaxChannels) return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 8");
    if (weight_index)
        for (int u = 0; u < n_utts; ++u)
            if (weight_index[u] < 0 || weight_index[u] >= n_sets)
                return fail(h, SETK_ERR_INVALID, "weight index out of range");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const bool pcm16 = (flags & SETK_FLAG_OUT_PCM16) != 0;

    std::vector<UttDesc> uds = zeroed_utts(n_utts);
    std::vector<WorkItem> items;
    std::vector<int> all_frames(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        all_frames[u] = setk_stft_num_frames(h, num_samples[u]);
        if (all_frames[u] < 0) return all_frames[u];
    }
    const int target = choose_target(all_frames, h->p2_items, kSuperTile, kSuperTile * 4);
    int max_len = 0, max_samples = 0;
    for (int u = 0; u < n_utts; ++u) {
        UttDesc& ud = uds[u];
        if (!audio[u] || !wave[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        ud.audio = audio[u];
        ud.num_samples = num_samples[u];
        ud.num_frames = all_frames[u];
        ud.out_len = setk_istft_num_samples(h, ud.num_frames, -1);
        ud.wave_out = wave[u];
        max_len = std::max(max_len, ud.out_len);
        max_samples = std::max(max_samples, ud.num_samples);
        push_items(&items, u, ud.num_frames, target, kSuperTile);
    }
    SETK_TRY(carve_wave_f32(h, uds, wave, pcm16));
    DescTables t;
    SETK_TRY(upload_tables(h, uds, items, s, &t));
    const int* d_idx = nullptr;
    if (weight_index) SETK_TRY(upload(h, weight_index, (size_t)n_utts, s, &d_idx));
    const float* d_sets;
    SETK_TRY(stage_in(h, weights, (size_t)n_sets * kBins * C * 2, s, &d_sets));
    float* d_w;
    unsigned* d_norm;
    SETK_TRY(arena_get(h, (size_t)n_utts * C * kBinsPad * sizeof(float2), &d_w));
    SETK_TRY(arena_get(h, (size_t)2 * n_utts * sizeof(unsigned), &d_norm));
    unsigned* d_omax = d_norm + n_utts;
    HIP_TRY(h, hipMemsetAsync(d_norm, 0, (size_t)2 * n_utts * sizeof(unsigned), s));
    // norm stays 0 with SETK_FLAG_NO_RENORM: scale_kernel then only converts the sample type
    if (!(flags & SETK_FLAG_NO_RENORM))
        HIP_TRY(h, launch_maxabs(t.utts, C, d_norm, n_utts, max_samples, s));
    HIP_TRY(h, launch_pack_fixed_weights(d_sets, d_idx, n_utts, C, d_w, s));

    Pass2Args p2 = pass2_args(h, t.utts, t.items, d_omax);
    p2.weight = d_w;
    HIP_TRY(h, launch_pass2(C, false, p2, t.n_items, s));
    HIP_TRY(h, launch_scale(scale_args(t.utts, d_norm, d_omax, pcm16), n_utts, max_len, s));
    // the uploaded descriptors live in the arena: the next call on this handle may
    // reuse it, so this one must have drained
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_enhance_batch(setk_handle_t h, const setk_bf_opts* opts, int n_utts, int num_channels,
                       const float* const* audio, const int* num_samples,
                       const float* const* mask_s, const float* const* mask_n,
                       void* const* wave, int* status, void* stream) {
    return setk_enhance_batch_taps(h, opts, n_utts, num_channels, audio, num_samples, mask_s,
                                   mask_n, wave, status, nullptr, stream);
}

int setk_enhance_batch_taps(setk_handle_t h, const setk_bf_opts* opts, int n_utts,
                            int num_channels, const float* const* audio, const int* num_samples,
                            const float* const* mask_s, const float* const* mask_n,
                            void* const* wave, int* status, const setk_batch_taps* taps,
                            void* stream) {
    if (!h || !opts || n_utts <= 0 || !audio || !num_samples || !mask_s || !wave)
        return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int C = num_channels;
    if (C < 1 || C > kMaxChannels16) return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 16");
    const int kind = opts->kind;
    const bool mpdr = (kind == SETK_BF_MPDR || kind == SETK_BF_MPDR_WHITEN);
    SETK_TRY(check_bf_opts(h, *opts, C, SETK_ERR_UNSUPPORTED,
                           (mpdr && mask_n) ? "fused MPDR derives Ry from mask_s + (1 - mask_s); use the modular API "
                                              "with an interferer mask"
                                            : nullptr));
    const bool in_pcm = (opts->flags & SETK_FLAG_IN_PCM16) != 0;
    if (in_pcm && C > kMaxChannels)
        return fail(h, SETK_ERR_UNSUPPORTED,
                    "16-bit PCM input (SETK_FLAG_IN_PCM16) is taken for up to 8 channels; convert with "
                    "setk_pcm16_to_float_batch");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    if (C > kMaxChannels)
        return enhance_wide(h, opts, n_utts, C, audio, num_samples, mask_s, mask_n, wave, status, taps, s);
    const bool pcm16 = (opts->flags & SETK_FLAG_OUT_PCM16) != 0;
    const int NP = npairs(C);
    const StftGeom g = geom_of(h);

    // ---- descriptors and work lists ----
    std::vector<UttDesc> uds = zeroed_utts(n_utts);
    std::vector<WorkItem> items1, items2;
    int max_len = 0;
    std::vector<int> all_frames(n_utts);
    for (int u = 0; u < n_utts; ++u) {
        all_frames[u] = setk_stft_num_frames(h, num_samples[u]);
        if (all_frames[u] < 0) return all_frames[u];
    }
    const int target1 = choose_target(all_frames, h->p1_items, pass1_tile_frames(C), pass1_tile_frames(C) * 8);
    // pass 2 on the matrix cores: hop = n_fft / 2 only (wave-resident overlap-add, pass2_mc.hip)
    const bool mc2 = h->mc_enabled && 2 * g.hop == kNfft && g.keep == 1 &&
                     !(getenv("SETK_MC_PASS2") && atoi(getenv("SETK_MC_PASS2")) == 0);
    if (in_pcm && !mc2)
        return fail(h, SETK_ERR_UNSUPPORTED,
                    "16-bit PCM input (SETK_FLAG_IN_PCM16) needs hop = n_fft / 2 and the matrix-core "
                    "pass 2; convert with setk_pcm16_to_float_batch");
    const int quant2 = mc2 ? 8 : kSuperTile;
    const int target2 = mc2 ? choose_target(all_frames, h->mc_p2_items > 0 ? h->mc_p2_items : h->mc_cus * pass2_mc_wgs_per_cu(C, in_pcm), quant2, 64)
                            : choose_target(all_frames, h->p2_items, kSuperTile, kSuperTile * 4);
    int nparts_total = 0, max_parts = 0;
    for (int u = 0; u < n_utts; ++u) {
        UttDesc& ud = uds[u];
        if (!audio[u] || !mask_s[u] || !wave[u] || (mask_n && !mask_n[u]))
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        ud.audio = audio[u];
        ud.audio_fmt = in_pcm ? kAudioPcm16 : kAudioF32;
        ud.ch_stride = in_pcm ? setk_pcm16_channel_stride(num_samples[u]) : num_samples[u];
        if (in_pcm && (reinterpret_cast<uintptr_t>(audio[u]) & 3))
            return fail(h, SETK_ERR_INVALID, "16-bit PCM input must be 4-byte aligned");
        ud.mask_s = mask_s[u];
        ud.mask_n = mask_n ? mask_n[u] : nullptr;
        ud.num_samples = num_samples[u];
        ud.num_frames = all_frames[u];
        ud.out_len = setk_istft_num_samples(h, ud.num_frames, -1);
        ud.wave_out = wave[u];
        max_len = std::max(max_len, ud.out_len);
        ud.part0 = nparts_total;
        ud.nparts = push_items(&items1, u, ud.num_frames, target1, pass1_tile_frames(C), &nparts_total);
        max_parts = std::max(max_parts, ud.nparts);
        push_items(&items2, u, ud.num_frames, target2, quant2);
    }
    SETK_TRY(carve_wave_f32(h, uds, wave, pcm16));
    // descriptors: [uds | items1 | items2], cached on the device while unchanged
    const size_t b_ud = uds.size() * sizeof(UttDesc);
    const size_t b_i1 = items1.size() * sizeof(WorkItem);
    const size_t b_i2 = items2.size() * sizeof(WorkItem);
    std::vector<char> blob(b_ud + b_i1 + b_i2);
    memcpy(blob.data(), uds.data(), b_ud);
    memcpy(blob.data() + b_ud, items1.data(), b_i1);
    memcpy(blob.data() + b_ud + b_i1, items2.data(), b_i2);
    if (blob != h->desc_cache) {
        if (blob.size() > h->d_desc_cap) {
            HIP_TRY(h, hipStreamSynchronize(s));
            if (h->d_desc) (void)hipFree(h->d_desc);
            h->d_desc = nullptr;
            h->d_desc_cap = 0;
            HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_desc), blob.size() * 2));
            h->d_desc_cap = blob.size() * 2;
        }
        // ordered on the stream behind the previous call's kernels (which read the old
        // contents) and ahead of this call's; a previous call on ANOTHER stream was drained
        // by arena_reset.  No host synchronisation: the launching thread runs ahead.
        HIP_TRY(h, h2d_small(h, h->d_desc, blob.data(), blob.size(), s));
        h->desc_cache.swap(blob);
    }
    const UttDesc* d_uds = reinterpret_cast<const UttDesc*>(h->d_desc);
    const WorkItem* d_items1 = reinterpret_cast<const WorkItem*>(h->d_desc + b_ud);
    const WorkItem* d_items2 = reinterpret_cast<const WorkItem*>(h->d_desc + b_ud + b_i1);

    // ---- scratch ----
    const int planes_out = mpdr ? 6 * NP : 4 * NP;
    float *d_part, *d_covar, *d_w;
    unsigned* d_small;
    SETK_TRY(arena_get(h, (size_t)nparts_total * nplanes_partial(C) * kBinsPad * 4, &d_part));
    SETK_TRY(arena_get(h, (size_t)n_utts * planes_out * kBinsPad * 4, &d_covar));
    SETK_TRY(arena_get(h, (size_t)n_utts * C * kBinsPad * 8, &d_w));
    SETK_TRY(arena_get(h, (size_t)n_utts * 3 * 4, &d_small));
    unsigned* d_norm = d_small;
    unsigned* d_omax = d_small + n_utts;
    int* d_status = reinterpret_cast<int*>(d_small + 2 * n_utts);
    HIP_TRY(h, hipMemsetAsync(d_small, 0, (size_t)n_utts * 3 * 4, s));

    SETK_TRY(profile_begin(h, s));

    // ---- stage 1: STFT + covariance partials (timed alone), then finalize ----
    Pass1Args p1 = pass1_args(h, d_uds, d_items1);
    p1.partials = d_part;
    p1.norm_bits = d_norm;
    p1.flags = opts->flags;
    p1.mc_tab = h->d_mc_tab;
    p1.mc_win = h->d_mc_win;
    // pass 1 on the matrix cores is opt-in (SETK_MC_PASS1=1): parity-green, but its transform
    // waves are the long pole of the tile pipeline (0.95 ms against 0.88)
    const bool mc1 = !in_pcm && h->mc_enabled && pass1_mc_supported(C, g.hop) && getenv("SETK_MC_PASS1") &&
                     atoi(getenv("SETK_MC_PASS1")) != 0;
    if (in_pcm) p1.window = h->d_window_pcm;
    if (mc1)
        HIP_TRY(h, launch_pass1_mc(C, p1, (int)items1.size(), s));
    else
        HIP_TRY(h, launch_pass1(C, false, p1, (int)items1.size(), s, in_pcm));
    SETK_TRY(profile_mark(h, 1, s));
    FinalizeArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.utts = d_uds;
    fa.partials = d_part;
    fa.covar = d_covar;
    fa.num_channels = C;
    fa.with_ry = mpdr ? 1 : 0;
    fa.num_scale = mc1 ? (float)((h->mc_peak / 1024.0) * (h->mc_peak / 1024.0)) : 1.f;
    // With a few slabs per utterance (the shard of the bench: two) the solve sums them itself and
    // this launch -- 26 us of an 87 us stage, mostly launch and tail -- falls away.  Not when the
    // covariances are tapped, not for PMWF's reference search (never measured fused; its
    // select kernel used to read Rn back for BAN), not for long utterances (32 slabs: the parallel reduction is the better one).
    const bool fuse_reduce = !(taps && (taps->Rs || taps->Rn)) && max_parts <= 4 &&
                             !(kind == SETK_BF_PMWF && opts->pmwf_ref < 0) &&
                             !(getenv("SETK_FUSED_REDUCE") && atoi(getenv("SETK_FUSED_REDUCE")) == 0);
    if (!fuse_reduce) HIP_TRY(h, launch_finalize(fa, n_utts, s));
    OutBuf tap_rs, tap_rn, tap_w;
    if (taps && taps->Rs) {
        SETK_TRY(stage_out(h, taps->Rs, (size_t)n_utts * kBins * C * C * sizeof(float2), &tap_rs));
        HIP_TRY(h, launch_unpack_covar(d_covar, n_utts, planes_out, 0, kBins, C,
                                       static_cast<float*>(tap_rs.dev), s));
        SETK_TRY(copy_back(h, tap_rs, s));
    }
    if (taps && taps->Rn) {
        SETK_TRY(stage_out(h, taps->Rn, (size_t)n_utts * kBins * C * C * sizeof(float2), &tap_rn));
        HIP_TRY(h, launch_unpack_covar(d_covar, n_utts, planes_out, 2 * NP, kBins, C,
                                       static_cast<float*>(tap_rn.dev), s));
        SETK_TRY(copy_back(h, tap_rn, s));
    }

    // ---- stage 2: weights ----
    SolveArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.covar = d_covar;
    sa.weight = d_w;
    sa.status = d_status;
    sa.n_utts = n_utts;
    sa.num_bins = kBins;
    sa.num_channels = C;
    sa.planes = planes_out;
    sa.kind = kind;
    sa.flags = opts->flags;
    sa.rank1 = opts->rank1;
    sa.pmwf_ref = opts->pmwf_ref;
    sa.pmwf_beta = opts->pmwf_beta;
    sa.partials = fuse_reduce ? d_part : nullptr;
    sa.utts = d_uds;
    sa.num_scale = fa.num_scale;
    if (kind == SETK_BF_PMWF && opts->pmwf_ref < 0) {
        SETK_TRY(arena_get(h, (size_t)n_utts * kBins * C * 2 * sizeof(double), &sa.snr_acc));
        SETK_TRY(arena_get(h, (size_t)n_utts * kBins * C * C * 8, &sa.wmat));
    }
    HIP_TRY(h, launch_solve(sa, s));
    if (kind == SETK_BF_PMWF && opts->pmwf_ref < 0) HIP_TRY(h, launch_pmwf_select(sa, nullptr, s));
    SETK_TRY(profile_mark(h, 2, s));
    if (taps && taps->weight) {
        SETK_TRY(stage_out(h, taps->weight, (size_t)n_utts * kBins * C * sizeof(float2), &tap_w));
        HIP_TRY(h, launch_unpack_weight_batch(d_w, n_utts, kBins, C,
                                              static_cast<float*>(tap_w.dev), s));
        SETK_TRY(copy_back(h, tap_w, s));
    }

    // ---- stage 3: beamform + iSTFT ----
    Pass2Args p2 = pass2_args(h, d_uds, d_items2, d_omax);
    p2.weight = d_w;
    p2.norm_bits = d_norm;
    p2.flags = opts->flags;
    p2.mc_tab = h->d_mc_tab;
    p2.mc_win = h->d_mc_win;
    p2.mc_syn = h->d_mc_syn;
    p2.mc_edge = h->d_mc_edge;
    if (mc2)
        HIP_TRY(h, launch_pass2_mc(C, p2, (int)items2.size(), s, in_pcm));
    else
        HIP_TRY(h, launch_pass2(C, false, p2, (int)items2.size(), s));
    SETK_TRY(profile_mark(h, 3, s));

    // ---- stage 4: renorm ----
    HIP_TRY(h, launch_scale(scale_args(d_uds, d_norm, d_omax, pcm16), n_utts, max_len, s));
    SETK_TRY(profile_mark(h, 4, s));
    bool sync_owed = tap_rs.host || tap_rn.host || tap_w.host;
    // max |audio| per utterance (WaveReader.maxabs): the float bit patterns
    if (taps && taps->maxabs) SETK_TRY(copy_out(h, taps->maxabs, d_norm, (size_t)n_utts * 4, s, &sync_owed));
    if (status) SETK_TRY(copy_out(h, status, d_status, (size_t)n_utts * 4, s, &sync_owed));
    if (sync_owed) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
