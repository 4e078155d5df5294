// capi_online.hip -- front end (include/setk_hip.h): block-online MVDR / GEV beamforming of a
// batch, setk_online_num_chunks and setk_enhance_online_batch.  The stages are setk_enhance_batch's
// (capi_fused.hip) with every chunk of every utterance as a virtual utterance of the weight solve:
// pass 1 on work items cut at the chunk boundaries, the smoothing recursion, the solve, BAN with
// the chunks' own noise covariances, pass 2 with the weight set chosen per frame, renorm
// (kernels: online.hip; pass1.hip, solve.hip unchanged; pass2.hip's ONLINE form).
#include "capi.h"

using namespace setk;

extern "C" {

// ceil(T / chunk_size): the loop count of do_online_beamform (apply_adaptive_beamformer.py:25-47)
int setk_online_num_chunks(setk_handle_t h, int num_samples, int chunk_size) {
    if (!h) return SETK_ERR_INVALID;
    if (chunk_size < 1) return fail(h, SETK_ERR_INVALID, "chunk_size must be at least 1");
    const int T = setk_stft_num_frames(h, num_samples);
    if (T < 0) return T;
    return (T + chunk_size - 1) / chunk_size;
}

// OnlineMvdrBeamformer / OnlineGevdBeamformer.run (libs/beamformer.py:286-320, 685-724) under
// do_online_beamform (apply_adaptive_beamformer.py:25-47), post-mask, inverse_stft and renorm
// (:174-178); the block-online form of apply-supervised-mvdr.cc:198-217.  R_c = alpha R_{c-1} +
// phi_c r_c with phi_0 = 1 and phi_c = 1 - alpha afterwards (the reference class never clears its
// `reset` member, :296-317, so its phi stays 1; the stated recursion is the specification here).
int setk_enhance_online_batch(setk_handle_t h, const setk_bf_opts* opts, const setk_online_opts* online,
                              int n_utts, int num_channels, const float* const* audio,
                              const int* num_samples, const float* const* mask_s,
                              const float* const* mask_n, void* const* wave, int* status,
                              const setk_online_taps* taps, void* stream) {
    if (!h || !opts || !online || n_utts <= 0 || !audio || !num_samples || !mask_s || !wave)
        return fail(h, SETK_ERR_INVALID, "bad args");
    if (online->chunk_size < 1) return fail(h, SETK_ERR_INVALID, "chunk_size must be at least 1");
    if (!(online->alpha >= 0.f && online->alpha < 1.f))
        return fail(h, SETK_ERR_INVALID, "alpha must lie in [0, 1)");
    SETK_TRY(require_plan512(h));
    const int C = num_channels;
    if (C < 1 || C > kMaxChannels) return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 8");
    const int kind = opts->kind;
    if (kind != SETK_BF_MVDR && kind != SETK_BF_GEVD)
        return fail(h, SETK_ERR_UNSUPPORTED, "the online beamformer is MVDR or GEVD");
    const int known = SETK_FLAG_BAN | SETK_FLAG_CLAMP_MASK | SETK_FLAG_POST_MASK | SETK_FLAG_NO_GAUGE |
                      SETK_FLAG_OUT_PCM16 | SETK_FLAG_NO_RENORM | SETK_FLAG_IN_PCM16;
    if (opts->flags & ~known) return fail(h, SETK_ERR_UNSUPPORTED, "a flag the online beamformer does not take");
    if (opts->rank1 != SETK_RANK1_NONE)
        return fail(h, SETK_ERR_UNSUPPORTED, "the online beamformer takes no rank-1 approximation");
    const StftGeom g = geom_of(h);
    const bool pcm16 = (opts->flags & SETK_FLAG_OUT_PCM16) != 0;
    const bool in_pcm = (opts->flags & SETK_FLAG_IN_PCM16) != 0;
    const bool ban = (opts->flags & SETK_FLAG_BAN) != 0;
    if (in_pcm && (g.hop & 1))
        return fail(h, SETK_ERR_UNSUPPORTED, "16-bit PCM input (SETK_FLAG_IN_PCM16) needs an even hop");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const int NP = npairs(C);
    const int S = online->chunk_size;

    // ---- descriptors and work lists ----
    std::vector<UttDesc> uds = zeroed_utts(n_utts);
    std::vector<WorkItem> items1, items2;
    std::vector<int> all_frames(n_utts), chunk0(n_utts + 1, 0);
    std::vector<int2> chunk_parts;
    for (int u = 0; u < n_utts; ++u) {
        all_frames[u] = setk_stft_num_frames(h, num_samples[u]);
        if (all_frames[u] < 0) return all_frames[u];
    }
    // pass 1: a chunk is cut into runs of whole tiles, about 64 frames each (a 32-frame chunk is
    // one work item; the smoothing sums a long chunk's slabs)
    const int quant1 = pass1_tile_frames(C);
    const int target2 = choose_target(all_frames, h->p2_items, kSuperTile, kSuperTile * 4);
    int nparts_total = 0, max_len = 0;
    for (int u = 0; u < n_utts; ++u) {
        UttDesc& ud = uds[u];
        if (!audio[u] || !mask_s[u] || !wave[u] || (mask_n && !mask_n[u]))
            return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        if (in_pcm && (reinterpret_cast<uintptr_t>(audio[u]) & 3))
            return fail(h, SETK_ERR_INVALID, "16-bit PCM input must be 4-byte aligned");
        ud.audio = audio[u];
        ud.audio_fmt = in_pcm ? kAudioPcm16 : kAudioF32;
        ud.ch_stride = in_pcm ? setk_pcm16_channel_stride(num_samples[u]) : num_samples[u];
        ud.mask_s = mask_s[u];
        ud.mask_n = mask_n ? mask_n[u] : nullptr;
        ud.num_samples = num_samples[u];
        ud.num_frames = all_frames[u];
        ud.out_len = setk_istft_num_samples(h, ud.num_frames, -1);
        ud.wave_out = wave[u];
        max_len = std::max(max_len, ud.out_len);
        ud.part0 = nparts_total;
        const int T = ud.num_frames;
        for (int c0 = 0; c0 < T; c0 += S) {
            const int c1 = (int)std::min<long long>((long long)c0 + S, T);
            const size_t first = items1.size();
            const int n = push_items(&items1, u, c1 - c0, 64, quant1, &nparts_total);
            for (size_t i = first; i < items1.size(); ++i) {  // push_items counts from frame 0
                items1[i].t0 += c0;
                items1[i].t1 += c0;
                items1[i].last = items1[i].t1 == T;
            }
            chunk_parts.push_back(make_int2(nparts_total - n, n));
        }
        ud.nparts = nparts_total - ud.part0;
        chunk0[u + 1] = (int)chunk_parts.size();
        push_items(&items2, u, T, target2, kSuperTile);
    }
    const int n_chunks = (int)chunk_parts.size();
    if (taps && (taps->Rs || taps->Rn || taps->weight) && n_chunks > 65535)
        return fail(h, SETK_ERR_UNSUPPORTED, "taps are laid out for at most 65535 chunks per call");
    SETK_TRY(carve_wave_f32(h, uds, wave, pcm16));
    const UttDesc* d_uds;
    const WorkItem *d_items1, *d_items2;
    const int2* d_parts;
    const int* d_chunk0;
    SETK_TRY(upload(h, uds, s, &d_uds));
    SETK_TRY(upload(h, items1, s, &d_items1));
    SETK_TRY(upload(h, items2, s, &d_items2));
    SETK_TRY(upload(h, chunk_parts, s, &d_parts));
    SETK_TRY(upload(h, chunk0, s, &d_chunk0));

    // ---- scratch ----
    float *d_part, *d_covar, *d_w, *d_rn = nullptr;
    unsigned* d_small;
    int* d_cstatus;
    SETK_TRY(arena_get(h, (size_t)nparts_total * nplanes_partial(C) * kBinsPad * 4, &d_part, "online: partial slabs"));
    SETK_TRY(arena_get(h, (size_t)n_chunks * 4 * NP * kBinsPad * 4, &d_covar, "online: smoothed covariances"));
    if (ban) SETK_TRY(arena_get(h, (size_t)n_chunks * 2 * NP * kBinsPad * 4, &d_rn, "online: chunk noise covariances"));
    SETK_TRY(arena_get(h, (size_t)n_chunks * C * kBinsPad * 8, &d_w, "online: weights"));
    SETK_TRY(arena_get(h, (size_t)n_chunks * 4, &d_cstatus));
    SETK_TRY(arena_get(h, (size_t)n_utts * 4 * 4, &d_small));
    unsigned* d_norm = d_small;
    unsigned* d_omax = d_small + n_utts;
    int* d_status = reinterpret_cast<int*>(d_small + 2 * n_utts);
    const unsigned* d_zero = d_small + 3 * n_utts;  // SETK_FLAG_NO_RENORM: a norm of 0 only converts
    HIP_TRY(h, hipMemsetAsync(d_small, 0, (size_t)n_utts * 4 * 4, s));
    HIP_TRY(h, hipMemsetAsync(d_cstatus, 0, (size_t)n_chunks * 4, s));

    SETK_TRY(profile_begin(h, s));

    // ---- stage 1: STFT + the chunks' covariance partials ----
    Pass1Args p1 = pass1_args(h, d_uds, d_items1);
    p1.partials = d_part;
    p1.norm_bits = d_norm;
    p1.flags = opts->flags;
    if (in_pcm) p1.window = h->d_window_pcm;
    HIP_TRY(h, launch_pass1(C, false, p1, (int)items1.size(), s, in_pcm));
    SETK_TRY(profile_mark(h, 1, s));

    // ---- stage 2: smoothing, weights of every chunk, BAN, status ----
    OnlineArgs oa;
    memset(&oa, 0, sizeof(oa));
    oa.partials = d_part;
    oa.chunk_parts = d_parts;
    oa.chunk0 = d_chunk0;
    oa.covar = d_covar;
    oa.rn_chunk = d_rn;
    oa.num_channels = C;
    oa.alpha = online->alpha;
    HIP_TRY(h, launch_online_smooth(oa, n_utts, s));
    OutBuf tap_rs, tap_rn, tap_w;
    if (taps && taps->Rs) {
        SETK_TRY(stage_out(h, taps->Rs, (size_t)n_chunks * kBins * C * C * sizeof(float2), &tap_rs));
        HIP_TRY(h, launch_unpack_covar(d_covar, n_chunks, 4 * NP, 0, kBins, C, static_cast<float*>(tap_rs.dev), s));
        SETK_TRY(copy_back(h, tap_rs, s));
    }
    if (taps && taps->Rn) {
        SETK_TRY(stage_out(h, taps->Rn, (size_t)n_chunks * kBins * C * C * sizeof(float2), &tap_rn));
        HIP_TRY(h, launch_unpack_covar(d_covar, n_chunks, 4 * NP, 2 * NP, kBins, C, static_cast<float*>(tap_rn.dev), s));
        SETK_TRY(copy_back(h, tap_rn, s));
    }
    SolveArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.covar = d_covar;
    sa.weight = d_w;
    sa.status = d_cstatus;
    sa.n_utts = n_chunks;  // every chunk a virtual utterance
    sa.num_bins = kBins;
    sa.num_channels = C;
    sa.planes = 4 * NP;
    sa.kind = kind;
    sa.flags = opts->flags & ~SETK_FLAG_BAN;  // BAN takes the chunk's own rn_c: below
    sa.rank1 = SETK_RANK1_NONE;
    sa.pmwf_ref = -1;
    sa.num_scale = 1.f;
    HIP_TRY(h, launch_solve(sa, s));
    if (ban) HIP_TRY(h, launch_online_ban(C, d_w, d_rn, n_chunks, s));
    HIP_TRY(h, launch_online_status(d_cstatus, d_chunk0, n_utts, d_status, s));
    SETK_TRY(profile_mark(h, 2, s));
    if (taps && taps->weight) {
        SETK_TRY(stage_out(h, taps->weight, (size_t)n_chunks * kBins * C * sizeof(float2), &tap_w));
        HIP_TRY(h, launch_unpack_weight_batch(d_w, n_chunks, kBins, C, static_cast<float*>(tap_w.dev), s));
        SETK_TRY(copy_back(h, tap_w, s));
    }

    // ---- stage 3: beamform + iSTFT, the weight set chosen per frame ----
    Pass2Args p2 = pass2_args(h, d_uds, d_items2, d_omax);
    p2.weight = d_w;
    p2.norm_bits = d_norm;
    p2.flags = opts->flags;
    p2.chunk0 = d_chunk0;
    p2.chunk_size = S;
    HIP_TRY(h, launch_pass2_online(C, p2, (int)items2.size(), s, in_pcm));
    SETK_TRY(profile_mark(h, 3, s));

    // ---- stage 4: renorm ----
    HIP_TRY(h, launch_scale(scale_args(d_uds, (opts->flags & SETK_FLAG_NO_RENORM) ? d_zero : d_norm, d_omax, pcm16), n_utts, max_len, s));
    SETK_TRY(profile_mark(h, 4, s));
    if (status) SETK_TRY(copy_out(h, status, d_status, (size_t)n_utts * 4, s, nullptr));
    // the uploaded descriptors live in the arena: the next call on this handle may reuse it, so
    // this one must have drained
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
