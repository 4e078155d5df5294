// capi_stft.hip -- front end (include/setk_hip.h): setk_stft, setk_stft_batch, setk_istft.
// n_fft = 512 runs the fused path's kernels in their dump / ISTFT-only modes, any other
// length the generic LDS radix-2 and Bluestein kernels of modular.hip.
#include "capi.h"

using namespace setk;

namespace {

BluesteinPlan bluestein_of(setk_handle_t h) {
    return {h->blu_M, reinterpret_cast<const float*>(h->d_chirp), reinterpret_cast<const float*>(h->d_bhat)};
}

// frames that contribute to `nsamps` output samples (all T of them when nsamps < 0)
int istft_frames(setk_handle_t h, int T, int nsamps) {
    if (nsamps < 0) return T;
    const long padded = (long)nsamps + (h->center ? h->n_fft : 0);
    return (int)std::max<long>(1, std::min<long>(T, (padded + h->hop - 1) / h->hop));
}

// the per-item norm of setk_istft on the device: the caller's (host or device) values, or -1
// (none) for every item
int stage_norm(setk_handle_t h, const float* norm, int B, hipStream_t s, const float** d_norm) {
    std::vector<float> hn(B, -1.f);
    if (norm) {
        if (is_device_ptr(norm)) {
            HIP_TRY(h, hipMemcpyAsync(hn.data(), norm, B * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipStreamSynchronize(s));
        } else
            memcpy(hn.data(), norm, B * sizeof(float));
    }
    return upload(h, hn, s, d_norm);
}

// n_fft != 512: generic LDS radix-2 kernels (modular.hip)
int stft_generic(setk_handle_t h, const float* audio, int C, int N, float* spec, hipStream_t s) {
    const int T = setk_stft_num_frames(h, N);
    if (T < 0) return T;
    const int F = h->n_fft / 2 + 1;
    const BluesteinPlan bp = bluestein_of(h);
    arena_reset(h, s);
    const float* d_audio;
    SETK_TRY(stage_in(h, audio, (size_t)C * N, s, &d_audio));
    OutBuf ob;
    SETK_TRY(stage_out(h, spec, (size_t)C * T * F * sizeof(float2), &ob));
    HIP_TRY(h, launch_stft_generic(d_audio, C, N, T, h->n_fft, h->hop, h->center ? h->n_fft / 2 : 0,
                                   h->d_window, reinterpret_cast<const float*>(h->d_twn),
                                   static_cast<float*>(ob.dev), &bp, s));
    return finish_out(h, ob, s);
}

int istft_generic(setk_handle_t h, const float* spec, int B, int T, int nsamps, const float* norm,
                  float* wave, hipStream_t s) {
    const int F = h->n_fft / 2 + 1;
    const BluesteinPlan bp = bluestein_of(h);
    const int L = setk_istft_num_samples(h, T, nsamps);
    const float* d_spec;
    SETK_TRY(stage_in(h, spec, (size_t)B * T * F * 2, s, &d_spec));
    OutBuf ob;
    SETK_TRY(stage_out(h, wave, (size_t)B * L * sizeof(float), &ob));
    const float* d_norm;
    SETK_TRY(stage_norm(h, norm, B, s, &d_norm));
    float* d_frames;
    unsigned* d_omax;
    SETK_TRY(arena_get(h, (size_t)B * T * h->n_fft * 4, &d_frames));
    SETK_TRY(arena_get(h, (size_t)B * 4, &d_omax));
    HIP_TRY(h, hipMemsetAsync(d_omax, 0, (size_t)B * 4, s));
    // the frames kernel indexes spec with the caller's T; only T_eff frames are overlap-added
    HIP_TRY(h, launch_istft_generic(d_spec, B, T, h->n_fft, h->hop, h->center ? h->n_fft / 2 : 0, L,
                                    h->d_window, h->d_winsq,
                                    reinterpret_cast<const float*>(h->d_twn), d_frames,
                                    static_cast<float*>(ob.dev), d_omax, norm ? d_norm : nullptr,
                                    istft_frames(h, T, nsamps), &bp, s));
    return finish_out(h, ob, s);
}

}  // namespace

extern "C" {

int setk_stft(setk_handle_t h, const float* audio, int num_channels, int num_samples,
              float* spec, void* stream) {
    if (!h || !audio || !spec || num_channels <= 0) return fail(h, SETK_ERR_INVALID, "bad args");
    if (h->planned && h->n_fft != kNfft) {
        // (the generic path checks the length before it recycles the arena)
        HIP_TRY(h, hipSetDevice(h->device));
        return stft_generic(h, audio, num_channels, num_samples, spec,
                            static_cast<hipStream_t>(stream));
    }
    SETK_TRY(require_plan512(h));
    const int T = setk_stft_num_frames(h, num_samples);
    if (T < 0) return T;
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const float* d_audio;
    SETK_TRY(stage_in(h, audio, (size_t)num_channels * num_samples, s, &d_audio));
    OutBuf ob;
    SETK_TRY(stage_out(h, spec, (size_t)num_channels * T * kBins * sizeof(float2), &ob));
    for (int c0 = 0; c0 < num_channels; c0 += kMaxChannels) {
        const int C = std::min(kMaxChannels, num_channels - c0);
        std::vector<UttDesc> uds = zeroed_utts(1);
        uds[0].audio = d_audio + (size_t)c0 * num_samples;
        uds[0].num_samples = num_samples;
        uds[0].num_frames = T;
        std::vector<WorkItem> items;
        push_items(&items, 0, T, 64, 32);
        DescTables t;
        SETK_TRY(upload_tables(h, uds, items, s, &t));
        Pass1Args a = pass1_args(h, t.utts, t.items);
        a.spec_dump = static_cast<float*>(ob.dev) + (size_t)c0 * T * kBins * 2;
        HIP_TRY(h, launch_pass1(C, true, a, t.n_items, s));
    }
    return finish_out(h, ob, s);
}

int setk_stft_batch(setk_handle_t h, int n_utts, int num_channels, const float* const* audio,
                    const int* num_samples, float* const* spec, int spec_pitch, void* stream) {
    if (spec_pitch != 0 && spec_pitch < kBins) return fail(h, SETK_ERR_INVALID, "spec_pitch < F");
    if (!h || n_utts <= 0 || !audio || !num_samples || !spec)
        return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(require_plan512(h));
    const int C = num_channels;
    if (C < 1 || C > kMaxChannels) return fail(h, SETK_ERR_UNSUPPORTED, "1 <= num_channels <= 8");
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    std::vector<UttDesc> uds = zeroed_utts(n_utts);
    std::vector<WorkItem> items;
    for (int u = 0; u < n_utts; ++u) {
        const int T = setk_stft_num_frames(h, num_samples[u]);
        if (T < 0) return T;
        if (!audio[u] || !spec[u]) return fail(h, SETK_ERR_INVALID, "null utterance pointer");
        uds[u].audio = audio[u];
        uds[u].num_samples = num_samples[u];
        uds[u].num_frames = T;
        uds[u].wave_out = spec[u];
        push_items(&items, u, T, 128, 32);
    }
    DescTables t;
    SETK_TRY(upload_tables(h, uds, items, s, &t));
    Pass1Args a = pass1_args(h, t.utts, t.items);
    a.spec_dump = nullptr;  // per-utterance outputs: UttDesc::wave_out
    a.dump_pitch = spec_pitch;
    HIP_TRY(h, launch_pass1(C, true, a, t.n_items, s));
    return SETK_OK;
}

int setk_istft(setk_handle_t h, const float* spec, int batch, int num_frames, int nsamps,
               const float* norm, float* wave, void* stream) {
    if (!h || !spec || !wave || batch <= 0 || num_frames <= 0)
        return fail(h, SETK_ERR_INVALID, "bad args");
    hipStream_t s;
    if (h->planned && h->n_fft != kNfft) {
        SETK_TRY(begin_call(h, stream, &s));
        return istft_generic(h, spec, batch, num_frames, nsamps, norm, wave, s);
    }
    SETK_TRY(require_plan512(h));
    SETK_TRY(begin_call(h, stream, &s));
    const int T = num_frames, F = kBins;
    const int L = setk_istft_num_samples(h, T, nsamps);
    const int T_eff = istft_frames(h, T, nsamps);
    const float* d_spec;
    SETK_TRY(stage_in(h, spec, (size_t)batch * T * F * 2, s, &d_spec));
    OutBuf ob;
    SETK_TRY(stage_out(h, wave, (size_t)batch * L * sizeof(float), &ob));
    if (L > 0) HIP_TRY(h, hipMemsetAsync(ob.dev, 0, (size_t)batch * L * sizeof(float), s));
    const float* d_norm;
    SETK_TRY(stage_norm(h, norm, batch, s, &d_norm));
    std::vector<UttDesc> uds = zeroed_utts(batch);
    std::vector<WorkItem> items;
    for (int b = 0; b < batch; ++b) {
        UttDesc& ud = uds[b];
        ud.audio = d_spec + (size_t)b * T * F * 2;  // ISTFT mode: per-item spectrogram
        ud.num_frames = T_eff;
        ud.out_len = L;
        ud.wave_f32 = static_cast<float*>(ob.dev) + (size_t)b * L;
        ud.wave_out = ud.wave_f32;
        push_items(&items, b, T_eff, 128, kSuperTile);
    }
    DescTables t;
    SETK_TRY(upload_tables(h, uds, items, s, &t));
    unsigned* d_omax;
    SETK_TRY(arena_get(h, batch * sizeof(unsigned), &d_omax));
    HIP_TRY(h, hipMemsetAsync(d_omax, 0, batch * sizeof(unsigned), s));
    const Pass2Args a = pass2_args(h, t.utts, t.items, d_omax);
    HIP_TRY(h, launch_pass2(1, true, a, t.n_items, s));
    if (norm) {
        ScaleArgs sa = scale_args(a.utts, nullptr, a.outmax_bits, false);
        sa.norm_override = d_norm;
        HIP_TRY(h, launch_scale(sa, batch, L, s));
    }
    return finish_out(h, ob, s);
}

}  // extern "C"
