// capi_simu.hip -- front end (include/setk_hip.h): data simulation (simu.hip).  setk_fir_reverb
// reverberates one source with one RIR; setk_simu_batch runs a ragged batch of mixture recipes
// (wav_simulate.py's run_simu) in a handful of launches.
#include <map>
#include <tuple>

#include "capi.h"

using namespace setk;

namespace {

constexpr int kB = kSimuBlock;

int blocks_of(int n) { return (n + kB - 1) / kB; }

// The transforms and convolutions of a call, collected and launched together.
struct Plan {
    setk_handle_t h;
    std::vector<SimuFwd> fwd;
    std::vector<SimuItem> fitems;
    std::vector<SimuConv> conv;
    std::vector<SimuConvItem> citems[2];  // by channels per pass: 2, 1
    std::map<std::tuple<const void*, int, int>, const float2*> rirs;  // one H per (RIR, N, R) of the call

    void add_fwd(const void* src, int fmt, int len, int n, bool rir, float2* X) {
        SimuFwd j;
        memset(&j, 0, sizeof(j));
        j.src = src;
        j.X = X;
        j.fmt = fmt;
        j.len = len;
        j.n = n;
        j.wrap = n > len;
        j.frames = blocks_of(n);
        j.rir = rir;
        for (int f0 = 0; f0 < j.frames; f0 += 16) fitems.push_back({(int)fwd.size(), f0});
        fwd.push_back(j);
    }

    // out[N][n] = the first n samples of (src, repeated when n > len) * rir[N][R]
    int add_reverb(const void* src, int fmt, int len, int n, const float* rir, int N, int R, float* out) {
        const int K = blocks_of(n), P = blocks_of(R);
        float2* X;
        SETK_TRY(arena_get(h, (size_t)K * 256 * sizeof(float2), &X));
        add_fwd(src, fmt, len, n, false, X);
        const auto key = std::make_tuple((const void*)rir, N, R);
        auto it = rirs.find(key);
        if (it == rirs.end()) {
            float2* H;
            SETK_TRY(arena_get(h, (size_t)N * P * 256 * sizeof(float2), &H));
            for (int c = 0; c < N; ++c) add_fwd(rir + (size_t)c * R, kAudioF32, R, R, true, H + (size_t)c * P * 256);
            it = rirs.emplace(key, H).first;
        }
        SimuConv j;
        memset(&j, 0, sizeof(j));
        j.X = X;
        j.H = it->second;
        j.out = out;
        j.K = K;
        j.P = P;
        j.N = N;
        j.S = n;
        const int nc = simu_conv_channels(N);
        std::vector<SimuConvItem>& items = citems[nc == 2 ? 0 : 1];
        for (int c0 = 0; c0 < N; c0 += nc)
            for (int k0 = 0; k0 < K; k0 += 16) items.push_back({(int)conv.size(), k0, c0, 0});
        conv.push_back(j);
        return SETK_OK;
    }

    int launch_transforms(hipStream_t s) {
        if (fwd.empty()) return SETK_OK;
        const SimuFwd* d_jobs;
        const SimuItem* d_items;
        SETK_TRY(upload(h, fwd, s, &d_jobs));
        SETK_TRY(upload(h, fitems, s, &d_items));
        HIP_TRY(h, launch_simu_fwd(d_jobs, d_items, (int)fitems.size(), s));
        return SETK_OK;
    }

    int launch_convolutions(hipStream_t s) {
        if (conv.empty()) return SETK_OK;
        const SimuConv* d_jobs;
        SETK_TRY(upload(h, conv, s, &d_jobs));
        for (int q = 0; q < 2; ++q) {
            if (citems[q].empty()) continue;
            const SimuConvItem* d_items;
            SETK_TRY(upload(h, citems[q], s, &d_items));
            HIP_TRY(h, launch_simu_conv(d_jobs, d_items, q == 0 ? 2 : 1, (int)citems[q].size(), s));
        }
        return SETK_OK;
    }
};

int check_rir(setk_handle_t h, int N, int R) {
    if (N < 1 || N > kSimuMaxChannels) return fail(h, SETK_ERR_UNSUPPORTED, "a RIR has 1 to 16 channels");
    if (R < 1 || R > kSimuMaxTaps) return fail(h, SETK_ERR_UNSUPPORTED, "a RIR has 1 to 16384 taps");
    return SETK_OK;
}

SimuImage image(const void* data, int fmt, int len, int pitch, int nch, int beg, int dur, int pw_n, double snr) {
    SimuImage im;
    memset(&im, 0, sizeof(im));
    im.data = data;
    im.fmt = fmt;
    im.len = len;
    im.pitch = pitch;
    im.nch = nch;
    im.beg = beg;
    im.dur = dur;
    im.pw_n = pw_n;
    im.snr = snr;
    return im;
}

// what a source contributes: its image (reverberated into the arena when it has a RIR)
// take: the samples of the source that are used (repeat: beyond its length it wraps)
int source_image(Plan* plan, const setk_simu_source& src, int fmt, int dump_channel, int take, int beg,
                 SimuImage* out) {
    setk_handle_t h = plan->h;
    if (src.rir) {
        SETK_TRY(check_rir(h, src.rir_channels, src.rir_taps));
        if (src.channels != 1)  // add_room_response :38-39
            return fail(h, SETK_ERR_INVALID, "Can not convolve rir with a multi-channel signal");
        const float* rir = static_cast<const float*>(src.rir);
        int N = src.rir_channels;
        if (dump_channel >= 0) {  // :77-79
            if (dump_channel >= N) return fail(h, SETK_ERR_INVALID, "dump_channel beyond the RIR's channels");
            rir += (size_t)dump_channel * src.rir_taps;
            N = 1;
        }
        float* img;
        SETK_TRY(arena_get(h, (size_t)N * take * sizeof(float), &img));
        SETK_TRY(plan->add_reverb(src.audio, fmt, src.num_samples, take, rir, N, src.rir_taps, img));
        *out = image(img, kAudioF32, take, take, N, beg, take, take, src.snr);
    } else {
        if (take > src.num_samples && src.channels != 1)
            return fail(h, SETK_ERR_UNSUPPORTED, "a repeated noise without a RIR has one channel");
        *out = image(src.audio, fmt, src.num_samples, src.num_samples, src.channels, beg,
                     std::max(take, src.num_samples), take, src.snr);
    }
    return SETK_OK;
}

int check_source(setk_handle_t h, const setk_simu_source& s) {
    if (!s.audio) return fail(h, SETK_ERR_INVALID, "null source");
    if (s.num_samples < 1) return fail(h, SETK_ERR_UNSUPPORTED, "a source has at least one sample");
    if (s.channels < 1 || s.channels > kSimuMaxChannels)
        return fail(h, SETK_ERR_UNSUPPORTED, "a source has 1 to 16 channels");
    if (s.begin < 0) return fail(h, SETK_ERR_UNSUPPORTED, "begin >= 0");
    if (!is_device_ptr(s.audio) || (s.rir && !is_device_ptr(s.rir)))
        return fail(h, SETK_ERR_INVALID, "setk_simu_batch takes device pointers");
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_fir_reverb(setk_handle_t h, const void* spk, int num_samples, const float* rir, int num_channels,
                    int num_taps, float* out, double* power0, int flags, void* stream) {
    if (!h || !spk || !rir || !out) return fail(h, SETK_ERR_INVALID, "bad args");
    SETK_TRY(check_rir(h, num_channels, num_taps));
    if (num_samples < 1) return fail(h, SETK_ERR_UNSUPPORTED, "a source has at least one sample");
    const int S = num_samples, N = num_channels, R = num_taps;
    const bool in16 = (flags & SETK_FLAG_IN_PCM16) != 0;
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    const void* d_spk;
    if (in16) {
        const int16_t* d;
        SETK_TRY(stage_in(h, static_cast<const int16_t*>(spk), (size_t)S, s, &d));
        d_spk = d;
    } else {
        const float* d;
        SETK_TRY(stage_in(h, static_cast<const float*>(spk), (size_t)S, s, &d));
        d_spk = d;
    }
    const float* d_rir;
    SETK_TRY(stage_in(h, rir, (size_t)N * R, s, &d_rir));
    OutBuf ob;
    SETK_TRY(stage_out(h, out, (size_t)N * S * sizeof(float), &ob));
    Plan plan;
    plan.h = h;
    SETK_TRY(plan.add_reverb(d_spk, in16 ? kAudioPcm16 : kAudioF32, S, S, d_rir, N, R, static_cast<float*>(ob.dev)));
    SETK_TRY(plan.launch_transforms(s));
    SETK_TRY(plan.launch_convolutions(s));
    bool owed = false;
    if (power0) {  // np.mean(revb[0]**2), :54
        SimuImage im = image(ob.dev, kAudioF32, S, S, N, 0, S, S, 0.0);
        im.nparts = (S + kSimuPowChunk - 1) / kSimuPowChunk;
        double *d_partial, *d_power;
        SETK_TRY(arena_get(h, (size_t)im.nparts * sizeof(double), &d_partial));
        SETK_TRY(arena_get(h, 4 * sizeof(double), &d_power));
        const SimuImage* d_img;
        SETK_TRY(upload(h, &im, 1, s, &d_img));
        SimuMix m;
        memset(&m, 0, sizeof(m));
        m.img = d_img;
        m.coeff = d_power + 2;
        m.power = d_power;
        m.n_spk = m.n_img = 1;
        m.N = N;
        m.L = S;
        const SimuMix* d_mix;
        SETK_TRY(upload(h, &m, 1, s, &d_mix));
        HIP_TRY(h, launch_simu_power(d_img, 1, S, d_partial, s));
        HIP_TRY(h, launch_simu_coeff(d_mix, 1, 0, d_partial, s));
        SETK_TRY(copy_out(h, power0, d_power, sizeof(double), s, &owed));
    }
    SETK_TRY(copy_back(h, ob, s));
    // the spectra and staged operands live in the arena: drained before the next call reuses it
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_simu_num_samples(const setk_simu_recipe* r) {
    if (!r || r->n_speakers < 1 || !r->speakers) return SETK_ERR_INVALID;
    long L = 0;
    for (int i = 0; i < r->n_speakers; ++i)  // max(b + s.size), :195: `size` counts every channel
        L = std::max(L, (long)r->speakers[i].begin + (long)r->speakers[i].num_samples * r->speakers[i].channels);
    return L > 0x7fffffffL ? SETK_ERR_UNSUPPORTED : (int)L;
}

int setk_simu_num_channels(const setk_simu_recipe* r) {
    if (!r || r->n_speakers < 1 || !r->speakers) return SETK_ERR_INVALID;
    const setk_simu_source& s = r->speakers[0];
    if (!s.rir) return s.channels;
    return r->dump_channel >= 0 ? 1 : s.rir_channels;
}

int setk_simu_batch(setk_handle_t h, int n_mix, const setk_simu_recipe* recipes, int* status, int flags,
                    void* stream) {
    if (!h || n_mix <= 0 || !recipes) return fail(h, SETK_ERR_INVALID, "bad args");
    if (n_mix > 65535) return fail(h, SETK_ERR_UNSUPPORTED, "at most 65535 mixtures per batch");
    const int fmt = (flags & SETK_FLAG_IN_PCM16) ? kAudioPcm16 : kAudioF32;
    const bool out16 = (flags & SETK_FLAG_OUT_PCM16) != 0;
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    Plan plan;
    plan.h = h;
    std::vector<SimuImage> imgs;
    std::vector<SimuMix> mixes(n_mix);
    std::vector<int> img0(n_mix);
    std::vector<void*> refs;
    std::vector<int> ref0(n_mix);
    int n_partial = 0, max_pw = 1, max_len = 1;
    int max_ch = 1;
    memset(mixes.data(), 0, mixes.size() * sizeof(SimuMix));
    for (int u = 0; u < n_mix; ++u) {
        const setk_simu_recipe& r = recipes[u];
        if (r.n_speakers < 1 || !r.speakers || r.n_noises < 0 || (r.n_noises && !r.noises) || !r.mix || !r.spk_ref)
            return fail(h, SETK_ERR_INVALID, "a recipe needs speakers, mix and spk_ref");
        if (!is_device_ptr(r.mix)) return fail(h, SETK_ERR_INVALID, "setk_simu_batch takes device pointers");
        for (int i = 0; i < r.n_speakers; ++i) SETK_TRY(check_source(h, r.speakers[i]));
        for (int i = 0; i < r.n_noises; ++i) SETK_TRY(check_source(h, r.noises[i]));
        const int L = setk_simu_num_samples(&r);
        if (L < 0) return fail(h, SETK_ERR_UNSUPPORTED, "mixture too long");
        const int ch = r.dump_channel;
        img0[u] = (int)imgs.size();
        ref0[u] = (int)refs.size();
        // ---- speakers (add_speaker, :57-93) ----
        int N = 0;
        for (int i = 0; i < r.n_speakers; ++i) {
            const setk_simu_source& sp = r.speakers[i];
            SimuImage im;
            SETK_TRY(source_image(&plan, sp, fmt, ch, sp.num_samples, sp.begin, &im));
            if (i == 0) N = im.nch;
            if (im.nch != N && im.nch != 1)  // numpy cannot broadcast the image into N x L
                return fail(h, SETK_ERR_INVALID, "speaker images differ in their channel count");
            imgs.push_back(im);
            refs.push_back(r.spk_ref[i]);
            if (r.spk_ref[i] && !is_device_ptr(r.spk_ref[i]))
                return fail(h, SETK_ERR_INVALID, "setk_simu_batch takes device pointers");
        }
        // ---- point noises (add_point_noise, :96-143): every noise is mixed over the LAST one's
        // duration (:113-115 leave `dur` behind, :142 uses it) ----
        std::vector<int> ilen(r.n_noises);
        int dur_last = 0;
        for (int i = 0; i < r.n_noises; ++i) {
            const setk_simu_source& nz = r.noises[i];
            const bool repeat = (nz.flags & SETK_SIMU_REPEAT) != 0;
            const int dur = repeat ? L - nz.begin : std::min(nz.num_samples, L - nz.begin);
            if (dur < 1) return fail(h, SETK_ERR_UNSUPPORTED, "a point noise begins behind the mixture's end");
            SimuImage im;
            SETK_TRY(source_image(&plan, nz, fmt, ch, dur, nz.begin, &im));
            ilen[i] = nz.rir ? dur : std::max(nz.num_samples, dur * (repeat ? 1 : 0));
            imgs.push_back(im);
            dur_last = dur;
        }
        for (int i = 0; i < r.n_noises; ++i) {
            SimuImage& im = imgs[img0[u] + r.n_speakers + i];
            const int lhs = std::max(0, std::min(dur_last, L - im.beg)), rhs = std::min(dur_last, ilen[i]);
            if (lhs != rhs)  // mix[..., beg:beg + dur] += coeff * img[..., :dur] raises
                return fail(h, SETK_ERR_INVALID, "point noises: the last noise's duration does not fit the others");
            im.dur = lhs;
            const int Nn = imgs[img0[u] + r.n_speakers].nch;
            if (im.nch != Nn && im.nch != 1)
                return fail(h, SETK_ERR_INVALID, "noise images differ in their channel count");
            if (Nn != N)  // :266-269
                return fail(h, SETK_ERR_INVALID, "Channel mismatch between source speaker configuration and "
                                                 "pointsource noise's");
        }
        // ---- the isotropic chunk (:275-302): channel 0 of the file goes to every channel ----
        if (r.iso) {
            if (!is_device_ptr(r.iso)) return fail(h, SETK_ERR_INVALID, "setk_simu_batch takes device pointers");
            if (r.iso_samples < 1 || r.iso_channels < 1)
                return fail(h, SETK_ERR_UNSUPPORTED, "the isotropic noise has at least one sample");
            int c = 0;
            if (N == 1) {
                if (r.iso_channels > 1) {
                    if (ch < 0) return fail(h, SETK_ERR_INVALID, "Single channel mixture vs multi-channel isotropic noise");
                    if (ch >= r.iso_channels)
                        return fail(h, SETK_ERR_INVALID, "dump_channel beyond the isotropic noise's channels");
                    c = ch;
                }
            } else if (r.iso_channels != N)
                return fail(h, SETK_ERR_INVALID, "Channel number mismatch between mixture and isotropic noise");
            const int dur = std::min(L, r.iso_samples);
            const char* p = static_cast<const char*>(r.iso) + (size_t)c * r.iso_samples * (fmt ? 2 : 4);
            imgs.push_back(image(p, fmt, r.iso_samples, r.iso_samples, 1, 0, dur, dur, r.iso_snr));
        }
        const bool has_noise = r.n_noises > 0 || r.iso;
        if (has_noise && r.noise_ref && !is_device_ptr(r.noise_ref))
            return fail(h, SETK_ERR_INVALID, "setk_simu_batch takes device pointers");
        SimuMix& m = mixes[u];
        m.n_spk = r.n_speakers;
        m.n_img = (int)imgs.size() - img0[u];
        m.N = N;
        m.L = L;
        m.norm_factor = r.norm_factor;
        m.mix = r.mix;
        m.noise_ref = has_noise ? r.noise_ref : nullptr;
        for (int i = img0[u]; i < (int)imgs.size(); ++i) {
            imgs[i].part0 = n_partial;
            imgs[i].nparts = (imgs[i].pw_n + kSimuPowChunk - 1) / kSimuPowChunk;
            n_partial += imgs[i].nparts;
            max_pw = std::max(max_pw, imgs[i].pw_n);
        }
        max_len = std::max(max_len, L);
        max_ch = std::max(max_ch, N);
    }
    // ---- scratch of the mixing, the tables ----
    double *d_partial, *d_coeff, *d_power, *d_spkpart;
    unsigned long long* d_peak;
    int* d_st;
    size_t n_spkpart = 0;
    for (int u = 0; u < n_mix; ++u) n_spkpart += (mixes[u].L + kSimuPowChunk - 1) / kSimuPowChunk;
    SETK_TRY(arena_get(h, (size_t)std::max(n_partial, 1) * sizeof(double), &d_partial));
    SETK_TRY(arena_get(h, imgs.size() * sizeof(double), &d_coeff));
    SETK_TRY(arena_get(h, (imgs.size() + n_mix) * sizeof(double), &d_power));
    SETK_TRY(arena_get(h, n_spkpart * sizeof(double), &d_spkpart));
    SETK_TRY(arena_get(h, (size_t)n_mix * sizeof(unsigned long long), &d_peak));
    SETK_TRY(arena_get(h, (size_t)n_mix * sizeof(int), &d_st));
    HIP_TRY(h, hipMemsetAsync(d_peak, 0, (size_t)n_mix * sizeof(unsigned long long), s));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, (size_t)n_mix * sizeof(int), s));
    const SimuImage* d_imgs;
    void* const* d_refs;
    SETK_TRY(upload(h, imgs, s, &d_imgs));
    SETK_TRY(upload(h, refs, s, &d_refs));
    size_t sp = 0;
    for (int u = 0; u < n_mix; ++u) {
        SimuMix& m = mixes[u];
        m.img = d_imgs + img0[u];
        m.coeff = d_coeff + img0[u];
        m.power = d_power + img0[u] + u;
        m.spk_partial = d_spkpart + sp;
        sp += (m.L + kSimuPowChunk - 1) / kSimuPowChunk;
        m.peak = d_peak + u;
        m.status = d_st + u;
        m.spk_ref = d_refs + ref0[u];
    }
    const SimuMix* d_mixes;
    SETK_TRY(upload(h, mixes, s, &d_mixes));

    SETK_TRY(plan.launch_transforms(s));
    SETK_TRY(profile_mark(h, 1, s));
    SETK_TRY(plan.launch_convolutions(s));
    SETK_TRY(profile_mark(h, 2, s));
    HIP_TRY(h, launch_simu_power(d_imgs, (int)imgs.size(), max_pw, d_partial, s));
    HIP_TRY(h, launch_simu_coeff(d_mixes, n_mix, 0, d_partial, s));
    HIP_TRY(h, launch_simu_spkpow(d_mixes, n_mix, max_len, s));
    HIP_TRY(h, launch_simu_coeff(d_mixes, n_mix, 1, d_partial, s));
    HIP_TRY(h, launch_simu_peak(d_mixes, n_mix, max_ch, max_len, s));
    SETK_TRY(profile_mark(h, 3, s));
    HIP_TRY(h, launch_simu_out(d_mixes, n_mix, max_ch, max_len, out16, s));
    SETK_TRY(profile_mark(h, 4, s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)n_mix * sizeof(int), s, nullptr));
    // the images, spectra and tables live in the arena: the call drains
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

}  // extern "C"
