// capi_rir.hip -- front end (include/setk_hip.h): room impulse responses by the image method
// (rir.hip) for ragged batches of RIRs, and for one.
#include <cmath>

#include "capi.h"

using namespace setk;

namespace {

constexpr int kRirFlags = SETK_RIR_NO_SPLIT;
constexpr double kPi = 3.14159265358979323846;

// What the reference asserts (rir-generator.cc:29-31, :98) and the limits of the kernels; the images
// per microphone of a spec that passes, through *n_img (0 for NaN / inf among the inputs).
int check_spec(setk_handle_t h, const setk_rir_spec& sp, long long* n_img, int n[3], bool* bad) {
    if (!sp.room || !sp.source || !sp.mics || !sp.beta) return fail(h, SETK_ERR_INVALID, "null array in setk_rir_spec");
    if (sp.n_mics < 1 || sp.n_mics > kRirMaxMics)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 to 16 microphones per RIR");
    if (sp.num_samples < 1 || sp.num_samples > kRirMaxTaps)
        return fail(h, SETK_ERR_UNSUPPORTED, "1 to 16384 taps per RIR");
    if (!(sp.samp_frequency >= 1)) return fail(h, SETK_ERR_INVALID, "samp_frequency >= 1");
    if (!(sp.sound_velocity >= 1)) return fail(h, SETK_ERR_INVALID, "sound_velocity >= 1");
    if (sp.order < -1) return fail(h, SETK_ERR_INVALID, "order >= -1");
    if (sp.n_beta != 6) return fail(h, SETK_ERR_INVALID, "six reflection coefficients");
    if (sp.mic_type < SETK_RIR_MIC_BIDIRECTIONAL || sp.mic_type > SETK_RIR_MIC_OMNIDIRECTIONAL)
        return fail(h, SETK_ERR_INVALID, "mic_type: SETK_RIR_MIC_*");
    if (!std::isfinite(sp.samp_frequency) || !std::isfinite(sp.sound_velocity))
        return fail(h, SETK_ERR_INVALID, "samp_frequency and sound_velocity are finite");
    if (2 * (int)(0.004 * (double)sp.samp_frequency + 0.5) > kRirMaxWindow)
        return fail(h, SETK_ERR_UNSUPPORTED, "samp_frequency up to 64 kHz (a window of at most 512 taps)");
    *bad = false;
    for (int a = 0; a < 3; ++a) *bad |= !std::isfinite(sp.room[a]) || !std::isfinite(sp.source[a]);
    for (int a = 0; a < 3 * sp.n_mics; ++a) *bad |= !std::isfinite(sp.mics[a]);
    for (int a = 0; a < 6; ++a) *bad |= !std::isfinite(sp.beta[a]);
    if (sp.angle) *bad |= !std::isfinite(sp.angle[0]) || !std::isfinite(sp.angle[1]);
    *n_img = 0;
    n[0] = n[1] = n[2] = 0;
    if (*bad) return SETK_OK;
    const double cts = (double)sp.sound_velocity / (double)sp.samp_frequency;
    double total = 8.0;
    for (int a = 0; a < 3; ++a) {
        if (!(sp.room[a] > 0)) return fail(h, SETK_ERR_INVALID, "room dimensions > 0");
        const double cells = std::ceil((double)sp.num_samples / (2.0 * ((double)sp.room[a] / cts)));
        total *= 2.0 * cells + 1.0;
        if (total > 2147483647.0) return fail(h, SETK_ERR_UNSUPPORTED, "at most 2^31 - 1 images per microphone");
        n[a] = (int)cells;
    }
    *n_img = (long long)total;
    return SETK_OK;
}

// The two launches of a batch whose results are device memory: d_out[r] [n_mics][ns], d_status [n_rirs].
int run_rir(setk_handle_t h, hipStream_t s, int n_rirs, const setk_rir_spec* specs, float* const* d_out,
            int* d_status, int flags) {
    std::vector<RirChan> chans;
    std::vector<RirItem> items;
    std::vector<long long> imgs;
    int max_ns = 1, max_tw = 0;
    for (int r = 0; r < n_rirs; ++r) {
        const setk_rir_spec& sp = specs[r];
        long long n_img;
        int n[3];
        bool bad;
        SETK_TRY(check_spec(h, sp, &n_img, n, &bad));
        const double fs = sp.samp_frequency, cts = (double)sp.sound_velocity / fs;
        const double a0 = sp.angle ? sp.angle[0] : 0.0, a1 = sp.angle ? sp.angle[1] : 0.0;
        const double W = 2.0 * kPi * 100.0 / fs, R1 = std::exp(-W);
        static const double rho[5] = {0.0, 0.25, 0.5, 0.75, 1.0};
        for (int m = 0; m < sp.n_mics; ++m) {
            RirChan c;
            memset(&c, 0, sizeof c);
            for (int a = 0; a < 3; ++a) {
                c.S[a] = (double)sp.source[a] / cts;
                c.T[a] = (double)sp.room[a] / cts;
                c.R[a] = (double)sp.mics[3 * m + a] / cts;
                c.n[a] = n[a];
            }
            for (int a = 0; a < 6; ++a) c.beta[a] = sp.beta[a];
            // sin(pi/2 - a1) sin(theta) cos(a0 - phi) + cos(pi/2 - a1) cos(theta)  (:216-220)  =  u.p / |p|
            c.u[0] = std::sin(kPi / 2 - a1) * std::cos(a0);
            c.u[1] = std::sin(kPi / 2 - a1) * std::sin(a0);
            c.u[2] = std::cos(kPi / 2 - a1);
            c.rho = rho[sp.mic_type];
            c.cts = cts;
            c.hp[0] = 2.0 * R1 * std::cos(W);
            c.hp[1] = -R1 * R1;
            c.hp[2] = -1.0 - R1;
            c.hp[3] = R1;
            c.out = d_out[r] + (size_t)m * sp.num_samples;
            c.status = d_status + r;
            c.ns = sp.num_samples;
            c.order = sp.order;
            c.Tw = 2 * (int)(0.004 * fs + 0.5);
            c.hp_on = sp.hp_filter ? 1 : 0;
            c.bad = bad ? 1 : 0;
            max_ns = std::max(max_ns, c.ns);
            max_tw = std::max(max_tw, c.Tw);
            chans.push_back(c);
            imgs.push_back(n_img);
        }
    }
    // Parts: enough workgroups for the device when the batch is small (about 1024 in all), runs of at
    // least 4096 images, whole steps of 256.  The result does not depend on the cut (rir.hip).
    const int n_chans = (int)chans.size();
    const long long want = (flags & SETK_RIR_NO_SPLIT) ? 1 : std::max(1, (1024 + n_chans - 1) / n_chans);
    size_t slab = 0;
    for (int ch = 0; ch < n_chans; ++ch) {
        const long long n_img = imgs[ch];
        const long long parts = std::max(1LL, std::min(std::min(want, 64LL), n_img / 4096));
        long long step = (n_img + parts - 1) / parts;
        step = (step + kRirThreads - 1) / kRirThreads * kRirThreads;
        int np = 0;
        for (long long i0 = 0; np == 0 || i0 < n_img; i0 += step)
            items.push_back(RirItem{ch, np++, i0, std::min(n_img, i0 + step)});
        chans[ch].nparts = np;
        slab += (size_t)np * chans[ch].ns;
    }
    long long* d_part;
    SETK_TRY(arena_get(h, slab * sizeof(long long), &d_part, "the RIR parts"));
    slab = 0;
    for (RirChan& c : chans) {
        c.part = d_part + slab;
        slab += (size_t)c.nparts * c.ns;
    }
    const RirChan* d_chans;
    const RirItem* d_items;
    SETK_TRY(upload(h, chans, s, &d_chans));
    SETK_TRY(upload(h, items, s, &d_items));
    HIP_TRY(h, hipMemsetAsync(d_status, 0, (size_t)n_rirs * sizeof(int), s));
    SETK_TRY(profile_mark(h, 1, s));
    HIP_TRY(h, launch_rir_images(d_chans, d_items, (int)items.size(), max_ns, max_tw, s));
    SETK_TRY(profile_mark(h, 2, s));
    HIP_TRY(h, launch_rir_finish(d_chans, n_chans, s));
    SETK_TRY(profile_mark(h, 3, s));
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_rir_generate_batch(setk_handle_t h, int n_rirs, const setk_rir_spec* specs, float* const* out,
                            int* status, int flags, void* stream) {
    if (!h || n_rirs <= 0 || !specs || !out) return fail(h, SETK_ERR_INVALID, "bad args");
    if (flags & ~kRirFlags) return fail(h, SETK_ERR_INVALID, "flags: SETK_RIR_NO_SPLIT");
    for (int r = 0; r < n_rirs; ++r) {
        long long n_img;
        int n[3];
        bool bad;
        if (!out[r]) return fail(h, SETK_ERR_INVALID, "null output pointer");
        SETK_TRY(check_spec(h, specs[r], &n_img, n, &bad));  // before anything is staged
    }
    hipStream_t s;
    SETK_TRY(begin_call(h, stream, &s));
    SETK_TRY(profile_begin(h, s));
    std::vector<OutBuf> obs(n_rirs);
    std::vector<float*> d_out(n_rirs);
    for (int r = 0; r < n_rirs; ++r) {
        SETK_TRY(stage_out(h, out[r], (size_t)specs[r].n_mics * specs[r].num_samples * sizeof(float), &obs[r]));
        d_out[r] = static_cast<float*>(obs[r].dev);
    }
    int* d_st;
    SETK_TRY(arena_get(h, (size_t)n_rirs * sizeof(int), &d_st));
    SETK_TRY(run_rir(h, s, n_rirs, specs, d_out.data(), d_st, flags));
    for (int r = 0; r < n_rirs; ++r) SETK_TRY(copy_back(h, obs[r], s));
    if (status) SETK_TRY(copy_out(h, status, d_st, (size_t)n_rirs * sizeof(int), s, nullptr));
    SETK_TRY(profile_mark(h, 4, s));
    // the tables, the parts and staged results live in the arena: the call drains
    HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int setk_rir_generate(setk_handle_t h, const setk_rir_spec* spec, float* out, int* status, int flags,
                      void* stream) {
    if (!h || !spec || !out) return fail(h, SETK_ERR_INVALID, "bad args");
    return setk_rir_generate_batch(h, 1, spec, &out, status, flags, stream);
}

}  // extern "C"
