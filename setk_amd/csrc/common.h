// common.h -- argument blocks and launcher prototypes shared by the kernel
// translation units and the C-ABI front end (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace setk {

constexpr int kNfft = 512;        // fused kernels are specialised for n_fft = 512
constexpr int kBins = 257;        // n_fft / 2 + 1
constexpr int kBinsPad = 264;     // row pitch of per-bin planes (multiple of 8)
constexpr int kMaxChannels = 8;   // register-resident covariance accumulators
constexpr int kMaxChannels16 = 16; // modular (unfused) operators: covariance, solve, beamform
// pass 2: frames per super-tile = quad-rows per workgroup (16 lanes each) and the
// waves per SIMD its register budget is set for
constexpr int kSuperTile = 16;    // frames per inverse-transform batch (pass 2)
constexpr int kPass2Threads = 16 * kSuperTile;
constexpr int kPass2WavesPerSimd = 2;
constexpr int kMaxKeep = 7;       // ceil(512 / hop) - 1 for hop >= 64

// number of Hermitian pairs (i <= j)
__host__ __device__ constexpr int npairs(int c) { return c * (c + 1) / 2; }
// pass 1: frames per tile -- 32/C transforms fill the 32 transform quad-rows,
// capped at 8 (small C then rotates several quad-row sets)
__host__ __device__ constexpr int pass1_tile_frames(int c) { return (32 / c) < 8 ? (32 / c) : 8; }
// planes of one packed covariance pair set: [s.re | s.im | n.re | n.im | sums(2)]
__host__ __device__ constexpr int nplanes_partial(int c) { return 4 * npairs(c) + 2; }
// upper-triangular row-major pair index, i <= j
__host__ __device__ constexpr int pair_index(int i, int j, int c) {
    return i * c - i * (i - 1) / 2 + (j - i);
}

// sample formats of UttDesc::audio
constexpr int kAudioF32 = 0;    // float32 [C][ch_stride]   (the reference's C x N, read_wav's int16 / 32768)
constexpr int kAudioPcm16 = 1;  // int16   [C][ch_stride]   planar 16-bit PCM as stored in the wave file
                                // (setk_pcm16_deinterleave_batch); the kernels scale by 2^-15, exactly
                                // libs/utils.py:80-90's dtype="float32" read.  ch_stride is even: a
                                // pair of samples (x[2n], x[2n+1]) is ONE aligned dword

struct UttDesc {
    const float* audio;   // float32 [C][num_samples], or (audio_fmt) int16 [C][ch_stride]
    const float* mask_s;  // [T][F]
    const float* mask_n;  // [T][F] or null
    float* wave_f32;      // pass-2 float output [out_len]
    void* wave_out;       // final output (float32 or int16), may alias wave_f32
    int num_samples;
    int num_frames;
    int out_len;
    int part0;   // first partial slab of this utterance
    int nparts;  // number of partial slabs
    int audio_fmt;  // kAudioF32 | kAudioPcm16
    int ch_stride;  // kAudioPcm16: samples between channels (even, >= num_samples)
    int pad_;
};

struct WorkItem {
    int utt;
    int t0, t1;  // frame range [t0, t1)
    int part;    // partial slab index (pass 1) / unused (pass 2)
    int last;    // 1 if t1 == num_frames
};

struct StftGeom {
    int hop;
    int pad;      // n_fft/2 when center else 0
    int center;
    int keep;     // ceil(n_fft / hop) - 1
};

struct Pass1Args {
    const UttDesc* utts;
    const WorkItem* items;
    float* partials;        // [nparts_total][nplanes][kBinsPad]
    const float* window;    // [512] analysis window (padded, centred); PCM16 launches: x 2^-15
    const float2* tw256;    // [16][16]  exp(-2 pi i la q / 256) at [q*16+la]
    const float2* tw512;    // [129]     exp(-2 pi i k / 512)
    unsigned* norm_bits;    // [n_utts] max |audio| as float bits (atomicMax)
    float* spec_dump;       // DUMP mode: [C][T][F]
    int dump_pitch;         // DUMP mode: row pitch in complex entries (0 = F)
    StftGeom g;
    int flags;
    // matrix-core transforms (pass1_mc.hip / mcdft.h)
    const unsigned* mc_tab;  // [mc::kTabWords][64] operand tiles
    const float* mc_win;     // [8][64] analysis window rows x 2^10 / peak
};

struct FinalizeArgs {
    const UttDesc* utts;
    const float* partials;
    float* covar;  // [n_utts][4*NP (+2*NP when with_ry)][kBinsPad]
    int num_channels;
    int with_ry;   // also emit Ry = (Rs_num + Rn_num) / T  (MPDR)
    float num_scale;  // numerators x this (matrix-core pass 1: (peak / 2^10)^2; else 1)
};

struct SolveArgs {
    const float* covar;   // packed planes, see FinalizeArgs
    float* weight;        // [n_utts][C][kBinsPad] float2
    int* status;          // [n_utts] (atomicMax) or per-bin when per_bin != 0
    int* bin_status;      // [n_problems] or null
    double* snr_acc;      // PMWF ref<0: [n_problems][C][2] per-bin (ps, pn)
    float* wmat;          // PMWF ref<0: [n_problems][C][C] float2 (column major)
    int n_utts;
    int num_bins;
    int num_channels;
    int planes;           // planes per utterance in covar
    int kind, flags, rank1, pmwf_ref;
    float pmwf_beta;
    // fused partial reduction (enhance_batch with few slabs per utterance and no covariance
    // taps): the solve sums pass 1's partial slabs itself, exactly as covar_finalize_kernel
    // would have (same order, same float32 expressions), and that launch falls away
    const float* partials;  // null: read `covar`
    const UttDesc* utts;
    float num_scale;
};

struct Pass2Args {
    const UttDesc* utts;
    const WorkItem* items;
    const float* weight;     // [n_utts][C][kBinsPad] float2
    const float* spec_in;    // ISTFT mode: [B][T][F] float2
    const float* window;     // analysis window [512]
    const float* synwin;     // synthesis window [512] (same padded window)
    const float* winsq;      // window^2 [512]
    const float2* tw256;
    const float2* tw512;
    unsigned* outmax_bits;   // [n_utts]
    const unsigned* norm_bits;  // [n_utts] max |audio| (pass 1): pass2_mc's input range (may be null)
    StftGeom g;
    int flags;
    // matrix-core transforms (pass2_mc.hip / mcdft.h)
    const unsigned* mc_tab;  // [mc::kTabWords][64]
    const float* mc_win;     // [8][64] analysis window rows x 2^10 / peak
    const float* mc_syn;     // [8][64] synthesis window rows x peak / 2^10 / 512 / sum(window^2)
    const float* mc_edge;    // [8][64] corrections of the single-contribution blocks (first | last)
    // block-online beamforming (launch_pass2_online): frame t of utterance u takes weight set
    // chunk0[u] + t / chunk_size of `weight` ([chunks_total][C][kBinsPad] float2)
    const int* chunk0;       // [n_utts]
    int chunk_size;
};

// block-online beamforming (online.hip): chunk k of the batch (utterance u owns chunks
// [chunk0[u], chunk0[u + 1])) is a virtual utterance of the weight solve
struct OnlineArgs {
    const float* partials;    // pass 1's slabs, each over frames of one chunk
    const int2* chunk_parts;  // [chunks_total] (first slab, slabs)
    const int* chunk0;        // [n_utts + 1]
    float* covar;             // [chunks_total][4 NP][kBinsPad]: the smoothed Rs_c | Rn_c
    float* rn_chunk;          // [chunks_total][2 NP][kBinsPad]: the chunk's own rn_c (BAN), or null
    int num_channels;
    float alpha;              // R_c = alpha R_{c-1} + phi_c r_c; phi_0 = 1, phi_c = 1 - alpha
};

struct ScaleArgs {
    const UttDesc* utts;
    const unsigned* norm_bits;
    const unsigned* outmax_bits;
    const float* norm_override;  // istft API: per-batch norm (<=0: none) or null
    int pcm16;
};

// 9 to 16 channels (wide.hip): covariance and beamformer on the bin-major spectra.  The
// utterance table is read as: audio (the samples), wave_out = the spectra X[f][c][t] that
// stft_binmajor_kernel writes, wave_f32 = the beamformed [T][F] spectrogram (complex64),
// mask_s / mask_n, num_frames, part0 / nparts (slabs of kWideSlab frames).
constexpr int kWideSlab = 128;    // frames per covariance slab: a constant, so that the order of
                                  // the sums depends on the utterance alone (a multiple of 8)
// floats of one (slab, bin): three tiles [re 136 | im 136] (speech, noise, all-ones) in the pair
// order of the 16 x 16 embedding, then sum_t m_s, sum_t m_n (padded to 32 bytes)
constexpr int kWidePartFloats = 3 * 2 * npairs(kMaxChannels16) + 8;
struct WideArgs {
    const UttDesc* utts;
    const WorkItem* items;  // covariance: one per slab
    float* partials;        // [nparts_total][kBins][kWidePartFloats]
    float* covar;           // [n_utts][4 * 136 (+ 2 * 136 when with_ry)][kBinsPad]
    const float* weight;    // [n_utts][16][kBinsPad] float2
    int num_channels;       // 9 .. 16
    int with_ry;            // also the unmasked covariance (MPDR)
    int flags;
};
hipError_t launch_covar_wide(const WideArgs& a, int n_items, hipStream_t s);
hipError_t launch_wide_finalize(const WideArgs& a, int n_utts, hipStream_t s);
hipError_t launch_beamform_binmajor(const WideArgs& a, int n_utts, int max_frames, hipStream_t s);
hipError_t launch_wide_unpack_covar(const float* planes, int n_utts, int n_planes, int plane0, int C,
                                    float* out, hipStream_t s);
hipError_t launch_wide_unpack_weight(const float* wplanes, int n_utts, int C, float* w, hipStream_t s);

// launchers (implemented in the kernel TUs)
hipError_t launch_pass1(int C, bool dump, const Pass1Args& a, int n_items, hipStream_t s, bool pcm16 = false);
hipError_t launch_pass1_mc(int C, const Pass1Args& a, int n_items, hipStream_t s);
bool pass1_mc_supported(int C, int hop);
hipError_t launch_pass2_mc(int C, const Pass2Args& a, int n_items, hipStream_t s, bool pcm16 = false);
int pass2_mc_wgs_per_cu(int C, bool pcm16 = false);
// STFT of whole utterances into the bin-major [F][C][Tp] layout of cgmm_bin.hip
// (items: 64-frame blocks; UttDesc::wave_out = the utterance's output)
hipError_t launch_stft_binmajor(int C, const Pass1Args& a, int n_items, hipStream_t s);
hipError_t launch_finalize(const FinalizeArgs& a, int n_utts, hipStream_t s);
hipError_t launch_solve(const SolveArgs& a, hipStream_t s);
hipError_t launch_pmwf_select(const SolveArgs& a, int* ref_out, hipStream_t s);
hipError_t launch_pass2(int C, bool istft_only, const Pass2Args& a, int n_items, hipStream_t s);
hipError_t launch_pass2_online(int C, const Pass2Args& a, int n_items, hipStream_t s, bool pcm16);
hipError_t launch_scale(const ScaleArgs& a, int n_utts, int max_len, hipStream_t s);
hipError_t launch_online_smooth(const OnlineArgs& a, int n_utts, hipStream_t s);
hipError_t launch_online_ban(int C, float* weight, const float* rn_chunk, int n_chunks, hipStream_t s);
hipError_t launch_online_status(const int* chunk_status, const int* chunk0, int n_utts, int* status,
                                hipStream_t s);
size_t pass2_lds_bytes(int C, int keep);

// modular helpers
hipError_t launch_covar_spec(int C, const float* spec, const float* mask, int T, int F,
                             float* partials, int t_split, hipStream_t s);
hipError_t launch_covar_spec_finalize(int C, const float* partials, int nparts, int F,
                                      float* covar_fcc, hipStream_t s);
hipError_t launch_pack_covar(const float* fcc, int F, int C, int Cp, float pad_diag,
                             float* planes, int plane0, hipStream_t s);
hipError_t launch_unpack_weight(const float* wplanes, int F, int C, float* w_fc, hipStream_t s);
hipError_t launch_unpack_covar(const float* planes, int n_utts, int n_planes, int plane0, int F,
                               int C, float* out, hipStream_t s);
hipError_t launch_unpack_weight_batch(const float* wplanes, int n_utts, int F, int C, float* w,
                                      hipStream_t s);
// n_fft that is not a power of two: Bluestein tables (device), M = 0 when unused.
// `tw` of the generic launchers then holds exp(-2 pi i k / M), k < M / 2.
struct BluesteinPlan {
    int M;                 // convolution length, power of two >= 2 n_fft - 1
    const float* chirp;    // [n_fft] float2 exp(-i pi k^2 / n_fft)
    const float* bhat_br;  // [M] float2 FFT_M of the wrapped conj(chirp), bit-reversed order
};
hipError_t launch_stft_generic(const float* audio, int C, int n_samp, int T, int n_fft, int hop,
                               int pad, const float* window, const float* tw, float* spec,
                               const BluesteinPlan* bp, hipStream_t s);
hipError_t launch_istft_generic(const float* spec, int B, int T, int n_fft, int hop, int pad,
                                int out_len, const float* window, const float* winsq,
                                const float* tw, float* frames, float* wave, unsigned* outmax,
                                const float* norm, int T_eff, const BluesteinPlan* bp,
                                hipStream_t s);
size_t cgmm_fill_args(void* args_out, int C, const float* spec, int T, int F,
                      const float* init_mask, float* gamma_opt, float* mask_out, void* scratch,
                      int update_alpha, int spec_pitch);
size_t cgmm_args_bytes();
size_t cgmm_scratch_bytes(int C, int T, int F);
hipError_t launch_cgmm_batch(int C, const void* d_tbl, int n_utts, int F, int max_frames,
                             int num_iters, hipStream_t s);
// general EM: any number of classes (<= 4), up to 16 channels (cgmm_k.hip)
size_t cgmm_k_work_bytes(int K, int T, int F);
bool cgmm_k_supported(int C, int K);
hipError_t launch_cgmm_k(const float* spec, const double* gamma0, const float* init_mask, float* gamma_out,
                         double* work, int* status, int C, int T, int F, int K, int num_iters,
                         int update_alpha, hipStream_t s);
// bin-resident EM (cgmm_bin.hip)
size_t cgmm_bin_args_bytes();
int cgmm_bin_timing_slots();
int cgmm_bin_pitch(int T);
int cgmm_bin_threads(int C, int max_frames);
int cgmm_bin_config(int C, int max_frames);
void cgmm_bin_config_info(int cfg, int info[3]);
void cgmm_bin_fill_args(void* out, const float* xb, const float* init_mask, float* gamma_bm, int T,
                        int F, int update_alpha, int nout, void* timing);
hipError_t launch_cgmm_bin(int C, const void* d_tbl, const float* const* d_spec_ptrs, int spec_pitch,
                           float* const* d_mask_ptrs, float* const* d_gamma_ptrs, int n_utts, int F,
                           int max_frames, int num_iters, int nout, hipStream_t s);
hipError_t launch_ban(const float* w, const float* Rn, int F, int C, float* out, hipStream_t s);
hipError_t launch_rank1(const float* pv, const float* Rs, const float* Rn, int F, int C,
                        float* out, hipStream_t s);
hipError_t launch_directional_feats(const float* spec, const float* sv, const int* pairs, int n_pairs,
                                    int C, int T, int F, float* out, hipStream_t s);
hipError_t launch_maxabs(const UttDesc* utts, int C, unsigned* norm_bits, int n_utts, int max_samples,
                         hipStream_t s);
hipError_t launch_pack_fixed_weights(const float* sets, const int* index, int n_utts, int C,
                                     float* out, hipStream_t s);
hipError_t launch_float_to_pcm16(const float* in, int C, int N, int16_t* out, hipStream_t s);
hipError_t launch_pcm16_to_float(const int16_t* pcm, int C, int N, float* out, hipStream_t s);
size_t cm_item_bytes();
void cm_item_fill(void* tbl, int i, const void* src, float* dst, float vmin, float vrange, int rows, int cols,
                  int kind, int transpose);
hipError_t launch_kaldi_cm_decode_batch(const void* d_items, int n, long max_elems, hipStream_t s);
size_t pcm_item_bytes();
void pcm_item_fill(void* dst, int i, const int16_t* pcm, float* out, int n);
hipError_t launch_pcm16_to_float_batch(const void* d_items, int n_utts, int C, int max_n,
                                       double* power0, hipStream_t s);
void pcm_item_fill_planar(void* dst, int i, const int16_t* pcm, int16_t* out, int n, int stride);
hipError_t launch_pcm16_deinterleave_batch(const void* d_items, int n_utts, int C, int max_n,
                                           double* power0, hipStream_t s);
hipError_t launch_beamform_spec(const float* w_fc, const float* spec, int C, int T, int F,
                                float* out, hipStream_t s);

// WPE (wpe.hip)
bool wpe_supported(int N, int taps);
const char* wpe_limit_message(int N, int taps);
hipError_t launch_wpe_transpose(const float* in, int C, int T, int F, float* out, bool to_fct,
                                hipStream_t s);
hipError_t launch_wpe_lambda(const float* d_fct, int C, int T, int F, int ctx, double* lam,
                             hipStream_t s);
hipError_t launch_wpe_lambda_from_enh(const float* enh_tf, int T, int F, double* lam,
                                      hipStream_t s);
hipError_t launch_wpe_inv_lambda(const double* lam, int T, int F, float* out, hipStream_t s);
size_t wpe_args_bytes();
void wpe_fill_args(void* dst, const float* x_fct, const double* lam, float* out_fct, int* status,
                   int N, int T, int taps, int delay, long long* timing = nullptr,
                   void* rwork = nullptr);
// bytes of global scratch per (utterance, bin) when channels x taps does not fit LDS, else 0
size_t wpe_wide_bytes_per_bin(int N, int taps);
hipError_t launch_wpe_step_batch(const void* d_tbl, int n_utts, int N, int F, int taps,
                                 hipStream_t s);
// what launch_wpe_step_batch picks for a supported shape (host only): R in global memory?,
// accumulator tiles per wavefront of the instantiation, frames per staged chunk
void wpe_form(int N, int taps, int* wide, int* tiles_per_wave, int* chunk_frames);

// CACGMM (cacgmm.hip): one launch runs the whole EM of every (bin, utterance); observations
// [F][C][Tp] complex64 with Tp = cacgmm_pitch(T), work area cacgmm_work_bytes per utterance
bool cacgmm_supported(int C, int K);
const char* cacgmm_limit_message();
int cacgmm_pitch(int T);
size_t cacgmm_work_bytes(int K, int T, int F);
int cacgmm_resident_frames(int C, int max_frames, bool force_streaming);
size_t cacgmm_args_bytes();
void cacgmm_fill_args(void* dst, const float* x_bin, const double* gamma0, float* gamma_out, double* work,
                      int* status, int T);
hipError_t launch_cacgmm(const void* d_tbl, int n_utts, int C, int F, int K, int num_iters, int flags,
                         int res_frames, hipStream_t s);

// AuxIVA (auxiva.hip): observations [F][C][Tp] complex64, powers [F][C][Tp] float64 (y as
// complex64 after the last launch), weights [C][Tp] float64, W [F][C][C] complex128
bool auxiva_supported(int C);
const char* auxiva_limit_message();
size_t auxiva_args_bytes();
void auxiva_fill_args(void* dst, const float* x_bin, double* power, double* g, void* W, int* status,
                      int T, int Tp);
hipError_t launch_auxiva_norm(const void* d_tbl, int n_utts, int C, int F, int max_frames,
                              hipStream_t s);
hipError_t launch_auxiva_epoch(const void* d_tbl, int n_utts, int C, int F, bool update, bool write_y,
                               hipStream_t s);
hipError_t launch_auxiva_transpose(const float* in, int C, int T, int F, int Tp, float* out,
                                   bool to_bin, hipStream_t s);
hipError_t launch_auxiva_spread_norm(const unsigned* norm_bits, int C, int n, unsigned* out,
                                     hipStream_t s);

// Sound source localisation (ssl.hip).  Frame scores S [T][A] float32 out of observations
// prepared per tile of kSslTile frames (xt: [tiles][F][K][32] complex64, K = channels (ML) or
// pairs (SRP); pm: [tiles][F][2][32] float32, ML only) and steer-vector operands laid out
// direction-fastest ([F][K][ssl_apad(A)] complex64); scores per window float64 [W][A].
constexpr int kSslMl = 0, kSslSrp = 1, kSslMusic = 2;  // = SETK_SSL_*
constexpr int kSslTile = 32;

// exp(i angle(z)) as np.angle has it, shared by ssl.hip and spatial.hip: angle(0) = 0, a NaN
// component gives (NaN, NaN), every finite non-zero complex64 gives its phase.  |z|^2 is formed in
// float32; where it leaves [2^-124, 2^124] (the squares underflow below |z| = 2^-63 and overflow
// above 2^64) z is first rescaled by an exact power of two, which moves |z| into [2^-49, 2^59]
// and not one bit of the phase.  Inside the range nothing is rescaled.  The rare cases all rejoin
// the one straight line of square root, reciprocal and products (a zero as z = 1).
__device__ __forceinline__ float2 phasor(float2 z) {
    float n2 = z.x * z.x + z.y * z.y;
    if (!(n2 >= 0x1p-124f && n2 <= 0x1p124f)) {
        const float k = n2 > 0x1p124f ? 0x1p-70f : 0x1p100f;
        z.x *= k;
        z.y *= k;
        n2 = z.x * z.x + z.y * z.y;
        if (n2 == 0.f) {
            z = make_float2(1.f, 0.f);
            n2 = 1.f;
        }
    }
    const float n = sqrtf(n2);
    const float r = 1.f / n;
    return make_float2(z.x * r, z.y * r);
}
struct SslUtt {         // one utterance of a prep / fold / frame-score launch
    const float* spec;  // [C][T][pitch] complex64
    const float* mask;  // [T][F] or null
    float* xt;          // [tiles][F][K][32] float2: x (ML, normalised when asked) / mask x u_p (SRP)
    float* pm;          // ML: [tiles][F][2][32]: sum_m |x|^2 | mask.  SRP fold: its partial sums,
                        // float64 [chunks][P][F][2]
    float* S;           // [T][A]
    int T, pitch;
    int t0, t1;         // SRP fold: the frames summed
};
struct SslWin {         // one window of the reduction
    const float* S;     // [T][A] of the window's utterance (null: the scores are already there)
    int t0, t1;
};
int ssl_apad(int A);
int ssl_tiles(int T);
size_t ssl_xt_bytes(int T, int F, int K);
size_t ssl_pm_bytes(int T, int F);
size_t ssl_fold_bytes(int frames, int F, int P);  // SRP fold: the partial sums (SslUtt::pm)
hipError_t launch_ssl_sv_prep(const float* sv, const int* d_pairs, int mode, int A, int C, int F, int K,
                              float* out, hipStream_t s);
hipError_t launch_ssl_obs_prep(const SslUtt* d_utts, const int* d_pairs, int mode, int n_utts, int max_frames, int C,
                               int F, int K, int norm, float eps, hipStream_t s);
hipError_t launch_ssl_srp_fold(const SslUtt* d_utts, const int* d_pairs, int n_utts, int max_frames, int F, int P,
                               hipStream_t s);
hipError_t launch_ssl_frame_scores(const SslUtt* d_utts, const float* svt, int mode, int n_utts, int max_frames, int A,
                                   int F, int K, float inv1pe, float eps, float compression, hipStream_t s);
hipError_t launch_ssl_music_prep(const float* spec, const float* mask, int C, int T, int F, int pitch, int t0, int t1,
                                 float* xo, float* m2, hipStream_t s);
// (cov [F][C][C] complex64: a zero bin is reported in status [F], SETK_NUM_SINGULAR)
hipError_t launch_ssl_music_score(const float* svt, const float* v, const float* cov, int A, int F, int C,
                                  double* score, int* status, hipStream_t s);
hipError_t launch_ssl_windows(const SslWin* d_wins, int n_wins, int A, bool take_min, double* score, int* index,
                              hipStream_t s);

// Geometry-driven spatial features (spatial.hip): IPD maps, directional features over several
// directions, SRP-PHAT angular spectra.  All start from the pair coherence u_p = exp(i (arg X_l -
// arg X_r)).  SRP reads the observations in ssl.hip's tile layout (ssl_obs_prep_kernel<kSslSrp>
// without a mask) and a table W [P][F][ssl_apad(D)] complex64, direction fastest.
constexpr int kSpatialIpd = 0, kSpatialCosIpd = 1, kSpatialCosSinIpd = 2, kSpatialDf = 3,
              kSpatialSrp = 4;  // = SETK_SPATIAL_*
constexpr int kSpatialMaxPairs = 120;
struct SpatialUtt {
    const float* spec;  // [C][T][F] complex64
    float* out;         // the features, [T][width]
    float* sp;          // SRP: s_p [P][T][Dpad] float32
    unsigned* pmax;     // SRP: [P] the bits of max_{t,d} |s_p|
    int T;
    int idx0;           // DF: where this utterance's direction indices start
};
hipError_t launch_spatial_ipd(const SpatialUtt* d_utts, const int* d_pairs, int kind, int n_utts, int max_frames,
                              int F, int P, hipStream_t s);
hipError_t launch_spatial_df(const SpatialUtt* d_utts, const int* d_pairs, const float* sv, const int* d_idx,
                             int n_idx, int n_utts, int max_frames, int C, int F, int P, hipStream_t s);
hipError_t launch_spatial_srp_pairs(const SslUtt* d_obs, const SpatialUtt* d_utts, const float* table, int n_utts,
                                    int max_frames, int D, int F, int P, hipStream_t s);
hipError_t launch_spatial_srp_combine(const SpatialUtt* d_utts, const float* d_weight, int n_utts, int max_frames,
                                      int D, int P, hipStream_t s);

// OM-LSA noise suppression with MCRA / iMCRA noise tracking (ns.hip): one workgroup per
// utterance, the bins over the lanes, a loop over the frames; float64 throughout.
constexpr int kNsMcra = 0, kNsImcra = 1;  // = SETK_NS_*
constexpr int kNsMaxBins = 1025;          // n_fft <= 2048
constexpr int kNsMaxHalf = 31;            // a smoothing window has at most 2 x 31 + 1 taps
constexpr int kNsMaxRing = 32;            // iMCRA: U
struct NsParams {
    int kind, F;
    int half_m, half_l, half_g;  // half widths of w_mcra / w_local / w_global
    int L, mean_bins;            // MCRA: the reset period, min(M / 2 + 1, F)
    int V, U;                    // iMCRA
    int pad_;
    double alpha, alpha_s, alpha_d, alpha_p, beta, delta, gmin, xi_min, q_max;
    double zeta_min, zeta_max, zeta_p_min, zeta_p_max;  // MCRA, linear
    double inv_b_min, gamma0, gamma1, zeta0;            // iMCRA
    double eps;
    double taps[3][2 * kNsMaxHalf + 1];  // w_mcra | w_local | w_global, as np.convolve takes them
};
struct NsUtt {
    const float* spec;  // [T][F] complex64
    double* gain;       // [T][F] or null
    float* out;         // gain x spec, [T][F] complex64, or null
    int* status;        // one word
    int T;
    int pad_;
};
bool ns_supported(int F);
hipError_t launch_ns(const NsUtt* d_utts, const NsParams* d_params, int kind, int n_utts, int F, hipStream_t s);
hipError_t launch_expint_e1(const double* x, double* y, int n, hipStream_t s);

// Data simulation (simu.hip): partitioned overlap-save reverberation on the 512-point transform,
// block 256, spectra in the transform's lane layout (256 complex64 per transform), and the mixing.
constexpr int kSimuBlock = 256;
constexpr int kSimuMaxTaps = 16384;    // = SETK_SIMU_MAX_TAPS
constexpr int kSimuMaxChannels = 16;   // = SETK_SIMU_MAX_CHANNELS
constexpr int kSimuPowChunk = 8192;    // samples per partial sum
struct SimuFwd {      // a run of forward transforms of one signal
    const void* src;  // float32 or (fmt) int16
    float2* X;        // [frames][256]
    int fmt, len;     // kAudioF32 | kAudioPcm16; samples behind src
    int n;            // samples taken (beyond them zeros); wrap: sample i is src[i % len]
    int wrap, frames;
    int rir;          // 1: frame p is RIR block p (256 samples, 256 zeros); 0: source frame k
};
struct SimuItem { int job, f0; };  // 16 transforms from f0
struct SimuConv {
    const float2* X;  // [K][256]
    const float2* H;  // [N][P][256]
    float* out;       // [N][S]
    int K, P, N, S;
};
struct SimuConvItem { int job, k0, c0, pad_; };  // 16 frames from k0, the kernel's channels from c0
struct SimuImage {     // one image of a mixture: a reverberated source, or the source itself
    const void* data;  // [nch][pitch]
    int fmt, len, pitch, nch;
    int beg, dur;      // mixed into [beg, beg + dur); sample i >= len is data[i % len]
    int pw_n;          // the mean square of channel 0 runs over [0, pw_n)
    int part0, nparts; // its partial sums
    int pad_;
    double snr;
};
struct SimuMix {
    const SimuImage* img;  // speakers, point noises, the isotropic chunk
    double* coeff;         // [n_img]
    double* power;         // [n_img + 1]: the images', the speaker-only mixture's
    double* spk_partial;   // [ceil(L / kSimuPowChunk)]
    unsigned long long* peak;  // the bits of max |mix| (float64)
    int* status;
    void* mix;             // float32 [N][L] or int16 [L][N]
    void* noise_ref;       // [L] or null
    void* const* spk_ref;  // [n_spk] -> [L] (entries may be null)
    double norm_factor;
    int n_spk, n_img, N, L;
};
int simu_conv_channels(int N);
hipError_t launch_simu_fwd(const SimuFwd* d_jobs, const SimuItem* d_items, int n_items, hipStream_t s);
hipError_t launch_simu_conv(const SimuConv* d_jobs, const SimuConvItem* d_items, int nc, int n_items, hipStream_t s);
hipError_t launch_simu_power(const SimuImage* d_imgs, int n_imgs, int max_n, double* d_partial, hipStream_t s);
hipError_t launch_simu_coeff(const SimuMix* d_mixes, int n_mix, int stage, const double* d_partial, hipStream_t s);
hipError_t launch_simu_spkpow(const SimuMix* d_mixes, int n_mix, int max_len, hipStream_t s);
hipError_t launch_simu_peak(const SimuMix* d_mixes, int n_mix, int max_channels, int max_len, hipStream_t s);
hipError_t launch_simu_out(const SimuMix* d_mixes, int n_mix, int max_channels, int max_len, bool pcm16,
                           hipStream_t s);

// SI-SNR scoring with permutation alignment (metric.hip): K estimates against K references per
// utterance, float64 sums over tiles of kMetricTile samples, one owner per sum.
constexpr int kMetricMaxSrc = 8;      // K <= 8: 8! = 40 320 orders per utterance
constexpr int kMetricTile = 8192;     // samples of every signal per (utterance, tile) workgroup
constexpr int kMetricThreads = 256;
struct MetricUtt {
    const void* sig[2 * kMetricMaxSrc];  // estimates at [0, K), references at [8, 8 + K); float32 or int16
    int stride[2 * kMetricMaxSrc];       // in samples (C for channel 0 of interleaved frames)
    int K, L;
    int tile0, ntiles;  // this utterance's rows of the partial slab
    double* mean;       // [16], the slots of sig
    double* gram;       // [8] e_j | [64] d_ij | [64] a_ij  (pitch 8)
    double* pair;       // [K][K] si_snr(estimate i, reference j)
    double* best;       // or null
    int* perm;          // [K] or null
    int* status;
};
struct MetricItem { int utt, tile; };
// quantities per row of the partial slab for the launch's padded source count KP (2, 4 or 8)
__host__ __device__ constexpr int metric_row(int kp) { return kp * kp + kp; }
int metric_padded_sources(int max_k);
hipError_t launch_metric_means(const MetricUtt* d_utts, const MetricItem* d_items, int n_items, int n_utts, int kp,
                               bool pcm16, double* d_partial, hipStream_t s);
hipError_t launch_metric_gram(const MetricUtt* d_utts, const MetricItem* d_items, int n_items, int n_utts, int kp,
                              bool pcm16, double eps, double* d_partial, int* d_flags, hipStream_t s);
hipError_t launch_metric_residual(const MetricUtt* d_utts, const MetricItem* d_items, int n_items, int kp,
                                  bool pcm16, double* d_partial, hipStream_t s);
hipError_t launch_metric_search(const MetricUtt* d_utts, int n_utts, int kp, double eps, const double* d_partial,
                                hipStream_t s);

// Room impulse responses by the image method (rir.hip): one channel is a (RIR, microphone) pair,
// its images are cut into parts, each part's workgroup sums its taps in 64-bit fixed point in LDS.
constexpr int kRirMaxTaps = 16384;   // = SETK_RIR_MAX_TAPS
constexpr int kRirMaxMics = 16;      // = SETK_RIR_MAX_MICS
constexpr int kRirMaxWindow = 512;   // Tw = 2 int(0.004 fs + 0.5): fs up to 64 kHz
constexpr int kRirThreads = 512;     // of the images kernel
constexpr int kRirFixShift = 40;     // a tap is an integer multiple of 2^-40
struct RirChan {
    double S[3], T[3], R[3];  // source, room, microphone in samples (metres / cts)
    double beta[6];
    double u[3];              // the pattern's look direction: gain = rho + (1 - rho) u.p / |p|
    double rho;               // 1: omnidirectional
    double cts;
    double hp[4];             // B1, B2, A1, R1 of rir-generator.cc:121
    long long* part;          // [nparts][ns] fixed-point sums
    float* out;               // [ns]
    int* status;              // of the RIR (its microphones share it)
    int ns, order, Tw, hp_on;
    int n[3];                 // nx, ny, nz
    int bad;                  // NaN / inf among the inputs: no image is walked
    int nparts, pad_;
};
struct RirItem {
    int chan, part;
    long long img0, img1;     // images [img0, img1) in the reference's loop order (x, y, z, q, j, k)
};
size_t rir_lds_bytes(int ns, int Tw);
hipError_t launch_rir_images(const RirChan* d_chans, const RirItem* d_items, int n_items, int max_ns, int max_tw,
                             hipStream_t s);
hipError_t launch_rir_finish(const RirChan* d_chans, int n_chans, hipStream_t s);

// Oracle TF masks and mask-based separation (tfmask.hip): the cell arithmetic of compute_mask.py
// and oracle_separate.py on stored spectra, and fused behind the 512-point forward transform.
constexpr int kTfIbm = 0, kTfIrm = 1, kTfIam = 2, kTfPsm = 3, kTfPsa = 4, kTfCrm = 5;  // = SETK_TFMASK_*
constexpr int kTfModeMask = 0, kTfModeSeparate = 1, kTfModeOracle = 2;
constexpr int kTfMaxTargets = 8;      // = SETK_TFMASK_MAX_TARGETS
constexpr int kTfChunk = 2048;        // cells per workgroup of the stored-spectra kernels (one slot each)
struct TfStats {                      // = setk_tfmask_stats
    long long over, below;
    double below_sum;
};
struct TfFold {                       // one mask's statistics: the slots summed in their order by one owner
    const unsigned long long* counts; // [2] over | below
    const double* slots;
    TfStats* out;
    int nslots, pad_;
};
struct TfUtt {                        // one utterance of a forward launch
    const void* mix;                  // float32 or int16 [num_samples]
    const void* aux[kTfMaxTargets];   // mask: [0] the target; separation: [0] the phase reference or null;
                                      // oracle: the K targets
    void* out[kTfMaxTargets];         // mask: [0] float32 [T][F] ([T][2F] crm); separation: [0] complex64
                                      // [T][F]; oracle: K times complex64 [T][F]
    const float* mask;                // separation: [T][F]
    int* status;                      // one word
    unsigned long long* counts;       // mask: [2]
    int num_samples, num_frames;
};
struct TfFwdArgs {
    const TfUtt* utts;
    const WorkItem* items;            // WorkItem::part: the item's slot
    const float* window;              // [512], x 0.5 (PCM16: x 2^-16)
    const float2* tw256;
    const float2* tw512;
    double* slots;                    // mask: one partial sum per item
    StftGeom g;
    float cutoff;
    int num_targets;
};
hipError_t launch_tf_mask(int kind, const float* tgt, const float* mix, size_t cells, int F, float cutoff,
                          float* mask, unsigned long long* counts, double* slots, int* status, hipStream_t s);
hipError_t launch_tf_fold(const TfFold* d_jobs, int n, hipStream_t s);
hipError_t launch_tf_apply(const float* spec, const float* mask, const float* phase_ref, size_t cells, float* out,
                           hipStream_t s);
hipError_t launch_tf_forward(int mode, int kind, bool pcm16, const TfFwdArgs& a, int n_items, hipStream_t s);

}  // namespace setk
