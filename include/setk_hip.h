/*
 * setk_hip.h -- C ABI of libsetk_hip.so: the MI355X (gfx950) implementation of
 * setk's mask-based adaptive-beamformer hot path
 *
 *     STFT -> masked spatial covariance -> MVDR/GEV/PMWF/MPDR weights
 *          -> beamform -> iSTFT (+ max-abs renorm)
 *
 * The reference (funcwj/setk) has no FFI for this path: the seam is the python
 * call surface of scripts/sptk/libs/{utils,beamformer}.py.  Each entry point
 * below names the reference function it replaces; the python mirror in
 * setk_amd/libs binds them through ctypes (see INTEGRATION.md for the stub a
 * maintainer would add on the reference side).
 *
 * Conventions
 *   - plain C, no exceptions; every call returns an int status:
 *       0            SETK_OK
 *       < 0          API misuse / unsupported  (python: ValueError/RuntimeError)
 *       > 0          never returned; numerical failures are reported per
 *                    frequency bin / per utterance through `status` arrays
 *                    (python: numpy.linalg.LinAlgError)
 *   - all data pointers are caller-owned and contiguous.  Every pointer may be
 *     DEVICE memory (hipMalloc / torch tensor data_ptr) or ordinary HOST
 *     memory; the library detects which (hipPointerGetAttributes) and stages
 *     host buffers through its own device arena.  setk_enhance_batch takes
 *     device pointers only.
 *   - complex values are interleaved float pairs (numpy complex64).
 *   - spectrogram layout is "time major": X[c][t][f], f fastest, F = n_fft/2+1.
 *     (numpy view of the reference's N x F x T array:
 *      np.ascontiguousarray(obs.transpose(0, 2, 1)))
 *   - masks are T x F row major (the layout apply_adaptive_beamformer.py
 *     normalises to, :146-151), covariances F x C x C, weights F x C.
 *   - all work is enqueued on the hipStream_t passed as `stream` (NULL = the
 *     default stream).  When any OUTPUT pointer is host memory the call
 *     synchronises the stream before returning; otherwise it is asynchronous.
 *   - a handle is used by one host thread at a time; no global state.
 */
#ifndef SETK_HIP_H_
#define SETK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SETK_ABI_VERSION 1

/* return codes */
#define SETK_OK 0
#define SETK_ERR_INVALID (-1)     /* bad argument / shape mismatch            */
#define SETK_ERR_UNSUPPORTED (-2) /* valid request outside the built kernels  */
#define SETK_ERR_HIP (-3)         /* HIP runtime error, see setk_last_error   */
#define SETK_ERR_NOMEM (-4)

/* per-bin / per-utterance numerical status values (written to status arrays) */
#define SETK_NUM_OK 0
#define SETK_NUM_SINGULAR 1 /* noise covariance not positive definite        */
#define SETK_NUM_NOCONV 2   /* Jacobi sweep limit reached                    */
#define SETK_NUM_NONFINITE 3 /* NaN / inf in this bin's input (reported even where it also makes the
                              factorisation fail), or a non-finite result of finite input   */
#define SETK_NUM_RANKDEF 4  /* WPE only, NOT an error: the tap correlation was rank deficient
                              (fewer frames than channels x taps, a silent or duplicated channel),
                              columns at the noise level were dropped and a filter was produced;
                              numpy.linalg.solve in the reference also goes through on such
                              input, with a different, noise-determined filter */

/* beamformer kinds (apply_adaptive_beamformer.py:22, --beamformer) */
#define SETK_BF_MVDR 0
#define SETK_BF_GEVD 1
#define SETK_BF_PMWF 2        /* beta / ref channel / rank1 via setk_bf_opts */
#define SETK_BF_MPDR 3
#define SETK_BF_MPDR_WHITEN 4

/* rank-1 approximation of Rs for PMWF (libs/beamformer.py:66-84, 642-645) */
#define SETK_RANK1_NONE 0
#define SETK_RANK1_EIG 1
#define SETK_RANK1_GEV 2

/* flags */
#define SETK_FLAG_BAN 0x1        /* blind analytic normalisation, do_ban      */
#define SETK_FLAG_CLAMP_MASK 0x2 /* speech mask <- min(mask, 1)   (:141)      */
#define SETK_FLAG_POST_MASK 0x4  /* enh <- enh * mask^T           (:174-175)  */
#define SETK_FLAG_NO_GAUGE 0x8   /* leave eigenvector phase as computed       */
#define SETK_FLAG_OUT_PCM16 0x10 /* enhance_batch writes int16 PCM, not f32   */
#define SETK_FLAG_NO_RENORM 0x20 /* apply_weights_batch: inverse_stft(norm=None) */
/* Reference failure semantics (setk_weights, setk_enhance_batch; CLI --strict-reference true).
 * The reference solves Rn x = b with numpy.linalg.solve (LAPACK ?gesv: LU with partial pivoting
 * in the matrix's own precision, complex64) and raises LinAlgError("Singular matrix") only on an
 * EXACT zero pivot (libs/beamformer.py:536 MVDR, :568 MPDR on Ry, :646 PMWF; the CLI logs and
 * skips the utterance, apply_adaptive_beamformer.py:170-172); its GEV never raises (hegvd's
 * refusal is caught and scipy.linalg.eig takes over, libs/beamformer.py:54-59).  With this flag
 * the same decision is taken on the device: a complex64 LU with partial pivoting (cabs1 pivot
 * search, no fused multiply-adds) of the matrix the reference would hand to solve, per bin, and
 * SETK_NUM_SINGULAR where a pivot column is exactly zero -- a duplicated / silent / power-of-two
 * scaled channel, an all-zero noise covariance; GEV goes through even on an all-zero Rn (as the
 * pencil (Rs, I)).  Without the flag (the default) such input is regularised (floored / loaded
 * Cholesky) and only an all-zero or non-finite covariance is refused.  The weights of the bins
 * that pass are the same in both modes. */
#define SETK_FLAG_STRICT_REFERENCE 0x40
/* setk_enhance_batch(_taps): audio[u] is 16-bit PCM, planar int16 [C][setk_pcm16_channel_stride(
 * num_samples[u])] as setk_pcm16_deinterleave_batch lays it out, not float32 [C][N].  Both
 * streaming kernels then read 2 bytes per sample and scale by 2^-15 inside their transforms
 * (folded into the window tables: a power of two, so the results are bit for bit those of the
 * float32 call on pcm / 32768, i.e. on read_wav's dtype="float32" samples, libs/utils.py:80-90).
 * Needs hop = n_fft / 2 (the CLI default 512 / 256) and at most 8 channels; otherwise
 * SETK_ERR_UNSUPPORTED -- convert with setk_pcm16_to_float_batch. */
#define SETK_FLAG_IN_PCM16 0x80

typedef struct setk_context* setk_handle_t;

typedef struct setk_bf_opts {
    int kind;        /* SETK_BF_*                                            */
    int flags;       /* SETK_FLAG_*                                          */
    float pmwf_beta; /* 0 -> pmwf-0, 1 -> pmwf-1                             */
    int pmwf_ref;    /* < 0: pick the channel with max estimated SNR         */
    int rank1;       /* SETK_RANK1_*                                         */
} setk_bf_opts;

/* ---- lifetime ---------------------------------------------------------- */
int setk_abi_version(void);
int setk_create(setk_handle_t* out, int device_ordinal);
int setk_destroy(setk_handle_t h);
/* text of the last error on this handle (never NULL) */
const char* setk_last_error(setk_handle_t h);
/* PCI bus id of the handle's device ("0000:c1:00.0", NUL terminated, into out[len]): what a
 * host needs to place its reader threads and pinned staging on the GPU's NUMA node
 * (/sys/bus/pci/devices/<id>/numa_node; setk_amd/numa.py, --numa auto).  The reference has no
 * such notion: its processes are CPU only (scripts/run_adapt_beamformer.sh:69-92). */
int setk_device_pci_bus_id(setk_handle_t h, char* out, int len);

/* ---- host-memory plumbing (used by the streaming host pipeline) -----------
 * Pin an existing host range (e.g. the mmap of a wave file in the page cache) so
 * that setk_memcpy_h2d_async DMAs straight out of it, and release it again once
 * the copy has completed.  Thread safe; independent of the handle's arena. */
int setk_host_register(setk_handle_t h, void* ptr, size_t bytes);
int setk_host_unregister(setk_handle_t h, void* ptr);
int setk_memcpy_h2d_async(setk_handle_t h, void* dst, const void* src, size_t bytes,
                          void* stream);
int setk_memcpy_d2h_async(setk_handle_t h, void* dst, const void* src, size_t bytes,
                          void* stream);
/* Buffers, streams and events on the handle's device, for a host program that brings no HIP
 * runtime binding of its own (setk_amd/pipeline.py runs without importing torch): device and
 * page-locked host memory, non-blocking streams (pass them as the `stream` argument of any
 * entry point), events without timing.  Thread safe.  What the reference has in their place:
 * nothing -- it is single-threaded numpy (apply_adaptive_beamformer.py:130-178). */
int setk_device_alloc(setk_handle_t h, size_t bytes, void** out);
int setk_device_free(setk_handle_t h, void* ptr);
int setk_host_alloc(setk_handle_t h, size_t bytes, void** out);
int setk_host_free(setk_handle_t h, void* ptr);
/* The read stage of the command line's pipeline for one batch in one call (no handle: host code
 * only).  Payload i is nbytes[i] bytes at offsets[i] of the file paths[i] -- a wave file's 16-bit
 * frames, a mask's float32 rows, exactly as stored -- and is copied to dst[i] (the batch's
 * page-locked slab) by a process-wide pool of n_threads native threads: a MADV_SEQUENTIAL
 * mapping + memcpy for payloads of at least mmap_min_bytes, pread below.  status[i]: 0 or the
 * errno of the failing call (EIO: the file ends inside the payload).  Thread safe; concurrent
 * calls share the pool.  What the reference has in its place: WaveReader / ScriptReader._load,
 * one utterance at a time on the interpreter's thread (libs/data_handler.py:345-413). */
int setk_host_read_payloads(int n, const char* const* paths, const long long* offsets,
                            const long long* nbytes, void* const* dst, int n_threads,
                            long long mmap_min_bytes, int* status);
int setk_stream_create(setk_handle_t h, void** out);
int setk_stream_destroy(setk_handle_t h, void* stream);
int setk_stream_synchronize(setk_handle_t h, void* stream);
int setk_stream_wait_event(setk_handle_t h, void* stream, void* event);
int setk_event_create(setk_handle_t h, void** out);
int setk_event_destroy(setk_handle_t h, void* event);
int setk_event_record(setk_handle_t h, void* event, void* stream);
int setk_event_synchronize(setk_handle_t h, void* event);

/* ---- STFT plan ---------------------------------------------------------
 * Mirrors the arguments of forward_stft / inverse_stft
 * (scripts/sptk/libs/utils.py:96-173) after the host resolved
 * n_fft = nextpow2(frame_len) | frame_len and evaluated the window
 * (scipy.signal.get_window(name, frame_len, fftbins=True) or sqrt-hann).
 * `window` = frame_len host floats, NULL = periodic hann.
 * n_fft must be even, in [16, 4096]; n_fft == 512 selects the register/LDS
 * radix-16 kernels, other powers of two (>= 64) a generic LDS radix-2 kernel,
 * anything else (--round-power-of-two false with e.g. frame_len 400) Bluestein's
 * chirp-z form on top of the radix-2 kernel. */
int setk_stft_plan(setk_handle_t h, int frame_len, int frame_hop, int n_fft,
                   int center, const float* window);
/* frames produced for `num_samples` input samples, < 0 on error */
int setk_stft_num_frames(setk_handle_t h, int num_samples);
/* samples produced by the inverse for `num_frames` frames (nsamps < 0: the
 * librosa default length) */
int setk_istft_num_samples(setk_handle_t h, int num_frames, int nsamps);

/* ---- modular operators -------------------------------------------------- */

/* forward_stft per channel (libs/utils.py:96-138; SpectrogramReader._load,
 * libs/data_handler.py:492-503).  audio[C][N] float32 -> spec[C][T][F]. */
int setk_stft(setk_handle_t h, const float* audio, int num_channels,
              int num_samples, float* spec, void* stream);

/* The same for a batch of utterances in ONE launch (device pointers, host tables;
 * spec[u] = [C][T_u][spec_pitch], F entries used per row; spec_pitch = 0 means F, a
 * multiple of 16 entries keeps every row 128-byte aligned for a streaming consumer;
 * n_fft = 512 plan, C <= 8).  Asynchronous on `stream`. */
int setk_stft_batch(setk_handle_t h, int n_utts, int num_channels,
                    const float* const* audio, const int* num_samples,
                    float* const* spec, int spec_pitch, void* stream);

/* inverse_stft (libs/utils.py:142-173) for `batch` independent spectrograms
 * spec[B][T][F] -> wave[B][L], L = setk_istft_num_samples(h, T, nsamps).
 * norm: NULL or B floats; norm[b] > 0 rescales wave b to that max-abs
 * (samps * norm / (max|samps| + eps), :166-168). */
int setk_istft(setk_handle_t h, const float* spec, int batch, int num_frames,
               int nsamps, const float* norm, float* wave, void* stream);

/* compute_covar (libs/beamformer.py:87-103):
 * covar[f] = sum_t m[t][f] x x^H / max(sum_t m[t][f], 1e-6).
 * spec[C][T][F], mask[T][F] -> covar[F][C][C] complex64.  1 <= C <= 16 (the wide
 * kernel serves 9 - 16 channels). */
int setk_covar(setk_handle_t h, const float* spec, const float* mask,
               int num_channels, int num_frames, int num_bins, float* covar,
               void* stream);

/* solve_pevd (libs/beamformer.py:31-63): principal eigenvector of Rs (Rn NULL)
 * or of the pencil (Rs, Rn).  Output pvec[F][C] complex64, unit 2-norm
 * (Rn NULL) or Rn-normalised v^H Rn v = 1.  Gauge (unless SETK_FLAG_NO_GAUGE):
 * component 0 real >= 0; for the pencil the rule applies to y = L^H v,
 * Rn = L L^H.  status[F] (may be NULL) receives SETK_NUM_*. */
int setk_pevd(setk_handle_t h, const float* Rs, const float* Rn, int num_bins,
              int num_channels, int flags, float* pvec, int* status,
              void* stream);

/* {Mvdr,Gevd,Pmwf,Mpdr}Beamformer.weight (+ do_ban), libs/beamformer.py:
 * 14-28, 527-539, 555-571, 632-659, 674-682.  Rs, Rn: [F][C][C]; Ry only for
 * MPDR kinds (covariance of the all-ones mask).  weight[F][C] complex64.
 * status[F] may be NULL.  ref_out (may be NULL) receives the PMWF reference
 * channel actually used. */
int setk_weights(setk_handle_t h, const setk_bf_opts* opts, const float* Rs,
                 const float* Rn, const float* Ry, int num_bins,
                 int num_channels, float* weight, int* status, int* ref_out,
                 void* stream);

/* read_wav with dtype float32 + transpose (libs/utils.py:65-92,
 * data_handler.py:372-393) for 16-bit PCM: interleaved frames pcm[n][c] ->
 * audio[c][n] = pcm / 32768 (soundfile's scaling, exact in float32).  Lets a
 * caller upload the 2-byte samples of a wav as they lie in the file. */
int setk_pcm16_to_float(setk_handle_t h, const int16_t* pcm, int num_channels,
                        int num_samples, float* audio, void* stream);

/* The same for a batch in ONE launch (device pointers; the tables are host
 * arrays): what the streaming host pipeline runs on a staging slab of wav
 * payloads.  power0 (device double[n_utts], may be NULL) receives sum(x0^2) of
 * channel 0 -- SpectrogramReader.power * N (data_handler.py:398-403), which the
 * CLI only logs.  Asynchronous on `stream`. */
int setk_pcm16_to_float_batch(setk_handle_t h, int n_utts, int num_channels,
                              const int16_t* const* pcm, const int* num_samples,
                              float* const* audio, double* power0, void* stream);

/* 16-bit PCM ingest WITHOUT a float32 copy: interleaved frames pcm[u][n][c] (a wave file's
 * data chunk) -> planar int16 out[u][c][stride], stride = setk_pcm16_channel_stride(num_samples[u])
 * (the samples between channels: num_samples rounded up to a multiple of 8, the padding
 * zeroed), the layout SETK_FLAG_IN_PCM16 reads.  4 C N bytes of traffic where the float32
 * conversion moves 6 C N, and half the bytes in both streaming passes afterwards.  power0 as
 * setk_pcm16_to_float_batch.  Device pointers, host tables, asynchronous on `stream`. */
int setk_pcm16_channel_stride(int num_samples);
int setk_pcm16_deinterleave_batch(setk_handle_t h, int n_utts, int num_channels,
                                  const int16_t* const* pcm, const int* num_samples,
                                  int16_t* const* out, double* power0, void* stream);

/* Kaldi CompressedMatrix bodies -> float32 matrices on the device, a batch per launch: the masks
 * of the streaming command line travel as the 1 - 2 bytes per element the archive holds.
 * Replaces `uncompress` (scripts/sptk/libs/kaldi_io.py:248-292; formats CM / CM2 / CM3 =
 * kOneByteWithColHeaders / kTwoByte / kOneByte) with the same float32 operations in the same
 * order: results equal numpy's bit for bit.  Per matrix i: kinds[i] (SETK_KALDI_CM..CM3), the global
 * header's (vmin, vrange, rows, cols), src[i] = the bytes that follow that 16-byte header (CM: the
 * per-column headers, then the column-major bytes), dst[i] = rows x cols float32 row-major -- or, with
 * transpose[i] != 0, cols x rows: the transpose (a mask stored F x T, apply_adaptive_beamformer.py:
 * 146-151).  Device pointers (CM / CM2 bodies 2-byte aligned), host tables, asynchronous on `stream`. */
#define SETK_KALDI_CM 1
#define SETK_KALDI_CM2 2
#define SETK_KALDI_CM3 3
int setk_kaldi_cm_decode_batch(setk_handle_t h, int n, const int* kinds, const float* vmin, const float* vrange,
                               const int* rows, const int* cols, const int* transpose,
                               const void* const* src, float* const* dst, void* stream);

/* The way back for a multi-channel result (apply_wpe.py:58-61 -> write_wav,
 * libs/utils.py:45-62 -> soundfile.write, float -> PCM_16): float32 rows audio[C][N] ->
 * interleaved frames pcm[N][C], lrint(x * 32767) without clipping (libsndfile's default;
 * out-of-range values wrap).  Host or device pointers. */
int setk_float_to_pcm16(setk_handle_t h, const float* audio, int num_channels, int num_samples,
                        int16_t* pcm, void* stream);

/* do_ban (libs/beamformer.py:14-28) on an arbitrary weight:
 * out[f] = w[f] * sqrt(|w^H Rn Rn w|) / max(Re w^H Rn w, eps_f32). */
int setk_ban(setk_handle_t h, const float* weight, const float* Rn, int num_bins,
             int num_channels, float* out, void* stream);

/* rank1_constraint (libs/beamformer.py:66-84): p = principal eigenvector of Rs
 * (Rn NULL) or Rn v for the pencil (Rs, Rn);
 * out[f] = tr(Rs) / max(tr(p p^H), eps_f32) * p p^H,  [F][C][C] complex64. */
int setk_rank1(setk_handle_t h, const float* Rs, const float* Rn, int num_bins,
               int num_channels, float* out, int* status, void* stream);

/* Beamformer.beamform (libs/beamformer.py:220-234):
 * out[t][f] = sum_c conj(w[f][c]) spec[c][t][f]. */
int setk_beamform(setk_handle_t h, const float* weight, const float* spec,
                  int num_channels, int num_frames, int num_bins, float* out,
                  void* stream);

/* ---- CGMM mask estimation (BASELINE configs[4]) ---------------
 * CgmmTrainer(obs, 2, gamma=init).train(num_iters) of
 * scripts/sptk/libs/cluster.py:396-465 as used by estimate_cgmm_masks.py:44-64:
 * K = 2 complex-Gaussian mixture, alpha fixed at 1/2 (or SETK_CGMM_UPDATE_ALPHA), deterministic start
 * (Rs = x x^H / T, Rn = I) or an initial speech mask.
 * spec[C][T][F] complex64, init_mask[T][F] or NULL.
 * gamma_out (may be NULL) receives the posteriors [2][T][F]; mask_out[T][F]
 * receives gamma[0] (the speech mask the CLI saves).  1 <= C <= 8. */
#define SETK_CGMM_UPDATE_ALPHA 0x1 /* --update-alpha: alpha_k = mean_t gamma_k in every M-step
                                     (Cgmm.update, cluster.py:246-257) instead of 1/2 */
int setk_cgmm_masks(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                    int num_bins, int num_iters, const float* init_mask, float* gamma_out,
                    float* mask_out, int flags, void* stream);

/* The general form: num_classes K in [2, 4], 1 <= C <= 16 channels -- CgmmTrainer with
 * num_classes != 2 (cluster.py:427-434), and the K = 2 starts for arrays wider than 8.
 * gamma0[K][F][T] float64 (host or device) is the start: for K > 2 the reference's
 * np.random.uniform(size=[K, F, T]) / sum over K, drawn from the legacy global generator that
 * estimate_cgmm_masks.py:28 seeds with --seed (the caller draws it: setk_amd/libs/cluster.py);
 * NULL with K = 2 selects init_mask[T][F] or the deterministic start as in setk_cgmm_masks.
 * gamma_out[K][T][F] float32 receives every class's posteriors.  float64 throughout, like
 * the reference; a straightforward kernel (cgmm_k.hip), not the tuned K = 2 path. */
int setk_cgmm_masks_k(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                      int num_bins, int num_classes, int num_iters, const double* gamma0,
                      const float* init_mask, float* gamma_out, int flags, void* stream);
/* The same, reporting per bin what the reference's np.linalg.eigh would have refused
 * (cluster.py:104-113, uncaught by estimate_cgmm_masks.py: its run ends with LinAlgError):
 * status[F] (host or device, may be NULL) receives the worst SETK_NUM_* over classes and
 * iterations -- SETK_NUM_NONFINITE for a covariance with NaN / inf, SETK_NUM_NOCONV when the
 * Jacobi sweep limit was reached.  The posteriors are written either way. */
int setk_cgmm_masks_k_status(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                             int num_bins, int num_classes, int num_iters, const double* gamma0,
                             const float* init_mask, float* gamma_out, int flags, int* status,
                             void* stream);

/* Batched form: n_utts utterances per EM stage launch (device pointers only;
 * spec[u] = [C][num_frames[u]][spec_pitch] (0 = F), mask_out[u] = [num_frames[u]][F],
 * init_mask NULL or per-utterance NULL-able table).  Asynchronous on `stream`. */
int setk_cgmm_masks_batch(setk_handle_t h, int n_utts, int num_channels,
                          const float* const* spec, const int* num_frames, int num_bins,
                          int num_iters, const float* const* init_mask, float* const* mask_out,
                          int flags, int spec_pitch, void* stream);

/* The compute loop of estimate_cgmm_masks.py:44-64 for a batch, audio in, mask out:
 * STFT (n_fft = 512 plan) written straight into the bin-major layout of the
 * bin-resident EM, the EM itself, masks as float32 [T][F].  audio[u] device float32
 * [C][num_samples[u]]; init_mask / mask_out / flags as setk_cgmm_masks_batch.
 * SETK_ERR_UNSUPPORTED when one bin of the longest utterance does not fit a CU
 * (then: setk_stft_batch + setk_cgmm_masks_batch). */
int setk_cgmm_estimate_batch(setk_handle_t h, int n_utts, int num_channels,
                             const float* const* audio, const int* num_samples, int num_iters,
                             const float* const* init_mask, float* const* mask_out, int flags,
                             void* stream);

/* Which kernel form the three entries above run for `num_channels` channels when the longest
 * utterance of the call has `max_frames` frames: the index of the bin-resident EM's
 * configuration (cgmm_bin.hip), or -1 for the streaming kernels (cgmm.hip: one bin of that
 * utterance does not fit a CU, or SETK_CGMM_STREAMING=1; SETK_CGMM_CFG is honoured as by the
 * dispatcher).  info (may be NULL) receives that configuration's threads per bin, frames per
 * thread, and how many of those a thread keeps in registers (the others sit in LDS); thread t
 * owns frames t, t + threads, ...  No handle, no device work. */
int setk_cgmm_bin_config(int num_channels, int max_frames, int info[3]);

/* ---- CACGMM mask estimation ---------------------------------------------------
 * CacgmmTrainer(obs, K, gamma=gamma0, cgmm_init, update_alpha).train(num_iters) of
 * scripts/sptk/libs/cluster.py:468-535 as used by estimate_cacgmm_masks.py:31-66: the complex
 * angular central Gaussian mixture on the normalised observation z = x / max(||x||, eps)
 * (norm_observation, :39-45), Cacgmm.update / predict (:352-393), CacgDistribution
 * (:298-337), Covariance (:94-135).  One launch runs the start, every iteration and the closing
 * posterior of every bin, float64 throughout (z too: the reference normalises in complex64).
 * spec[C][T][F] complex64, 1 <= C <= 8, 2 <= K <= 4 (otherwise SETK_ERR_UNSUPPORTED).
 * gamma0[K][F][T] float64 is the start (:509-515): an initial mask, or the reference's
 * np.random.uniform(size=[K, F, T]) / sum over K from the legacy global generator that
 * estimate_cacgmm_masks.py:28 seeds with --seed; the caller draws it (setk_amd/libs/cluster.py).
 * gamma0 = NULL needs SETK_CACGMM_CGMM_INIT, otherwise SETK_ERR_INVALID.
 * gamma_out[K][T][F] float32 receives every class's posteriors (num_iters = 0: the start).
 * status[F] (host or device, may be NULL) receives the worst SETK_NUM_* of the bin over classes
 * and iterations: what np.linalg.eigh refuses (:104) -- SETK_NUM_NONFINITE for NaN / inf in the
 * bin's input or covariance, SETK_NUM_NOCONV when the Jacobi sweep limit was reached.  The
 * posteriors are written either way.  The environment variable SETK_CACGMM_STREAMING=1 (read at
 * call time) keeps the bin out of LDS as for an utterance too long to fit: the same bits. */
#define SETK_CACGMM_UPDATE_ALPHA 0x1 /* --update-alpha: alpha_k = mean_t gamma_k in every M-step
                                       (Cacgmm.update, cluster.py:364-365) instead of 1 / K */
#define SETK_CACGMM_CGMM_INIT 0x2    /* --cgmm-init: B_0 = sum_t z z^H / T, B_1 = I, one E-step
                                       (cluster.py:496-507); K = 2 and gamma0 = NULL only */
int setk_cacgmm_masks(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                      int num_bins, int num_classes, int num_iters, const double* gamma0, int flags,
                      float* gamma_out, int* status, void* stream);

/* The compute loop of estimate_cacgmm_masks.py:31-66 for a batch, audio in, masks out: one STFT
 * launch (n_fft = 512 plan) straight into the bin-major layout, one EM launch.  Device pointers:
 * audio[u] float32 [C][num_samples[u]] (16-bit PCM is converted in front, as for
 * setk_cgmm_estimate_batch: setk_pcm16_to_float_batch), gamma0[u] float64 [K][257][T_u] (the
 * table may be NULL with SETK_CACGMM_CGMM_INIT), gamma_out[u] float32 [K][T_u][257].  status[u]
 * (host memory, may be NULL) receives the worst SETK_NUM_* over the bins of utterance u; the call
 * then returns after the stream has drained. */
int setk_cacgmm_estimate_batch(setk_handle_t h, int n_utts, int num_channels,
                               const float* const* audio, const int* num_samples, int num_classes,
                               int num_iters, const double* const* gamma0, int flags,
                               float* const* gamma_out, int* status, void* stream);

/* directional_feats (libs/spatial.py:184-208, compute_df_on_mask.py:40-54):
 * out[t][f] = mean over the n_pairs microphone pairs (i, j) = (pairs[2p],
 * pairs[2p+1], host array) of cos((arg X_i - arg X_j) - (arg v_i - arg v_j)),
 * spec [C][T][F] and steer_vector [F][C] complex64, out [T][F] float32. */
int setk_directional_feats(setk_handle_t h, const float* spec, const float* steer_vector,
                           const int* pairs, int n_pairs, int num_channels, int num_frames,
                           int num_bins, float* out, void* stream);

/* FixedBeamformer.run + inverse_stft for a batch (apply_fixed_beamformer.py:
 * 38-48, libs/beamformer.py:323-340): wave[u] = istft(sum_c conj(w[f][c]) X_c),
 * rescaled to max |audio[u]| (SpectrogramReader.maxabs).  weights: n_sets
 * filters in the reference layout [set][F = 257][C] complex64 (host or device);
 * weight_index[u] (host, may be NULL = set 0) picks the beam of utterance u.
 * audio / wave: device pointers as for setk_enhance_batch; flags:
 * SETK_FLAG_OUT_PCM16, SETK_FLAG_NO_RENORM (the wave as inverse_stft(norm=None)
 * leaves it: apply_classic_beamformer.py:109-110 without --normalize).  Needs the
 * n_fft = 512 plan. */
int setk_apply_weights_batch(setk_handle_t h, int n_utts, int num_channels,
                             const float* const* audio, const int* num_samples,
                             const float* weights, int n_sets, const int* weight_index,
                             void* const* wave, int flags, void* stream);

/* ---- WPE dereverberation --------------------------------------
 * wpe_step of scripts/sptk/libs/wpe.py:58-81 (tap-stacked correlation, solve,
 * filter; fp64 like the reference) iterated `num_iters` times as wpe() does
 * (:84-110): spec / out [C][T][F] complex64.  lambda of the first iteration is
 * compute_lambda(spec, context) (:32-55) or, when lambda_enh != NULL,
 * max(|lambda_enh[t][f]|^2, eps) -- the previous enhanced signal of
 * facted_wpd() (:146-149); later iterations use compute_lambda(dereverb).
 * inv_lambda_out (may be NULL) receives 1 / lambda of the last iteration as a
 * float32 [T][F] array: passed to setk_covar as the mask it yields the
 * power-weighted covariance of facted_wpd (:160-162, up to a per-bin scale that
 * cancels in the MVDR weight).  status[F] (may be NULL) receives SETK_NUM_*;
 * SETK_NUM_SINGULAR is numpy's LinAlgError, SETK_NUM_RANKDEF a note (columns at the noise
 * level were dropped; the result is finite).  Limits: channels <= 16, NK = channels * taps
 * <= 256.  While R fits LDS (NK^2 + NK N + 16 (NK + N) complex128 <= 160 KB: up to 8
 * channels x 11 taps, 16 x 5) a workgroup never leaves its CU; beyond that (8 x 12, 16 x 6,
 * 16 x 10 ...) R is factored in global scratch of the handle's arena (NK^2 complex128 per
 * bin and utterance in flight).  NK > 256: SETK_ERR_UNSUPPORTED names the bound. */
int setk_wpe(setk_handle_t h, const float* spec, int num_channels, int num_frames,
             int num_bins, int taps, int delay, int context, int num_iters,
             const float* lambda_enh, float* out, float* inv_lambda_out,
             int* status, void* stream);

/* One wpe_step (scripts/sptk/libs/wpe.py:58-81) with the caller's variances used AS
 * GIVEN: lambda_ft is float64 [F][T] (the reference's F x T), no floor, no
 * re-estimation.  spec / out [C][T][F] complex64; taps / delay describe the tap
 * matrix compute_tap_mat(reverb, taps, delay) (:13-29) that the kernel indexes in
 * place.  status as setk_wpe. */
int setk_wpe_step(setk_handle_t h, const float* spec, int num_channels, int num_frames,
                  int num_bins, int taps, int delay, const double* lambda_ft, float* out,
                  int* status, void* stream);

/* wpe() (libs/wpe.py:84-110) for n_utts utterances of the same channel count in one
 * call: every iteration is ONE launch over (bin, utterance) instead of 257 workgroups
 * per utterance.  spec[u] / out[u] [C][num_frames[u]][F] complex64 (host or device),
 * status [n_utts][F] or NULL.  Same limits as setk_wpe. */
int setk_wpe_batch(setk_handle_t h, int n_utts, const float* const* spec, int num_channels,
                   const int* num_frames, int num_bins, int taps, int delay, int context,
                   int num_iters, float* const* out, int* status, void* stream);

/* setk_wpe_batch for facted_wpd's batch (libs/wpe.py:113-177, apply_wpd.py:20-60): the
 * variances of iteration 0 come per utterance from lambda_enh[u] (complex64 [T_u][F], |.|^2 of
 * the previous enhanced signal; a NULL array or entry: compute_lambda of the input, as
 * setk_wpe_batch), and inv_lambda_out[u] (float32 [T_u][F], NULL array: not wanted) receives
 * 1 / lambda of the LAST iteration -- the per-utterance arguments of setk_wpe, for n_utts
 * utterances behind one launch per iteration. */
int setk_wpe_batch_var(setk_handle_t h, int n_utts, const float* const* spec, int num_channels,
                       const int* num_frames, int num_bins, int taps, int delay, int context,
                       int num_iters, const float* const* lambda_enh, float* const* out,
                       float* const* inv_lambda_out, int* status, void* stream);

/* The same with spec[u] / out[u] in the reference's own layout, F x N x T_u complex64 (the
 * `reverb` / return value of wpe(), libs/wpe.py:84-110): it is the layout the step kernel
 * works in, so no transposition happens on either side.  out[u] must not alias spec[u]. */
int setk_wpe_batch_fnt(setk_handle_t h, int n_utts, const float* const* spec, int num_channels,
                       const int* num_frames, int num_bins, int taps, int delay, int context,
                       int num_iters, float* const* out, int* status, void* stream);

/* Which form of the step kernel the entries above launch for `num_channels` x `taps`: *wide is 1
 * when R is factored in global scratch and 0 when it stays in LDS, *tiles_per_wave the
 * accumulator tiles per wavefront of the kernel instantiation (the wide form: per pass over the
 * frames), *chunk_frames how many frames are staged at a time (64, 32 or 16).  Any of the three
 * may be NULL.  SETK_ERR_UNSUPPORTED for a shape the entries refuse.  No handle, no device
 * work. */
int setk_wpe_form(int num_channels, int taps, int* wide, int* tiles_per_wave, int* chunk_frames);

/* ---- AuxIVA blind source separation (scripts/sptk/apply_auxiva.py) ----------
 * auxiva(X, epochs) (:24-57): as many sources as channels, demixing matrices W_f = I to start
 * with; per epoch r_n(t) = sqrt(sum_f |y_n(f, t)|^2), g = 1 / (r + float32 eps) (:42-44), per bin
 * and source in order V_n = sum_t g_n x x^H / T, w = solve(W^H V_n, e_n), W[:, n] = w / (w^H V_n w)
 * (:45-52), y = W^H x (:54).  Observations are complex64 like the reference's; g, V, W, the
 * solves, y and r are float64 (the reference's complex128 -- in float32 the doc recording
 * deviates by 5e-4).  Two runs on the same input give the same bits (no floating-point atomics).
 *   spec / out  [C][T][F] complex64, host or device: the reference's N x T x F.  Any F, any T.
 *               num_epochs = 0 returns spec (Y = X conj(I)).
 *   status      [F] or NULL, host or device: SETK_NUM_SINGULAR where a pivot of the LU with
 *               partial pivoting of some W^H V_n was exactly zero (a silent channel, an all-zero
 *               utterance: numpy.linalg.solve raises LinAlgError("Singular matrix") there, :51,
 *               and the reference's run ends), SETK_NUM_NONFINITE for NaN / inf in the bin's
 *               input or result; worst over epochs and sources.  The output of such a bin is
 *               not meaningful.
 * SETK_ERR_UNSUPPORTED: num_channels outside 1 .. 8. */
int setk_auxiva(setk_handle_t h, const float* spec, int num_channels, int num_frames, int num_bins,
                int num_epochs, float* out, int* status, void* stream);

/* The loop body of run() (apply_auxiva.py:60-79) for a batch of utterances with the same channel
 * count: STFT straight into the bin-major layout of the epoch kernels, the epochs, the
 * inverse STFT of every source, renorm to max |audio[u]| (inverse_stft(norm=maxabs), :74-76).
 *   audio[u]   device float32 [C][num_samples[u]]
 *   wave[u]    device float32 [C][L_u], L_u = setk_istft_num_samples(T_u, -1) (hop (T_u - 1) when
 *              centred); with SETK_FLAG_OUT_PCM16 int16 [C][L_u] (libsndfile's float -> PCM_16)
 *   status[u]  worst bin status of the utterance, host or device, or NULL
 * The pointer tables and num_samples are HOST arrays of n_utts entries.  Requires the
 * n_fft = 512 plan and 1 <= C <= 8; scratch comes from the handle's arena; the call returns
 * when the work has run.  With setk_set_profiling the stage times of setk_last_stage_ms are
 * out[0] STFT + max |audio|, out[1] the epochs (with their projections), out[2] transposition
 * + inverse STFT, out[3] renorm. */
int setk_auxiva_batch(setk_handle_t h, int n_utts, int num_channels, const float* const* audio,
                      const int* num_samples, int num_epochs, void* const* wave, int* status,
                      int flags, void* stream);

/* ---- sound source localisation (scripts/sptk/do_ssl.py, libs/ssl.py) ------
 * One direction of arrival per window of frames, out of the spectrogram, an optional TF mask and
 * a steer-vector set sv [A][C][F] complex64 (compute_steer_vector.py's A x M x F file).
 *   SETK_SSL_ML     ml_ssl (libs/ssl.py:12-43): sv normalised over the microphones, delta =
 *                   sum_m |x|^2 - |sum_m sv conj(x)|^2 / (1 + eps), ll = -log(max(delta, eps))
 *                   (compression <= 0) or -delta^compression, score[a] = sum_{t,f} mask ll;
 *                   `norm` first divides x by max(|x|, eps).  The argmax.
 *   SETK_SSL_SRP    srp_ssl (:46-77): score[a] = sum_{t,f} mask mean_p cos((arg x_l - arg x_r) -
 *                   (arg sv_l - arg sv_r)) over the n_pairs microphone pairs (l, r) =
 *                   (pairs[2p], pairs[2p + 1]) (host array), computed on unit phasors (arg 0 = 0 as
 *                   np.angle has it) without atan2 / cos.  The argmax.
 *   SETK_SSL_MUSIC  music_ssl (:80-110): score[a] = sum_f |sv^H E_n E_n^H sv| with E_n E_n^H =
 *                   I - v v^H, v the principal eigenvector (setk_pevd) of the covariance of
 *                   stft * mask (setk_covar with the mask squared).  The argmin.
 * ML and SRP compute float32 frame scores S[t][a] once and sum them per window in frame order
 * (float64); SRP with a single window folds the frames first.  No floating-point atomics: two
 * runs give the same bits. */
#define SETK_SSL_ML 0
#define SETK_SSL_SRP 1
#define SETK_SSL_MUSIC 2
typedef struct setk_ssl_opts {
    int backend;       /* SETK_SSL_*                                            */
    int n_pairs;       /* SRP: number of microphone pairs                       */
    const int* pairs;  /* SRP: host array of 2 n_pairs channel indices          */
    float compression; /* ML: <= 0 selects the logarithm (do_ssl.py passes -1)  */
    int norm;          /* ML: normalise the observations                        */
    double eps;        /* ML: do_ssl.py passes float32 eps, ml_ssl's default is 1e-8 */
} setk_ssl_opts;

/* get_doa (do_ssl.py:30-37) for every window [windows[2w], windows[2w + 1]) of frames (host
 * array; NULL: the one window [0, num_frames), the offline case, do_ssl.py:94-98; the online
 * loop :101-112 is one call with its windows).
 *   spec    [C][T][F] complex64, mask [T][F] float32 or NULL, steer_vector [A][C][F] complex64
 *   score   [W][A] float64 or NULL, index [W] int32: the lowest index attaining the extremum,
 *           as np.argmax / np.argmin choose
 *   status  one int or NULL: MUSIC, the worst setk_pevd status over bins and windows (a bin
 *           whose covariance is zero has no defined eigenvector: SETK_NUM_SINGULAR); 0 for the
 *           other backends
 * All data pointers host or device.  Any A, T, F; SETK_ERR_UNSUPPORTED outside 1 <= C <= 16. */
int setk_ssl_scores(setk_handle_t h, const setk_ssl_opts* opts, const float* spec, const float* mask,
                    const float* steer_vector, int num_doas, int num_channels, int num_frames,
                    int num_bins, const int* windows, int num_windows, double* score, int* index,
                    int* status, void* stream);

/* The loop body of run() (do_ssl.py:80-114) for a batch of utterances with the same channel
 * count and one steer-vector set: STFT into scratch of the handle's arena (one launch for the
 * batch up to 8 channels, the stand-alone transform per utterance beyond), frame scores,
 * windows.
 *   audio[u]       device float32 [C][num_samples[u]]
 *   mask           NULL, or per utterance a device float32 [T_u][F] array or NULL
 *   windows        host, the window tables of all utterances one after another;
 *                  num_windows[u] >= 1 windows belong to utterance u
 *   index          [sum W] int32, score [sum W][A] float64 or NULL, status [n_utts] or NULL;
 *                  host or device
 * The pointer tables and num_samples are HOST arrays of n_utts entries.  Requires the
 * n_fft = 512 plan and 1 <= C <= 16; the call returns when the work has run.  With
 * setk_set_profiling the stage times of setk_last_stage_ms are out[0] STFT, out[1] frame scores
 * (MUSIC: covariances, eigenvectors and scores), out[2] window reduction and arg-extremum. */
int setk_ssl_batch(setk_handle_t h, const setk_ssl_opts* opts, int n_utts, int num_channels,
                   const float* const* audio, const int* num_samples, const float* const* mask,
                   const float* steer_vector, int num_doas, const int* windows, const int* num_windows,
                   int* index, double* score, int* status, void* stream);

/* ---- geometry-driven spatial features (scripts/sptk/libs/spatial.py) -------
 * All kinds start from the pair coherence u_p[t][f] = exp(i (arg X_l - arg X_r)) of the n_pairs
 * microphone pairs (l, r) = (pairs[2p], pairs[2p + 1]) (host array), computed on unit phasors
 * (arg 0 = 0, as np.angle has it).  out is float32 [T][width]:
 *   SETK_SPATIAL_IPD          ipd() (libs/spatial.py:163-176): the phase difference wrapped into
 *                             [-pi, pi), the pairs side by side (np.hstack,
 *                             compute_ipd_and_linear_srp.py:36-47); width = n_pairs F
 *   SETK_SPATIAL_COS_IPD      cos=True (:177-179); width = n_pairs F
 *   SETK_SPATIAL_COS_SIN_IPD  sin=True (:180-181): [cos | sin] per pair; width = 2 n_pairs F
 *   SETK_SPATIAL_DF           directional_feats (:184-208) for n_index directions of the
 *                             steer-vector set sv [num_sv][C][F] complex64 (host or device),
 *                             laid out as compute_df_on_geometry.py:49-60 does:
 *                             out[t][k F + f] = mean_p cos((arg X_l - arg X_r) - (arg v_l - arg v_r)),
 *                             v = sv[doa_index[k]]; width = n_index F
 *   SETK_SPATIAL_SRP          the SRP-PHAT angular spectrum of gcc_phat_linear / srp_phat_linear
 *                             (:37-57, :95-123) and gcc_phat_diag (:60-92) averaged as
 *                             compute_circular_srp.py:40-51 does: per pair s_p[t][d] =
 *                             Re sum_f u_p[t][f] W_p[f][d], divided by max(max_{t,d} |s_p|,
 *                             float32 eps), floored at 0, then out[t][d] = sum_p pair_weight[p] x
 *                             that (the pairs in order); width = num_doas.  The table W_p =
 *                             exp(-i omega_f tau_{p,d}) is the caller's: [n_pairs][F][Dpad]
 *                             complex64 (host or device), Dpad = num_doas rounded up to a multiple
 *                             of 64, zero beyond num_doas; pair_weight is a host array.
 * Maxima are integer maxima on the bits of non-negative floats: no floating-point atomics, two
 * runs give the same bits.  2 <= C <= 16, n_pairs <= 120, F >= 2 (otherwise
 * SETK_ERR_UNSUPPORTED); any T >= 1, any num_doas >= 1. */
#define SETK_SPATIAL_IPD 0
#define SETK_SPATIAL_COS_IPD 1
#define SETK_SPATIAL_COS_SIN_IPD 2
#define SETK_SPATIAL_DF 3
#define SETK_SPATIAL_SRP 4
typedef struct setk_spatial_opts {
    int kind;                  /* SETK_SPATIAL_*                                        */
    int n_pairs;               /* number of microphone pairs                            */
    const int* pairs;          /* host array of 2 n_pairs channel indices               */
    int num_doas;              /* SRP: directions D of the table                        */
    const float* table;        /* SRP: W [n_pairs][F][Dpad] complex64                   */
    const float* pair_weight;  /* SRP: host [n_pairs]                                   */
    int num_sv;                /* DF: directions of the steer-vector set                */
    const float* steer_vector; /* DF: [num_sv][C][F] complex64                          */
    int n_index;               /* DF: directions per utterance                          */
    const int* doa_index;      /* DF: host [n_utts][n_index], each in [0, num_sv)       */
} setk_spatial_opts;

/* One spectrogram spec [C][T][F] complex64 -> out [T][width] float32; data pointers host or
 * device.  With device operands the call is asynchronous, like the other stand-alone operators. */
int setk_spatial_feats(setk_handle_t h, const setk_spatial_opts* opts, const float* spec,
                       int num_channels, int num_frames, int num_bins, float* out, void* stream);

/* The loop bodies of compute_ipd_and_linear_srp.py:52-73, compute_circular_srp.py:38-55 and
 * compute_df_on_geometry.py:47-69 behind the STFT, for a batch of spectrograms of one channel
 * count: spec[u] device complex64 [C][num_frames[u]][F] (what setk_stft_batch wrote), out[u]
 * device float32 [num_frames[u]][width]; the pointer tables and num_frames are HOST arrays of
 * n_utts entries.  One set of launches for the batch (IPD, DF: one; SRP: the observation tiles,
 * the pair contraction, the combination), scratch from the handle's arena (SRP: per utterance
 * n_pairs T (F 256 bytes per 32 frames + 4 Dpad bytes)); asynchronous on `stream`.  Each
 * utterance's result has the bits of setk_spatial_feats on the same spectrogram. */
int setk_spatial_batch(setk_handle_t h, const setk_spatial_opts* opts, int n_utts, int num_channels,
                       const float* const* spec, const int* num_frames, int num_bins,
                       float* const* out, void* stream);

/* ---- OM-LSA noise suppression (scripts/sptk/libs/ns.py, apply_ns.py) --------
 * MCRA.run (libs/ns.py:56-209) and iMCRA.run (:247-387): the spectral gain of the optimally
 * modified log-spectral amplitude estimator with minima-controlled recursive averaging of the
 * noise, one channel.  float64 throughout like the reference, the exponential integral of
 * :65-66 / :259-260 (scipy.integrate.quad per cell there) in closed form.  One workgroup per
 * utterance walks the frames; the fields are the constructor arguments (:18-54, :221-245) after
 * the conversions the constructors make. */
#define SETK_NS_MCRA 0
#define SETK_NS_IMCRA 1
#define SETK_NS_OUT_GAIN 0x1 /* the gain, float64 [T][F]                              */
#define SETK_NS_OUT_SPEC 0x2 /* gain x spectrogram, complex64 [T][F], in the same pass */
#define SETK_NS_MAX_TAPS 63
typedef struct setk_ns_opts {
    int kind;  /* SETK_NS_*                                                          */
    int flags; /* SETK_NS_OUT_*                                                      */
    double alpha, alpha_s, alpha_d;
    double gmin;   /* 10^(gmin_db / 10)                                              */
    double xi_min; /* 10^(xi_min_db / 10)                                            */
    /* the smoothing windows as np.convolve takes them: scipy.signal.get_window(h, 2 w + 1),
     * fftbins=True (periodic: hann, 3 taps is [0, 0.75, 0.75]); host arrays of n_* taps, each odd
     * and at most SETK_NS_MAX_TAPS.  iMCRA reads w_mcra alone. */
    int n_mcra, n_local, n_global;
    const double *w_mcra, *w_local, *w_global;
    /* MCRA */
    double delta, beta, alpha_p, q_max;
    double zeta_min, zeta_max, zeta_p_min, zeta_p_max; /* 10^(*_db / 10)             */
    int L, M;
    /* iMCRA (beta above is its bias factor, 1.47) */
    double inv_b_min; /* 1 / b_min                                                   */
    double gamma0, gamma1, zeta0;
    int V, U; /* 1 <= U <= 32                                                        */
    double eps; /* run(stft, eps): 1e-7 in the reference                             */
} setk_ns_opts;

/* suppressor.run(stft) (apply_ns.py:41, :48) for one stored spectrogram spec [T][F] complex64,
 * host or device: gain [T][F] float64 (SETK_NS_OUT_GAIN) and / or out [T][F] complex64 = gain x
 * spec (SETK_NS_OUT_SPEC, apply_ns.py:42's operand), host or device; an output whose flag is not
 * set may be NULL.  status (one int, host or device, may be NULL): SETK_NUM_NONFINITE for NaN /
 * inf in the input or a non-finite gain.  iMCRA has no floor under its a-posteriori SNR
 * (:272): a cell of digital silence makes the reference's integral diverge and every later frame
 * NaN; here E1 alone sees that SNR floored at eps, as MCRA.run floors it (:84).
 * SETK_ERR_UNSUPPORTED: F > 1025, a window longer than SETK_NS_MAX_TAPS or than F (np.convolve's
 * "same" then changes its length), U > 32. */
int setk_ns_gain(setk_handle_t h, const setk_ns_opts* opts, const float* spec, int num_frames,
                 int num_bins, double* gain, float* out, int* status, void* stream);

/* The loop body of run() (apply_ns.py:37-49) for a batch of single-channel utterances: one STFT
 * launch (n_fft = 512 plan), one launch of the recursion, and for waveforms one inverse-STFT
 * launch (inverse_stft(gain * stft) without norm, :42).
 *   audio[u]   device float32 [num_samples[u]]; with SETK_FLAG_IN_PCM16 device int16
 *              [num_samples[u]] as the wave file stores it, scaled by 2^-15 on the device
 *   wave[u]    SETK_NS_OUT_SPEC: device float32 [L_u], L_u = setk_istft_num_samples(T_u, -1), or
 *              int16 with SETK_FLAG_OUT_PCM16 (libsndfile's float -> PCM_16); may be NULL otherwise
 *   gain[u]    SETK_NS_OUT_GAIN: device float64 [T_u][257]; may be NULL otherwise
 *   status[u]  as setk_ns_gain, host or device, or NULL
 * flags: SETK_FLAG_IN_PCM16 | SETK_FLAG_OUT_PCM16; what comes out is opts->flags.  The pointer
 * tables and num_samples are HOST arrays of n_utts entries; scratch comes from the handle's arena;
 * the call returns when the work has run.  Every utterance has the bits of setk_stft ->
 * setk_ns_gain -> setk_istft on its own.  With setk_set_profiling the stage times of
 * setk_last_stage_ms are out[0] conversion + STFT, out[1] the recursion, out[2] inverse STFT,
 * out[3] rounding to 16 bits. */
int setk_ns_batch(setk_handle_t h, const setk_ns_opts* opts, int n_utts, const void* const* audio,
                  const int* num_samples, void* const* wave, double* const* gain, int* status,
                  int flags, void* stream);

/* The exponential integral E1(x) = int_x^inf exp(-t) / t dt of libs/ns.py:65-66 on its own:
 * y[i] = E1(x[i]) for x > 0 (float64, host or device), relative error below 1e-13; 0 where it
 * underflows (x > 745). */
int setk_expint_e1(setk_handle_t h, const double* x, double* y, int n, void* stream);

/* ---- oracle TF masks and mask-based separation -------------------------------
 * scripts/sptk/compute_mask.py, wav_separate.py, oracle_separate.py.  float32 throughout, as the
 * reference is once its spectra are complex64; |z| is cmat_abs (libs/utils.py:30-42), sqrt(re^2 +
 * im^2); the cosine of a phase difference is formed without trigonometry.  A cell with an operand
 * that is exactly zero follows numpy: np.angle(0) = 0, 0 / 0 = NaN, x / 0 = +-inf, and the clips
 * hand a NaN on as np.minimum / np.maximum do. */
#define SETK_TFMASK_IBM 0 /* |tgt| > |mix - tgt|                                           */
#define SETK_TFMASK_IRM 1 /* |tgt| / sqrt(|tgt|^2 + |mix - tgt|^2 + eps)                   */
#define SETK_TFMASK_IAM 2 /* |tgt| / |mix|                                                 */
#define SETK_TFMASK_PSM 3 /* |tgt| cos(arg mix - arg tgt) / |mix|                          */
#define SETK_TFMASK_PSA 4 /* |tgt| max(0, cos(arg mix - arg tgt))                          */
#define SETK_TFMASK_CRM 5 /* tgt / (mix + eps), both parts through 10 tanh(0.05 x); [T][2F] */
#define SETK_TFMASK_MAX_TARGETS 8
/* what run() logs per utterance (compute_mask.py:136-152): cells above the cutoff, cells below
 * zero after that clip, and the sum of the latter (float64, a fixed order: the same bits in any
 * batch) */
typedef struct setk_tfmask_stats {
    long long over;
    long long below;
    double below_sum;
} setk_tfmask_stats;

/* compute_mask(tgt, mix, kind) (compute_mask.py:59-107) and the clips of run() (:136-152) --
 * min(mask, cutoff) when cutoff > 0, then max(mask, 0), for every kind as the tool has it -- on
 * stored spectra tgt, mix [T][F] complex64: mask [T][F] float32 ([T][2F] for SETK_TFMASK_CRM, real
 * parts then imaginary parts).  A NaN cutoff leaves both clips out: the mask as compute_mask()
 * itself returns it (the statistics are then zero).  All data pointers host or device; stats may
 * be NULL.  Any T, F. */
int setk_tf_mask(setk_handle_t h, int kind, const float* tgt, const float* mix, int num_frames,
                 int num_bins, float cutoff, float* mask, setk_tfmask_stats* stats, void* stream);

/* wav_separate.py:63-74 in front of the inverse: out = spec x mask, or with phase_ref
 * |spec| x mask x exp(i angle(phase_ref)); spec, phase_ref, out [T][F] complex64, mask [T][F]
 * float32, host or device; phase_ref may be NULL. */
int setk_tf_apply(setk_handle_t h, const float* spec, const float* mask, const float* phase_ref,
                  int num_frames, int num_bins, float* out, void* stream);

/* The loop body of compute_mask.py:128-153 for a batch of (clean, noisy) pairs, n_fft = 512 plan:
 * ONE launch transforms both signals of every frame and stores the mask alone.
 *   tgt[u], mix[u]  device float32 [num_samples[u]] (one length per pair), or with
 *                   SETK_FLAG_IN_PCM16 device int16 as the wave file stores it (x 2^-15 on the
 *                   device, the bits of the float32 form)
 *   mask[u]         device float32 [T_u][257] ([T_u][514] for crm)
 *   stats           n_utts entries, host or device, or NULL
 *   status[u]       SETK_NUM_NONFINITE when the mask holds NaN / inf (it is delivered all the
 *                   same: the reference writes such masks too); host or device, or NULL
 * The pointer tables and num_samples are HOST arrays; scratch from the handle's arena; the call
 * returns when the work has run.  Every output value has one owner and a fixed order: an
 * utterance has the same bits alone and in any batch.  With setk_set_profiling the stage times of
 * setk_last_stage_ms are out[0] the fused forward, out[1] the statistics. */
int setk_tf_mask_batch(setk_handle_t h, int kind, int n_utts, const void* const* tgt,
                       const void* const* mix, const int* num_samples, float cutoff,
                       float* const* mask, setk_tfmask_stats* stats, int* status, int flags,
                       void* stream);

/* The loop body of wav_separate.py:39-75 for a batch: one fused forward launch (the mixture, and
 * the phase reference where given, transformed and masked in registers), one inverse-STFT launch,
 * one scaling launch.
 *   mix[u]        device samples as above;  phase_ref: NULL, or a table whose entries may be NULL
 *   mask[u]       device float32 [T_u][257]
 *   norm          HOST array or NULL: norm[u] > 0 scales the wave to that max-abs
 *                 (inverse_stft(norm=), --use-mixed-norm), otherwise the wave stays as it is
 *   nsamps        HOST array or NULL: nsamps[u] >= 0 is the wave's length (--keep-length),
 *                 otherwise setk_istft_num_samples(T_u, -1)
 *   wave[u]       device float32, or int16 with SETK_FLAG_OUT_PCM16
 *   status[u]     SETK_NUM_NONFINITE for NaN / inf in the masked spectrum; host or device, or NULL
 * Stage times: out[0] forward, out[1] inverse, out[2] scaling. */
int setk_tf_separate_batch(setk_handle_t h, int n_utts, const void* const* mix,
                           const void* const* phase_ref, const int* num_samples,
                           const float* const* mask, const float* norm, const int* nsamps,
                           void* const* wave, int* status, int flags, void* stream);

/* The loop body of oracle_separate.py:65-82 for a batch with num_targets references per mixture:
 * compute_mask (:19-45) for SETK_TFMASK_IBM / IRM / IAM / PSM (any other kind: SETK_ERR_INVALID,
 * the tool's choices) and inverse_stft(mixture x mask_k) without norm.  One fused forward launch
 * runs num_targets + 1 transforms per frame and stores the masked spectra alone; one inverse
 * launch takes them as n_utts x num_targets utterances.  targets[u * K + k], wave[u * K + k];
 * nsamps as above.  More than SETK_TFMASK_MAX_TARGETS targets: SETK_ERR_UNSUPPORTED. */
int setk_oracle_separate_batch(setk_handle_t h, int kind, int n_utts, int num_targets,
                               const void* const* mix, const void* const* targets,
                               const int* num_samples, const int* nsamps, void* const* wave,
                               int* status, int flags, void* stream);

/* ---- SI-SNR scoring (scripts/sptk/libs/metric.py, compute_si_snr.py) --------
 * si_snr (libs/metric.py:13-33): with x' = x - mean(x), s' = s - mean(s) (remove_dc), a = <x', s'> /
 * (|s'|^2 + eps) and n = x' - a s' formed per sample, 20 log10(|a s'| / (|n| + eps) + eps).
 * permute_si_snr (:36-60): the largest of sum_n si_snr(x[n], s[order[n]]) / K over
 * itertools.permutations(range(K)) in its order, summed left to right from 0, and that order (the
 * first on ties, np.argmax).  Float64 sums on the samples as given, where the reference computes
 * in float32; every sum has one owner and a fixed order, so an utterance has the same bits in any
 * batch.  A silent or constant signal and num_samples = 1 give 20 log10(eps). */
#define SETK_FLAG_KEEP_DC 0x100 /* si_snr(remove_dc=False): the means stay in                     */

/* si_snr (libs/metric.py:13-33) for every (estimate, reference) pair of every utterance and
 * permute_si_snr (:36-60) over them; the loop bodies of compute_si_snr.py:80-105 for a batch.
 *   num_src[u]     K_u estimates and K_u references, 1 <= K_u <= 8 (beyond: SETK_ERR_UNSUPPORTED,
 *                  the search walks K! orders)
 *   est / ref      sum(num_src) device pointers, utterance-major: float32 samples, or with
 *                  SETK_FLAG_IN_PCM16 int16 samples as the wave file stores them (v / 32768, the
 *                  same bits as the float32 form of those samples)
 *   *_stride       the distance between samples of a signal: 1 for a mono buffer, C for channel 0
 *                  of interleaved N x C frames (compute_si_snr.py:36 scores wave[0])
 *   num_samples[u] one length per utterance, >= 1
 *   pair           sum(num_src^2) float64: pair[i * K + j], estimate i against reference j
 *   best           n_utts float64, may be NULL;  perm: sum(num_src) int, the chosen order, may be NULL
 *   status[u]      SETK_NUM_NONFINITE for NaN / inf among the utterance's samples, may be NULL
 * flags: SETK_FLAG_IN_PCM16 | SETK_FLAG_KEEP_DC, anything else is SETK_ERR_INVALID.  The tables
 * num_src, est, ref, the strides and num_samples are HOST arrays; pair, best, perm and status host
 * or device.  Six launches for the batch whatever its size (four with SETK_FLAG_KEEP_DC), scratch
 * from the handle's arena; the call returns when the work has run.  With setk_set_profiling the
 * stage times of setk_last_stage_ms are out[0] the means, out[1] the centred Gram sums, out[2] the
 * residuals, out[3] the table, the search and the copies. */
int setk_si_snr_batch(setk_handle_t h, int n_utts, const int* num_src, const void* const* est,
                      const int* est_stride, const void* const* ref, const int* ref_stride,
                      const int* num_samples, double eps, int flags, double* pair, double* best,
                      int* perm, int* status, void* stream);

/* One pair of host or device vectors of num_samples samples: what libs.metric.si_snr calls
 * (libs/metric.py:13-33); out one float64, host or device.  Flags as above. */
int setk_si_snr(setk_handle_t h, const float* x, const float* s, int num_samples, double eps, int flags,
                double* out, void* stream);

/* ---- data simulation: scripts/sptk/wav_simulate.py -------------------------
 * Reverberation, mixing at an SDR / SNR and peak normalisation of far-field training data.
 * Float32 data, float64 sums and coefficients. */
#define SETK_SIMU_MAX_TAPS 16384
#define SETK_SIMU_MAX_CHANNELS 16
#define SETK_SIMU_REPEAT 0x1 /* setk_simu_source::flags: --point-noise-repeat (:114-118) */

/* add_room_response (wav_simulate.py:29-54, early_energy=False): out[c][n] = sum_j spk[n - j]
 * rir[c][j], n < num_samples -- scipy.signal.convolve(spk[None], rir)[..., :S] -- as a uniformly
 * partitioned overlap-save convolution on the 512-point real transform (block 256): exact up to
 * float32 rounding, worst error about 2e-7 of the peak.
 *   spk     [num_samples] float32, or int16 with SETK_FLAG_IN_PCM16 (scaled by 2^-15)
 *   rir     [num_channels][num_taps] float32
 *   out     [num_channels][num_samples] float32
 *   power0  NULL, or one float64: np.mean(out[0]**2) (:54), a float64 sum in a fixed order
 * Buffers may be host or device memory.  1 <= num_channels <= 16, 1 <= num_taps <= 16384,
 * num_samples >= 1; otherwise SETK_ERR_UNSUPPORTED.  Needs no STFT plan. */
int setk_fir_reverb(setk_handle_t h, const void* spk, int num_samples, const float* rir, int num_channels,
                    int num_taps, float* out, double* power0, int flags, void* stream);

/* One source of a mixture: a speaker (add_speaker, :57-93) or a point noise (add_point_noise,
 * :96-143). */
typedef struct setk_simu_source {
    const void* audio;  /* device float32 [channels][num_samples], planar; int16 with
                         * SETK_FLAG_IN_PCM16.  What read_wav returned: a noise is already cut to
                         * [offset, offset + mixture length) (:199-205) */
    const void* rir;    /* device float32 [rir_channels][rir_taps], or NULL (the close-talk forms:
                         * the source itself is the image, :69-72, :120-124) */
    int num_samples;
    int channels;       /* 1 with a RIR (:38-39) */
    int rir_channels, rir_taps;
    int begin;          /* --src-begin / --point-noise-begin, >= 0 */
    int flags;          /* SETK_SIMU_REPEAT (noises) */
    double snr;         /* --src-sdr of a speaker against the first (ignored for the first, :91),
                         * --point-noise-snr of a noise */
} setk_simu_source;

/* One mixture: the arguments of run_simu (:166-312) after its files are read. */
typedef struct setk_simu_recipe {
    const setk_simu_source* speakers; /* host array [n_speakers], n_speakers >= 1 */
    const setk_simu_source* noises;   /* host array [n_noises] or NULL */
    int n_speakers, n_noises;
    const void* iso;      /* NULL, or the isotropic noise cut to [offset, offset + mixture length):
                           * device [iso_channels][iso_samples], planar, same sample type as audio.
                           * Channel 0 of it is added to EVERY channel (:293-302) */
    int iso_samples, iso_channels;
    double iso_snr;
    int dump_channel;     /* --dump-channel: >= 0 takes that channel of every RIR (:77-79) */
    int pad_;
    double norm_factor;   /* --norm-factor */
    /* results (device memory) */
    void* mix;              /* float32 [N][L], or with SETK_FLAG_OUT_PCM16 int16 [L][N], the frames of a
                             * wave file; N = setk_simu_num_channels, L = setk_simu_num_samples */
    void* const* spk_ref;   /* host array [n_speakers]: channel 0 of every scaled speaker image, [L]
                             * float32 or int16 (:307); an entry may be NULL */
    void* noise_ref;        /* channel 0 of the scaled noise, [L] (:309-312), or NULL.  Not written
                             * when the recipe has neither point nor isotropic noise */
} setk_simu_recipe;

/* L = max_i(begin_i + size_i) (:195; `size` counts the samples of every channel) and N, the
 * channels of the first speaker's image; negative SETK_ERR_* for a recipe without speakers. */
int setk_simu_num_samples(const setk_simu_recipe* r);
int setk_simu_num_channels(const setk_simu_recipe* r);

/* run_simu (:244-312) for a ragged batch of mixtures -- length, source count, tap count and
 * channel count differ freely -- in a handful of launches: the transforms of all sources and RIRs
 * (a RIR that several sources of the call share is transformed once), the convolutions, the image
 * powers, the coefficients (coeff_snr, :17-26, EPSILON inside), the speaker-only power (:255), the
 * peak max |mix| (:304, an integer maximum on the float64 bits) and the scaled outputs.  Sums run in
 * a fixed order: two runs, and a mixture alone or inside any batch, give the same bits.
 *   status[u]  host or device, or NULL: SETK_NUM_NONFINITE when NaN / inf reached the mixture
 * flags: SETK_FLAG_IN_PCM16 (every audio / iso buffer is int16) | SETK_FLAG_OUT_PCM16 (libsndfile's
 * float -> PCM_16 on float32(value), what write_wav does, libs/utils.py:45-62).
 * What the reference's numpy refuses is SETK_ERR_INVALID with its reason: a multi-channel source
 * with a RIR, images whose channel counts cannot be broadcast, noise against speaker channels,
 * isotropic channels, and point noises whose durations do not fit the LAST noise's (:110-142 mix
 * every noise over the duration left behind by the first loop).  Limits (SETK_ERR_UNSUPPORTED): 1 to
 * 16 channels, RIRs of at most 16384 taps, at least one sample per source, begin >= 0.  A recipe
 * without RIRs runs the mixing only.  Scratch comes from the handle's arena; the call returns
 * when the work has run.  With setk_set_profiling the stage times of setk_last_stage_ms are
 * out[0] transforms, out[1] convolutions, out[2] powers, coefficients and peak, out[3] scaling
 * and rounding. */
int setk_simu_batch(setk_handle_t h, int n_mix, const setk_simu_recipe* recipes, int* status, int flags,
                    void* stream);

/* ---- room impulse responses by the image method: include/rir-generator.{h,cc}, src/rir-simulate.cc,
 * scripts/sptk/rir_generate_{1d,2d}.py ------------------------------------------
 * RirGenerator::GenerateRir (rir-generator.cc:108-192) with MicrophoneSim (:194-223): per
 * microphone every image (x, y, z, q, j, k) of the source within |x| <= nx = ceil(num_samples /
 * (2 T.x)) (likewise y, z; T the room in samples) that passes the reflection-order test (:153-155)
 * and floor(dist) < num_samples (:158) adds a Tw = 2 int(0.004 fs + 0.5) tap Hann-windowed sinc at
 * pos = floor(dist) - Tw / 2 + 1, clipped to [0, num_samples), with the gain mic(p) Refl / (4 pi dist
 * cts), cts = c / fs; then the optional second-order high-pass recursion (:180-190).
 * Arithmetic: the inputs are the reference's float32 values; geometry, fractional delay and the
 * sums are float64 (the reference: float32 throughout), rounded to float32 once at the end.  The
 * sums are kept in 64-bit fixed point (2^-40): integer adds do not depend on their order, so a RIR
 * has the same bits run to run, alone or in any batch, however its images are split over
 * workgroups.  tests/PARITY_NOTES_RIR.md has the measured distances. */
#define SETK_RIR_MAX_TAPS 16384
#define SETK_RIR_MAX_MICS 16
#define SETK_RIR_MIC_BIDIRECTIONAL 0 /* the polar patterns of rir-generator.h:32-38, in their order */
#define SETK_RIR_MIC_HYPERCARDIOID 1
#define SETK_RIR_MIC_CARDIOID 2
#define SETK_RIR_MIC_SUBCARDIOID 3
#define SETK_RIR_MIC_OMNIDIRECTIONAL 4
#define SETK_RIR_NO_SPLIT 0x1 /* flags: one workgroup walks all images of a (RIR, microphone) pair */

/* One RIR: RirGeneratorOptions (rir-generator.h:63-113) after ComputeDerived (rir-generator.cc:25-106)
 * has parsed it.  A reverberation time is turned into coefficients by the caller (:78-92 in the
 * reference's float32 steps: setk_amd.libs.rir.beta_from_rt60).  The arrays are HOST memory. */
typedef struct setk_rir_spec {
    const float* room;   /* [3] --room-topo, metres                                             */
    const float* source; /* [3] --source-location                                               */
    const float* mics;   /* [n_mics][3] --receiver-location                                     */
    const float* beta;   /* [n_beta] the reflection coefficients; n_beta must be 6 (:98)        */
    const float* angle;  /* [2] --angle: azimuth, elevation (radians), or NULL for 0, 0         */
    int n_mics;          /* 1 .. SETK_RIR_MAX_MICS                                              */
    int n_beta;
    int mic_type;        /* SETK_RIR_MIC_*                                                      */
    int order;           /* --order, -1: every image                                            */
    int num_samples;     /* --number-samples, 1 .. SETK_RIR_MAX_TAPS                            */
    int hp_filter;       /* --hp-filter                                                         */
    float samp_frequency, sound_velocity;
} setk_rir_spec;

/* GenerateRir for a ragged batch of RIRs: microphone counts, tap counts and rooms differ freely.
 *   out[r]     [n_mics][num_samples] float32, host or device: the generator's matrix, unscaled
 *              (the * 32767 of rir-simulate.cc:64 is the writer's business)
 *   status[r]  host or device, or NULL: SETK_NUM_NONFINITE for NaN / inf among the RIR's inputs
 *              or an image whose gain is not below 2^10 (a source on a microphone; the reference
 *              writes inf / NaN taps there); such an image is left out, the other RIRs of the batch
 *              are not touched
 * flags: SETK_RIR_NO_SPLIT.  specs and out are HOST arrays of n_rirs entries.  Two launches for the
 * batch (the images; the fold of the parts, the high-pass recursion and the rounding), scratch
 * from the handle's arena (8 bytes per tap and part); the call returns when the work has run.
 * SETK_ERR_UNSUPPORTED outside 1 to 16 microphones and 1 to 16384 taps (what setk_simu_batch takes
 * RIRs at), for samp_frequency above 64 kHz (Tw > 512) and more than 2^31 - 1 images per
 * microphone; SETK_ERR_INVALID for what the reference asserts (rir-generator.cc:29-31, :98):
 * samp_frequency < 1, sound_velocity < 1, order < -1, n_beta != 6, an unknown mic_type, and a room
 * dimension that is not positive.  With setk_set_profiling the stage times of
 * setk_last_stage_ms are out[0] the tables, out[1] the images, out[2] fold + high-pass, out[3] the
 * copies. */
int setk_rir_generate_batch(setk_handle_t h, int n_rirs, const setk_rir_spec* specs, float* const* out,
                            int* status, int flags, void* stream);

/* One RIR (what rir-simulate computes for one command line, rir-simulate.cc:54-59): out
 * [n_mics][num_samples] float32 and status (one int, may be NULL), host or device.  The bits of the
 * batch call. */
int setk_rir_generate(setk_handle_t h, const setk_rir_spec* spec, float* out, int* status, int flags,
                      void* stream);

/* ---- fused hot path ------------------------------------------------------
 * The compute body of apply_adaptive_beamformer.py:130-178 for a batch of
 * utterances that share the channel count, in four kernel stages:
 *   1. windowed rFFT + masked outer-product accumulation (never stores X; C > 8: below)
 *   2. batched per-bin weight solve
 *   3. rFFT recompute + w^H x + irFFT + overlap-add
 *   4. max-abs renorm (to max|input|) and emit float32 (or PCM16)
 * audio[u]   device float32 [C][num_samples[u]]; with SETK_FLAG_IN_PCM16 device int16
 *            [C][setk_pcm16_channel_stride(num_samples[u])] (cast to const float*).
 *            Float samples of any magnitude are accepted: the matrix-core transforms of
 *            stage 3 bring an utterance whose max |x| exceeds 1, or stays below 2^-15, into
 *            their fp16 operand range by a power of two taken from stage 1's max |x| (exact,
 *            undone on the way out; nothing changes for 2^-15 <= max |x| <= 1).  Two limits:
 *            stage 1's covariances are float32, so |X|^2 must stay finite (max |x| up to about
 *            2^50; beyond it the utterance is reported SETK_NUM_NONFINITE); and the opt-in
 *            matrix-core stage 1 (SETK_MC_PASS1=1) has no such power of two -- it is meant for
 *            max |x| <= 1, reports SETK_NUM_NONFINITE where a sum leaves fp16 above that, and
 *            below 2^-15 its covariances carry the absolute fp16 floor (2^-34 of full scale per
 *            sample; measured figures in tests/PARITY_NOTES_STFT.md)
 * mask_s[u]  device float32 [T_u][F]
 * mask_n     NULL, or per-utterance interferer masks (--itf-mask)
 * wave[u]    device float32 (or int16) [hop*(T_u-1)] when center, see
 *            setk_istft_num_samples
 * status[u]  int, SETK_NUM_* (worst bin of the utterance); host memory (the call
 *            then synchronises the stream), device memory (asynchronous) or NULL
 * The pointer tables and num_samples are HOST arrays of n_utts entries.
 * Requires the n_fft = 512 plan and 1 <= C <= 16 (otherwise SETK_ERR_UNSUPPORTED).
 *
 * 9 <= C <= 16 (the wide path, csrc/wide.hip): the same four stages and the same results, every
 * kind, BAN, post mask, interferer mask, status, taps, either output type, any stream; but X IS
 * stored once -- stage 1 writes the spectra bin-major, X[f][c][t] complex64 with the frames
 * contiguous at pitch Tp = (T + 3) & ~3, and accumulates the covariances from them on the fp32
 * matrix cores (one 32 x 32 real tile per covariance and bin, slabs of 128 frames summed in
 * order: a result does not depend on what else is in the batch); stage 2 solves the problems
 * embedded in 16 x 16 ones (blkdiag(Rs, 0), blkdiag(Rn, max diag(Rn) I)); stage 3 beamforms from
 * the stored spectra and inverts.  SETK_FLAG_IN_PCM16 is refused there with
 * SETK_ERR_UNSUPPORTED: convert with setk_pcm16_to_float_batch.  Scratch from the handle's
 * arena, per utterance (F = 257):
 *     8 F C Tp                    the spectra
 *   + 8 F T                       the beamformed spectrogram
 *   + 4 F 824 ceil(T / 128)       the covariance slabs
 *   + 4 264 (4 x 136 + 2 x 16)    planes and weights (6 x 136 planes for MPDR; PMWF with the
 *                                 SNR-selected reference: + F 16 (16 + 256 x 8) bytes)
 *   + 4 L_u                       the float32 wave, with SETK_FLAG_OUT_PCM16 only
 * -- about 21 MB for 16 channels x 10 s.  When the arena cannot provide it the call returns
 * SETK_ERR_NOMEM and has launched nothing. */
int setk_enhance_batch(setk_handle_t h, const setk_bf_opts* opts, int n_utts,
                       int num_channels, const float* const* audio,
                       const int* num_samples, const float* const* mask_s,
                       const float* const* mask_n, void* const* wave,
                       int* status, void* stream);

/* The same call with taps on the intermediate results of the fused kernels
 * (parity tests compare them with compute_covar / the weight classes directly;
 * a caller may also keep the weights).  Every member may be NULL; device or
 * host memory:
 *   Rs, Rn   [n_utts][F][C][C] complex64  normalised covariances out of the fused
 *            STFT+covariance kernel and its reduction (libs/beamformer.py:87-103)
 *   weight   [n_utts][F][C]    complex64  beamformer weights (libs/beamformer.py
 *            weight() of the selected class, after BAN when requested)
 *   maxabs   [n_utts] float32  max |audio| (WaveReader.maxabs, the renorm target)
 * With 9 <= C <= 16 the taps are the C x C matrices and C weights as well (the padding of the
 * 16 x 16 embedding is not shown), Hermitian bit for bit. */
typedef struct setk_batch_taps {
    float* Rs;
    float* Rn;
    float* weight;
    float* maxabs;
} setk_batch_taps;
int setk_enhance_batch_taps(setk_handle_t h, const setk_bf_opts* opts, int n_utts,
                            int num_channels, const float* const* audio,
                            const int* num_samples, const float* const* mask_s,
                            const float* const* mask_n, void* const* wave,
                            int* status, const setk_batch_taps* taps, void* stream);

/* ---- block-online beamforming ----------------------------------------------
 * setk_online_num_chunks: ceil(T / chunk_size) for a signal of num_samples under the plan (T =
 * setk_stft_num_frames), i.e. the loop count of do_online_beamform
 * (apply_adaptive_beamformer.py:25-47); negative (SETK_ERR_*) without a plan or for
 * chunk_size < 1. */
int setk_online_num_chunks(setk_handle_t h, int num_samples, int chunk_size);

/* setk_enhance_online_batch: OnlineMvdrBeamformer / OnlineGevdBeamformer.run
 * (libs/beamformer.py:286-320, 685-724) under do_online_beamform
 * (apply_adaptive_beamformer.py:25-47), then post-mask, inverse_stft and renorm as
 * setk_enhance_batch, for a batch of utterances that share the channel count; the block-online
 * form of apply-supervised-mvdr.cc:198-217 (--update-periods).  Chunk c of an utterance covers the
 * frames [c S, min((c + 1) S, T)), S = chunk_size:
 *   rs_c, rn_c   compute_covar over the chunk's frames alone (masks mask_s, and mask_n or
 *                1 - mask_s; denominator max(sum of the chunk's mask, 1e-6))
 *   Rs_c = alpha Rs_{c-1} + phi_c rs_c, Rn_c likewise, Rs_{-1} = 0
 *   phi_0 = 1, phi_c = 1 - alpha for c > 0.  (The reference class never clears its `reset`
 *                member (:296-317), so its phi stays 1; this library follows the stated recursion.)
 *   w_c          the MVDR / GEV weight of (Rs_c, Rn_c) under the library's gauge; with
 *                SETK_FLAG_BAN scaled by do_ban(w_c, rn_c) -- the chunk's own UNSMOOTHED rn_c
 *   frame t      is beamformed with w_{t / S}
 * No state survives an utterance.  audio, num_samples, mask_s, mask_n, wave, status, stream: as
 * setk_enhance_batch; status[u] is the worst bin of the utterance's worst chunk.  Taps (every
 * member may be NULL; device or host memory), chunks utterance by utterance, chunks_total = sum of
 * setk_online_num_chunks:
 *   Rs, Rn   [chunks_total][F][C][C] complex64  the smoothed Rs_c, Rn_c
 *   weight   [chunks_total][F][C]    complex64  w_c (after BAN when requested)
 * Supported: kinds SETK_BF_MVDR and SETK_BF_GEVD; flags BAN, POST_MASK, CLAMP_MASK, IN_PCM16
 * (an even hop), OUT_PCM16, NO_RENORM, NO_GAUGE; 1 <= C <= 8; the n_fft = 512 plan -- anything
 * else is SETK_ERR_UNSUPPORTED.  SETK_ERR_INVALID: chunk_size < 1, alpha outside [0, 1), null
 * pointers.  Scratch (the slabs and planes of every chunk) comes from the handle's arena; the call
 * returns when the work has run.  With setk_set_profiling the stage times of setk_last_stage_ms
 * are out[0] STFT + chunk covariances, out[1] smoothing + weights + BAN, out[2] beamform + iSTFT,
 * out[3] renorm. */
typedef struct setk_online_opts {
    int chunk_size;
    float alpha;
} setk_online_opts;
typedef struct setk_online_taps {
    float* Rs;
    float* Rn;
    float* weight;
} setk_online_taps;
int setk_enhance_online_batch(setk_handle_t h, const setk_bf_opts* opts, const setk_online_opts* online,
                              int n_utts, int num_channels, const float* const* audio,
                              const int* num_samples, const float* const* mask_s,
                              const float* const* mask_n, void* const* wave, int* status,
                              const setk_online_taps* taps, void* stream);

/* ---- multi-GPU: the work-queue barrier on RCCL ------------------------------
 * The path shards by utterance with no data exchange (the reference: split_scp.pl + run.pl
 * JOB=1:nj, scripts/run_adapt_beamformer.sh:69-92).  One process per GPU needs a start / finish
 * barrier and the sums of its "Processed N utterances" counters: an all-reduce of a few
 * doubles over xGMI.  librccl is dlopen'ed on first use.  Rendezvous: rank 0 calls
 * setk_comm_unique_id, the caller carries the SETK_COMM_ID_BYTES to every rank (setk_amd/
 * dist.py: a TCP socket on MASTER_ADDR:MASTER_PORT), every rank calls setk_comm_create
 * (collective).  values: host array, reduced in place over all ranks (n <= 64).
 * SETK_ERR_UNSUPPORTED: librccl is not available (setk_comm_last_error has the reason). */
#define SETK_COMM_ID_BYTES 128
#define SETK_COMM_SUM 0
#define SETK_COMM_MAX 1
typedef struct setk_comm* setk_comm_t;
int setk_comm_unique_id(char out[SETK_COMM_ID_BYTES]);
int setk_comm_create(setk_comm_t* out, int device_ordinal, const char id[SETK_COMM_ID_BYTES],
                     int rank, int world);
int setk_comm_allreduce_f64(setk_comm_t c, double* values, int n, int op);
int setk_comm_barrier(setk_comm_t c);
int setk_comm_destroy(setk_comm_t c);
const char* setk_comm_last_error(void);

/* Stage timings (ms, hipEvent on `stream`) of the most recent
 * setk_enhance_batch when profiling was enabled with setk_set_profiling(h,1):
 * out[0] = the fused STFT+covariance kernel alone, out[1] = partial reduction +
 * weight solve, out[2] = beamform+iSTFT kernel, out[3] = renorm kernel.  */
int setk_set_profiling(setk_handle_t h, int enable);
int setk_last_stage_ms(setk_handle_t h, float out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SETK_HIP_H_ */
