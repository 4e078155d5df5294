// capi.h -- what the units of the extern "C" front end of libsetk_hip.so (capi_*.hip;
// include/setk_hip.h) share: the handle, error plumbing, the per-call device arena, staging of
// caller buffers, descriptor tables and the argument blocks of the fused kernels.  Host-side
// orchestration only; internal to the library (helpers are defined in capi_support.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/setk_hip.h"
#include "common.h"

namespace setk {
struct Block {
    char* ptr = nullptr;
    size_t cap = 0;
    size_t off = 0;
};
}  // namespace setk

struct setk_context {
    int device = 0;
    std::string err;
    // STFT plan
    bool planned = false;
    int frame_len = 0, hop = 0, n_fft = 0, center = 0;
    float* d_window = nullptr;  // [n_fft] padded analysis/synthesis window, scaled by 0.5
                                // (the rfft split / irfft merge omit their 1/2)
    float* d_winsq = nullptr;   // [n_fft]
    float2* d_tw256 = nullptr;  // [256]
    float2* d_tw512 = nullptr;  // [129]
    // matrix-core transforms of the fused path (n_fft = 512; mcdft.h)
    unsigned* d_mc_tab = nullptr;  // [mc::kTabWords][64] operand tiles (once per handle)
    float* d_window_pcm = nullptr; // d_window x 2^-15: pass 1 on 16-bit PCM (SETK_FLAG_IN_PCM16)
    float* d_mc_win = nullptr;     // [8][64] analysis window rows x mc_scale
    float* d_mc_syn = nullptr;     // [8][64] synthesis window rows / 512 / sum(window^2) (hop = n_fft / 2)
    float* d_mc_edge = nullptr;    // [8][64] corrections of the single-contribution blocks
    int mc_cus = 256;
    int mc_p2_items = 0;           // SETK_MC_P2_ITEMS: resident workgroup slots of pass2_mc (0: from the kernel)
    double mc_peak = 1.0;          // |audio| <= mc_peak (a power of two)
    bool mc_enabled = true;        // SETK_LEGACY_FFT=1: the fp32 butterfly kernels
    float2* d_twn = nullptr;    // [n_fft / 2] exp(-2 pi i k / n_fft), generic kernels
                                // (Bluestein plans: [M / 2] exp(-2 pi i k / M))
    // n_fft that is not a power of two: Bluestein tables (modular.hip)
    int blu_M = 0;
    float2* d_chirp = nullptr;  // [n_fft]
    float2* d_bhat = nullptr;   // [M], bit-reversed order
    // device arena (bump allocated per call, blocks reused across calls)
    std::vector<setk::Block> blocks;
    // descriptor cache of the fused path
    std::vector<char> desc_cache;
    char* d_desc = nullptr;
    size_t d_desc_cap = 0;
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;   // free events
    std::vector<hipEvent_t> ev_used;   // 5 per profiled call, in call order
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // stream of the most recent call (arena_reset)
    hipStream_t last_stream = nullptr;
    bool have_last_stream = false;
    // page-locked staging of the small host tables (h2d_small)
    char* pin_base = nullptr;
    size_t pin_head = 0;
    bool pin_failed = false;
    std::vector<hipEvent_t> pin_live;  // one per copy issued out of the buffer since the last lap
    std::vector<hipEvent_t> pin_free;
    // tunables
    int p1_items = 1024;
    int p2_items = 1024;
};

namespace setk {

int fail(setk_handle_t h, int code, const std::string& msg);

#define HIP_TRY(h, expr)                                                              \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess)                                                         \
            return fail(h, SETK_ERR_HIP,                                              \
                        std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

// a step that reports through the handle: leave with its code when it failed
#define SETK_TRY(expr)          \
    do {                        \
        const int rc_ = (expr); \
        if (rc_) return rc_;    \
    } while (0)

bool is_device_ptr(const void* p);

// ---- the per-call arena ----
// Every entry point starts by recycling the per-handle arena (and may rewrite
// the cached descriptor block).  Work of the previous call may still be in
// flight on ITS stream: calls on the same stream are ordered behind it, a call
// on a different stream first drains the previous one.
void arena_reset(setk_handle_t h, hipStream_t s);
// the prologue of an entry point: the caller's stream, the handle's device, a recycled arena
int begin_call(setk_handle_t h, void* stream, hipStream_t* s);
void* arena_alloc(setk_handle_t h, size_t bytes);  // null when the device is out of memory
int arena_bytes(setk_handle_t h, size_t bytes, void** out, const char* what);
// hand scratch back inside a call: everything allocated since the mark (in-order stream; see
// capi_support.hip)
std::vector<size_t> arena_mark(setk_handle_t h);
void arena_rewind(setk_handle_t h, const std::vector<size_t>& mark);

// `bytes` of arena as a T*, or SETK_ERR_NOMEM
template <typename T>
int arena_get(setk_handle_t h, size_t bytes, T** out, const char* what = "arena") {
    void* p = nullptr;
    const int rc = arena_bytes(h, bytes, &p, what);
    *out = static_cast<T*>(p);
    return rc;
}

// ---- caller buffers ----
constexpr const char* kStagingNomem = "device arena allocation failed";

// Stage an input: device pointers pass through, host data is copied.
template <typename T>
int stage_in(setk_handle_t h, const T* src, size_t count, hipStream_t s, const T** out) {
    if (is_device_ptr(src)) {
        *out = src;
        return SETK_OK;
    }
    T* d;
    SETK_TRY(arena_get(h, count * sizeof(T), &d, kStagingNomem));
    HIP_TRY(h, hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    *out = d;
    return SETK_OK;
}

// Prepare an output: device pointers are written in place, host outputs get a
// device twin that copy_back() drains.
struct OutBuf {
    void* user = nullptr;
    void* dev = nullptr;
    size_t bytes = 0;
    bool host = false;
};
int stage_out(setk_handle_t h, void* dst, size_t bytes, OutBuf* ob);
int copy_back(setk_handle_t h, const OutBuf& ob, hipStream_t s);
// the end of a call with one output: copy_back, and wait for it when it went to host memory
int finish_out(setk_handle_t h, const OutBuf& ob, hipStream_t s);
// `n` bytes of device data to a caller pointer that may be host or device memory; a copy to
// host memory sets *sync_owed (the caller reads it once the stream has drained; null when the
// call drains anyway)
int copy_out(setk_handle_t h, void* dst, const void* d_src, size_t n, hipStream_t s, bool* sync_owed);
// `n` bytes the host has computed to such a pointer, at once
int put_result(setk_handle_t h, void* dst, const void* src, size_t n);

// Small host tables (descriptors, pointer lists, argument blocks) go to the device through a
// page-locked buffer of the handle; see capi_support.hip.
hipError_t h2d_small(setk_handle_t h, void* dst, const void* src, size_t bytes, hipStream_t s);
// Descriptor tables are built in ordinary host vectors that die when the entry point
// returns: h2d_small copies them into the handle's page-locked buffer first (or, for a large
// table, lets the runtime stage the pageable source before hipMemcpyAsync returns), so the
// source may be released either way.
int upload_bytes(setk_handle_t h, const void* src, size_t bytes, hipStream_t s, void** out);

template <typename T>
int upload(setk_handle_t h, const T* src, size_t count, hipStream_t s, const T** out) {
    void* d = nullptr;
    const int rc = upload_bytes(h, src, count * sizeof(T), s, &d);
    *out = static_cast<const T*>(d);
    return rc;
}
template <typename T>
int upload(setk_handle_t h, const std::vector<T>& v, hipStream_t s, const T** out) {
    return upload(h, v.data(), v.size(), s, out);
}

// ---- the n_fft = 512 plan, descriptors and work lists ----
StftGeom geom_of(setk_handle_t h);
int require_plan512(setk_handle_t h);

// Frames per work item such that the work list fills whole "waves" of resident
// workgroups: among the splits of the longest utterance into 1..32 ranges pick
// the one minimising  ceil(items / slots) * frames_per_item  (makespan in
// frames); utterances shorter than the target become single items.
int choose_target(const std::vector<int>& frames, int slots, int quant, int min_frames);

// UttDesc and WorkItem go to the device (and into desc_cache, which compares bytes): both are
// zeroed with memset, padding included, before their fields are set.
std::vector<UttDesc> zeroed_utts(int n);
// [0, T) of utterance `utt` in ranges of about `target` frames, multiples of `quant`, appended
// to `items`; *next_part numbers them (pass 1's partial slabs).  Returns how many.
int push_items(std::vector<WorkItem>* items, int utt, int T, int target, int quant,
               int* next_part = nullptr);

struct DescTables {
    const UttDesc* utts = nullptr;
    const WorkItem* items = nullptr;
    int n_items = 0;
};
int upload_tables(setk_handle_t h, const std::vector<UttDesc>& uds, const std::vector<WorkItem>& items,
                  hipStream_t s, DescTables* out);

// argument blocks over the handle's tables (every other field zero)
Pass1Args pass1_args(setk_handle_t h, const UttDesc* utts, const WorkItem* items);
Pass2Args pass2_args(setk_handle_t h, const UttDesc* utts, const WorkItem* items, unsigned* outmax_bits);
ScaleArgs scale_args(const UttDesc* utts, const unsigned* norm_bits, const unsigned* outmax_bits, bool pcm16);

// The STFT of whole utterances into bin-major arrays xb[u] ([F][C][Tp] complex64, device), in
// 64-frame items: uploads the tables and hands back what launch_stft_binmajor takes.  (The
// caller launches: setk_auxiva_batch clears its norm words between the two.)
int prepare_stft_binmajor(setk_handle_t h, int n_utts, const float* const* audio, const int* num_samples,
                          const int* frames, float* const* xb, hipStream_t s, Pass1Args* a, int* n_items);

// UttDesc::wave_f32 of every utterance: the caller's buffer, or (16-bit output) its 256-byte
// aligned share of one float32 scratch block
int carve_wave_f32(setk_handle_t h, std::vector<UttDesc>& uds, void* const* wave, bool pcm16);

// The option checks setk_weights and setk_enhance_batch_taps share, in the order both report
// them: the kind's range, the caller's own operand check (`own`: its message, null when it
// passed; `own_code`), MPDR + BAN, PMWF's reference channel against C.
int check_bf_opts(setk_handle_t h, const setk_bf_opts& o, int C, int own_code, const char* own);

// setk_pevd (Rn NULL) inside another entry point: operands and results are device memory of the
// running call, whose arena is kept (capi_modular.hip)
int pevd_in_arena(setk_handle_t h, const float* d_Rs, int F, int C, float* d_pvec, int* d_status,
                  hipStream_t s);

// ---- stage events of a profiled call (setk_set_profiling / setk_last_stage_ms) ----
int profile_begin(setk_handle_t h, hipStream_t s);          // five events, the first recorded
int profile_mark(setk_handle_t h, int i, hipStream_t s);    // record event i (1..4)

}  // namespace setk
