// capi_handle.hip -- front end (include/setk_hip.h): the handle, device and host memory,
// streams and events for a host pipeline that brings no runtime of its own, and the STFT plan.
#include <cmath>

#include "capi.h"
#include "mcdft_tables.h"

using namespace setk;

namespace {

constexpr double kPi = 3.14159265358979323846;

// ---- the tables of a plan: pure host functions ----

// exp(-2 pi i k / n), k < count
std::vector<float2> unit_roots(int n, int count) {
    std::vector<float2> t(count);
    for (int k = 0; k < count; ++k) {
        const double ang = -2.0 * kPi * (double)k / (double)n;
        t[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    return t;
}

// [16][16] exp(-2 pi i la q / 256) at [q * 16 + la]
std::vector<float2> twiddles256() {
    std::vector<float2> t(256);
    for (int q = 0; q < 16; ++q)
        for (int la = 0; la < 16; ++la) {
            const double ang = -2.0 * kPi * (double)(la * q) / 256.0;
            t[q * 16 + la] = make_float2((float)std::cos(ang), (float)std::sin(ang));
        }
    return t;
}

// the window padded to n_fft and scaled by 0.5 (`w`), and its square unscaled (`w2`);
// window == null: periodic Hann
void plan_windows(int frame_len, int n_fft, const float* window, std::vector<float>* w,
                  std::vector<float>* w2) {
    w->assign(n_fft, 0.f);
    w2->assign(n_fft, 0.f);
    const int lpad = (n_fft - frame_len) / 2;
    for (int i = 0; i < frame_len; ++i) {
        double v = window ? (double)window[i] : 0.5 - 0.5 * std::cos(2.0 * kPi * i / frame_len);
        (*w)[lpad + i] = 0.5f * (float)v;
        (*w2)[lpad + i] = (float)(v * v);
    }
}

int bit_reverse(int i, int bits) {
    int r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

// Bluestein: chirp c[k] = exp(-i pi k^2 / n) (k^2 reduced mod 2n in integers), and the
// length-M spectrum of the wrapped conj(c), in bit-reversed order.  Returns M.
int bluestein_tables(int n_fft, std::vector<float2>* chirp, std::vector<float2>* bhat) {
    int M = 1;
    while (M < 2 * n_fft - 1) M <<= 1;
    int logM = 0;
    while ((1 << logM) < M) ++logM;
    std::vector<double> cr(n_fft), ci(n_fft);
    for (int k = 0; k < n_fft; ++k) {
        const long k2 = ((long)k * k) % (2L * n_fft);
        const double ang = -kPi * (double)k2 / (double)n_fft;
        cr[k] = std::cos(ang);
        ci[k] = std::sin(ang);
    }
    std::vector<double> br(M, 0.0), bi(M, 0.0);
    for (int k = 0; k < n_fft; ++k) {
        br[k] = cr[k];
        bi[k] = -ci[k];
        if (k) {
            br[M - k] = cr[k];
            bi[M - k] = -ci[k];
        }
    }
    // iterative radix-2 DIT in double (bit reversal first)
    for (int i = 0; i < M; ++i) {
        const int r = bit_reverse(i, logM);
        if (r > i) {
            std::swap(br[i], br[r]);
            std::swap(bi[i], bi[r]);
        }
    }
    for (int len = 2; len <= M; len <<= 1) {
        const double a0 = -2.0 * kPi / (double)len;
        for (int i0 = 0; i0 < M; i0 += len)
            for (int k = 0; k < len / 2; ++k) {
                const double wr = std::cos(a0 * k), wi = std::sin(a0 * k);
                const int a = i0 + k, b = a + len / 2;
                const double tr = br[b] * wr - bi[b] * wi, ti = br[b] * wi + bi[b] * wr;
                br[b] = br[a] - tr;
                bi[b] = bi[a] - ti;
                br[a] += tr;
                bi[a] += ti;
            }
    }
    chirp->resize(n_fft);
    bhat->resize(M);
    for (int k = 0; k < n_fft; ++k) (*chirp)[k] = make_float2((float)cr[k], (float)ci[k]);
    for (int i = 0; i < M; ++i) (*bhat)[bit_reverse(i, logM)] = make_float2((float)br[i], (float)bi[i]);
    return M;
}

// matrix-core DFT-512: the window rows of a plan.  `w` holds 0.5 x window, `w2` window^2.
struct McRows {
    std::vector<float> win, syn, edge;
};
McRows mc_rows(const std::vector<float>& w, const std::vector<float>& w2, double peak) {
    const int n_fft = (int)w.size();
    std::vector<float> wt(n_fft);
    for (int i = 0; i < n_fft; ++i) wt[i] = 2.f * w[i];  // w holds 0.5 x window (exact)
    McRows r;
    r.win = mc::build_window_rows(wt.data(), 1024.0 / peak);
    // pass2_mc (hop = n_fft / 2): a block of hop samples is first half of frame t + second
    // half of frame t - 1, both over the same sum(window^2) -- folded into the rows
    // (librosa.istft: divided only where it exceeds tiny); blocks with one contribution
    // (first / last of an utterance, center = False) take the ratio as a correction
    const double tiny = 1.17549435e-38;
    std::vector<float> syn(n_fft), edge(n_fft);
    for (int m = 0; m < n_fft / 2; ++m) {
        const double a2 = (double)w2[m], b2 = (double)w2[m + n_fft / 2];
        const double mid = (a2 + b2 > tiny) ? a2 + b2 : 1.0;
        syn[m] = (float)((double)wt[m] * peak / 1024.0 / 512.0 / mid);
        syn[m + n_fft / 2] = (float)((double)wt[m + n_fft / 2] * peak / 1024.0 / 512.0 / mid);
        edge[m] = (float)(mid / (a2 > tiny ? a2 : 1.0));
        edge[m + n_fft / 2] = (float)(mid / (b2 > tiny ? b2 : 1.0));
    }
    r.syn = mc::build_synth_rows(syn.data(), 1.0);
    r.edge = mc::build_synth_rows(edge.data(), 1.0);
    return r;
}

// ---- device tables of the handle ----
// (three steps, not one "replace": a plan frees, allocates and fills its tables in groups, and
// the order of those runtime calls is kept)
template <typename T>
void table_free(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
template <typename T>
int table_alloc(setk_handle_t h, T*& p, size_t n) {
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)));
    return SETK_OK;
}
template <typename T, typename V>
int table_fill(setk_handle_t h, T* p, const std::vector<V>& v) {
    static_assert(sizeof(T) == sizeof(V), "table element size");
    HIP_TRY(h, hipMemcpy(p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice));
    return SETK_OK;
}

}  // namespace

extern "C" {

int setk_abi_version(void) { return SETK_ABI_VERSION; }

int setk_create(setk_handle_t* out, int device_ordinal) {
    if (!out) return SETK_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return SETK_ERR_HIP;
    }
    if (device_ordinal < 0 || device_ordinal >= n) return SETK_ERR_INVALID;
    if (hipSetDevice(device_ordinal) != hipSuccess) return SETK_ERR_HIP;
    setk_context* h = new setk_context();
    h->device = device_ordinal;
    // resident workgroup slots: pass 1 runs 1 workgroup per CU, pass 2 two; the
    // work lists are cut to fill whole waves of those slots (choose_target)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) {
        h->p1_items = prop.multiProcessorCount;
        h->p2_items = 2 * prop.multiProcessorCount;
        h->mc_cus = prop.multiProcessorCount;
    }
    if (const char* e = getenv("SETK_MC_P2_ITEMS")) h->mc_p2_items = std::max(1, atoi(e));
    if (const char* e = getenv("SETK_P1_ITEMS")) h->p1_items = std::max(1, atoi(e));
    if (const char* e = getenv("SETK_P2_ITEMS")) h->p2_items = std::max(1, atoi(e));
    *out = h;
    return SETK_OK;
}

int setk_destroy(setk_handle_t h) {
    if (!h) return SETK_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (auto& b : h->blocks) (void)hipFree(b.ptr);
    table_free(h->d_window);
    table_free(h->d_winsq);
    table_free(h->d_tw256);
    table_free(h->d_tw512);
    table_free(h->d_mc_tab);
    table_free(h->d_mc_win);
    table_free(h->d_window_pcm);
    table_free(h->d_mc_syn);
    table_free(h->d_mc_edge);
    table_free(h->d_twn);
    table_free(h->d_chirp);
    table_free(h->d_bhat);
    table_free(h->d_desc);
    for (auto& e : h->ev_pool) (void)hipEventDestroy(e);
    for (auto& e : h->ev_used) (void)hipEventDestroy(e);
    for (auto& e : h->pin_live) {
        (void)hipEventSynchronize(e);
        (void)hipEventDestroy(e);
    }
    for (auto& e : h->pin_free) (void)hipEventDestroy(e);
    if (h->pin_base) (void)hipHostFree(h->pin_base);
    delete h;
    return SETK_OK;
}

const char* setk_last_error(setk_handle_t h) { return h ? h->err.c_str() : "null handle"; }

int setk_device_pci_bus_id(setk_handle_t h, char* out, int len) {
    if (!h || !out || len < 13) return SETK_ERR_INVALID;
    HIP_TRY(h, hipDeviceGetPCIBusId(out, len, h->device));
    return SETK_OK;
}

int setk_set_profiling(setk_handle_t h, int enable) {
    if (!h) return SETK_ERR_INVALID;
    h->profiling = enable != 0;
    return SETK_OK;
}

// mean stage times (ms) over the profiled setk_enhance_batch calls since the
// last query; the recorded events are recycled.
int setk_last_stage_ms(setk_handle_t h, float out[4]) {
    if (!h || !out) return SETK_ERR_INVALID;
    const size_t calls = h->ev_used.size() / 5;
    if (calls == 0) return fail(h, SETK_ERR_INVALID, "no profiled run available");
    double acc[4] = {0, 0, 0, 0};
    for (size_t c = 0; c < calls; ++c) {
        hipEvent_t* e = &h->ev_used[c * 5];
        HIP_TRY(h, hipEventSynchronize(e[4]));
        for (int i = 0; i < 4; ++i) {
            float ms = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&ms, e[i], e[i + 1]));
            acc[i] += ms;
        }
    }
    for (int i = 0; i < 4; ++i) out[i] = (float)(acc[i] / (double)calls);
    for (auto& e : h->ev_used) h->ev_pool.push_back(e);
    h->ev_used.clear();
    return SETK_OK;
}

// ---- host-memory plumbing of the streaming pipeline (setk_amd/pipeline.py) ----
// A wave or mask file that sits in the page cache can be DMA'd from where it is:
// mmap it, pin the mapping, copy from it.  Measured (profiles/r02j_*): pinning a
// 7.7 MB mapping costs 0.23 ms and the copy then runs at 52 GB/s, against 0.9 ms
// for reading the same bytes into a staging buffer first.
int setk_host_register(setk_handle_t h, void* ptr, size_t bytes) {
    if (!h || !ptr || !bytes) return SETK_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, SETK_ERR_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e));
    }
    return SETK_OK;
}

int setk_host_unregister(setk_handle_t h, void* ptr) {
    if (!h || !ptr) return SETK_ERR_INVALID;
    hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, SETK_ERR_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e));
    }
    return SETK_OK;
}

int setk_memcpy_h2d_async(setk_handle_t h, void* dst, const void* src, size_t bytes, void* stream) {
    if (!h || !dst || !src) return SETK_ERR_INVALID;
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice,
                              static_cast<hipStream_t>(stream)));
    return SETK_OK;
}

int setk_memcpy_d2h_async(setk_handle_t h, void* dst, const void* src, size_t bytes, void* stream) {
    if (!h || !dst || !src) return SETK_ERR_INVALID;
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost,
                              static_cast<hipStream_t>(stream)));
    return SETK_OK;
}

// ---- buffers, streams and events for a host pipeline that brings no runtime of its own ----
int setk_device_alloc(setk_handle_t h, size_t bytes, void** out) {
    if (!h || !out || !bytes) return SETK_ERR_INVALID;
    *out = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    if (hipMalloc(out, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, SETK_ERR_NOMEM, "hipMalloc");
    }
    return SETK_OK;
}

int setk_device_free(setk_handle_t h, void* ptr) {
    if (!h) return SETK_ERR_INVALID;
    if (ptr) HIP_TRY(h, hipFree(ptr));
    return SETK_OK;
}

int setk_host_alloc(setk_handle_t h, size_t bytes, void** out) {
    if (!h || !out || !bytes) return SETK_ERR_INVALID;
    *out = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, SETK_ERR_NOMEM, "hipHostMalloc");
    }
    return SETK_OK;
}

int setk_host_free(setk_handle_t h, void* ptr) {
    if (!h) return SETK_ERR_INVALID;
    if (ptr) HIP_TRY(h, hipHostFree(ptr));
    return SETK_OK;
}

int setk_stream_create(setk_handle_t h, void** out) {
    if (!h || !out) return SETK_ERR_INVALID;
    hipStream_t s = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return SETK_OK;
}

int setk_stream_destroy(setk_handle_t h, void* stream) {
    if (!h) return SETK_ERR_INVALID;
    // The arena remembers the stream of the handle's last call and drains it when the next call
    // comes on another one (arena_reset).  A destroyed stream must not stay remembered: the next
    // call would synchronise a dangling hipStream_t.  Drain it here instead.
    hipError_t drained = hipSuccess;
    if (stream && h->have_last_stream && h->last_stream == static_cast<hipStream_t>(stream)) {
        drained = hipStreamSynchronize(h->last_stream);
        h->have_last_stream = false;
        h->last_stream = nullptr;
    }
    // (destroyed whatever the drain said: an error there must not leak the stream)
    if (stream) HIP_TRY(h, hipStreamDestroy(static_cast<hipStream_t>(stream)));
    HIP_TRY(h, drained);
    return SETK_OK;
}

int setk_stream_synchronize(setk_handle_t h, void* stream) {
    if (!h) return SETK_ERR_INVALID;
    HIP_TRY(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return SETK_OK;
}

int setk_stream_wait_event(setk_handle_t h, void* stream, void* event) {
    if (!h || !event) return SETK_ERR_INVALID;
    HIP_TRY(h, hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(event), 0));
    return SETK_OK;
}

int setk_event_create(setk_handle_t h, void** out) {
    if (!h || !out) return SETK_ERR_INVALID;
    hipEvent_t e = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *out = e;
    return SETK_OK;
}

int setk_event_destroy(setk_handle_t h, void* event) {
    if (!h) return SETK_ERR_INVALID;
    if (event) HIP_TRY(h, hipEventDestroy(static_cast<hipEvent_t>(event)));
    return SETK_OK;
}

int setk_event_record(setk_handle_t h, void* event, void* stream) {
    if (!h || !event) return SETK_ERR_INVALID;
    HIP_TRY(h, hipEventRecord(static_cast<hipEvent_t>(event), static_cast<hipStream_t>(stream)));
    return SETK_OK;
}

int setk_event_synchronize(setk_handle_t h, void* event) {
    if (!h || !event) return SETK_ERR_INVALID;
    HIP_TRY(h, hipEventSynchronize(static_cast<hipEvent_t>(event)));
    return SETK_OK;
}

int setk_stft_plan(setk_handle_t h, int frame_len, int frame_hop, int n_fft, int center,
                   const float* window) {
    if (!h) return SETK_ERR_INVALID;
    const bool pow2 = (n_fft & (n_fft - 1)) == 0;
    if (frame_len <= 0 || frame_hop <= 0 || n_fft < 16 || n_fft > 4096 || (n_fft & 1) ||
        (pow2 && n_fft < 64))
        return fail(h, SETK_ERR_INVALID,
                    "n_fft must be even, in [16, 4096] (powers of two: [64, 4096])");
    if (frame_len > n_fft) return fail(h, SETK_ERR_INVALID, "frame_len > n_fft");
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<float> w, w2;
    plan_windows(frame_len, n_fft, window, &w, &w2);
    HIP_TRY(h, hipDeviceSynchronize());
    table_free(h->d_window);
    table_free(h->d_winsq);
    SETK_TRY(table_alloc(h, h->d_window, n_fft));
    SETK_TRY(table_alloc(h, h->d_winsq, n_fft));
    if (!h->d_tw256) SETK_TRY(table_alloc(h, h->d_tw256, 256));
    if (!h->d_tw512) SETK_TRY(table_alloc(h, h->d_tw512, 129));
    SETK_TRY(table_fill(h, h->d_window, w));
    {
        // the same window with read_wav's 1 / 32768 folded in (exact: a power of two)
        std::vector<float> wp(n_fft);
        for (int i = 0; i < n_fft; ++i) wp[i] = w[i] * 3.0517578125e-05f;
        table_free(h->d_window_pcm);
        SETK_TRY(table_alloc(h, h->d_window_pcm, n_fft));
        SETK_TRY(table_fill(h, h->d_window_pcm, wp));
    }
    SETK_TRY(table_fill(h, h->d_winsq, w2));
    SETK_TRY(table_fill(h, h->d_tw256, twiddles256()));
    SETK_TRY(table_fill(h, h->d_tw512, unit_roots(512, 129)));
    h->blu_M = 0;
    table_free(h->d_chirp);
    table_free(h->d_bhat);
    int tw_n = n_fft;
    if (!pow2) {
        std::vector<float2> chirp, bhat;
        const int M = bluestein_tables(n_fft, &chirp, &bhat);
        SETK_TRY(table_alloc(h, h->d_chirp, n_fft));
        SETK_TRY(table_alloc(h, h->d_bhat, M));
        SETK_TRY(table_fill(h, h->d_chirp, chirp));
        SETK_TRY(table_fill(h, h->d_bhat, bhat));
        h->blu_M = M;
        tw_n = M;
    }
    table_free(h->d_twn);
    SETK_TRY(table_alloc(h, h->d_twn, tw_n / 2));
    SETK_TRY(table_fill(h, h->d_twn, unit_roots(tw_n, tw_n / 2)));
    if (n_fft == kNfft) {
        // matrix-core DFT-512: operand tiles once per handle, window rows per plan
        if (!h->d_mc_tab) {
            const std::vector<uint32_t> tab = mc::build_table();
            SETK_TRY(table_alloc(h, h->d_mc_tab, tab.size()));
            SETK_TRY(table_fill(h, h->d_mc_tab, tab));
        }
        if (!h->d_mc_win) SETK_TRY(table_alloc(h, h->d_mc_win, 8 * 64));
        if (!h->d_mc_syn) SETK_TRY(table_alloc(h, h->d_mc_syn, 8 * 64));
        if (!h->d_mc_edge) SETK_TRY(table_alloc(h, h->d_mc_edge, 8 * 64));
        const McRows rows = mc_rows(w, w2, h->mc_peak);
        SETK_TRY(table_fill(h, h->d_mc_win, rows.win));
        SETK_TRY(table_fill(h, h->d_mc_syn, rows.syn));
        SETK_TRY(table_fill(h, h->d_mc_edge, rows.edge));
        h->mc_enabled = !(getenv("SETK_LEGACY_FFT") && atoi(getenv("SETK_LEGACY_FFT")) != 0);
    }
    h->frame_len = frame_len;
    h->hop = frame_hop;
    h->n_fft = n_fft;
    h->center = center ? 1 : 0;
    h->planned = true;
    h->desc_cache.clear();
    return SETK_OK;
}

int setk_stft_num_frames(setk_handle_t h, int num_samples) {
    if (!h || !h->planned) return SETK_ERR_INVALID;
    if (h->center) {
        if (num_samples < h->n_fft / 2 + 1)
            return fail(h, SETK_ERR_INVALID, "signal shorter than n_fft/2+1 (reflect padding)");
        return 1 + num_samples / h->hop;
    }
    if (num_samples < h->n_fft) return fail(h, SETK_ERR_INVALID, "signal shorter than n_fft");
    return 1 + (num_samples - h->n_fft) / h->hop;
}

int setk_istft_num_samples(setk_handle_t h, int num_frames, int nsamps) {
    if (!h || !h->planned || num_frames <= 0) return SETK_ERR_INVALID;
    if (nsamps >= 0) return nsamps;
    return h->center ? h->hop * (num_frames - 1) : h->n_fft + h->hop * (num_frames - 1);
}

}  // extern "C"
