// capi_support.hip -- the helpers of capi.h: error plumbing, the per-call arena, staging of
// caller buffers, descriptor tables, argument blocks and profiling events.  No entry point
// and no kernel.
#include "capi.h"

namespace setk {

int fail(setk_handle_t h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

void arena_reset(setk_handle_t h, hipStream_t s) {
    if (h->have_last_stream && h->last_stream != s) (void)hipStreamSynchronize(h->last_stream);
    h->last_stream = s;
    h->have_last_stream = true;
    for (auto& b : h->blocks) b.off = 0;
}

int begin_call(setk_handle_t h, void* stream, hipStream_t* s) {
    *s = static_cast<hipStream_t>(stream);
    HIP_TRY(h, hipSetDevice(h->device));
    arena_reset(h, *s);
    return SETK_OK;
}

void* arena_alloc(setk_handle_t h, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    for (auto& b : h->blocks) {
        if (b.cap - b.off >= bytes) {
            void* p = b.ptr + b.off;
            b.off += bytes;
            return p;
        }
    }
    size_t cap = std::max(bytes, (size_t)64 << 20);
    if (!h->blocks.empty()) cap = std::max(cap, h->blocks.back().cap);
    Block nb;
    if (hipMalloc(reinterpret_cast<void**>(&nb.ptr), cap) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    nb.cap = cap;
    nb.off = bytes;
    h->blocks.push_back(nb);
    return nb.ptr;
}

// Scratch handed back INSIDE a call (a host loop whose steps need the same scratch): the bump
// offsets are restored, blocks that came later are emptied, nothing is freed.  Safe because a
// call's launches and copies run in order on its one stream: what reuses the bytes is queued
// behind what last read them.  Whatever the caller allocated since the mark is gone with it.
std::vector<size_t> arena_mark(setk_handle_t h) {
    std::vector<size_t> m;
    for (auto& b : h->blocks) m.push_back(b.off);
    return m;
}
void arena_rewind(setk_handle_t h, const std::vector<size_t>& m) {
    for (size_t i = 0; i < h->blocks.size(); ++i) h->blocks[i].off = i < m.size() ? m[i] : 0;
}

int arena_bytes(setk_handle_t h, size_t bytes, void** out, const char* what) {
    *out = arena_alloc(h, bytes);
    return *out ? SETK_OK : fail(h, SETK_ERR_NOMEM, what);
}

// Small host tables (descriptors, pointer lists, argument blocks) go to the device through a
// page-locked buffer of the handle.  hipMemcpyAsync from PAGEABLE memory does not return
// before the copy has run, i.e. before everything queued on the stream ahead of it has -- in
// the streaming pipeline that is the 300 MB slab transfer the compute stream is waiting for,
// ~6 ms per batch during which the launching thread could not queue the next batch.  From the
// page-locked buffer the copy is queued and the call returns.  The buffer is used linearly;
// when it is full, every copy issued out of it is waited for (an event each) and it starts
// over.  Tables larger than a quarter of it, or a failed allocation, take the pageable path.
static size_t pin_cap() {
    // 8 MB; SETK_PIN_CAP_KB shrinks it so that tests see the buffer wrap
    static const size_t cap = [] {
        const char* e = getenv("SETK_PIN_CAP_KB");
        const long kb = e ? atol(e) : 0;
        return kb >= 4 ? (size_t)kb << 10 : (size_t)8 << 20;
    }();
    return cap;
}

hipError_t h2d_small(setk_handle_t h, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (!bytes) return hipSuccess;
    const size_t kPinCap = pin_cap();
    if (bytes > kPinCap / 4 || h->pin_failed)
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    if (!h->pin_base) {
        void* p = nullptr;
        if (hipHostMalloc(&p, kPinCap, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            h->pin_failed = true;
            return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
        }
        h->pin_base = static_cast<char*>(p);
    }
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (h->pin_head + need > kPinCap || h->pin_live.size() >= 4096) {
        for (hipEvent_t e : h->pin_live) {
            (void)hipEventSynchronize(e);
            h->pin_free.push_back(e);
        }
        h->pin_live.clear();
        h->pin_head = 0;
    }
    char* p = h->pin_base + h->pin_head;
    h->pin_head += need;
    memcpy(p, src, bytes);
    hipError_t e = hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    hipEvent_t ev = nullptr;
    if (!h->pin_free.empty()) {
        ev = h->pin_free.back();
        h->pin_free.pop_back();
    } else {
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    e = hipEventRecord(ev, s);
    h->pin_live.push_back(ev);
    return e;
}

int upload_bytes(setk_handle_t h, const void* src, size_t bytes, hipStream_t s, void** out) {
    void* d;
    SETK_TRY(arena_bytes(h, bytes, &d, kStagingNomem));
    HIP_TRY(h, h2d_small(h, d, src, bytes, s));
    *out = d;
    return SETK_OK;
}

int stage_out(setk_handle_t h, void* dst, size_t bytes, OutBuf* ob) {
    ob->user = dst;
    ob->bytes = bytes;
    ob->host = !is_device_ptr(dst);
    if (!ob->host) {
        ob->dev = dst;
        return SETK_OK;
    }
    return arena_bytes(h, bytes, &ob->dev, kStagingNomem);
}

int copy_back(setk_handle_t h, const OutBuf& ob, hipStream_t s) {
    if (ob.host && ob.bytes)
        HIP_TRY(h, hipMemcpyAsync(ob.user, ob.dev, ob.bytes, hipMemcpyDeviceToHost, s));
    return SETK_OK;
}

int finish_out(setk_handle_t h, const OutBuf& ob, hipStream_t s) {
    SETK_TRY(copy_back(h, ob, s));
    if (ob.host) HIP_TRY(h, hipStreamSynchronize(s));
    return SETK_OK;
}

int copy_out(setk_handle_t h, void* dst, const void* d_src, size_t n, hipStream_t s, bool* sync_owed) {
    const bool dev = is_device_ptr(dst);
    HIP_TRY(h, hipMemcpyAsync(dst, d_src, n, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!dev && sync_owed) *sync_owed = true;
    return SETK_OK;
}

int put_result(setk_handle_t h, void* dst, const void* src, size_t n) {
    if (is_device_ptr(dst))
        HIP_TRY(h, hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
    else
        memcpy(dst, src, n);
    return SETK_OK;
}

StftGeom geom_of(setk_handle_t h) {
    StftGeom g;
    g.hop = h->hop;
    g.center = h->center;
    g.pad = h->center ? h->n_fft / 2 : 0;
    g.keep = (h->n_fft + h->hop - 1) / h->hop - 1;
    return g;
}

int require_plan512(setk_handle_t h) {
    if (!h->planned) return fail(h, SETK_ERR_INVALID, "setk_stft_plan has not been called");
    if (h->n_fft != kNfft)
        return fail(h, SETK_ERR_UNSUPPORTED,
                    "only the n_fft = 512 kernels are built (n_fft = " + std::to_string(h->n_fft) +
                        ")");
    if (h->hop > h->n_fft) return fail(h, SETK_ERR_UNSUPPORTED, "frame_hop > n_fft");
    if (geom_of(h).keep > kMaxKeep)
        return fail(h, SETK_ERR_UNSUPPORTED, "frame_hop < 64 is not supported");
    return SETK_OK;
}

int choose_target(const std::vector<int>& frames, int slots, int quant, int min_frames) {
    int tmax = 1;
    for (int t : frames) tmax = std::max(tmax, t);
    long best_cost = -1;
    int best = tmax;
    for (int parts = 1; parts <= 32; ++parts) {
        int target = (tmax + parts - 1) / parts;
        target = ((target + quant - 1) / quant) * quant;
        if (target < min_frames && parts > 1) break;
        long items = 0;
        for (int t : frames) items += (t + target - 1) / target;
        const long waves = (items + slots - 1) / slots;
        const long cost = waves * (long)target + 8 * waves;  // + per-wave fixed cost
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = target;
        }
    }
    return best;
}

std::vector<UttDesc> zeroed_utts(int n) {
    std::vector<UttDesc> uds(n);
    memset(uds.data(), 0, uds.size() * sizeof(UttDesc));
    return uds;
}

int push_items(std::vector<WorkItem>* items, int utt, int T, int target, int quant, int* next_part) {
    const int nparts = std::max(1, (T + target - 1) / target);
    int fw = (T + nparts - 1) / nparts;
    fw = ((fw + quant - 1) / quant) * quant;
    int n = 0;
    for (int t = 0; t < T; t += fw, ++n) {
        WorkItem w;
        memset(&w, 0, sizeof(w));
        w.utt = utt;
        w.t0 = t;
        w.t1 = std::min(T, t + fw);
        w.part = next_part ? (*next_part)++ : 0;
        w.last = w.t1 == T;
        items->push_back(w);
    }
    return n;
}

int upload_tables(setk_handle_t h, const std::vector<UttDesc>& uds, const std::vector<WorkItem>& items,
                  hipStream_t s, DescTables* out) {
    SETK_TRY(upload(h, uds, s, &out->utts));
    SETK_TRY(upload(h, items, s, &out->items));
    out->n_items = (int)items.size();
    return SETK_OK;
}

Pass1Args pass1_args(setk_handle_t h, const UttDesc* utts, const WorkItem* items) {
    Pass1Args a;
    memset(&a, 0, sizeof(a));
    a.utts = utts;
    a.items = items;
    a.window = h->d_window;
    a.tw256 = h->d_tw256;
    a.tw512 = h->d_tw512;
    a.g = geom_of(h);
    return a;
}

Pass2Args pass2_args(setk_handle_t h, const UttDesc* utts, const WorkItem* items, unsigned* outmax_bits) {
    Pass2Args a;
    memset(&a, 0, sizeof(a));
    a.utts = utts;
    a.items = items;
    a.window = h->d_window;
    a.synwin = h->d_window;
    a.winsq = h->d_winsq;
    a.tw256 = h->d_tw256;
    a.tw512 = h->d_tw512;
    a.outmax_bits = outmax_bits;
    a.g = geom_of(h);
    return a;
}

ScaleArgs scale_args(const UttDesc* utts, const unsigned* norm_bits, const unsigned* outmax_bits, bool pcm16) {
    ScaleArgs a;
    memset(&a, 0, sizeof(a));
    a.utts = utts;
    a.norm_bits = norm_bits;
    a.outmax_bits = outmax_bits;
    a.pcm16 = pcm16 ? 1 : 0;
    return a;
}

int prepare_stft_binmajor(setk_handle_t h, int n_utts, const float* const* audio, const int* num_samples,
                          const int* frames, float* const* xb, hipStream_t s, Pass1Args* a, int* n_items) {
    std::vector<UttDesc> uds = zeroed_utts(n_utts);
    std::vector<WorkItem> items;
    for (int u = 0; u < n_utts; ++u) {
        uds[u].audio = audio[u];
        uds[u].num_samples = num_samples[u];
        uds[u].num_frames = frames[u];
        uds[u].wave_out = xb[u];
        push_items(&items, u, frames[u], 64, 64);
    }
    DescTables t;
    SETK_TRY(upload_tables(h, uds, items, s, &t));
    *a = pass1_args(h, t.utts, t.items);
    *n_items = t.n_items;
    return SETK_OK;
}

int carve_wave_f32(setk_handle_t h, std::vector<UttDesc>& uds, void* const* wave, bool pcm16) {
    const auto share = [](const UttDesc& ud) { return ((size_t)ud.out_len * 4 + 255) & ~(size_t)255; };
    char* d_f32 = nullptr;
    if (pcm16) {
        size_t total = 0;
        for (const UttDesc& ud : uds) total += share(ud);
        SETK_TRY(arena_get(h, total, &d_f32));
    }
    for (size_t u = 0; u < uds.size(); ++u) {
        uds[u].wave_f32 = pcm16 ? reinterpret_cast<float*>(d_f32) : static_cast<float*>(wave[u]);
        if (pcm16) d_f32 += share(uds[u]);
    }
    return SETK_OK;
}

int check_bf_opts(setk_handle_t h, const setk_bf_opts& o, int C, int own_code, const char* own) {
    if (o.kind < SETK_BF_MVDR || o.kind > SETK_BF_MPDR_WHITEN)
        return fail(h, SETK_ERR_INVALID, "unknown beamformer kind");
    if (own) return fail(h, own_code, own);
    if (o.kind == SETK_BF_MPDR && (o.flags & SETK_FLAG_BAN))
        return fail(h, SETK_ERR_INVALID, "BAN needs a noise covariance (mpdr without whiten)");
    if (o.kind == SETK_BF_PMWF && o.pmwf_ref >= C)
        return fail(h, SETK_ERR_INVALID, "Reference channel ID exceeds total channels");
    return SETK_OK;
}

int profile_begin(setk_handle_t h, hipStream_t s) {
    if (!h->profiling) return SETK_OK;
    for (int i = 0; i < 5; ++i) {
        hipEvent_t e;
        if (!h->ev_pool.empty()) {
            e = h->ev_pool.back();
            h->ev_pool.pop_back();
        } else {
            HIP_TRY(h, hipEventCreate(&e));
        }
        h->ev[i] = e;
        h->ev_used.push_back(e);
    }
    return profile_mark(h, 0, s);
}

int profile_mark(setk_handle_t h, int i, hipStream_t s) {
    if (h->profiling) HIP_TRY(h, hipEventRecord(h->ev[i], s));
    return SETK_OK;
}

}  // namespace setk
