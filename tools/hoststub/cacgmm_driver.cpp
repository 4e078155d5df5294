// Stand-alone driver for the host side of setk_cacgmm_masks / setk_cacgmm_estimate_batch under
// AddressSanitizer + UBSan, against the HIP stand-in (kernels do nothing, copies are memcpy):
// argument checks and refusals, staging of the spectrogram, the start and the status words, the
// argument table and work areas of a ragged batch, the resident / streaming choice.
//
//   bash tools/hoststub/build.sh
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname "$($CXX -print-file-name=libclang_rt.asan-x86_64.so)")   # the shared ASan runtime
//   $CXX -std=c++17 -g -fsanitize=address,undefined -shared-libsan -Iinclude \
//       tools/hoststub/cacgmm_driver.cpp -L_abl -lsetk_hostasan -Wl,-rpath,$PWD/_abl -Wl,-rpath,$RT \
//       -o _abl/cacgmm_driver && _abl/cacgmm_driver
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "setk_hip.h"

extern "C" int hipMalloc(void** p, size_t n);
extern "C" int hipFree(void* p);

#define CHECK(expr, want)                                                                    \
    do {                                                                                     \
        const int rc_ = (expr);                                                              \
        if (rc_ != (want)) {                                                                 \
            std::fprintf(stderr, "%s:%d: %s = %d (%s), wanted %d\n", __FILE__, __LINE__, #expr, rc_, \
                         setk_last_error(h), (want));                                        \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

int main() {
    setk_handle_t h = nullptr;
    if (setk_create(&h, 0) != SETK_OK) return 1;
    const int UA = SETK_CACGMM_UPDATE_ALPHA, CI = SETK_CACGMM_CGMM_INIT;
    // ---- the operator on host arrays: odd sizes, every K, with and without the status words ----
    for (int C : {1, 3, 8})
        for (int K : {2, 3, 4}) {
            const int T = 37, F = 5;
            std::vector<float> spec((size_t)C * T * F * 2, 0.5f), out((size_t)K * T * F, -1.f);
            std::vector<double> g0((size_t)K * F * T, 1.0 / K);
            std::vector<int> status(F, -1);
            CHECK(setk_cacgmm_masks(h, spec.data(), C, T, F, K, 3, g0.data(), UA, out.data(), status.data(), nullptr),
                  SETK_OK);
            CHECK(setk_cacgmm_masks(h, spec.data(), C, T, F, K, 0, g0.data(), 0, out.data(), nullptr, nullptr), SETK_OK);
            if (K == 2)
                CHECK(setk_cacgmm_masks(h, spec.data(), C, T, F, K, 3, nullptr, CI, out.data(), status.data(), nullptr),
                      SETK_OK);
        }
    {
        // ---- refusals ----
        const int T = 9, F = 3;
        std::vector<float> spec((size_t)9 * T * F * 2, 0.5f), out((size_t)5 * T * F);
        std::vector<double> g0((size_t)5 * F * T, 0.2);
        CHECK(setk_cacgmm_masks(h, spec.data(), 9, T, F, 2, 1, g0.data(), 0, out.data(), nullptr, nullptr),
              SETK_ERR_UNSUPPORTED);
        CHECK(setk_cacgmm_masks(h, spec.data(), 0, T, F, 2, 1, g0.data(), 0, out.data(), nullptr, nullptr),
              SETK_ERR_UNSUPPORTED);
        CHECK(setk_cacgmm_masks(h, spec.data(), 4, T, F, 5, 1, g0.data(), 0, out.data(), nullptr, nullptr),
              SETK_ERR_UNSUPPORTED);
        CHECK(setk_cacgmm_masks(h, spec.data(), 4, T, F, 1, 1, g0.data(), 0, out.data(), nullptr, nullptr),
              SETK_ERR_UNSUPPORTED);
        CHECK(setk_cacgmm_masks(h, spec.data(), 4, T, F, 2, 1, nullptr, UA, out.data(), nullptr, nullptr),
              SETK_ERR_INVALID);
        CHECK(setk_cacgmm_masks(h, spec.data(), 4, T, F, 3, 1, nullptr, CI, out.data(), nullptr, nullptr),
              SETK_ERR_INVALID);
        CHECK(setk_cacgmm_masks(h, spec.data(), 4, T, F, 2, 1, g0.data(), CI, out.data(), nullptr, nullptr),
              SETK_ERR_INVALID);
        CHECK(setk_cacgmm_masks(h, spec.data(), 4, T, F, 2, 1, g0.data(), 0x10, out.data(), nullptr, nullptr),
              SETK_ERR_INVALID);
        CHECK(setk_cacgmm_masks(h, spec.data(), 4, T, F, 2, -1, g0.data(), 0, out.data(), nullptr, nullptr),
              SETK_ERR_INVALID);
        CHECK(setk_cacgmm_masks(h, nullptr, 4, T, F, 2, 1, g0.data(), 0, out.data(), nullptr, nullptr),
              SETK_ERR_INVALID);
    }
    // ---- the batch on "device" audio: a ragged batch, both starts, both forms, no plan / a plan ----
    {
        const int C = 4, K = 3, F = 257;
        const int ns[3] = {256 * 36, 256 * 128 + 17, 256 * 299};
        const int frames[3] = {37, 129, 300};
        void *a[3], *g[3], *o[3];
        for (int u = 0; u < 3; ++u)
            if (hipMalloc(&a[u], (size_t)C * ns[u] * 4) || hipMalloc(&g[u], (size_t)K * F * frames[u] * 8) ||
                hipMalloc(&o[u], (size_t)K * frames[u] * F * 4))
                return 1;
        const float* audio[3] = {static_cast<float*>(a[0]), static_cast<float*>(a[1]), static_cast<float*>(a[2])};
        const double* g0[3] = {static_cast<double*>(g[0]), static_cast<double*>(g[1]), static_cast<double*>(g[2])};
        float* out[3] = {static_cast<float*>(o[0]), static_cast<float*>(o[1]), static_cast<float*>(o[2])};
        int status[3] = {-1, -1, -1};
        CHECK(setk_cacgmm_estimate_batch(h, 3, C, audio, ns, K, 2, g0, UA, out, status, nullptr), SETK_ERR_INVALID);
        CHECK(setk_stft_plan(h, 512, 256, 512, 1, nullptr), SETK_OK);
        CHECK(setk_cacgmm_estimate_batch(h, 3, C, audio, ns, K, 2, g0, UA, out, status, nullptr), SETK_OK);
        CHECK(setk_cacgmm_estimate_batch(h, 3, C, audio, ns, K, 2, g0, UA, out, nullptr, nullptr), SETK_OK);
        CHECK(setk_cacgmm_estimate_batch(h, 2, C, audio, ns, 2, 2, nullptr, CI, out, status, nullptr), SETK_OK);
        setenv("SETK_CACGMM_STREAMING", "1", 1);
        CHECK(setk_cacgmm_estimate_batch(h, 3, C, audio, ns, K, 2, g0, 0, out, status, nullptr), SETK_OK);
        unsetenv("SETK_CACGMM_STREAMING");
        // refusals: a missing start, a host pointer, a null entry, too many channels, too short
        CHECK(setk_cacgmm_estimate_batch(h, 3, C, audio, ns, K, 2, nullptr, UA, out, status, nullptr), SETK_ERR_INVALID);
        std::vector<float> host((size_t)C * ns[0]);
        const float* mixed[3] = {host.data(), audio[1], audio[2]};
        CHECK(setk_cacgmm_estimate_batch(h, 3, C, mixed, ns, K, 2, g0, UA, out, status, nullptr), SETK_ERR_INVALID);
        const double* hole[3] = {g0[0], nullptr, g0[2]};
        CHECK(setk_cacgmm_estimate_batch(h, 3, C, audio, ns, K, 2, hole, UA, out, status, nullptr), SETK_ERR_INVALID);
        CHECK(setk_cacgmm_estimate_batch(h, 3, 9, audio, ns, K, 2, g0, UA, out, status, nullptr), SETK_ERR_UNSUPPORTED);
        CHECK(setk_cacgmm_estimate_batch(h, 0, C, audio, ns, K, 2, g0, UA, out, status, nullptr), SETK_ERR_INVALID);
        for (int u = 0; u < 3; ++u) hipFree(a[u]), hipFree(g[u]), hipFree(o[u]);
    }
    // an utterance too long for LDS (8 channels, 2000 frames): the streaming form's launch
    {
        const int C = 8, K = 2, T = 2000, F = 2;
        std::vector<float> spec((size_t)C * T * F * 2, 0.25f), out((size_t)K * T * F);
        std::vector<double> g0((size_t)K * F * T, 0.5);
        CHECK(setk_cacgmm_masks(h, spec.data(), C, T, F, K, 1, g0.data(), UA, out.data(), nullptr, nullptr), SETK_OK);
    }
    setk_destroy(h);
    std::puts("cacgmm_driver: ok");
    return 0;
}
