// Stand-alone driver for the host side of setk_ssl_scores / setk_ssl_batch under
// AddressSanitizer + UBSan, against the HIP stand-in (kernels do nothing, copies are memcpy):
// argument checks, staging, descriptor and window tables, the per-window arena rewind of MUSIC.
//
//   bash tools/hoststub/build.sh
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname "$($CXX -print-file-name=libclang_rt.asan-x86_64.so)")   # the shared ASan runtime
//   $CXX -std=c++17 -g -fsanitize=address,undefined -shared-libsan -Iinclude \
//       tools/hoststub/ssl_driver.cpp -L_abl -lsetk_hostasan -Wl,-rpath,$PWD/_abl -Wl,-rpath,$RT \
//       -o _abl/ssl_driver && _abl/ssl_driver
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
    CHECK(setk_stft_plan(h, 512, 256, 512, 1, nullptr), SETK_OK);
    const int pairs[4] = {0, 2, 1, 3};
    for (int backend = SETK_SSL_ML; backend <= SETK_SSL_MUSIC; ++backend) {
        setk_ssl_opts o = {backend, backend == SETK_SSL_SRP ? 2 : 0, backend == SETK_SSL_SRP ? pairs : nullptr,
                           -1.f, 0, 1.1920929e-7};
        // ---- the stand-alone operator on host arrays: odd sizes, with and without windows ----
        const int C = 4, T = 37, F = 129, A = 5;
        std::vector<float> spec((size_t)C * T * F * 2, 0.5f), mask((size_t)T * F, 1.f), sv((size_t)A * C * F * 2, 1.f);
        const int wins[6] = {0, T, 0, 1, 30, 37};
        std::vector<double> score(3 * A);
        int index[3], status = -1;
        CHECK(setk_ssl_scores(h, &o, spec.data(), mask.data(), sv.data(), A, C, T, F, nullptr, 0, score.data(), index,
                              &status, nullptr), SETK_OK);
        CHECK(setk_ssl_scores(h, &o, spec.data(), nullptr, sv.data(), A, C, T, F, wins, 3, score.data(), index,
                              &status, nullptr), SETK_OK);
        CHECK(setk_ssl_scores(h, &o, spec.data(), nullptr, sv.data(), A, C, T, F, wins, 3, nullptr, index, nullptr,
                              nullptr), SETK_OK);
        const int bad[2] = {5, 38};
        CHECK(setk_ssl_scores(h, &o, spec.data(), nullptr, sv.data(), A, C, T, F, bad, 1, nullptr, index, nullptr,
                              nullptr), SETK_ERR_INVALID);
        CHECK(setk_ssl_scores(h, &o, spec.data(), nullptr, sv.data(), A, 17, T, F, nullptr, 0, nullptr, index, nullptr,
                              nullptr), SETK_ERR_UNSUPPORTED);
        // ---- the batch on "device" audio: 4 and 16 channels, masks present and absent ----
        for (int Cb : {4, 16}) {
            if (backend == SETK_SSL_SRP && Cb != 4) continue;
            const int ns[2] = {256 * 40, 256 * 9 + 17}, nw[2] = {2, 1};
            const int bw[6] = {0, 41, 7, 33, 0, 10};
            void *a0, *a1, *m1, *dsv;
            std::vector<float> svb((size_t)A * Cb * 257 * 2, 1.f);
            if (hipMalloc(&a0, (size_t)Cb * ns[0] * 4) || hipMalloc(&a1, (size_t)Cb * ns[1] * 4) ||
                hipMalloc(&m1, (size_t)10 * 257 * 4) || hipMalloc(&dsv, svb.size() * 4))
                return 1;
            const float* audio[2] = {static_cast<float*>(a0), static_cast<float*>(a1)};
            const float* masks[2] = {nullptr, static_cast<float*>(m1)};
            int bidx[3], bst[2];
            std::vector<double> bscore(3 * A);
            CHECK(setk_ssl_batch(h, &o, 2, Cb, audio, ns, masks, svb.data(), A, bw, nw, bidx, bscore.data(), bst,
                                 nullptr), SETK_OK);
            CHECK(setk_ssl_batch(h, &o, 2, Cb, audio, ns, nullptr, static_cast<float*>(dsv), A, bw, nw, bidx, nullptr,
                                 nullptr, nullptr), SETK_OK);
            const int toolong[6] = {0, 42, 7, 33, 0, 10};
            CHECK(setk_ssl_batch(h, &o, 2, Cb, audio, ns, nullptr, svb.data(), A, toolong, nw, bidx, nullptr, nullptr,
                                 nullptr), SETK_ERR_INVALID);
            hipFree(a0), hipFree(a1), hipFree(m1), hipFree(dsv);
        }
    }
    setk_destroy(h);
    std::puts("ssl_driver: ok");
    return 0;
}
