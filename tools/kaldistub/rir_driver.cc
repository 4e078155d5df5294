// The one translation unit tools/make_rir_golden.py compiles: the reference's RIR generator,
// included unmodified from the reference tree (-I <reference root>), behind a main of its own that
// takes rir-simulate's --name=value options and one destination.  What it writes is not a wave file
// but the generator's float32 matrix as it stands (before rir-simulate.cc:64's scaling):
//     int32 rows, int32 cols, float32 [rows][cols]
// and on stdout the seconds GenerateRir took.  Own code; the stand-in headers are beside it.
#include <chrono>
#include <cstdio>

#include "include/rir-generator.cc"

int main(int argc, char** argv) {
    try {
        kaldi::OptionsItf po;
        kaldi::RirGeneratorOptions opts;
        opts.Register(&po);
        std::string dest;
        for (int i = 1; i < argc; ++i) {
            const std::string a = argv[i];
            if (a.compare(0, 2, "--") != 0) {
                dest = a;
            } else if (!po.Set(a)) {
                std::fprintf(stderr, "unknown option %s\n", a.c_str());
                return 2;
            }
        }
        if (dest.empty()) return 2;
        kaldi::RirGenerator generator(opts);
        kaldi::Matrix<kaldi::BaseFloat> rir;
        const auto t0 = std::chrono::steady_clock::now();
        generator.GenerateRir(&rir);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::FILE* f = std::fopen(dest.c_str(), "wb");
        if (!f) return 3;
        const int32_t shape[2] = {rir.NumRows(), rir.NumCols()};
        std::fwrite(shape, sizeof(int32_t), 2, f);
        std::fwrite(rir.Data(), sizeof(float), static_cast<size_t>(shape[0]) * shape[1], f);
        std::fclose(f);
        std::printf("%.6f\n", sec);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
