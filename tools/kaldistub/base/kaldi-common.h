// Stand-in for Kaldi's base/kaldi-common.h: the handful of names the image-method RIR generator of
// the reference uses, so that its translation unit compiles with a host compiler alone
// (tools/make_rir_golden.py).  Own code; nothing here comes from Kaldi.
#ifndef SETK_KALDISTUB_BASE_KALDI_COMMON_H_
#define SETK_KALDISTUB_BASE_KALDI_COMMON_H_
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace kaldi {
typedef float BaseFloat;
typedef int32_t int32;
typedef int16_t int16;

inline double Log(double x) { return std::log(x); }

// KALDI_ERR << ...;  throws std::runtime_error with the message when the statement ends
class StubError {
 public:
    StubError() {}
    [[noreturn]] ~StubError() noexcept(false) { throw std::runtime_error(os_.str()); }
    template <typename T>
    StubError& operator<<(const T& v) { os_ << v; return *this; }
    StubError& operator<<(std::ostream& (*f)(std::ostream&)) { os_ << f; return *this; }
 private:
    std::ostringstream os_;
};
}  // namespace kaldi

#define KALDI_ERR ::kaldi::StubError()
#define KALDI_ASSERT(cond)                                              \
    do {                                                                \
        if (!(cond)) throw std::runtime_error("KALDI_ASSERT: " #cond);  \
    } while (0)
#endif
