// Stand-in for Kaldi's util/common-utils.h (see base/kaldi-common.h beside it): string splitting,
// a dense matrix and the option-registration interface, as far as the RIR generator needs them.
#ifndef SETK_KALDISTUB_UTIL_COMMON_UTILS_H_
#define SETK_KALDISTUB_UTIL_COMMON_UTILS_H_
#include <map>

#include "base/kaldi-common.h"

namespace kaldi {

inline void SplitStringToVector(const std::string& full, const char* delim, bool omit_empty,
                                std::vector<std::string>* out) {
    out->clear();
    size_t start = 0;
    while (true) {
        const size_t end = full.find_first_of(delim, start);
        const std::string piece = full.substr(start, end == std::string::npos ? end : end - start);
        if (!omit_empty || !piece.empty()) out->push_back(piece);
        if (end == std::string::npos) break;
        start = end + 1;
    }
}

template <typename F>
bool SplitStringToFloats(const std::string& full, const char* delim, bool omit_empty, std::vector<F>* out) {
    out->clear();
    if (full.empty()) return true;
    std::vector<std::string> pieces;
    SplitStringToVector(full, delim, omit_empty, &pieces);
    for (const std::string& p : pieces) {
        char* end = nullptr;
        const double v = std::strtod(p.c_str(), &end);
        if (end == p.c_str() || *end != '\0') return false;
        out->push_back(static_cast<F>(v));
    }
    return true;
}

template <typename T>
class Matrix {
 public:
    void Resize(int32 rows, int32 cols) {
        rows_ = rows;
        cols_ = cols;
        data_.assign(static_cast<size_t>(rows) * cols, T(0));
    }
    T& operator()(int32 r, int32 c) { return data_[static_cast<size_t>(r) * cols_ + c]; }
    int32 NumRows() const { return rows_; }
    int32 NumCols() const { return cols_; }
    const T* Data() const { return data_.data(); }
 private:
    int32 rows_ = 0, cols_ = 0;
    std::vector<T> data_;
};

// --name=value options, by type
class OptionsItf {
 public:
    void Register(const std::string& n, bool* p, const std::string&) { b_[n] = p; }
    void Register(const std::string& n, int32* p, const std::string&) { i_[n] = p; }
    void Register(const std::string& n, float* p, const std::string&) { f_[n] = p; }
    void Register(const std::string& n, std::string* p, const std::string&) { s_[n] = p; }
    // "--name=value"; false for an unknown name
    bool Set(const std::string& arg) {
        const size_t eq = arg.find('=');
        if (arg.compare(0, 2, "--") != 0 || eq == std::string::npos) return false;
        const std::string n = arg.substr(2, eq - 2), v = arg.substr(eq + 1);
        if (b_.count(n)) *b_[n] = (v == "true" || v == "1");
        else if (i_.count(n)) *i_[n] = std::atoi(v.c_str());
        else if (f_.count(n)) *f_[n] = static_cast<float>(std::strtod(v.c_str(), nullptr));
        else if (s_.count(n)) *s_[n] = v;
        else return false;
        return true;
    }
 private:
    std::map<std::string, bool*> b_;
    std::map<std::string, int32*> i_;
    std::map<std::string, float*> f_;
    std::map<std::string, std::string*> s_;
};

}  // namespace kaldi
#endif
