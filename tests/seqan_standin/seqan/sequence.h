// tests/seqan_standin/seqan/sequence.h -- the few SeqAn names that integration/gpu_filter.h and tests/gpufilter_driver.cpp use
// (String, StringSet, Dna5, length, resize, appendValue), written for this test suite with SeqAn's storage contract: a
// String<Dna5> keeps one ordinal byte per base (A,C,G,T,N = 0..4) contiguously, so &s[0] / length(s) bind to the C ABI.
// With it the GPU test of the binding builds from this repository alone; the binding against the real SeqAn headers is
// compiled and run by tests/test_boundary_compile_cpu.py wherever those headers are present.
#ifndef LNR_SEQAN_STANDIN_SEQUENCE_H
#define LNR_SEQAN_STANDIN_SEQUENCE_H

#include <cstddef>
#include <cstdint>
#include <vector>

namespace seqan {

struct Dna5 {
    uint8_t ord;
    Dna5() : ord(0) {}
    explicit Dna5(unsigned v) : ord(static_cast<uint8_t>(v > 4 ? 4 : v)) {}
};
static_assert(sizeof(Dna5) == 1, "one ordinal byte per base");

template <typename T>
struct String {
    std::vector<T> v;
    T &operator[](size_t i) { return v[i]; }
    const T &operator[](size_t i) const { return v[i]; }
};

template <typename T>
struct StringSet {
    std::vector<T> v;
    T &operator[](size_t i) { return v[i]; }
    const T &operator[](size_t i) const { return v[i]; }
};

template <typename T> size_t length(const String<T> &s) { return s.v.size(); }
template <typename T> size_t length(const StringSet<T> &s) { return s.v.size(); }
template <typename T> void resize(String<T> &s, size_t n) { s.v.resize(n); }
template <typename T> void resize(StringSet<T> &s, size_t n) { s.v.resize(n); }
template <typename T> void appendValue(StringSet<T> &s, const T &x) { s.v.push_back(x); }

}  // namespace seqan

#endif
