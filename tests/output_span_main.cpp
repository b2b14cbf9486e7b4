// output_span_main.cpp -- the store routine of the GPU writer (lnr_out::span_store with its copy and fill forms, linear_amd/csrc/lnr_span_hd.h)
// as a stand-alone program for the address and undefined-behaviour sanitizers (tests/test_output_span_cpu.py).  For every destination
// misalignment 0..3, source misalignment 0..3, length 0..20, 255..260 and 8191..8193 and team size 64 and 256 the routine is called once
// per lane t, as the lanes of a wave or a workgroup call it.  The destination lies in a heap block between two guards of 16 bytes: it must
// equal memcpy / memset and the guards must be untouched (a write outside the block is the sanitizer's).  The source lies in a heap block
// of its own that is the range plus exactly the documented slack -- down to the source's own dword in front, 3 bytes behind --, so that
// any wider read is an error.  Prints "ok <combinations>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../linear_amd/csrc/lnr_span_hd.h"

namespace {

constexpr uint32_t GUARD = 16;
constexpr uint8_t MARK = 0xa5;

struct Dest {                                     // [GUARD marks][dmis marks][len bytes][GUARD marks], malloc's alignment is 16
    uint8_t *block, *dst; uint32_t size;
    Dest(uint32_t dmis, uint32_t len) : size(GUARD + dmis + len + GUARD) {
        block = (uint8_t *)malloc(size);
        memset(block, MARK, size);
        dst = block + GUARD + dmis;
    }
    ~Dest() { free(block); }
    bool is(const uint8_t *want, uint32_t len) const {
        for (uint8_t *p = block; p < dst; p++) if (*p != MARK) return false;
        for (uint8_t *p = dst + len; p < block + size; p++) if (*p != MARK) return false;
        return len == 0 || memcmp(dst, want, len) == 0;
    }
};

}  // namespace

int main() {
    std::vector<uint32_t> lens;
    for (uint32_t l = 0; l <= 20; l++) lens.push_back(l);
    for (uint32_t l = 255; l <= 260; l++) lens.push_back(l);
    for (uint32_t l = 8191; l <= 8193; l++) lens.push_back(l);
    unsigned long long combos = 0;
    for (uint32_t nt : {64u, 256u})
        for (uint32_t len : lens)
            for (uint32_t dmis = 0; dmis < 4; dmis++) {
                {                                                        // the fill form
                    Dest d(dmis, len);
                    for (uint32_t t = 0; t < nt; t++) lnr_out::span_fill(d.dst, 0xff, len, t, nt);
                    std::vector<uint8_t> want(len, 0xff);
                    if (!d.is(want.data(), len)) { fprintf(stderr, "fill: dst %u len %u nt %u\n", dmis, len, nt); return 1; }
                    combos++;
                }
                for (uint32_t smis = 0; smis < 4; smis++) {              // the copy form
                    uint8_t *sblock = (uint8_t *)malloc(smis + len + 3);
                    for (uint32_t i = 0; i < smis + len + 3; i++) sblock[i] = (uint8_t)(i * 131u + 7u * smis + 1u);
                    const uint8_t *src = sblock + smis;
                    Dest d(dmis, len);
                    for (uint32_t t = 0; t < nt; t++) lnr_out::span_copy(d.dst, src, len, t, nt);
                    const bool ok = d.is(src, len);
                    free(sblock);
                    if (!ok) { fprintf(stderr, "copy: dst %u src %u len %u nt %u\n", dmis, smis, len, nt); return 1; }
                    combos++;
                }
            }
    printf("ok %llu\n", combos);
    return 0;
}
