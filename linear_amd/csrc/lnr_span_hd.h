// lnr_span_hd.h -- the one store routine of the GPU writer (lnr_output_kernels.hip): a byte range of global memory written by a team of
// lanes as destination-aligned dwords, with single bytes in the first and the last dword where the range covers only part of them.
//
// PRODUCT code as __host__ __device__ text: the kernels call it with `lane, 64` or `threadIdx.x, 256`; tests/output_span_main.cpp compiles
// the same text with g++ under the address and undefined-behaviour sanitizers and calls it once per lane (tests/test_output_span_cpu.py),
// so the address arithmetic that keeps the writer inside its buffers is pinned on a machine without a GPU.
//
// What is touched.  Writes: [dst, dst + len) and nothing else.  Reads are the word source's business; span_copy's source (SpanCopy) loads
// only aligned dwords that hold a byte of [src, src + len): never below src's own dword, at most 3 bytes past src + len.  The slack of the
// sort's segments (8 bytes behind, HOST_FRONT in front: lnr_output_kernels.hip) covers this with room to spare.
#pragma once
#include <stdint.h>

#ifndef LNR_HD
#if defined(__HIPCC__)
#define LNR_HD __host__ __device__
#else
#define LNR_HD
#endif
#endif

namespace lnr_out {

// Lane t of nt writes its share of [dst, dst + len).  The span is cut at dst's dword boundaries: position q counts bytes from dst rounded
// down to 4, and word(q, full) yields the 32 bits of the dword at q (a multiple of 4), of which byte b goes to position q + b.  The whole
// dwords of the range are dealt to the lanes t, t + nt, ... and stored in a loop without a branch (full = true); a first and a last dword
// that the range covers in part are written as single bytes, one byte to a lane: byte t of the first dword by the lanes t < 4, byte t - 4
// of the last by the lanes 4 <= t < 8, so nt is at least 8 (full = false: the word's bytes outside the range are not looked at, and a
// source must not read for them).  Always inlined: the word sources are lambdas over their caller's registers.
template <class W> LNR_HD inline __attribute__((always_inline)) void span_store(uint8_t *dst, uint32_t len, uint32_t t, uint32_t nt, W word) {
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3), end = mis + len;
    uint8_t *base = dst - mis;
    if (len == 0) return;
    const uint32_t first = mis ? 4 : 0, last = end & ~3u;      // the whole dwords: [first, last)
    for (uint32_t q = first + 4 * t; q < last; q += 4 * nt) *reinterpret_cast<uint32_t *>(base + q) = word(q, true);
    if (t >= 8) return;
    const uint32_t q = t < 4 ? 0 : last, p = q + (t & 3);      // this lane's byte of a partial dword, if there is one
    const bool partial = t < 4 ? mis != 0 : last >= first && last < end;
    if (partial && p >= mis && p < end) base[p] = (uint8_t)(word(q, false) >> (8 * (t & 3)));
}

// the word source of a copy: destination dword q put together from the two aligned source dwords that hold its bytes.  Word i of sw holds
// source offsets 4 i - back .. 4 i - back + 3, and destination dword q = 4 i takes its bytes from words i and i + 1 (from word i alone where
// source and destination are aligned alike).  Where only one of the two holds a byte of [src, src + len) -- in the first and the last dword
// of a span -- that one is loaded twice and the other not at all.
struct SpanCopy {
    const uint32_t *sw; uint32_t len, back, r;  // back: bytes from sw to src, 0 .. 6 (sw itself may lie below src's dword: word 0 is then never loaded); r: the shift in bits
    LNR_HD SpanCopy(uint8_t *dst, const uint8_t *src, uint32_t len_) : len(len_) {
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 3), sh = (uint32_t)(((uintptr_t)src - mis) & 3);
        back = mis + sh; r = 8 * sh;
        sw = reinterpret_cast<const uint32_t *>(src - back);
    }
    LNR_HD uint32_t operator()(uint32_t q, bool full) const {
        const uint32_t i = q >> 2;
        if (r == 0) return sw[i];
        const bool lo = q + 3 >= back, hi = q + 4 < len + back;     // word i / word i + 1 holds a byte of the range: both do where the dword is full
        if (full || (lo && hi)) return (sw[i] >> r) | (sw[i + 1] << (32 - r));
        const uint32_t w = sw[lo ? i : i + 1];
        return (w >> r) | (w << (32 - r));
    }
};
LNR_HD inline void span_copy(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t t, uint32_t nt) { span_store(dst, len, t, nt, SpanCopy(dst, src, len)); }
struct SpanFill { uint32_t v; LNR_HD uint32_t operator()(uint32_t, bool) const { return v; } };
LNR_HD inline void span_fill(uint8_t *dst, uint8_t byte, uint32_t len, uint32_t t, uint32_t nt) {
    span_store(dst, len, t, nt, SpanFill{0x01010101u * byte});
}

}  // namespace lnr_out
