// lnr_inflate_hd.h -- raw DEFLATE (RFC 1951) of ONE BGZF block and the CRC32 of its text, as __host__ __device__ code over plain arrays.
//
// PRODUCT code: k_bgzf_inflate (lnr_reader_kernels.hip) runs inflate_block on the device, one wave per BGZF block;
// tests/inflate_hd_shim.cpp compiles the same text with g++ (tests/test_inflate_hd_cpu.py: every block of every fixture against zlib,
// every corrupt case, the same under the address and undefined-behaviour sanitizers).
//
// The decoder is TOTAL: whatever the bytes are it reads only [c, c + clen), writes only [out, out + isize) -- through the Sink it is
// given -- and ends: every step of the decode loops takes at least one input bit or ends the block, and the input is bounded.
//   * stored, fixed-Huffman and dynamic-Huffman blocks, any number of them in one BGZF block;
//   * Huffman codes as counts per length + symbols in canonical order (Mark Adler's "puff" form: RFC 1951 3.2.2 read literally, a code is
//     walked bit by bit; a table of 2 * 16 + 288 + 30 halfwords is all a wave keeps in LDS);
//   * a match whose distance is smaller than its length repeats its period: byte i of the copy is byte (i mod distance) of the source,
//     so a Sink may copy all bytes of a match at once.
// The result is a status word: OK or the first reason found.  Nothing the caller may use has been produced unless it is OK.
//
// The work is written for a wave whose lanes all run it with the same values (the state is wave-uniform; LNR_INFLATE_UNIFORM, where
// the including file defines it, tells the compiler so); only the Sink knows about lanes.  The host runs it as one lane.
#pragma once
#include <stdint.h>

#ifndef LNR_HD
#if defined(__HIPCC__)
#define LNR_HD __host__ __device__
#else
#define LNR_HD
#endif
#endif
#ifndef LNR_INFLATE_UNIFORM
#define LNR_INFLATE_UNIFORM(x) (x)
#endif

namespace lnr_inf {

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t u8;

enum Status : u32 {
    OK = 0,
    E_INPUT_END = 1,        // a code or a field needs bits past the end of the block's data
    E_BLOCK_TYPE = 2,       // block type 3
    E_STORED_LEN = 3,       // stored block: LEN != ~NLEN
    E_COUNTS = 4,           // dynamic block: more than 286 length/literal or more than 30 distance codes
    E_OVERSUBSCRIBED = 5,   // code lengths that over-subscribe the code space
    E_INCOMPLETE = 6,       // code lengths that leave code space unused (other than one distance code of length 1, or none)
    E_REPEAT = 7,           // code-length repeat without a length before it, or past the last code
    E_NO_END_CODE = 8,      // no code for the end-of-block symbol
    E_SYMBOL = 9,           // length/literal symbol above 285, distance symbol above 29, or a code no symbol has
    E_DISTANCE = 10,        // a distance that reaches before the first byte of the block's text
    E_OUTPUT = 11,          // more text than ISIZE
    E_ISIZE = 12,           // less text than ISIZE
    E_CRC = 13,             // the text's CRC32 differs from the footer's
    E_TABLE = 14,           // the block's table entry lies outside the buffers it refers to (host error, checked on the device)
};
LNR_HD inline const char *status_text(u32 s) {
    switch (s) {
    case OK: return "ok";
    case E_INPUT_END: return "compressed data ends inside a code";
    case E_BLOCK_TYPE: return "DEFLATE block type 3";
    case E_STORED_LEN: return "stored block with LEN != ~NLEN";
    case E_COUNTS: return "too many length or distance codes";
    case E_OVERSUBSCRIBED: return "over-subscribed code lengths";
    case E_INCOMPLETE: return "incomplete code lengths";
    case E_REPEAT: return "bad code-length repeat";
    case E_NO_END_CODE: return "no end-of-block code";
    case E_SYMBOL: return "invalid length or distance symbol";
    case E_DISTANCE: return "distance reaches before the block's text";
    case E_OUTPUT: return "more text than ISIZE";
    case E_ISIZE: return "less text than ISIZE";
    case E_CRC: return "CRC32 differs from the footer";
    case E_TABLE: return "block table entry out of range";
    }
    return "unknown reason";
}

// ---- CRC32 (the gzip polynomial, reflected).  Bitwise: a block's text is CRC'd once, in 64 slices on the device.
constexpr u32 CRC_POLY = 0xEDB88320u;
LNR_HD inline u32 crc_byte(u32 crc, u8 b) {             // crc = the running register (starts at ~0, the CRC is its complement)
    crc ^= b;
    for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (CRC_POLY & (0u - (crc & 1u)));
    return crc;
}
LNR_HD inline u32 crc_of(const u8 *p, u64 n) {
    u32 c = ~0u;
    for (u64 i = 0; i < n; i++) c = crc_byte(c, p[i]);
    return ~c;
}
// a(x) * b(x) mod the polynomial, bits reflected as the CRC register holds them (zlib's multmodp)
LNR_HD inline u32 crc_mul(u32 a, u32 b) {
    u32 p = 0;
    for (u32 m = 1u << 31; m; m >>= 1) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod the polynomial
LNR_HD inline u32 crc_xpow8(u64 n) {
    u32 p = 1u << 31, sq = 1u << 23;                     // x^0; x^8
    for (; n; n >>= 1) { if (n & 1) p = crc_mul(sq, p); sq = crc_mul(sq, sq); }
    return p;
}
// the CRC of A followed by B from the CRC of A, the CRC of B and the length of B (zlib's crc32_combine).  Linear: the CRC of a text cut
// into slices is the XOR of crc_shift(crc of slice, bytes behind the slice) over the slices.
LNR_HD inline u32 crc_shift(u32 crc, u64 bytes_behind) { return crc_mul(crc_xpow8(bytes_behind), crc); }
LNR_HD inline u32 crc_combine(u32 crc_a, u32 crc_b, u64 len_b) { return crc_shift(crc_a, len_b) ^ crc_b; }

// ---- Huffman codes
constexpr u32 MAXBITS = 15, MAXL = 286, MAXD = 30, FIXL = 288;
struct Code { u16 count[16]; };                          // count[l] = codes of length l; the symbols lie beside it
struct Tables {                                          // one wave's (one host call's) work space
    Code lc, dc;
    u16 lsym[FIXL], dsym[MAXD + 2];
    u8 len[FIXL + MAXD + 2];                             // code lengths while a block's codes are read
    u16 offs[16];                                        // build_code's first symbol index per length
};

// counts + symbols in canonical order from n code lengths.  Returns the unused code space (0: complete) or ~0u when over-subscribed.
LNR_HD inline u32 build_code(Code &h, u16 *sym, const u8 *len, u32 n, u16 *offs) {
    for (u32 l = 0; l <= MAXBITS; l++) h.count[l] = 0;
    for (u32 s = 0; s < n; s++) { const u32 l = LNR_INFLATE_UNIFORM((u32)len[s]); h.count[l] = (u16)(LNR_INFLATE_UNIFORM((u32)h.count[l]) + 1); }
    int left = 1;
    for (u32 l = 1; l <= MAXBITS; l++) {
        left <<= 1;
        left -= (int)LNR_INFLATE_UNIFORM((u32)h.count[l]);
        if (left < 0) return ~0u;
    }
    u32 o = 0;
    for (u32 l = 1; l <= MAXBITS; l++) { offs[l] = (u16)o; o += LNR_INFLATE_UNIFORM((u32)h.count[l]); }
    for (u32 s = 0; s < n; s++) {
        const u32 l = LNR_INFLATE_UNIFORM((u32)len[s]);
        if (l) { const u32 at = LNR_INFLATE_UNIFORM((u32)offs[l]); sym[at] = (u16)s; offs[l] = (u16)(at + 1); }
    }
    return (u32)left;
}

struct Bits {
    const u8 *c; u32 clen, ip;                           // ip = next byte not yet in `b`
    u64 b; u32 n;                                        // n valid bits in b, the next bit lowest
};
LNR_HD inline void refill(Bits &s) {                     // afterwards n >= 32, or every byte of the input is in
    if (s.n >= 32) return;
    if (s.ip + 4 <= s.clen) {
        const u8 *p = s.c + s.ip;
        const u32 w = (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24);
        s.b |= (u64)LNR_INFLATE_UNIFORM(w) << s.n; s.n += 32; s.ip += 4;
        return;
    }
    while (s.ip < s.clen && s.n <= 56) { const u32 w = s.c[s.ip++]; s.b |= (u64)LNR_INFLATE_UNIFORM(w) << s.n; s.n += 8; }
}
// k <= 16 bits; false: the input ends before them
LNR_HD inline bool take(Bits &s, u32 k, u32 &v) {
    refill(s);
    if (s.n < k) return false;
    v = (u32)(s.b & ((1ULL << k) - 1ULL));
    s.b >>= k; s.n -= k;
    return true;
}
// one symbol of code h: >= 0 the symbol, -1 the input ends inside the code, -2 no symbol has this code (incomplete code)
LNR_HD inline int decode(Bits &s, const Code &h, const u16 *sym) {
    refill(s);
    u64 b = s.b;
    int code = 0, first = 0, index = 0;
    for (u32 l = 1; l <= MAXBITS; l++) {
        if (l > s.n) return -1;
        code |= (int)(b & 1); b >>= 1;
        const int count = (int)LNR_INFLATE_UNIFORM((u32)h.count[l]);
        if (code - count < first) {
            s.b = b; s.n -= l;
            return (int)LNR_INFLATE_UNIFORM((u32)sym[index + (code - first)]);
        }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -2;
}

LNR_HD inline u32 len_base(u32 i) {                      // i = symbol - 257, 0 .. 28
    return i < 8 ? 3 + i : i == 28 ? 258 : 3 + ((4 + (i & 3)) << ((i >> 2) - 1));
}
LNR_HD inline u32 len_extra(u32 i) { return i < 8 || i == 28 ? 0 : (i >> 2) - 1; }
LNR_HD inline u32 dist_base(u32 i) {                     // i = distance symbol, 0 .. 29
    return i < 4 ? 1 + i : 1 + ((2 + (i & 1)) << ((i >> 1) - 1));
}
LNR_HD inline u32 dist_extra(u32 i) { return i < 4 ? 0 : (i >> 1) - 1; }

// A Sink takes the text.  The decoder checks every position before it calls:
//   lit(pos, byte)                      pos < isize
//   match(pos, len, dist)               pos + len <= isize, 1 <= dist <= pos, 3 <= len <= 258
//   stored(pos, src, n)                 pos + n <= isize, [src, src + n) inside the input
struct HostSink {
    u8 *out;
    LNR_HD void lit(u32 pos, u8 b) { out[pos] = b; }
    LNR_HD void match(u32 pos, u32 len, u32 dist) { for (u32 i = 0; i < len; i++) out[pos + i] = out[pos - dist + i % dist]; }
    LNR_HD void stored(u32 pos, const u8 *src, u32 n) { for (u32 i = 0; i < n; i++) out[pos + i] = src[i]; }
};

template <class Sink>
LNR_HD inline u32 codes_block(Bits &s, Sink &o, u32 &pos, u32 isize, const Tables &T) {
    for (;;) {
        int sym = decode(s, T.lc, T.lsym);
        if (sym < 0) return sym == -1 ? E_INPUT_END : E_SYMBOL;
        if (sym < 256) {
            if (pos >= isize) return E_OUTPUT;
            o.lit(pos, (u8)sym); pos++;
            continue;
        }
        if (sym == 256) return OK;
        if (sym > 285) return E_SYMBOL;
        u32 li = (u32)sym - 257, x = 0;
        if (!take(s, len_extra(li), x)) return E_INPUT_END;
        const u32 len = len_base(li) + x;
        sym = decode(s, T.dc, T.dsym);
        if (sym < 0) return sym == -1 ? E_INPUT_END : E_SYMBOL;
        if (sym > 29) return E_SYMBOL;
        if (!take(s, dist_extra((u32)sym), x)) return E_INPUT_END;
        const u32 dist = dist_base((u32)sym) + x;
        if (dist > pos) return E_DISTANCE;
        if (len > isize - pos) return E_OUTPUT;
        o.match(pos, len, dist); pos += len;
    }
}

LNR_HD inline void fixed_tables(Tables &T) {
    u32 s = 0;
    for (; s < 144; s++) T.len[s] = 8;
    for (; s < 256; s++) T.len[s] = 9;
    for (; s < 280; s++) T.len[s] = 7;
    for (; s < FIXL; s++) T.len[s] = 8;
    (void)build_code(T.lc, T.lsym, T.len, FIXL, T.offs);
    for (s = 0; s < MAXD + 2; s++) T.len[s] = 5;         // 32 codes: 30 and 31 are E_SYMBOL when they occur
    (void)build_code(T.dc, T.dsym, T.len, MAXD + 2, T.offs);
}

LNR_HD inline u32 dynamic_tables(Bits &s, Tables &T) {
    u32 nlen, ndist, ncode, v;
    if (!take(s, 5, nlen) || !take(s, 5, ndist) || !take(s, 4, ncode)) return E_INPUT_END;
    nlen += 257; ndist += 1; ncode += 4;
    if (nlen > MAXL || ndist > MAXD) return E_COUNTS;
    const u8 order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (u32 i = 0; i < 19; i++) T.len[i] = 0;
    for (u32 i = 0; i < ncode; i++) { if (!take(s, 3, v)) return E_INPUT_END; T.len[order[i]] = (u8)v; }
    u32 left = build_code(T.lc, T.lsym, T.len, 19, T.offs);      // the code-length code, kept in the length/literal table for now
    if (left == ~0u) return E_OVERSUBSCRIBED;
    if (left) return E_INCOMPLETE;
    u32 i = 0;
    while (i < nlen + ndist) {
        const int sym = decode(s, T.lc, T.lsym);
        if (sym < 0) return sym == -1 ? E_INPUT_END : E_SYMBOL;
        if (sym < 16) { T.len[i++] = (u8)sym; continue; }
        u32 rep, val = 0;
        if (sym == 16) {
            if (i == 0) return E_REPEAT;
            val = LNR_INFLATE_UNIFORM((u32)T.len[i - 1]);
            if (!take(s, 2, rep)) return E_INPUT_END;
            rep += 3;
        } else if (sym == 17) { if (!take(s, 3, rep)) return E_INPUT_END; rep += 3; }
        else { if (!take(s, 7, rep)) return E_INPUT_END; rep += 11; }
        if (i + rep > nlen + ndist) return E_REPEAT;
        while (rep--) T.len[i++] = (u8)val;
    }
    if (LNR_INFLATE_UNIFORM((u32)T.len[256]) == 0) return E_NO_END_CODE;
    // the distance lengths first: building the length/literal code overwrites nothing of T.len, but keep the order of use plain
    left = build_code(T.dc, T.dsym, T.len + nlen, ndist, T.offs);
    if (left == ~0u) return E_OVERSUBSCRIBED;
    const u32 d0 = LNR_INFLATE_UNIFORM((u32)T.dc.count[0]), d1 = LNR_INFLATE_UNIFORM((u32)T.dc.count[1]);
    if (left && !(d0 == ndist || (d1 == 1 && d0 + 1u == ndist))) return E_INCOMPLETE;
    left = build_code(T.lc, T.lsym, T.len, nlen, T.offs);
    if (left == ~0u) return E_OVERSUBSCRIBED;
    if (left) return E_INCOMPLETE;
    return OK;
}

// Inflates [c, c + clen) through the sink.  OK: exactly isize bytes were produced (the CRC is the caller's: crc_of / its slices).
template <class Sink>
LNR_HD inline u32 inflate_block(const u8 *c, u32 clen, Sink &o, u32 isize, Tables &T, u32 *deflate_blocks = nullptr) {
    Bits s; s.c = c; s.clen = clen; s.ip = 0; s.b = 0; s.n = 0;
    u32 pos = 0, last = 0;
    while (!last) {
        u32 type;
        if (!take(s, 1, last) || !take(s, 2, type)) return E_INPUT_END;
        if (deflate_blocks) ++*deflate_blocks;
        u32 st = OK;
        if (type == 0) {
            u32 len, nlen;
            s.b >>= (s.n & 7); s.n &= ~7u;                // to the byte boundary
            if (!take(s, 16, len) || !take(s, 16, nlen)) return E_INPUT_END;
            if (len != (~nlen & 0xFFFFu)) return E_STORED_LEN;
            s.ip -= s.n >> 3; s.b = 0; s.n = 0;          // bytes the bit buffer holds go back to the input
            if (len > s.clen - s.ip) return E_INPUT_END;
            if (len > isize - pos) return E_OUTPUT;
            o.stored(pos, s.c + s.ip, len);
            pos += len; s.ip += len;
        } else if (type == 1) {
            fixed_tables(T);
            st = codes_block(s, o, pos, isize, T);
        } else if (type == 2) {
            st = dynamic_tables(s, T);
            if (st == OK) st = codes_block(s, o, pos, isize, T);
        } else return E_BLOCK_TYPE;
        if (st != OK) return st;
    }
    return pos == isize ? (u32)OK : (u32)E_ISIZE;
}

// ---- the BGZF member header (RFC 1952 + the SAM specification 4.1): magic 1f 8b, CM 8, FLG = FEXTRA alone, an extra subfield 'B','C' of
// length 2 that holds BSIZE = member size - 1.  Other subfields may stand before or behind it.  avail = bytes of the file from p on.
// Returns the member's size (0: not a BGZF member, or it does not fit) and the offset of its DEFLATE data.
LNR_HD inline u32 bgzf_member(const u8 *p, u64 avail, u32 &data_off) {
    if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0;
    const u32 xlen = (u32)p[10] | ((u32)p[11] << 8);
    if (12ULL + xlen > avail) return 0;
    u32 bsize = 0, found = 0;
    for (u32 o = 0; o + 4 <= xlen;) {
        const u8 *f = p + 12 + o;
        const u32 sl = (u32)f[2] | ((u32)f[3] << 8);
        if (o + 4 + sl > xlen) return 0;
        if (f[0] == 'B' && f[1] == 'C' && sl == 2) { bsize = (u32)f[4] | ((u32)f[5] << 8); found = 1; break; }
        o += 4 + sl;
    }
    if (!found) return 0;
    const u32 total = bsize + 1;
    if (total < 12 + xlen + 8 || total > avail) return 0;   // too small for header + footer, or the chain runs past the end of the file
    data_off = 12 + xlen;
    return total;
}

}  // namespace lnr_inf
