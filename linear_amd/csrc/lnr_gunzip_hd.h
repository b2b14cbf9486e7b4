// lnr_gunzip_hd.h -- ONE plain gzip member (RFC 1952 around RFC 1951) inflated in parallel, as __host__ __device__ code over plain arrays.
//
// PRODUCT code: the k_gz_* kernels (lnr_reader_kernels.hip) run it on the device; tests/gunzip_hd_shim.cpp compiles the same text with g++
// (tests/test_gunzip_hd_cpu.py: every fixture against zlib at several chunk and round sizes, the finder against zlib's block starts,
// seeded bit flips, the same under the address and undefined-behaviour sanitizers).
//
// A ROUND is a run of compressed bytes with a known start bit, the 32 KiB of text in front of it (the window) and the number of those
// bytes that exist.  It is cut into CHUNKS of compressed bytes.  The method is speculate / verify / repair (pugz, rapidgzip):
//   find      every chunk but the first is searched for the first bit offset that passes is_dynamic_start: a CANDIDATE
//   measure   a piece = the decode from a candidate (chunk 0: from the round's start) to the first block boundary at or past the next
//             candidate, counting only: the size of a block's text does not depend on the history
//   stitch    in order: piece 0 is true; a later piece is true iff a true piece's decode ended exactly on its start.  A true piece that
//             overshoots goes on counting to the next candidate it lands on exactly; the candidates it passed are false
//   emit      every true piece once more, into one u16 per text byte: < 256 a literal, 0x8000 | k "byte k + 1 before this piece's first
//             byte".  A match that copies such symbols copies them unchanged: a piece never needs its history to be decoded
//   chain     pieces in order: the last 32 Ki symbols in front of every piece start are resolved; afterwards every window is final
//   resolve   every other symbol through its piece's window, into bytes
// Nothing rests on a guess: a candidate the chain does not land on contributes nothing, whatever its decode produced.
//
// Like lnr_inf::inflate_block the decoder is TOTAL (it reads only [comp, comp + clen), writes only through its Sink and below the text
// budget, and ends) and wave-uniform; is_dynamic_start is total and lane-local (it uses no LNR_INFLATE_UNIFORM value).
#pragma once
#include "lnr_inflate_hd.h"
#include <stdlib.h>
#include <vector>

namespace lnr_gz {

using lnr_inf::u8; using lnr_inf::u16; using lnr_inf::u32; using lnr_inf::u64;
using lnr_inf::Bits; using lnr_inf::Tables;

constexpr u32 WIN = 32768;                               // DEFLATE's history
constexpr u64 NONE = ~0ULL;                              // no candidate / no stop bit / no text budget
// statuses beyond lnr_inf::Status (status_text below)
constexpr u32 E_HEADER = 20, E_TEXT_CAP = 21, E_LIMIT = 22;
LNR_HD inline const char *status_text(u32 s) {
    switch (s) {
    case E_HEADER: return "not a gzip member header";
    case E_TEXT_CAP: return "the text does not fit the buffer";
    case E_LIMIT: return "a round beyond the staging limit";
    case lnr_inf::E_DISTANCE: return "distance reaches before the member's text";
    case lnr_inf::E_ISIZE: return "text size differs from the trailer's ISIZE";
    case lnr_inf::E_CRC: return "CRC32 differs from the trailer's";
    }
    return lnr_inf::status_text(s);
}

// ---- RFC 1952 member header with any of FEXTRA, FNAME, FCOMMENT, FHCRC.  0: data_off = offset of the DEFLATE data; E_HEADER: not one
// (magic, CM, reserved flag bits); E_INPUT_END: the bytes end inside it.
LNR_HD inline u32 member_header(const u8 *p, u64 avail, u64 *data_off) {
    if (avail < 2) return lnr_inf::E_INPUT_END;
    if (p[0] != 0x1f || p[1] != 0x8b) return E_HEADER;
    if (avail < 10) return lnr_inf::E_INPUT_END;
    if (p[2] != 8 || (p[3] & 0xe0)) return E_HEADER;
    const u32 flg = p[3];
    u64 o = 10;
    if (flg & 4) {                                       // FEXTRA
        if (o + 2 > avail) return lnr_inf::E_INPUT_END;
        o += 2 + ((u64)p[o] | ((u64)p[o + 1] << 8));
        if (o > avail) return lnr_inf::E_INPUT_END;
    }
    for (u32 f = 8; f <= 16; f <<= 1)                    // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (o < avail && p[o]) o++;
            if (o >= avail) return lnr_inf::E_INPUT_END;
            o++;
        }
    if (flg & 2) o += 2;                                 // FHCRC (not checked: gzread does not check it either)
    if (o > avail) return lnr_inf::E_INPUT_END;
    *data_off = o;
    return 0;
}

// ---- the finder's test.  Lane-local: one bit offset per lane on the device, so nothing here is wave-uniform.
// k <= 24 bits at bit offset `bit`; false: they do not lie inside [comp, comp + clen)
LNR_HD inline bool peek(const u8 *comp, u64 clen, u64 bit, u32 k, u32 &v) {
    if (bit + k > clen * 8) return false;
    const u64 by = bit >> 3;
    u32 w = comp[by];
    if (by + 1 < clen) w |= (u32)comp[by + 1] << 8;
    if (by + 2 < clen) w |= (u32)comp[by + 2] << 16;
    if (by + 3 < clen) w |= (u32)comp[by + 3] << 24;
    v = (u32)(((u64)w >> (bit & 7)) & ((1u << k) - 1u));
    return true;
}
// BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, a complete code-length code, lengths that decode within HLIT + HDIST, an end-of-block
// code, a complete literal/length code, a distance code that is complete, single (one code of length 1) or empty.  Completeness is the
// Kraft sum: a code is complete iff the sum of 2^(max - length) over its symbols is 2^max, over-subscribed iff it is more.
LNR_HD inline bool is_dynamic_start(const u8 *comp, u64 clen, u64 bit) {
    u32 h;
    if (!peek(comp, clen, bit, 17, h)) return false;
    if ((h & 7u) != 4u) return false;                    // BFINAL 0, BTYPE 2 (bits 1..2 = 10b, the low bit first)
    const u32 hlit = (h >> 3) & 31u, hdist = (h >> 8) & 31u, ncode = ((h >> 13) & 15u) + 4u;
    if (hlit > 29 || hdist > 29) return false;
    const u32 nlen = hlit + 257, ndist = hdist + 1;
    u64 p = bit + 17;
    // the code-length code: 19 lengths of 3 bits, packed; counts per length, 5 bits each
    u64 cl = 0, cnt = 0;
    u32 kraft = 0;
    for (u32 i = 0; i < ncode; i++) {
        u32 v;
        if (!peek(comp, clen, p, 3, v)) return false;
        p += 3;
        // RFC order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: behind the 0, even places count up from 8, odd ones down from 7
        const u32 s = i < 4 ? (i < 3 ? 16 + i : 0) : ((i & 1) ? 7u - ((i - 5) >> 1) : 8u + ((i - 4) >> 1));
        cl |= (u64)v << (3 * s);
        if (v) { cnt += 1ULL << (5 * v); kraft += 128u >> v; }
    }
    if (kraft != 128) return false;
    u32 i = 0, prev = 0, lsum = 0, dsum = 0, dn = 0, d1 = 0, end_code = 0;
    while (i < nlen + ndist) {
        // one symbol of the code-length code, canonical (lnr_inf::decode with the counts and symbols computed from the packed lengths)
        u32 code = 0, first = 0, l = 1, sym = 19;
        for (; l <= 7; l++) {
            u32 b;
            if (!peek(comp, clen, p, 1, b)) return false;
            p++;
            code |= b;
            const u32 count = (u32)(cnt >> (5 * l)) & 31u;
            if (code < first + count) {                  // the (code - first)-th symbol of length l, in symbol order
                u32 want = code - first;
                for (u32 s = 0; s < 19; s++)
                    if (((cl >> (3 * s)) & 7u) == l) { if (!want) { sym = s; break; } want--; }
                break;
            }
            first = (first + count) << 1; code <<= 1;
        }
        if (sym > 18) return false;
        u32 rep = 1, val = sym;
        if (sym >= 16) {
            u32 x;
            if (sym == 16) { if (i == 0 || !peek(comp, clen, p, 2, x)) return false; p += 2; rep = 3 + x; val = prev; }
            else if (sym == 17) { if (!peek(comp, clen, p, 3, x)) return false; p += 3; rep = 3 + x; val = 0; }
            else { if (!peek(comp, clen, p, 7, x)) return false; p += 7; rep = 11 + x; val = 0; }
            if (i + rep > nlen + ndist) return false;
        }
        prev = val;
        if (val)
            for (u32 r = 0; r < rep; r++) {
                const u32 at = i + r;
                if (at < nlen) { lsum += 32768u >> val; if (at == 256) end_code = 1; }
                else { dsum += 32768u >> val; dn++; d1 += val == 1; }
            }
        i += rep;
        if (lsum > 32768 || dsum > 32768) return false;
    }
    if (!end_code || lsum != 32768) return false;
    return dsum == 32768 || dn == 0 || (dn == 1 && d1 == 1);
}

// ---- the chunk decoder
enum Stop : u32 {
    AT_BOUNDARY = 0,        // the first block boundary at or past stop_bit
    AT_FINAL = 1,           // behind a final block
    AT_INPUT = 2,           // the input ends inside a block: the last completed boundary is reported
    AT_BUDGET = 3,          // the text budget is reached inside a block: the last boundary that fits is reported
    AT_ERROR = 4,           // status says why; the last completed boundary is reported
};
struct Meas { u64 end_bit, text; u32 blocks, stop, status, pad; };

// Sinks take u64 text positions relative to the piece's first byte.  match: the source may lie in front of the piece (dist > pos).
struct CountSink {
    LNR_HD void lit(u64, u8) {}
    LNR_HD void match(u64, u32, u32) {}
    LNR_HD void stored(u64, const u8 *, u32) {}
};
LNR_HD inline u16 sym_copy(const u16 *sym, u64 pos, u32 dist, u32 i) {      // symbol i of a match at pos: byte (i mod dist) of the source
    const u64 back = dist - (dist >= 258 ? i : i % dist);                    // 1 .. dist bytes in front of pos
    return back <= pos ? sym[pos - back] : (u16)(0x8000u | (u32)(back - pos - 1));
}
struct HostSymSink {
    u16 *sym;
    LNR_HD void lit(u64 pos, u8 b) { sym[pos] = b; }
    LNR_HD void match(u64 pos, u32 len, u32 dist) { for (u32 i = 0; i < len; i++) sym[pos + i] = sym_copy(sym, pos, dist, i); }
    LNR_HD void stored(u64 pos, const u8 *src, u32 n) { for (u32 i = 0; i < n; i++) sym[pos + i] = src[i]; }
};

LNR_HD inline u64 bit_pos(const Bits &s) { return (u64)s.ip * 8 - s.n; }

// the length / literal + distance codes of one block; AT_BOUNDARY: the end-of-block code was read
template <class Sink>
LNR_HD inline u32 codes(Bits &s, Sink &o, u64 &pos, u64 budget, const Tables &T, u32 &status) {
    using namespace lnr_inf;
    for (;;) {
        int sym = decode(s, T.lc, T.lsym);
        if (sym < 0) { if (sym == -1) return AT_INPUT; status = E_SYMBOL; return AT_ERROR; }
        if (sym < 256) {
            if (pos >= budget) return AT_BUDGET;
            o.lit(pos, (u8)sym); pos++;
            continue;
        }
        if (sym == 256) return AT_BOUNDARY;
        if (sym > 285) { status = E_SYMBOL; return AT_ERROR; }
        u32 li = (u32)sym - 257, x = 0;
        if (!take(s, len_extra(li), x)) return AT_INPUT;
        const u32 len = len_base(li) + x;
        sym = decode(s, T.dc, T.dsym);
        if (sym < 0) { if (sym == -1) return AT_INPUT; status = E_SYMBOL; return AT_ERROR; }
        if (sym > 29) { status = E_SYMBOL; return AT_ERROR; }
        if (!take(s, dist_extra((u32)sym), x)) return AT_INPUT;
        const u32 dist = dist_base((u32)sym) + x;       // <= 32768; how far it may reach is the resolve's to check
        if (len > budget - pos) return AT_BUDGET;
        o.match(pos, len, dist); pos += len;
    }
}

// Decodes block after block from start_bit.  clen < 2^32; the caller passes stop_bit > start_bit (or NONE).
template <class Sink>
LNR_HD inline Meas decode_chunk(const u8 *comp, u64 clen, u64 start_bit, u64 stop_bit, u64 budget, Sink &o, Tables &T) {
    using namespace lnr_inf;
    Meas m; m.end_bit = start_bit; m.text = 0; m.blocks = 0; m.stop = AT_INPUT; m.status = OK; m.pad = 0;
    if (clen > 0xffffffffULL || (start_bit >> 3) >= clen) return m;
    Bits s; s.c = comp; s.clen = (u32)clen; s.ip = (u32)(start_bit >> 3); s.b = 0; s.n = 0;
    u32 v;
    if ((start_bit & 7) && !take(s, (u32)(start_bit & 7), v)) return m;      // the bits of the first byte in front of the start
    u64 pos = 0;
    for (;;) {
        if (m.end_bit >= stop_bit) { m.stop = AT_BOUNDARY; return m; }
        u32 last, type, st = AT_BOUNDARY;
        if (!take(s, 1, last) || !take(s, 2, type)) return m;
        if (type == 0) {
            u32 len, nlen;
            s.b >>= (s.n & 7); s.n &= ~7u;
            if (!take(s, 16, len) || !take(s, 16, nlen)) return m;
            if (len != (~nlen & 0xFFFFu)) { m.stop = AT_ERROR; m.status = E_STORED_LEN; return m; }
            s.ip -= s.n >> 3; s.b = 0; s.n = 0;
            if (len > s.clen - s.ip) return m;
            if (len > budget - pos) { m.stop = AT_BUDGET; return m; }
            o.stored(pos, s.c + s.ip, len);
            pos += len; s.ip += len;
        } else if (type == 3) { m.stop = AT_ERROR; m.status = E_BLOCK_TYPE; return m; }
        else {
            u32 ts = OK;
            if (type == 1) fixed_tables(T); else ts = dynamic_tables(s, T);
            if (ts == E_INPUT_END) return m;
            if (ts != OK) { m.stop = AT_ERROR; m.status = ts; return m; }
            st = codes(s, o, pos, budget, T, m.status);
        }
        if (st != AT_BOUNDARY) { m.stop = st; return m; }
        m.end_bit = bit_pos(s); m.text = pos; m.blocks++;
        if (last) { m.stop = AT_FINAL; return m; }
    }
}

// ---- chunks of a round.  The round's compressed bytes are [start_bit / 8, clen) of comp; chunk c covers `chunk` bytes from
// start_bit / 8 + c * chunk on.  Chunk 0 holds the round's start and is not searched.
LNR_HD inline u32 chunks_of(u64 start_bit, u64 clen, u64 chunk) { return (start_bit >> 3) >= clen ? 0u : (u32)((clen - (start_bit >> 3) + chunk - 1) / chunk); }
LNR_HD inline void chunk_bits(u64 start_bit, u64 clen, u64 chunk, u32 c, u64 &lo, u64 &hi) {
    const u64 b0 = (start_bit >> 3) + (u64)c * chunk, b1 = b0 + chunk < clen ? b0 + chunk : clen;
    lo = b0 * 8; hi = b1 * 8;
}
// the first chunk at or behind `from` that has a candidate (nchunk: none)
LNR_HD inline u32 next_cand(const u64 *cand, u32 nchunk, u32 from) {
    while (from < nchunk && cand[from] == NONE) from++;
    return from;
}
// the measure of chunk c (c == 0, or cand[c] != NONE)
LNR_HD inline Meas measure_chunk(const u8 *comp, u64 clen, u64 start_bit, const u64 *cand, u32 nchunk, u32 c, Tables &T) {
    const u32 nc = next_cand(cand, nchunk, c + 1);
    CountSink cs;
    return decode_chunk(comp, clen, c ? cand[c] : start_bit, nc < nchunk ? cand[nc] : NONE, NONE, cs, T);
}

// ---- the stitch
struct Piece { u64 start_bit, end_bit, text_off, text; };
struct Round {
    u64 end_bit, text, bad_bit;
    u32 pieces, falses, blocks, stop, status, cands;     // stop: why the last piece ended (never AT_BOUNDARY); status != 0: the piece at bad_bit failed
};                                                       // cands: the finder's candidates in front of end_bit, counted from its array (see stitch_round)
// a round in which nothing was decoded: what a round without a byte is
LNR_HD inline Round empty_round(u64 start_bit) {
    Round R; R.end_bit = start_bit; R.text = 0; R.bad_bit = 0; R.pieces = 0; R.falses = 0; R.blocks = 0; R.stop = AT_INPUT; R.status = lnr_inf::OK; R.cands = 0;
    return R;
}
// `write`: this caller stores the pieces (lane 0 of the wave; the host).  pieces has room for nchunk entries.  A round without a byte
// (nchunk == 0) has no piece and stops AT_INPUT; nothing is read.
// The counts: a candidate in front of the round's end bit is TRUE (a piece's decode ended exactly on it: it starts the next piece) or
// FALSE (it lies inside a piece).  falses is counted piece by piece, cands is counted at the end from the finder's array alone, so
// pieces + falses == cands + 1 is a check of the walk, not a definition.  Candidates at or behind the round's end bit -- behind a final
// block, behind the place where the input or the text cap ended the round -- are neither: the next round finds them again or never needs them.
LNR_HD inline Round stitch_round(const u8 *comp, u64 clen, u64 start_bit, const u64 *cand, const Meas *meas, u32 nchunk, u64 text_cap, Tables &T,
                                 Piece *pieces, bool write) {
    Round R = empty_round(start_bit);
    if (!nchunk) return R;
    u32 cur = 0;
    for (;;) {
        Meas M = meas[cur];
        const u64 pstart = cur ? cand[cur] : start_bit;
        u32 nc = cur + 1, landed = 0;
        while (M.stop == AT_BOUNDARY) {                  // the decode stood on a boundary at or past a candidate: on it, or past it?
            while (nc < nchunk && (cand[nc] == NONE || cand[nc] < M.end_bit)) nc++;
            if (nc < nchunk && cand[nc] == M.end_bit) { landed = 1; break; }
            CountSink cs;
            const Meas X = decode_chunk(comp, clen, M.end_bit, nc < nchunk ? cand[nc] : NONE, NONE, cs, T);
            M.end_bit = X.end_bit; M.text += X.text; M.blocks += X.blocks; M.stop = X.stop; M.status = X.status;
        }
        if (M.text > text_cap - R.text) {                // the round is cut at the text cap: the last boundary of this piece that fits
            CountSink cs;
            M = decode_chunk(comp, clen, pstart, M.end_bit, text_cap - R.text, cs, T);
            if (M.stop != AT_ERROR) M.stop = AT_BUDGET;
            landed = 0;
        }
        for (u32 k = cur + 1; k < nchunk && (cand[k] == NONE || cand[k] < M.end_bit); k++) R.falses += cand[k] != NONE;      // the candidates inside this piece
        if (M.blocks) {
            if (write) { Piece P; P.start_bit = pstart; P.end_bit = M.end_bit; P.text_off = R.text; P.text = M.text; pieces[R.pieces] = P; }
            R.pieces++; R.text += M.text; R.blocks += M.blocks; R.end_bit = M.end_bit;
        }
        R.stop = M.stop;
        if (M.stop == AT_ERROR) { R.status = M.status; R.bad_bit = M.end_bit; }
        if (!landed) break;
        cur = nc;
    }
    for (u32 k = 1; k < nchunk && (cand[k] == NONE || cand[k] < R.end_bit); k++) R.cands += cand[k] != NONE;
    return R;
}

// ---- resolve.  The byte of symbol t of the piece that starts at text offset s: the literal, or text[s - 1 - k], or -- where that lies
// before the round's text -- the byte of the window kept from the round before (win[WIN - 1] is the byte in front of the round; hist of
// its bytes exist).  -1: the reference reaches before the member's first byte.
LNR_HD inline int resolve_sym(const u16 *sym, u64 s, u64 t, const u8 *win, u32 hist) {
    const u32 v = sym[t];
    if (v < 256) return (int)v;
    const u64 back = (u64)(v & 0x7fffu) + 1;
    if (back <= s) return (int)(sym[s - back] & 0xffu);
    return back - s <= hist ? (int)win[WIN - (back - s)] : -1;
}
// the part of a piece the chain pass resolves: what of it lies in the window in front of the next piece's start
LNR_HD inline u64 chain_from(const Piece &P) { const u64 e = P.text_off + P.text; return e > P.text_off + WIN ? e - WIN : P.text_off; }

// a size from the environment (LNR_READER_GZ_ROUND / LNR_READER_GZ_CHUNK), clamped
inline u64 env_bytes(const char *name, u64 dflt, u64 lo, u64 hi) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return end == e ? dflt : v < lo ? lo : v > hi ? hi : (u64)v;
}

// what follows a member's final block: the trailer at the next byte boundary.  0: CRC32 and ISIZE agree
LNR_HD inline u32 check_trailer(const u8 *gz, u64 size, u64 end_bit, u32 crc, u64 text, u64 *next) {
    const u64 t = (end_bit + 7) >> 3;
    if (t + 8 > size) return lnr_inf::E_INPUT_END;
    const u32 c = (u32)gz[t] | ((u32)gz[t + 1] << 8) | ((u32)gz[t + 2] << 16) | ((u32)gz[t + 3] << 24);
    const u32 n = (u32)gz[t + 4] | ((u32)gz[t + 5] << 8) | ((u32)gz[t + 6] << 16) | ((u32)gz[t + 7] << 24);
    *next = t + 8;
    if (c != crc) return lnr_inf::E_CRC;
    return n == (u32)text ? 0u : (u32)lnr_inf::E_ISIZE;
}

// ---- the host driver: every stage serially with the device's chunking (the CPU tests; the yardstick of the stage tests)
struct Stats { u64 rounds, members, chunks, candidates, pieces, falses, blocks, comp_bytes, text_bytes, win_syms, grown; };
struct Scratch { std::vector<u64> cand; std::vector<Meas> meas; std::vector<Piece> pieces; std::vector<u16> syms; };

// one round over [start_bit / 8, clen) of comp: its text at out (room for cap bytes)
inline Round round_host(const u8 *comp, u64 clen, u64 start_bit, u64 chunk, const u8 *win, u32 hist, u8 *out, u64 cap, Scratch &W, Stats &S) {
    Tables T;
    const u32 nchunk = chunks_of(start_bit, clen, chunk);
    if (!nchunk) return empty_round(start_bit);          // not a byte: AT_INPUT
    W.cand.assign(nchunk, NONE); W.meas.resize(nchunk); W.pieces.resize(nchunk);
    for (u32 c = 1; c < nchunk; c++) {                   // find
        u64 lo, hi;
        chunk_bits(start_bit, clen, chunk, c, lo, hi);
        for (u64 b = lo; b < hi; b++) if (is_dynamic_start(comp, clen, b)) { W.cand[c] = b; break; }
    }
    for (u32 c = 0; c < nchunk; c++) if (c == 0 || W.cand[c] != NONE) W.meas[c] = measure_chunk(comp, clen, start_bit, W.cand.data(), nchunk, c, T);
    Round R = stitch_round(comp, clen, start_bit, W.cand.data(), W.meas.data(), nchunk, cap, T, W.pieces.data(), true);
    if (R.status || !R.pieces) return R;
    W.syms.resize(R.text + 1);
    u16 *syms = W.syms.data();
    for (u32 i = 0; i < R.pieces; i++) {                 // emit
        const Piece &P = W.pieces[i];
        HostSymSink o{syms + P.text_off};
        const Meas E = decode_chunk(comp, clen, P.start_bit, P.end_bit, P.text, o, T);
        if (E.end_bit != P.end_bit || E.text != P.text) { R.status = lnr_inf::E_TABLE; R.bad_bit = P.start_bit; return R; }
    }
    for (u32 i = 0; i < R.pieces; i++) {                 // chain
        const Piece &P = W.pieces[i];
        for (u64 t = chain_from(P); t < P.text_off + P.text; t++) {
            const int v = resolve_sym(syms, P.text_off, t, win, hist);
            if (v < 0) { R.status = lnr_inf::E_DISTANCE; R.bad_bit = P.start_bit; return R; }
            S.win_syms += syms[t] >= 256;
            syms[t] = (u16)v;
        }
    }
    for (u32 i = 0; i < R.pieces; i++) {                 // resolve
        const Piece &P = W.pieces[i];
        for (u64 t = P.text_off; t < P.text_off + P.text; t++) {
            const int v = resolve_sym(syms, P.text_off, t, win, hist);
            if (v < 0) { R.status = lnr_inf::E_DISTANCE; R.bad_bit = P.start_bit; return R; }
            S.win_syms += syms[t] >= 256;
            out[t] = (u8)v;
        }
    }
    S.chunks += nchunk; S.pieces += R.pieces; S.falses += R.falses; S.candidates += R.cands; S.blocks += R.blocks;
    S.rounds++;
    return R;
}
// the window behind a round: the last WIN bytes of (old window, round text); how many of them exist is the walker's (Member::hist)
inline void window_after(u8 *win, const u8 *text, u64 n) {
    if (n >= WIN) { for (u32 j = 0; j < WIN; j++) win[j] = text[n - WIN + j]; return; }
    for (u32 j = 0; j + n < WIN; j++) win[j] = win[j + n];
    for (u64 j = 0; j < n; j++) win[WIN - n + j] = text[j];
}
// a member starts at gz + off?  0: yes, *data = offset of its DEFLATE data; PASS_OVER: the bytes behind a member start none and are passed
// over, as gzread does; else the status
constexpr u32 PASS_OVER = ~0u;
inline u32 member_at(const u8 *gz, u64 size, u64 off, bool first, u64 *data) {
    const u32 st = member_header(gz + off, size - off, data);
    if (!st) { *data += off; return 0; }
    if (!first && (st == E_HEADER || size - off < 2)) return PASS_OVER;
    return st;
}

// ---- the member walker: where a driver stands in gz[0, size), and what a round moves.  Every driver (gunzip_host, lnr_rdgpu_gunzip, the
// reader's gzip source) loops: member_enter, a round of member_round_size bytes from start_bit, round_verdict, member_fold.
struct Member {
    bool in_member = false, end = false;                 // start_bit .. mtext are valid; no member starts at pos (or the file ends there)
    u64 pos = 0, start_bit = 0, mtext = 0, grow = 1;     // the next member's header; the member's next bit, in the file; its text so far; the round's factor
    u32 hist = 0, crc = 0;                               // bytes of history in the window; CRC32 of the member's text so far
};
// the member at pos, where the walker stands between two.  0 (then in_member or end holds), or the header's status (at pos)
inline u32 member_enter(Member &m, const u8 *gz, u64 size) {
    if (m.in_member || m.end) return 0;
    u64 data = 0;
    const u32 st = m.pos >= size ? PASS_OVER : member_at(gz, size, m.pos, m.pos == 0, &data);
    if (st) { m.end = st == PASS_OVER; return m.end ? 0 : st; }
    m.in_member = true; m.start_bit = data * 8; m.mtext = 0; m.hist = 0; m.crc = 0;
    return 0;
}
// base compressed bytes per round, times the factor of the rounds that completed no block
inline u64 member_round_size(const Member &m, u64 base) { return base > (1ULL << 31) / m.grow ? 1ULL << 31 : base * m.grow; }
// what a driver does with a round of rsize bytes up to file offset clen that failed or made no progress.  0: go on (grown: the same round
// again, doubled); else the status to report, *bad_off = the compressed offset it belongs to
inline u32 round_verdict(Member &m, const Round &R, u64 clen, u64 size, u64 rsize, bool &grown, u64 *bad_off) {
    grown = false;
    u32 st;
    if (R.status) st = R.status;
    else if (R.stop == AT_BUDGET) st = E_TEXT_CAP;
    else if (R.pieces) return 0;
    else if (clen >= size) st = lnr_inf::E_INPUT_END;    // the file ends inside a block
    else if (rsize >= (1ULL << 31)) st = E_LIMIT;
    else { m.grow *= 2; grown = true; return 0; }
    *bad_off = (R.status ? R.bad_bit : R.end_bit) >> 3;
    return st;
}
// a round with pieces joins the member: its text (CRC32 rcrc), the history, the next bit.  Behind a final block the trailer is checked
// (its status, at *bad_off: the round's text stands, as gzread delivers it) and the walker stands in front of the next member (*final)
inline u32 member_fold(Member &m, const u8 *gz, u64 size, const Round &R, u32 rcrc, bool *final, u64 *bad_off) {
    m.grow = 1;
    m.crc = lnr_inf::crc_combine(m.crc, rcrc, R.text);
    m.hist = m.hist + R.text > WIN ? WIN : (u32)(m.hist + R.text);
    m.mtext += R.text; m.start_bit = R.end_bit;
    *final = false;
    if (R.stop != AT_FINAL) return 0;
    u64 next = 0;
    const u32 st = check_trailer(gz, size, m.start_bit, m.crc, m.mtext, &next);
    if (st) { *bad_off = (m.start_bit + 7) >> 3; return st; }
    m.in_member = false; m.pos = next; *final = true;
    return 0;
}

// every member of gz[0, size): text at out (room for cap bytes).  0 or the status, *bad_off = the compressed offset it belongs to
inline u32 gunzip_host(const u8 *gz, u64 size, u8 *out, u64 cap, u64 *text_size, u64 chunk, u64 round, Stats &S, u64 *bad_off) {
    Scratch W;
    std::vector<u8> win(WIN);
    u64 total = 0;
    *text_size = 0; *bad_off = 0;
    if (size > (1ULL << 31)) return E_LIMIT;
    if (chunk < 1024) chunk = 1024;
    if (round < 1024) round = 1024;
    Member m;
    for (;;) {
        u32 st = member_enter(m, gz, size);
        if (st) { *bad_off = m.pos; return st; }
        if (m.end) break;
        const u64 rsize = member_round_size(m, round), rb = m.start_bit >> 3, clen = size - rb < rsize ? size : rb + rsize;
        const Round R = round_host(gz, clen, m.start_bit, chunk, win.data(), m.hist, out + total, cap - total, W, S);
        bool grown, final;
        if ((st = round_verdict(m, R, clen, size, rsize, grown, bad_off))) return st;
        if (grown) { S.grown++; continue; }
        window_after(win.data(), out + total, R.text);
        *text_size = total += R.text;
        if ((st = member_fold(m, gz, size, R, lnr_inf::crc_of(out + total - R.text, R.text), &final, bad_off))) return st;
        S.members += final;
    }
    S.comp_bytes += size; S.text_bytes += total;
    return 0;
}

}  // namespace lnr_gz
