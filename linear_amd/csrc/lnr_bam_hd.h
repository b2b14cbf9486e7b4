// lnr_bam_hd.h -- every decision of the BAM input path as __host__ __device__ code over plain data: the header span, the 36 fixed bytes of a
// record, which records are valid / delivered / reverse-complemented, the 4-bit code -> Dna5 ordinal table, the take decision, and the
// speculate / verify / repair scheme that finds the record starts of a window in parallel.
//
// PRODUCT code: lnr_reader.cpp (the host reader, the yardstick) and the kernels of lnr_reader_kernels.hip (k_bam_find, k_bam_stitch,
// k_bam_meta, k_bam_emit) call these functions; tests/reader_bam_hd_shim.cpp compiles the same text with g++ and runs the scheme on the
// host at small tile sizes (tests/test_reader_bam_cpu.py).
//
// BAM (SAMv1 4.2), all integers little-endian, behind the BGZF layer:
//   header   "BAM\1", l_text u32, text, n_ref i32, n_ref x { l_name u32, name, l_ref u32 }
//   record   block_size i32, then block_size bytes: refID i32, pos i32, l_read_name u8, mapq u8, bin u16, n_cigar_op u16, flag u16,
//            l_seq i32, next_refID i32, next_pos i32, tlen i32, read_name (NUL-terminated), cigar 4 x n_cigar_op, seq (l_seq + 1) / 2
//            (two bases a byte, first base in the high nibble), qual l_seq, aux to the end of the block
// Records are length-prefixed: record starts form a serial chain p -> p + 4 + block_size.  The chain is found per TILE of the window:
// each tile GUESSES its first start (the first offset that passes rec_plausible = rec_valid, necessary conditions only, so a true start
// always passes) and walks from there; one pass in tile order then carries the TRUE position through the tiles, accepts a tile's walk
// when its guess is the true position and walks the tile again from the true position when it is not.  Exactness never rests on a guess.
#pragma once
#include <stdint.h>

#ifndef LNR_HD
#if defined(__HIPCC__)
#define LNR_HD __host__ __device__
#else
#define LNR_HD
#endif
#endif

namespace lnr_bam {

typedef uint64_t u64;
typedef uint32_t u32;
typedef int32_t i32;
typedef uint8_t u8;

constexpr u32 NONE = 0xFFFFFFFFu;
constexpr u32 HEAD = 36;                       // block_size + the 32 fixed bytes
constexpr u32 MIN_REC = 4 + 33;                // the shortest valid record: the fixed bytes and a name that is its NUL alone
constexpr i32 MAX_BLOCK = 1 << 29;             // block_size stays below this: a record fits the reader's largest window (1 GiB) with room to spare
constexpr u32 F_REVERSE = 0x10, F_SKIP = 0x100 | 0x800;      // reverse strand; secondary / supplementary: not a read of its own

LNR_HD inline u32 le32(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }
LNR_HD inline u32 le16(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8); }

// ---- the header: where the first record starts
struct Header { int status; u64 first, need; i32 n_ref; };     // status 0: first / n_ref hold; 1: at least `need` bytes are needed; -1: not a BAM header
LNR_HD inline bool is_magic(const u8 *b, u64 len) { return len >= 4 && b[0] == 'B' && b[1] == 'A' && b[2] == 'M' && b[3] == 1; }
LNR_HD inline Header header_span(const u8 *b, u64 len) {
    Header h; h.status = 1; h.first = 0; h.need = 12; h.n_ref = 0;
    for (u32 i = 0; i < 4 && i < len; i++) if (b[i] != (u8)("BAM\1"[i])) { h.status = -1; return h; }
    if (len < 12) return h;
    u64 p = 8 + (u64)le32(b + 4);
    h.need = p + 4;
    if (len < h.need) return h;
    const i32 n_ref = (i32)le32(b + p);
    if (n_ref < 0) { h.status = -1; return h; }
    p += 4;
    for (i32 k = 0; k < n_ref; k++) {
        h.need = p + 4;
        if (len < h.need) return h;
        p += 4 + (u64)le32(b + p) + 4;
        h.need = p;
        if (len < h.need) return h;
    }
    h.status = 0; h.first = p; h.n_ref = n_ref;
    return h;
}

// ---- a record's fixed bytes
struct Fields { i32 block_size, refID, pos; u32 l_read_name, n_cigar_op, flag; i32 l_seq, next_refID, next_pos; };
LNR_HD inline Fields rec_fields(const u8 *p) {
    Fields f;
    f.block_size = (i32)le32(p); f.refID = (i32)le32(p + 4); f.pos = (i32)le32(p + 8);
    f.l_read_name = p[12]; f.n_cigar_op = le16(p + 16); f.flag = le16(p + 18);
    f.l_seq = (i32)le32(p + 20); f.next_refID = (i32)le32(p + 24); f.next_pos = (i32)le32(p + 28);
    return f;
}
LNR_HD inline u64 parts_size(const Fields &f) { return 32 + (u64)f.l_read_name + 4ULL * f.n_cigar_op + ((u64)f.l_seq + 1) / 2 + (u64)f.l_seq; }
// the conditions every real record meets.  f = rec_fields of the record's first 36 bytes (wherever the caller keeps them); rec = the record
// in a buffer of which `avail` bytes from its first byte on are there: the name's NUL is looked at only where it lies inside
LNR_HD inline bool fields_valid(const Fields &f, i32 n_ref) {
    return f.l_read_name >= 1 && f.l_seq >= 0 && f.block_size < MAX_BLOCK && f.block_size >= 0 && parts_size(f) <= (u64)f.block_size &&
           f.refID >= -1 && f.refID < n_ref && f.next_refID >= -1 && f.next_refID < n_ref && f.pos >= -1 && f.next_pos >= -1;
}
LNR_HD inline bool rec_valid(const Fields &f, i32 n_ref, const u8 *rec, u64 avail) {
    if (!fields_valid(f, n_ref)) return false;
    const u64 nul = HEAD + f.l_read_name - 1;
    return nul >= avail || rec[nul] == 0;
}
// a GUESS at an arbitrary offset: necessary conditions only
LNR_HD inline bool rec_plausible(const Fields &f, i32 n_ref, const u8 *rec, u64 avail) { return rec_valid(f, n_ref, rec, avail); }

// ---- bases.  SeqAn's char -> Dna5 table on "=ACMGRSVTWYHKDBN": A C G T keep their ordinals, every other code is N
LNR_HD inline u8 nib2ord(u32 nib) { return (u8)((0x4444444344424104ULL >> (4 * (nib & 15))) & 7); }
LNR_HD inline u8 ord_complement(u8 o) { return o < 4 ? (u8)(3 - o) : o; }
LNR_HD inline bool delivered(u32 flag) { return !(flag & F_SKIP); }
LNR_HD inline bool reversed(u32 flag) { return (flag & F_REVERSE) != 0; }
// base j of the delivered read (l bases) from the packed SEQ
LNR_HD inline u8 base_at(const u8 *seq, u64 l, u64 j, bool rev) {
    const u64 s = rev ? l - 1 - j : j;
    const u8 o = nib2ord((s & 1) ? (seq[s >> 1] & 15u) : (u32)(seq[s >> 1] >> 4));
    return rev ? ord_complement(o) : o;
}

// ---- the take: len[] = bases of the delivered records in order; free_ / allowed = bases still free in the block, records still allowed.
// full: a record was left that does not fit; too_big: it is the first of an empty block, so it can never fit (LNR_ERR_LIMIT)
struct Take { u64 n, bases; u32 full, too_big; };
LNR_HD inline Take take(const u32 *len, u64 count, u64 free_, u64 allowed, bool block_empty) {
    Take t; t.n = 0; t.bases = 0;
    while (t.n < count && t.n < allowed && t.bases + len[t.n] <= free_) { t.bases += len[t.n]; t.n++; }
    t.full = t.n < count && t.n < allowed;
    t.too_big = t.full && t.n == 0 && block_empty;
    return t;
}

// ---- the chain.  A walk starts at p and goes on while p lies in front of tend (the tile's end): every step is taken only after rec_valid
// has passed, which implies block_size >= 33, so p strictly increases; the record has to lie whole in front of len (the window's end)
constexpr u32 CH_OK = 0, CH_BAD = 1, CH_CUT = 2;          // left the tile; stands on a record that fails rec_valid; on one the window ends inside
LNR_HD inline u32 slice_cap(u32 tile) { return tile / MIN_REC + 2; }
LNR_HD inline u32 walk(const u8 *text, u64 len, i32 n_ref, u64 &p, u64 tend, u32 *slice, u32 cap, u32 &count, bool store) {
    while (p < tend) {
        if (p + HEAD > len) return CH_CUT;
        const Fields f = rec_fields(text + p);
        if (!rec_valid(f, n_ref, text + p, len - p)) return CH_BAD;
        if (p + 4 + (u64)f.block_size > len) return CH_CUT;
        if (store && count < cap) slice[count] = (u32)p;
        count++;
        p += 4 + (u64)f.block_size;
    }
    return CH_OK;
}
// what a tile's speculation leaves: its guess (offset in the tile, NONE: no plausible offset), the starts it stored, where its walk ended and how
struct Tile { u64 exit; u32 first, count, flag, pad; };
// the guess, one offset after the other (the device tests 64 offsets at a time, lane = offset, with the same rec_plausible)
LNR_HD inline u32 find_first(const u8 *text, u64 len, i32 n_ref, u64 t0, u64 tend) {
    for (u64 p = t0; p < tend && p + HEAD <= len; p++)
        if (rec_plausible(rec_fields(text + p), n_ref, text + p, len - p)) return (u32)(p - t0);
    return NONE;
}
LNR_HD inline Tile speculate(const u8 *text, u64 len, i32 n_ref, u64 t0, u64 tend, u32 first, u32 *slice, u32 cap, bool store) {
    Tile T; T.first = first; T.count = 0; T.flag = CH_OK; T.exit = tend; T.pad = 0;
    if (first != NONE) { u64 p = t0 + first; T.flag = walk(text, len, n_ref, p, tend, slice, cap, T.count, store); T.exit = p; }
    return T;
}
// verify and repair: p = the true position, inside the tile [t0, tend).  Returns the flag of the walk that stands; p moves to its end,
// count = the starts of the tile, repaired is raised when the tile's own walk could not be used
LNR_HD inline u32 stitch_tile(const u8 *text, u64 len, i32 n_ref, u64 &p, u64 t0, u64 tend, const Tile &T, u32 *slice, u32 cap, u32 &count, u32 &repaired, bool store) {
    if (T.first != NONE && t0 + T.first == p && (T.flag != CH_OK || T.exit >= tend)) { count = T.count; p = T.exit; return T.flag; }
    repaired++;
    count = 0;
    return walk(text, len, n_ref, p, tend, slice, cap, count, store);
}

// ---- per record, what the take and the emit need (16 bytes; the only record data that goes back to the host)
struct Meta { u32 off, l_seq, flag_name, n_cigar; };      // window offset of the record; flag | l_read_name << 16
LNR_HD inline Meta meta_of(u32 off, const Fields &f) { Meta m; m.off = off; m.l_seq = (u32)f.l_seq; m.flag_name = f.flag | (f.l_read_name << 16); m.n_cigar = f.n_cigar_op; return m; }

}  // namespace lnr_bam
