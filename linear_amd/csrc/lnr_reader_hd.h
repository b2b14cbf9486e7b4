// lnr_reader_hd.h -- the per-byte logic of the reader's GPU twin (lnr_reader_next_dev) as __host__ __device__ code over plain data.
//
// PRODUCT code: the kernels of lnr_reader_kernels.hip call these functions on the device; tests/reader_hd_shim.cpp compiles the same text
// with g++ and runs measure / scan / emit tile by tile on the host (tests/test_reader_hd_cpu.py).  The mapped parser of lnr_reader.cpp is
// the specification: same records, same ordinals, same header spans, same hand-over point.
//
// A WINDOW is a run of text bytes that starts at the first byte of a record ('>' or '@').  It is cut into TILES; a tile is walked in
// GROUPS of 64 bytes, lane = byte.  Everything here works on the 64-bit masks of a group (on the device: wave ballots) and on a small
// carried state, so the code below is scalar (wave-uniform) and identical on both sides.
//   FASTA  a record starts at a '>' at a line start (window offset 0 or after '\n'); its header runs to the first '\n'; every later
//          byte that is not '\n', '\r', blank or tab is a base.
//   FASTQ  four-line form: with l = number of '\n' before a byte, record k = lines 4k .. 4k+3; line 4k starts with '@', line 4k+2 with
//          '+', lines 4k+1 and 4k+3 hold no blank, tab or inner '\r' and have the same length once trailing '\r' are dropped.  The
//          first record that breaks this is the HAND-OVER point: nothing from there on is consumed, the serial parser goes on there.
// A tile does not know the line number it starts at, so its FASTQ summary is kept for all four phases (line number mod 4) at once:
// byte counts per local line residue, the first record end and the first offending line per phase.  Sum + sum_combine form a monoid:
// tiles combine in any grouping.
#pragma once
#include <stdint.h>

#ifndef LNR_HD
#if defined(__HIPCC__)
#define LNR_HD __host__ __device__
#else
#define LNR_HD
#endif
#endif

namespace lnr_rd {

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

constexpr u32 NONE = 0xFFFFFFFFu;
constexpr int FASTA = 1, FASTQ = 2;

LNR_HD inline bool is_ws(u8 c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t'; }
LNR_HD inline u8 ordinal(u8 c) {          // SeqAn's char -> Dna5 table
    c |= 0x20;
    return c == 'a' ? 0 : c == 'c' ? 1 : c == 'g' ? 2 : (c == 't' || c == 'u') ? 3 : 4;
}
LNR_HD inline u32 popc(u64 m) { return (u32)__builtin_popcountll(m); }
LNR_HD inline u32 ctz(u64 m) { return (u32)__builtin_ctzll(m); }
LNR_HD inline u64 below(u32 lane) { return (1ULL << lane) - 1ULL; }

// four small counters indexed by a runtime residue, written so that they stay in registers on the device
LNR_HD inline u32 get4(const u32 *a, u32 r) { return r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3]; }
LNR_HD inline void add4(u32 *a, u32 r, u32 v) { a[0] += r == 0 ? v : 0; a[1] += r == 1 ? v : 0; a[2] += r == 2 ? v : 0; a[3] += r == 3 ? v : 0; }
LNR_HD inline void set4(u32 *a, u32 r, u32 v) { a[0] = r == 0 ? v : a[0]; a[1] = r == 1 ? v : a[1]; a[2] = r == 2 ? v : a[2]; a[3] = r == 3 ? v : a[3]; }
LNR_HD inline void min4(u32 *a, u32 r, u32 v) { u32 c = get4(a, r); if (v < c) set4(a, r, v); }

// ---- the associative summary of a run of tiles.  Positions are window offsets + 1 (0 = none).
struct Sum {
    u64 kept;                   // FASTA: bases, counted as if the run started outside a header
    u64 last_rs1, last_nl1;     // last record start (FASTA) / last '\n'
    u32 recs, nl;               // record starts (FASTA), newlines
    u32 head_kept;              // FASTA: bases before the first line start of the run -- header bytes if the run before ends inside a header
    u32 ls_res;                 // FASTQ: bit r = a line whose local number is r mod 4 starts in the run
    u32 cnt[4];                 // FASTQ: bytes other than '\r' / '\n' per local line residue
    u32 fe_l[4], fe_w[4];       // FASTQ, per phase: local line and (sequence - quality) byte balance of the first record end
    u32 badmin[4];              // FASTQ, per phase: first local line that breaks the four-line form (NONE: none)
    u32 fe_has;                 // bit phase
};
LNR_HD inline Sum sum_identity() {
    Sum s;
    s.kept = 0; s.last_rs1 = 0; s.last_nl1 = 0; s.recs = 0; s.nl = 0; s.head_kept = 0; s.ls_res = 0; s.fe_has = 0;
    for (int i = 0; i < 4; i++) { s.cnt[i] = 0; s.fe_l[i] = 0; s.fe_w[i] = 0; s.badmin[i] = NONE; }
    return s;
}
// FASTA, how a run ends: 1 inside a header, 0 outside, 2 as the run before it ended (no line start in the run)
LNR_HD inline u32 sum_end(const Sum &s) { return (s.last_rs1 == 0 && s.last_nl1 == 0) ? 2u : (s.last_rs1 > s.last_nl1 ? 1u : 0u); }
LNR_HD inline u32 sum_wtot(const Sum &s, u32 ph) { return get4(s.cnt, (1 - ph) & 3) - get4(s.cnt, (3 - ph) & 3); }

LNR_HD inline Sum sum_combine(const Sum &A, const Sum &B) {
    Sum C;
    const u32 ea = sum_end(A), s = A.nl & 3;
    C.kept = A.kept + B.kept - (ea == 1 ? B.head_kept : 0);
    C.head_kept = A.head_kept + (ea == 2 ? B.head_kept : 0);
    C.last_rs1 = B.last_rs1 ? B.last_rs1 : A.last_rs1;
    C.last_nl1 = B.last_nl1 ? B.last_nl1 : A.last_nl1;
    C.recs = A.recs + B.recs; C.nl = A.nl + B.nl;
    C.ls_res = A.ls_res | (((B.ls_res << s) | (B.ls_res >> (4 - s))) & 15u);
    C.fe_has = 0;
    for (u32 r = 0; r < 4; r++) C.cnt[r] = A.cnt[r] + B.cnt[(r - s) & 3];
    for (u32 ph = 0; ph < 4; ph++) {
        const u32 pb = (ph + s) & 3;
        u32 bm = A.badmin[ph];
        if (B.badmin[pb] != NONE && A.nl + B.badmin[pb] < bm) bm = A.nl + B.badmin[pb];
        const bool ha = (A.fe_has >> ph) & 1, hb = (B.fe_has >> pb) & 1;
        const u32 wb = sum_wtot(A, ph) + B.fe_w[pb];        // B's first record end, seen from the start of A
        C.fe_l[ph] = A.fe_l[ph]; C.fe_w[ph] = A.fe_w[ph];
        if (ha) { C.fe_has |= 1u << ph; if (hb && wb != A.fe_w[ph] && A.nl + B.fe_l[pb] < bm) bm = A.nl + B.fe_l[pb]; }
        else if (hb) { C.fe_has |= 1u << ph; C.fe_l[ph] = A.nl + B.fe_l[pb]; C.fe_w[ph] = wb; }
        else { C.fe_l[ph] = 0; C.fe_w[ph] = 0; }
        C.badmin[ph] = bm;
    }
    return C;
}

// ---- group masks.  FASTA uses nl, gt ('>'), keep (not white space); FASTQ uses nl, keep (neither '\r' nor '\n') and, to measure, the three
// offence masks.  Bits of bytes past the end of the window are clear in `valid` and in every other mask.
struct Masks { u64 valid, nl, gt, keep, wsbad, notat, notplus; };
// one byte's share of the masks; prev = the byte before it ('\n' at window offset 0)
LNR_HD inline u32 byte_bits(int fmt, u8 c, u8 prev) {
    u32 b = 1u | (c == '\n' ? 2u : 0u);
    if (fmt == FASTA) return b | (c == '>' ? 4u : 0u) | (!is_ws(c) ? 8u : 0u);
    b |= (c != '\n' && c != '\r') ? 8u : 0u;
    b |= (c == ' ' || c == '\t' || (prev == '\r' && c != '\r' && c != '\n')) ? 16u : 0u;
    return b | (c != '@' ? 32u : 0u) | (c != '+' ? 64u : 0u);
}
struct Out { u64 base, rs, hdr; };      // per group: bases of the output, record starts, bytes of header lines (their '\n' included)

// the segment of `rest` up to and including its first '\n'
LNR_HD inline u64 segment(u64 rest, u64 nl, u64 &endbit) {
    const u64 nlm = nl & rest;
    endbit = nlm & (0 - nlm);
    return endbit ? (rest & ((endbit << 1) - 1ULL)) : rest;
}

// FASTA walk, used to measure (st starts at 2 unless the tile begins a line) and to emit (st, recs, kept carried in)
struct FaState { u64 kept, last_rs1, last_nl1; u32 recs, nl, head_kept, st, ls; };
LNR_HD inline FaState fa_begin(bool line_start, u32 st, u64 kept, u32 recs) {
    FaState s;
    s.kept = kept; s.last_rs1 = 0; s.last_nl1 = 0; s.recs = recs; s.nl = 0; s.head_kept = 0; s.st = st; s.ls = line_start ? 1u : 0u;
    return s;
}
LNR_HD inline void fa_step(FaState &s, const Masks &m, u64 pos0, Out &o) {
    o.base = 0; o.rs = 0; o.hdr = 0;
    u64 rest = m.valid;
    while (rest) {
        const u64 first = rest & (0 - rest);
        u64 endbit;
        const u64 seg = segment(rest, m.nl, endbit);
        if (s.ls) {
            s.ls = 0;
            if (m.gt & first) { s.st = 1; s.recs++; s.last_rs1 = pos0 + ctz(first) + 1; o.rs |= first; }
            else s.st = 0;
        }
        const u64 k = m.keep & seg;
        if (s.st == 1) o.hdr |= seg;
        else { o.base |= k; s.kept += popc(k); if (s.st == 2) s.head_kept += popc(k); }
        if (endbit) { s.nl++; s.last_nl1 = pos0 + ctz(endbit) + 1; s.ls = 1; }
        rest &= ~seg;
    }
}
LNR_HD inline Sum fa_sum(const FaState &s) {
    Sum r = sum_identity();
    r.kept = s.kept; r.last_rs1 = s.last_rs1; r.last_nl1 = s.last_nl1; r.recs = s.recs; r.nl = s.nl; r.head_kept = s.head_kept;
    return r;
}

// FASTQ, measuring: the local line number starts at 0 whatever the true one is
struct FqState { Sum s; u32 l, ls; };
LNR_HD inline FqState fq_begin(bool line_start) { FqState q; q.s = sum_identity(); q.l = 0; q.ls = line_start ? 1u : 0u; return q; }
LNR_HD inline void fq_measure_step(FqState &q, const Masks &m, u64 pos0) {
    u64 rest = m.valid;
    while (rest) {
        const u64 first = rest & (0 - rest);
        u64 endbit;
        const u64 seg = segment(rest, m.nl, endbit);
        const u32 r = q.l & 3;
        if (q.ls) {
            q.ls = 0;
            q.s.ls_res |= 1u << r;
            if (m.notat & first) min4(q.s.badmin, (0 - r) & 3, q.l);          // the phase under which this line is a header line
            if (m.notplus & first) min4(q.s.badmin, (2 - r) & 3, q.l);
        }
        if (m.wsbad & seg) { min4(q.s.badmin, (1 - r) & 3, q.l); min4(q.s.badmin, (3 - r) & 3, q.l); }
        add4(q.s.cnt, r, popc(m.keep & seg));
        if (endbit) {
            const u32 ph = (3 - r) & 3;                                         // the phase under which this '\n' ends a record
            const u32 v = get4(q.s.cnt, (r + 2) & 3) - get4(q.s.cnt, r);
            if (!((q.s.fe_has >> ph) & 1)) { q.s.fe_has |= 1u << ph; set4(q.s.fe_l, ph, q.l); set4(q.s.fe_w, ph, v); }
            else if (v != get4(q.s.fe_w, ph)) min4(q.s.badmin, ph, q.l);
            q.s.nl++; q.s.last_nl1 = pos0 + ctz(endbit) + 1;
            q.l++; q.ls = 1;
        }
        rest &= ~seg;
    }
}
// FASTQ, emitting: l is the true line number
struct FqEmit { u64 kept; u32 l, ls; };
LNR_HD inline void fq_emit_step(FqEmit &s, const Masks &m, Out &o) {
    o.base = 0; o.rs = 0; o.hdr = 0;
    u64 rest = m.valid;
    while (rest) {
        const u64 first = rest & (0 - rest);
        u64 endbit;
        const u64 seg = segment(rest, m.nl, endbit);
        const u32 t = s.l & 3;
        if (s.ls) { s.ls = 0; if (t == 0) o.rs |= first; }
        if (t == 0) o.hdr |= seg;
        if (t == 1) { const u64 k = m.keep & seg; o.base |= k; s.kept += popc(k); }
        if (endbit) { s.l++; s.ls = 1; }
        rest &= ~seg;
    }
}

// ---- the decision of the scan
struct Limits { int fmt; u32 eof; u64 len; u64 allowed, free; };      // records still allowed, bases still free in the block
struct Plan {
    u64 hrec;          // first record at or after the hand-over point (~0: none)
    u64 allowed;       // min(allowed, hrec): a record START with this index or less may end the take
    u64 total_real;    // record starts in the window
    u64 total_kept;    // bases before the end of the window
};
LNR_HD inline u64 sum_kept(int fmt, const Sum &s) { return fmt == FASTA ? s.kept : s.cnt[1]; }
LNR_HD inline Plan plan_of(const Limits &L, const Sum &G) {
    Plan p;
    p.hrec = ~0ULL;
    p.total_kept = sum_kept(L.fmt, G);
    if (L.fmt == FASTA) p.total_real = G.recs;
    else {
        u32 h = G.badmin[0];
        if ((G.fe_has & 1) && G.fe_w[0] != 0 && G.fe_l[0] < h) h = G.fe_l[0];
        const bool partial = G.last_nl1 != L.len;                              // bytes after the last '\n'
        if (L.eof) {                                                           // the last record may lack its final '\n', nothing else
            const u32 lf = G.nl, t = lf & 3;
            const bool bad = t == 0 ? partial : t == 3 ? sum_wtot(G, 0) != 0 : true;
            if (bad && lf < h) h = lf;
        }
        if (h != NONE) p.hrec = h / 4;
        p.total_real = (u64)(partial ? G.nl : G.nl - 1) / 4 + 1;
    }
    p.allowed = L.allowed < p.hrec ? L.allowed : p.hrec;
    return p;
}
// what the scan hands each tile: the state at its first byte
struct Carry { u64 kept; u32 rec, nl, st, pad; };
LNR_HD inline Carry carry_of(const Sum &S) {
    Carry c; c.kept = S.kept; c.rec = S.recs; c.nl = S.nl; c.st = sum_end(S) == 1 ? 1u : 0u; c.pad = 0;
    return c;
}
// may a record start inside tile `t` (summary T, prefix S before it) end the take?  (its own starts are looked at one by one later)
LNR_HD inline bool tile_candidate(const Limits &L, const Plan &p, const Sum &S, const Sum &T) {
    if (sum_kept(L.fmt, S) > L.free) return false;
    if (L.fmt == FASTA) return S.recs <= p.allowed && T.recs > 0;
    return (u64)S.nl <= 4 * p.allowed && ((T.ls_res >> ((4 - (S.nl & 3)) & 3)) & 1);
}
struct Take { u64 n, bases; u32 found; };
// record starts of one group against the limits; rec0 / kept0 = record starts and bases before the group (FASTQ: rec index of lane = line / 4)
LNR_HD inline void take_group(const Limits &L, const Plan &p, const Out &o, const Masks &m, u64 rec0, u32 line0, u64 kept0, Take &t) {
    for (u64 rs = o.rs; rs; rs &= rs - 1) {
        const u32 lane = ctz(rs);
        const u64 i = L.fmt == FASTA ? rec0 + popc(o.rs & below(lane)) : (u64)(line0 + popc(m.nl & below(lane))) / 4;
        const u64 kb = kept0 + popc(o.base & below(lane));
        if (i <= p.allowed && kb <= L.free) { t.n = i; t.bases = kb; t.found = 1; }
    }
}
struct Result { u64 n, bases, consumed; u32 handover, full, too_big, pad; };
// t = the last real record start that may end the take (always found: record start 0); the end of the file is one more
LNR_HD inline Result result_of(const Limits &L, const Plan &p, Take t) {
    Result r;
    r.consumed = ~0ULL;                                   // the emit kernel writes the position of record start n
    if (L.eof && p.total_real <= p.allowed && p.total_kept <= L.free) { t.n = p.total_real; t.bases = p.total_kept; r.consumed = L.len; }
    r.n = t.n; r.bases = t.bases;
    r.handover = p.hrec != ~0ULL && t.n == p.hrec;
    const bool next_exists = t.n + 1 < p.total_real || (L.eof && t.n + 1 == p.total_real);
    r.full = !r.handover && t.n < p.allowed && next_exists;
    r.too_big = r.full && t.n == 0;
    r.pad = 0;
    return r;
}

}  // namespace lnr_rd
