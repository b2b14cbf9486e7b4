// lnr_deflate_hd.h -- ONE block of at most 0xff00 text bytes -> one complete BGZF member (18-byte header with the 'BC' subfield, raw
// DEFLATE data, CRC32, ISIZE), as __host__ __device__ code over plain arrays.  The companion of lnr_inflate_hd.h, whose CRC32 it uses.
//
// PRODUCT code: k_bgzf_deflate (lnr_output_kernels.hip) runs deflate_member on the device, one workgroup per block;
// tests/deflate_hd_shim.cpp compiles the same text with g++ (tests/test_deflate_hd_cpu.py: every member against zlib and against
// lnr_inf::inflate_block, the same under the address and undefined-behaviour sanitizers).
//
// The work is a sequence of PHASES over a team of T.nt lanes, lane T.tid of them running this code; a phase is a loop
// `for (i = T.tid; i < n; i += T.nt)` (or a contiguous range per lane) whose iterations do not depend on one another, and T.sync() stands
// between phases.  Where lanes meet in memory they do so through T.amax / T.aadd / T.aor / T.axor, which commute, so a phase leaves the
// same bytes whatever order its iterations ran in.  The host is a team of one lane (HostTeam: sync is nothing, the four operations are
// plain); the device team is the workgroup.  Hence the member is a function of the text alone, and the same on both sides.
//   0 costs     a histogram of the block's bytes (aadd) gives every byte value a price in bits, about log2(n / count): what a literal will cost.
//   1 matches   LZ77 with one candidate per bucket: a table of 2^14 buckets indexed by a hash of 4 bytes holds the highest earlier
//               position that hashed there.  The text is taken in chunks (CHUNK positions; shorter ones at the start): every position of a chunk looks its bucket up (the table then
//               holds positions of EARLIER chunks only), verifies the candidate byte by byte (length 4 .. 258, distance 1 .. 32768, never
//               before the block's first byte) and notes (length, distance) when the literals it replaces are priced above an estimate of the match's
//               own bits (10 + the distance's extra bits: random DNA at 2 bits a base keeps its literals); then the chunk's positions enter the table, the highest
//               position winning a bucket (amax).  One lookup per position: a run of one byte costs its compares, linear in the text.
//   2 parse     greedy: a position that holds a match starts one and skips its length.  Positions inside a token are marked SKIP.  The
//               walk is a chain, done by one wave on the device (T.parse), by a loop on the host; both mark the same positions.
//   3 histogram literal/length and distance symbols of the tokens (aadd), plus the end-of-block symbol.
//   4 codes     lane 0: Huffman code lengths from the histograms, limited to 15 bits (7 for the code-length code) -- symbols ranked by
//               (count, symbol) by all lanes, the two-queue merge, depths clamped, the Kraft sum repaired, lengths dealt out by rank --
//               the code-length sequence with the run symbols 16/17/18, canonical codes, the size of the dynamic block in bits.  At
//               least two distance codes are always sent (two of length 1 when the block has no or one distance symbol), and the
//               length/literal code has the end symbol and a literal, so every code sent is complete: zlib and inflate_block accept it.
//   5 bits      every lane sums the bits of the tokens of its range of positions, an exclusive scan over the lanes gives each range its
//               bit position, and the lanes OR their tokens' codes into the (zeroed) member image (aor).
//   6 frame     header, footer (CRC32 from per-lane slices combined with lnr_inf::crc_shift, axor), or -- when the dynamic block would
//               not be smaller than isize + 5 bytes -- one stored block.  A member is at most isize + 31 and at most 65536 bytes.
// The member image `out` is the caller's (LDS on the device) and is written inside [out, out + member size rounded up to 4) only, which
// lies inside MEMBER_CAP; the caller copies it to its slot.
#pragma once
#include <stdint.h>

#include "lnr_inflate_hd.h"

namespace lnr_def {

using lnr_inf::u8;
using lnr_inf::u16;
using lnr_inf::u32;
using lnr_inf::u64;

constexpr u32 BLOCK_TEXT = 0xff00;             // text bytes of a BGZF block
constexpr u32 MEMBER_CAP = 65536;              // bytes of a member image / slot
constexpr u32 HASH_BITS = 14, HASH_SIZE = 1u << HASH_BITS;
constexpr u32 CHUNK = 512;                     // positions that look up before they enter the table
constexpr u32 MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr u32 SKIP = 0xFFFFFFFFu;              // tok[i]: position i lies inside a token
constexpr u32 NL = 286, ND = 30, NC = 19;
constexpr u32 MAX_LANES = 1024;

// tok[i] = length (0: literal) | (distance - 1) << 16, or SKIP
LNR_HD inline u32 tok_len(u32 t) { return t & 0xFFFFu; }
LNR_HD inline u32 tok_dist(u32 t) { return (t >> 16) + 1; }

LNR_HD inline u32 len_sym(u32 len) {           // 3 .. 258 -> 0 .. 28 (symbol - 257)
    if (len == 258) return 28;
    const u32 v = len - 3;
    if (v < 8) return v;
    u32 hb = 31 - (u32)__builtin_clz(v);
    return 4 * (hb - 1) + ((v >> (hb - 2)) & 3);
}
LNR_HD inline u32 dist_sym(u32 dist) {         // 1 .. 32768 -> 0 .. 29
    const u32 v = dist - 1;
    if (v < 4) return v;
    u32 hb = 31 - (u32)__builtin_clz(v);
    return 2 * hb + ((v >> (hb - 1)) & 1);
}

// the order the code-length code's lengths are sent in (RFC 1951 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, from a constant
LNR_HD inline u32 cl_order(u32 i) {
    return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? (19 - i) / 2 : (12 + i) / 2;
}

struct Work {                                  // one team's work space besides text, table / member image and tokens
    u32 lfreq[NL + 2], dfreq[ND + 2], cfreq[NC + 1];
    u8 llen[NL + 2], dlen[ND + 2], clen[NC + 1];
    u16 lcode[NL + 2], dcode[ND + 2], ccode[NC + 1];
    u16 rank[NL + 2];                          // build_lengths: rank of a symbol among the active ones, then scratch
    u16 order[NL + 2];                         // active symbols, ascending by (count, symbol)
    u32 weight[NL + 2];                        // internal nodes of the merge
    u16 lpar[NL + 2], ipar[NL + 2];            // parent (internal node index) of leaf k of `order` / of internal node k
    u8 idepth[NL + 2];
    u32 cnt[17], next[16];                     // codes per length / next code of a length (here, not on a lane's stack: lane 0 works in LDS)
    u8 seq[NL + ND + 4];                       // code lengths in the order sent
    u8 rsym[NL + ND + 4], rext[NL + ND + 4];   // ... as code-length symbols and their extra values
    u32 nrle, nlen, ndist, ncode;
    u32 lane_bits[MAX_LANES + 1];
    u32 crc;
    u32 bfreq[256];                            // phase 0: count per byte value
    u8 cost[256];                              // ... and its price in bits, 1 .. 15
    u32 dyn_bits;                              // bits of the dynamic block, header and end symbol included
    u32 head_bits;                             // bits before the first token
};

struct HostTeam {
    u32 tid = 0, nt = 1;
    LNR_HD void sync() {}
    LNR_HD void amax(u32 *p, u32 v) { if (v > *p) *p = v; }
    LNR_HD void aadd(u32 *p, u32 v) { *p += v; }
    LNR_HD void aor(u32 *p, u32 v) { *p |= v; }
    LNR_HD void axor(u32 *p, u32 v) { *p ^= v; }
    LNR_HD void parse(u32 *tok, u32 n) {
        for (u32 p = 0; p < n;) {
            const u32 l = tok_len(tok[p]);
            for (u32 i = 1; i < l; i++) tok[p + i] = SKIP;
            p += l ? l : 1;
        }
    }
};

LNR_HD inline u32 hash4(const u8 *p) {
    const u32 w = (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24);
    return (w * 2654435761u) >> (32 - HASH_BITS);
}

// phase 1.  tab: HASH_SIZE words, value = position + 1, 0 = empty
template <class Team>
LNR_HD inline void find_matches(Team &T, Work &W, const u8 *txt, u32 n, u32 *tab, u32 *tok) {
    for (u32 i = T.tid; i < HASH_SIZE; i += T.nt) tab[i] = 0;
    for (u32 i = T.tid; i < 256; i += T.nt) W.bfreq[i] = 0;
    T.sync();
    for (u32 i = T.tid; i < n; i += T.nt) T.aadd(&W.bfreq[txt[i]], 1);
    T.sync();
    for (u32 i = T.tid; i < 256; i += T.nt) {          // floor(log2(1.5 n / count)): log2(n / count) rounded, 1 .. 15
        const u32 f = W.bfreq[i];
        u32 c = 15;
        if (f) { const u32 x = (3 * n) / (2 * f); c = x < 2 ? 1 : 31 - (u32)__builtin_clz(x); if (c > 15) c = 15; }
        W.cost[i] = (u8)c;
    }
    T.sync();
    for (u32 c0 = 0, c1; c0 < n; c0 = c1) {            // chunks of 64, 64, 128, 256, then CHUNK positions: a short text finds its repeats too
        const u32 step = c0 >= CHUNK ? CHUNK : c0 < 64 ? 64 : c0;
        c1 = c0 + step < n ? c0 + step : n;
        for (u32 i = c0 + T.tid; i < c1; i += T.nt) {
            u32 t = 0;
            if (i + MIN_MATCH <= n) {
                const u32 cand = tab[hash4(txt + i)];
                if (cand && i - (cand - 1) <= MAX_DIST) {
                    const u32 j = cand - 1, cap = n - i < MAX_MATCH ? n - i : MAX_MATCH;
                    u32 l = 0, worth = 0;
                    while (l < cap && txt[j + l] == txt[i + l]) { worth += W.cost[txt[i + l]]; l++; }
                    const u32 d1 = i - j - 1;                      // distance - 1
                    const u32 price = 10 + (d1 >= 4 ? 30 - (u32)__builtin_clz(d1) : 0u);
                    if (l >= MIN_MATCH && worth > price) t = l | (d1 << 16);
                }
            }
            tok[i] = t;
        }
        T.sync();
        for (u32 i = c0 + T.tid; i < c1; i += T.nt)
            if (i + MIN_MATCH <= n) T.amax(&tab[hash4(txt + i)], i + 1);
        T.sync();
    }
}

// Code lengths of at most `limit` bits for the symbols with freq != 0 (at least two of them), by all lanes + lane 0.  Complete code.
template <class Team>
LNR_HD inline void build_lengths(Team &T, Work &W, const u32 *freq, u32 n, u32 limit, u8 *len) {
    // rank among the active symbols by (count, symbol): all lanes
    for (u32 s = T.tid; s < n; s += T.nt) {
        u32 r = 0;
        const u32 f = freq[s];
        if (f) for (u32 o = 0; o < n; o++) { const u32 g = freq[o]; r += (g != 0 && (g < f || (g == f && o < s))); }
        W.rank[s] = (u16)r;
        len[s] = 0;
    }
    T.sync();
    if (T.tid == 0) {
        u32 m = 0;
        for (u32 s = 0; s < n; s++) if (freq[s]) { W.order[W.rank[s]] = (u16)s; m++; }
        if (m < 2) { if (m) len[W.order[0]] = 1; }     // (an empty block: it is stored, the code is not sent)
        else {
        // two-queue merge: leaves ascending in `order`, internal nodes ascending as they are made
        u32 li = 0, ii = 0, made = 0;
        while (made + 1 < m) {
            u32 w = 0;
            for (int k = 0; k < 2; k++) {
                const bool leaf = li < m && (ii >= made || freq[W.order[li]] <= W.weight[ii]);
                if (leaf) { w += freq[W.order[li]]; W.lpar[li++] = (u16)made; }
                else { w += W.weight[ii]; W.ipar[ii++] = (u16)made; }
            }
            W.weight[made++] = w;
        }
        // depths from the root (the last node made) down, leaf depths clamped and counted
        u32 *cnt = W.cnt;
        for (u32 l = 0; l <= 16; l++) cnt[l] = 0;
        W.idepth[made - 1] = 0;
        for (u32 k = made - 1; k-- > 0;) { const u32 d = W.idepth[W.ipar[k]] + 1u; W.idepth[k] = (u8)(d > 15 ? 15 : d); }
        for (u32 k = 0; k < m; k++) { u32 d = W.idepth[W.lpar[k]] + 1u; if (d > limit) d = limit; cnt[d]++; }
        // Kraft sum in units of 2^-limit: down to 2^limit by pushing leaves one level deeper, deepest first (smallest steps) ...
        u32 K = 0;
        const u32 full = 1u << limit;
        for (u32 l = 1; l <= limit; l++) K += cnt[l] << (limit - l);
        while (K > full) {
            u32 l = limit - 1;
            while (cnt[l] == 0) l--;
            cnt[l]--; cnt[l + 1]++;
            K -= 1u << (limit - l - 1);
        }
        // ... and back up to it exactly where a step went past: the largest step that fits, shallowest first
        while (K < full) {
            const u32 d = full - K;
            u32 l = 2;
            while (l <= limit && !(cnt[l] && (1u << (limit - l)) <= d)) l++;
            if (l > limit) break;              // (cannot happen: d is a multiple of the deepest leaf's unit)
            cnt[l]--; cnt[l - 1]++;
            K += 1u << (limit - l);
        }
        // the longest lengths to the rarest symbols
        u32 k = 0;
        for (u32 l = limit; l >= 1; l--) for (u32 c = cnt[l]; c; c--) len[W.order[k++]] = (u8)l;
        }
    }
    T.sync();
}

// canonical codes, bit-reversed so that they go out lowest bit first: lane 0
LNR_HD inline void assign_codes(Work &W, const u8 *len, u32 n, u16 *code) {
    u32 *cnt = W.cnt, *next = W.next;
    for (u32 l = 0; l < 16; l++) cnt[l] = 0;
    for (u32 s = 0; s < n; s++) cnt[len[s]]++;
    cnt[0] = 0;
    u32 c = 0;
    for (u32 l = 1; l < 16; l++) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
    for (u32 s = 0; s < n; s++) {
        const u32 l = len[s];
        if (!l) { code[s] = 0; continue; }
        u32 v = next[l]++;                     // 16 bits reversed, then the top l of them
        v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
        v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
        v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
        v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
        code[s] = (u16)(v >> (16 - l));
    }
}

struct BitOut {                                // ORs bits into 32-bit words of the (zeroed) image
    u32 *words; u32 pos;                       // pos = bit position from words[0]
    template <class Team> LNR_HD void put(Team &T, u64 v, u32 nbits) {      // nbits <= 48; v has no bits above them
        if (!nbits) return;
        const u32 w = pos >> 5, s = pos & 31;
        const u64 lo = v << s;                 // bits 0 .. 63 of the shifted value
        T.aor(&words[w], (u32)lo);
        if (s + nbits > 32) T.aor(&words[w + 1], (u32)(lo >> 32));
        if (s + nbits > 64) T.aor(&words[w + 2], (u32)(v >> (64 - s)));
        pos += nbits;
    }
};

// the bits of the token at position i (not SKIP): value and count
LNR_HD inline u32 token_bits(const Work &W, const u8 *txt, u32 i, u32 t, u64 &v) {
    const u32 len = tok_len(t);
    if (!len) { v = W.lcode[txt[i]]; return W.llen[txt[i]]; }
    const u32 ls = len_sym(len), ds = dist_sym(tok_dist(t));
    u32 nb = W.llen[257 + ls];
    v = W.lcode[257 + ls];
    const u32 le = lnr_inf::len_extra(ls);
    v |= (u64)(len - lnr_inf::len_base(ls)) << nb; nb += le;
    v |= (u64)W.dcode[ds] << nb; nb += W.dlen[ds];
    const u32 de = lnr_inf::dist_extra(ds);
    v |= (u64)(tok_dist(t) - lnr_inf::dist_base(ds)) << nb; nb += de;
    return nb;
}

// phase 4 after the two Huffman codes: the code-length sequence, its code, all canonical codes and the size of the block.  Lane 0 alone
// except for build_lengths, which every lane enters.
template <class Team>
LNR_HD inline void plan_block(Team &T, Work &W) {
    if (T.tid == 0) {
        u32 nl = NL, nd = ND;
        while (nl > 257 && W.llen[nl - 1] == 0) nl--;
        while (nd > 1 && W.dlen[nd - 1] == 0) nd--;
        W.nlen = nl; W.ndist = nd;
        for (u32 i = 0; i < nl; i++) W.seq[i] = W.llen[i];
        for (u32 i = 0; i < nd; i++) W.seq[nl + i] = W.dlen[i];
        for (u32 i = 0; i <= NC; i++) W.cfreq[i] = 0;
        const u32 tot = nl + nd;
        u32 r = 0;
        for (u32 i = 0; i < tot;) {
            const u32 v = W.seq[i];
            u32 run = 1;
            while (i + run < tot && W.seq[i + run] == v) run++;
            u32 left = run;
            if (v == 0) {
                while (left >= 11) { const u32 k = left < 138 ? left : 138; W.rsym[r] = 18; W.rext[r++] = (u8)(k - 11); left -= k; }
                if (left >= 3) { W.rsym[r] = 17; W.rext[r++] = (u8)(left - 3); left = 0; }
            } else {
                W.rsym[r] = (u8)v; W.rext[r++] = 0; left--;
                while (left >= 3) { const u32 k = left < 6 ? left : 6; W.rsym[r] = 16; W.rext[r++] = (u8)(k - 3); left -= k; }
            }
            while (left) { W.rsym[r] = (u8)v; W.rext[r++] = 0; left--; }
            i += run;
        }
        W.nrle = r;
        for (u32 i = 0; i < r; i++) W.cfreq[W.rsym[i]]++;
        u32 active = 0;
        for (u32 i = 0; i < NC; i++) active += W.cfreq[i] != 0;
        for (u32 i = 0; active < 2 && i < NC; i++) if (!W.cfreq[i]) { W.cfreq[i] = 1; active++; }
    }
    T.sync();
    build_lengths(T, W, W.cfreq, NC, 7, W.clen);
    if (T.tid == 0) {
        u32 nc = NC;
        while (nc > 4 && W.clen[cl_order(nc - 1)] == 0) nc--;
        W.ncode = nc;
        assign_codes(W, W.llen, NL, W.lcode);
        assign_codes(W, W.dlen, ND, W.dcode);
        assign_codes(W, W.clen, NC, W.ccode);
        u32 bits = 3 + 5 + 5 + 4 + 3 * nc;
        for (u32 i = 0; i < W.nrle; i++) { const u32 s = W.rsym[i]; bits += W.clen[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u); }
        W.head_bits = bits;
        for (u32 s = 0; s < NL; s++) bits += W.lfreq[s] * (W.llen[s] + (s > 256 ? lnr_inf::len_extra(s - 257) : 0u));
        for (u32 s = 0; s < ND; s++) bits += W.dfreq[s] * (W.dlen[s] + lnr_inf::dist_extra(s));     // (a code forced in has count 0)
        W.dyn_bits = bits;
    }
    T.sync();
}

// One block -> one member.  txt: n <= BLOCK_TEXT bytes every lane can read.  tab: HASH_SIZE words.  tok: n words.  out: MEMBER_CAP bytes,
// 4-byte aligned; tab and out may be the same memory (the table is dead before the image is begun).  Returns the member's size; *stored
// (when not null) tells whether it holds a stored block.  Every lane of the team calls this with the same arguments and gets the same values.
template <class Team>
LNR_HD inline u32 deflate_member(Team &T, Work &W, const u8 *txt, u32 n, u32 *tab, u32 *tok, u8 *out, u32 *stored) {
    u32 *words = reinterpret_cast<u32 *>(out);
    find_matches(T, W, txt, n, tab, tok);
    if (T.tid == 0) {
        for (u32 s = 0; s < NL + 2; s++) W.lfreq[s] = 0;
        for (u32 s = 0; s < ND + 2; s++) W.dfreq[s] = 0;
        W.crc = 0;
    }
    T.parse(tok, n);
    T.sync();
    // 3 histogram
    for (u32 i = T.tid; i < n; i += T.nt) {
        const u32 t = tok[i];
        if (t == SKIP) continue;
        if (!tok_len(t)) T.aadd(&W.lfreq[txt[i]], 1);
        else { T.aadd(&W.lfreq[257 + len_sym(tok_len(t))], 1); T.aadd(&W.dfreq[dist_sym(tok_dist(t))], 1); }
    }
    // the CRC32 of the text: a slice per lane, shifted to its place
    {
        const u32 S = (n + T.nt - 1) / T.nt;
        const u32 a = T.tid * S < n ? T.tid * S : n, b = a + S < n ? a + S : n;
        if (b > a) T.axor(&W.crc, lnr_inf::crc_shift(lnr_inf::crc_of(txt + a, b - a), n - b));
    }
    T.sync();
    if (T.tid == 0) W.lfreq[256] = 1;
    T.sync();
    // 4 codes.  The counts the lengths are built from: the end symbol is there; a block of n >= 1 bytes has a literal (position 0) too.
    // Distances: two codes at least -- where the block has fewer, codes 0 and 1 (or the one in use and its neighbour) get length 1.
    build_lengths(T, W, W.lfreq, NL, 15, W.llen);
    {
        u32 active = 0, one = 0;
        for (u32 s = 0; s < ND; s++) if (W.dfreq[s]) { active++; one = s; }
        if (active >= 2) build_lengths(T, W, W.dfreq, ND, 15, W.dlen);
        else {
            T.sync();
            if (T.tid == 0) {
                for (u32 s = 0; s < ND; s++) W.dlen[s] = 0;
                W.dlen[active ? one : 0] = 1;
                W.dlen[active && one == 0 ? 1 : (active ? 0 : 1)] = 1;
            }
            T.sync();
        }
    }
    plan_block(T, W);
    const u32 dyn_bytes = (W.dyn_bits + 7) / 8;
    const bool store = n == 0 || dyn_bytes >= n + 5;
    const u32 data_bytes = store ? n + 5 : dyn_bytes;
    const u32 total = 18 + data_bytes + 8;
    T.sync();                                  // (every lane has read W before the image, which may alias the table, is begun)
    for (u32 i = T.tid; i < (total + 3) / 4; i += T.nt) words[i] = 0;
    T.sync();
    if (store) {
        if (T.tid == 0) { out[18] = 1; out[19] = (u8)n; out[20] = (u8)(n >> 8); out[21] = (u8)~n; out[22] = (u8)(~n >> 8); }
        T.sync();
        // bytes 23 .. 23 + n: whole words from 24 on by all lanes, the ragged ends by bytes
        for (u32 i = T.tid; i < n; i += T.nt) T.aor(&words[(23 + i) >> 2], (u32)txt[i] << (8 * ((23 + i) & 3)));
    } else {
        if (T.tid == 0) {
            BitOut b{words, 18 * 8};
            b.put(T, 1 | (2 << 1), 3);
            b.put(T, W.nlen - 257, 5); b.put(T, W.ndist - 1, 5); b.put(T, W.ncode - 4, 4);
            for (u32 i = 0; i < W.ncode; i++) b.put(T, W.clen[cl_order(i)], 3);
            for (u32 i = 0; i < W.nrle; i++) {
                const u32 s = W.rsym[i];
                b.put(T, W.ccode[s], W.clen[s]);
                if (s >= 16) b.put(T, W.rext[i], s == 16 ? 2u : s == 17 ? 3u : 7u);
            }
            BitOut e{words, 18 * 8 + W.dyn_bits - W.llen[256]};
            e.put(T, W.lcode[256], W.llen[256]);
        }
        // 5 bits: a contiguous range of positions per lane
        const u32 S = (n + T.nt - 1) / T.nt;
        const u32 a = T.tid * S < n ? T.tid * S : n, b = a + S < n ? a + S : n;
        u32 mine = 0;
        for (u32 i = a; i < b; i++) { const u32 t = tok[i]; u64 v; if (t != SKIP) mine += token_bits(W, txt, i, t, v); }
        W.lane_bits[T.tid] = mine;
        T.sync();
        u32 at = 18 * 8 + W.head_bits;
        for (u32 l = 0; l < T.tid; l++) at += W.lane_bits[l];
        BitOut o{words, at};
        for (u32 i = a; i < b; i++) { const u32 t = tok[i]; u64 v; if (t != SKIP) { const u32 nb = token_bits(W, txt, i, t, v); o.put(T, v, nb); } }
    }
    T.sync();
    if (T.tid == 0) {
        words[0] = 0x04088b1fu; words[1] = 0; words[2] = 0x0006ff00u; words[3] = 0x00024342u;      // 1f 8b 08 04, MTIME, XFL 0 OS ff XLEN 6, 'B' 'C' 2 0
        out[16] = (u8)(total - 1); out[17] = (u8)((total - 1) >> 8);
        u8 *f = out + 18 + data_bytes;
        const u32 crc = W.crc;
        for (u32 i = 0; i < 4; i++) { f[i] = (u8)(crc >> (8 * i)); f[4 + i] = (u8)(n >> (8 * i)); }
    }
    T.sync();
    if (stored) *stored = store ? 1u : 0u;
    return total;
}

// the 28-byte empty member that ends a BGZF file
constexpr u8 EOF_MEMBER[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace lnr_def
