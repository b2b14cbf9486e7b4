// lnr_output.cpp -- output shaping of the hot path: the cords of a batch -> SAM records and APF text, as the
// reference's calculator tail and printer produce them, on host threads.  Host code, no GPU involved.
//
// Restates (reference paths relative to the reference root):
//   cords2BamLink            src/f_io.cpp:899-1011   one BAM-link record per run of cords that ifCreateNew_ (f_io.cpp:674-692) keeps
//                                                     together: leading soft clip = first y, cord2cigar_ per cord, trailing soft clip
//   cord2cigar_              src/f_io.cpp:758-875    '=' / 'I' / 'D' rectangles of a cord, 'X' between non-overlapping cords, split of
//                                                     large diagonal shifts (thd_DI 80, thd_X 200: preset 1, mapper.cpp:185-186)
//   insertNewBamRecord       src/align_util.cpp:301-343   flag 16 for the reverse strand, 2048 for every record after a run ended
//   createSAZTagCigar & co.  src/align_util.cpp:452-744   SA:Z = the other records of the read as rname,pos,strand,xSyMz[ID]0S,mapq,nm;
//   writeSam                 src/f_io.cpp:313-412    the text line; MAPQ is SeqAn's default 255, RNEXT '*', PNEXT 0, TLEN 0, SEQ / QUAL '*'
//   print_cords_apf          src/f_io.cpp:100-207    '@' header per cord block + one '|' line per cord
//   BAM (-ot 4 / 8)          src/f_io.cpp:509-523 + SeqAn write_bam.h:99-203   the records of the SAM lines in binary: here the shared
//                                                     per-record logic of lnr_output_hd.h (bam_read) through a memory sink
// Parity: byte-identical to the reference's own functions on the goldens (tests/test_output_cpu.py; APF blank lines follow the
// reference's rule for a block = one call).
#include "../../include/linear_amd.h"
#include "lnr_output_hd.h"
#include "lnr_output_hook.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace {

typedef uint64_t u64;
typedef int64_t i64;

inline u64 cx(u64 v) { return (v >> 20) & ((1ULL << 30) - 1); }     // get_cord_x cords.cpp:159
inline u64 cy(u64 v) { return v & 0xfffffULL; }                     // get_cord_y
inline u64 cid(u64 v) { return (v >> 50) & 1023ULL; }               // get_cord_id
inline u64 cstrand(u64 v) { return (v >> 61) & 1ULL; }
inline bool cend(u64 v) { return (v >> 60) & 1ULL; }                // is_cord_block_end
inline u64 shift_cord(u64 v, i64 x, i64 y) { return (u64)((i64)v + (x << 20) + y); }   // cords.cpp:135-141 (packed domain)

struct Cig { char op; uint32_t n; };
struct Rec { int rid; i64 pos; unsigned flag; std::vector<Cig> cigar; u64 lead = 0, trail = 0; };      // lead / trail: the two clips as numbers (what the S elements hold)

inline void push_shrink(std::vector<Cig> &c, char op, uint32_t n) {   // appendCigarShrink f_io.cpp:659-669
    if (!c.empty() && c.back().op == op) c.back().n += n;
    else c.push_back({op, n});
}
inline void rect(u64 a, u64 b, int f_m, Cig &c1, Cig &c2) {           // createRectangleCigarPair f_io.cpp:697-718
    u64 dx = cx(b) - cx(a), dy = cy(b) - cy(a);
    c1.op = f_m ? 'X' : '=';
    if (dx >= dy) { c2.op = 'D'; c1.n = (uint32_t)dy; c2.n = (uint32_t)(dx - dy); }
    else { c2.op = 'I'; c1.n = (uint32_t)dx; c2.n = (uint32_t)(dy - dx); }
}
inline void put_pair(std::vector<Cig> &c, const Cig &c1, const Cig &c2) {
    if (c1.n) push_shrink(c, c1.op, c1.n);
    if (c2.n) push_shrink(c, c2.op, c2.n);
}

int if_create_new(u64 c1s, u64 c1e, u64 c2s, u64 thd_large_X) {      // ifCreateNew_ f_io.cpp:674-692
    u64 x11 = cx(c1s), y11 = cy(c1s), x12 = cx(c1e), y12 = cy(c1e), x21 = cx(c2s), y21 = cy(c2s);
    return cend(c1s) || x11 > x21 || y11 > y21 || ((i64)(x21 - x12) > (i64)thd_large_X && (i64)(y21 - y12) > (i64)thd_large_X) || cstrand(c1s ^ c2s);
}

u64 cord2cigar(u64 cigar_str, u64 c1s, u64 c1e, u64 c2s, std::vector<Cig> &cigar, i64 thd_DI, i64 thd_X) {   // cord2cigar_ f_io.cpp:758-875
    Cig g1, g2;
    u64 x0 = cx(cigar_str), y0 = cy(cigar_str), x11 = cx(c1s), y11 = cy(c1s), x12 = cx(c1e), y12 = cy(c1e), x21 = cx(c2s), y21 = cy(c2s);
    if (x0 - y0 != x11 - y11) return ~0ULL;
    if (x12 >= x21 && y12 >= y21) { rect(c1s, c2s, 0, g1, g2); put_pair(cigar, g1, g2); }
    else if (x12 < x21 && y12 < y21) {
        rect(c1s, c1e, 0, g1, g2); put_pair(cigar, g1, g2);
        i64 DI = (i64)(x21 - x12 - y21 + y12);
        i64 X = (i64)std::min(x21 - x12, y21 - y12);
        if (std::llabs(DI) > thd_DI && X > thd_X) {
            i64 split_n = std::min((i64)std::ceil((float)std::llabs(DI) / (float)thd_DI), X);
            i64 split_DI = thd_DI, split_X = X / split_n;
            u64 s = c1e;
            for (i64 i = 0; i < split_n - 1; i++) {
                u64 e = DI < 0 ? shift_cord(s, split_X, split_X + split_DI) : shift_cord(s, split_X + split_DI, split_X);
                rect(s, e, 0, g1, g2); put_pair(cigar, g1, g2);
                s = e;
            }
            rect(s, c2s, 1, g1, g2); put_pair(cigar, g1, g2);
        } else { rect(c1e, c2s, 1, g1, g2); put_pair(cigar, g1, g2); }
    } else { rect(c1s, c2s, 0, g1, g2); put_pair(cigar, g1, g2); }   // the two remaining cases share one body in the reference
    return c2s;
}

// cords2BamLink (single read) f_io.cpp:899-1011
void cords_to_records(const u64 *cs, const u64 *ce, u64 n, u64 L, std::vector<Rec> &recs, u64 thd_large_X, i64 thd_DI, i64 thd_X) {
    recs.clear();
    u64 cigar_str = 0;
    int f_new = 1;
    unsigned flag = 0;
    std::vector<size_t> rec_ptr, end_ptr;
    for (u64 i = 1; i < n; i++) {
        if (f_new) {
            if (i != 1) { rec_ptr.push_back(recs.size() - 1); end_ptr.push_back(i - 1); }
            f_new = 0;
            Rec r; r.rid = (int)cid(cs[i]); r.pos = (i64)cx(cs[i]); r.flag = flag | (cstrand(cs[i]) ? 16u : 0u);
            r.lead = cy(cs[i]);
            if (cy(cs[i]) != 0) r.cigar.push_back({'S', (uint32_t)cy(cs[i])});     // insertNewBamRecord align_util.cpp:325-333
            recs.push_back(std::move(r));
            cigar_str = cs[i];
            flag = 0;
        }
        u64 c1s = cs[i], c1e = ce[i], c2s;
        if (i == n - 1 || if_create_new(cs[i], ce[i], cs[i + 1], thd_large_X)) { c2s = ce[i]; f_new = 1; flag = 2048; }
        else c2s = cs[i + 1];
        cigar_str = cord2cigar(cigar_str, c1s, c1e, c2s, recs.back().cigar, thd_DI, thd_X);
        if (cigar_str == ~0ULL) break;
        if (i == n - 1) { rec_ptr.push_back(recs.size() - 1); end_ptr.push_back(n - 1); }
    }
    for (size_t k = 0; k < end_ptr.size(); k++) {
        i64 clipped = (i64)(int)(L - cy(ce[end_ptr[k]]));
        if (clipped > 0) { recs[rec_ptr[k]].cigar.push_back({'S', (uint32_t)clipped}); recs[rec_ptr[k]].trail = (u64)clipped; }
    }
}

void put_u(std::string &s, unsigned long long v) { char b[24]; int n = snprintf(b, sizeof b, "%llu", v); s.append(b, (size_t)n); }
void put_i(std::string &s, long long v) { char b[24]; int n = snprintf(b, sizeof b, "%lld", v); s.append(b, (size_t)n); }

// SA:Z entry of one record (createSAZTagCigar / createSAZTagOneChimeric, align_util.cpp:452-520,682-714): xS yM z[I|D] 0S, zeros kept
// `first_visit`: createSAZTagCigarOneChimeric (align_util.cpp:642-678) sums NM only while the record's saz_cigar is still empty, i.e. the
// first time any line of the read lists this record; every later listing prints 0 (the cached saz_cigar is merged, nm_i_sum stays at its
// sentinel).  Line 0 therefore carries the real NM of every other record, line 1 the real NM of record 0 only, all else 0.
void saz_entry(const Rec &r, const char *gname, bool first_visit, std::string &out) {
    unsigned long long s0 = 0, cm = 0, nm = 0;
    long long ci = 0;
    for (size_t i = 0; i < r.cigar.size(); i++) {
        const Cig &c = r.cigar[i];
        if (i == 0 && c.op == 'S') s0 = c.n;
        else if (c.op == '=') cm += c.n;
        else if (c.op == 'X') { cm += c.n; nm += c.n; }
        else if (c.op == 'I') { ci -= c.n; nm += c.n; }
        else if (c.op == 'D') { ci += c.n; nm += c.n; }
        // (the reference's branch for a trailing 'S' tests `i == length(cigar[i]) - 1`, i.e. i == 0: never taken, the last count stays 0)
    }
    out += gname; out += ',';
    put_i(out, r.pos + 1); out += ',';
    out += (r.flag & 16) ? '-' : '+'; out += ',';
    put_u(out, s0); out += 'S';
    put_u(out, (unsigned)cm); out += 'M';
    put_u(out, (unsigned)std::llabs(ci)); out += ci < 0 ? 'I' : 'D';
    out += "0S,255,";
    put_i(out, first_visit ? (int)nm : 0); out += ';';
}

struct Writer {
    std::vector<std::string> gid;
    std::vector<u64> glen;
    std::string text;
    u64 thd_large_X = 8000; i64 thd_DI = 80, thd_X = 200;      // mapper.cpp:465,185-186 (preset 1)
    std::string rg, sn;                                        // -rg / -sn
    const uint8_t *const *genome = nullptr;                    // lnr_writer_set_genome: gid.size() borrowed sequences (Dna5 ordinals), or off
};

// SEQ of one record as `-ss 1` prints it (fillBamRecordLinkRecords align_util.cpp:745-808 with f_is_align == 0, cigar2SamSeq :1434-1500): the
// genome walks on from (rid, pos), the read from its first base -- flag 16: from the first base of its reverse complement (_compltRvseStr).
// S and I print the read, '=' prints the GENOME, X prints the read's base where it differs from the genome's and N where it does not, D moves
// the genome on.  Defined here where the reference reads out of range: a position outside its sequence is ordinal 0; ordinals above 4 are N.
void sam_seq(const Writer &w, const Rec &r, const uint8_t *read, u64 L, std::string &out) {
    const bool rev = (r.flag & 16) != 0;
    const uint8_t *g = (size_t)r.rid < w.gid.size() ? w.genome[r.rid] : nullptr;
    const u64 gl = g ? w.glen[(size_t)r.rid] : 0;
    auto rd = [&](u64 p) -> unsigned { if (p >= L) return 0; unsigned b = rev ? read[L - 1 - p] : read[p]; return b > 3 ? 4u : (rev ? 3u - b : b); };
    auto gn = [&](u64 x) -> unsigned { if (x >= gl) return 0; unsigned b = g[x]; return b > 4 ? 4u : b; };
    u64 x = (u64)r.pos, y = 0;
    const size_t before = out.size();
    for (const Cig &c : r.cigar) {
        if (c.op == 'D') { x += c.n; continue; }
        for (uint32_t i = 0; i < c.n; i++) {
            unsigned o;
            if (c.op == '=') o = gn(x + i);
            else { o = rd(y + i); if (c.op == 'X' && o == gn(x + i)) o = 4; }
            out += "ACGTN"[o];
        }
        y += c.n;
        if (c.op == '=' || c.op == 'X') x += c.n;
    }
    if (out.size() == before) out += '*';
}

// read != nullptr: SEQ is printed (lnr_writer_format_seq)
void sam_read(const Writer &w, const u64 *cs, const u64 *ce, u64 n, u64 L, const char *qname, std::string &out, std::vector<Rec> &recs, const uint8_t *read = nullptr) {
    cords_to_records(cs, ce, n, L, recs, w.thd_large_X, w.thd_DI, w.thd_X);
    std::vector<char> saz_done(recs.size(), 0);       // "saz_cigar not empty" per record (fillBamRecordLinkRecords walks the heads in record order)
    for (size_t it = 0; it < recs.size(); it++) {
        const Rec &r = recs[it];
        const char *g = (size_t)r.rid < w.gid.size() ? w.gid[(size_t)r.rid].c_str() : "*";
        out += qname; out += '\t';
        put_u(out, r.flag); out += '\t';
        out += g; out += '\t';
        put_i(out, r.pos + 1); out += "\t255\t";
        if (r.cigar.empty()) out += '*';
        for (const Cig &c : r.cigar) { put_u(out, c.n); out += c.op; }
        out += "\t*\t0\t0\t";
        if (read) sam_seq(w, r, read, L, out); else out += '*';
        out += "\t*";
        if (recs.size() > 1) {                         // SA:Z: every other line of the read, in record order (createSAZTagOneLine)
            out += "\tSA:Z:";
            for (size_t j = 0; j < recs.size(); j++)
                if (j != it) {
                    saz_entry(recs[j], (size_t)recs[j].rid < w.gid.size() ? w.gid[(size_t)recs[j].rid].c_str() : "*", !saz_done[j], out);
                    saz_done[j] = 1;
                }
        }
        out += '\n';
    }
}

// PAF: one line per record of sam_read, the twelve columns and cg:Z: (the line's definition: include/linear_amd.h).  No counterpart in the
// reference; the yardstick of lnr_output_hd.h's paf_item, written on its own over the records' element lists.
void paf_read(const Writer &w, const u64 *cs, const u64 *ce, u64 n, u64 L, const char *qname, std::string &out, std::vector<Rec> &recs) {
    cords_to_records(cs, ce, n, L, recs, w.thd_large_X, w.thd_DI, w.thd_X);
    for (const Rec &r : recs) {
        const bool rev = (r.flag & 16) != 0, known = (size_t)r.rid < w.gid.size();
        u64 match = 0, block = 0, ref = 0;
        std::string cg;
        for (const Cig &c : r.cigar) {
            if (c.op == 'S') continue;
            block += c.n;
            if (c.op == '=') match += c.n;
            if (c.op != 'I') ref += c.n;
            put_u(cg, c.n); cg += c.op;
        }
        out += qname; out += '\t';
        put_u(out, L); out += '\t';
        put_u(out, rev ? r.trail : r.lead); out += '\t';
        put_u(out, L - (rev ? r.lead : r.trail)); out += '\t';
        out += rev ? '-' : '+'; out += '\t';
        out += known ? w.gid[(size_t)r.rid].c_str() : "*"; out += '\t';
        put_u(out, known ? w.glen[(size_t)r.rid] : 0); out += '\t';
        put_u(out, (u64)r.pos); out += '\t';
        put_u(out, (u64)r.pos + ref); out += '\t';
        put_u(out, match); out += '\t';
        put_u(out, block); out += "\t255";
        if (!cg.empty()) { out += "\tcg:Z:"; out += cg; }
        out += '\n';
    }
}

void apf_read(const Writer &w, const u64 *c, u64 n, u64 L, const char *rid, bool blank_before, std::string &out) {   // print_cords_apf f_io.cpp:100-207
    if (n == 0) return;
    int fflag = 0;
    for (u64 j = 1; j < n; j++) {
        if (cend(c[j - 1])) {
            u64 m = j; int main_cnt = 0, block_len = 0;
            while (m < n && !cend(c[m])) { if (cstrand(c[m])) main_cnt++; block_len++; m++; }
            char main_icon = main_cnt > block_len / 2 ? '-' : (main_cnt == block_len / 2 ? (cstrand(c[j]) ? '-' : '+') : '+');
            u64 r_end = 0, s_end = 0;
            for (u64 i = j;; i++)
                if (cend(c[i]) || i == n - 1) { r_end = cy(c[i]) + 96; s_end = cx(c[i]) + 96; break; }
            if (blank_before) out += '\n';
            u64 g = cid(c[j]);
            out += "@ "; out += rid; out += ' ';
            put_u(out, L); out += ' ';
            put_u(out, cy(c[j])); out += ' ';
            put_u(out, std::min(r_end, L)); out += ' ';
            out += main_icon; out += ' ';
            out += g < w.gid.size() ? w.gid[g].c_str() : "*"; out += ' ';
            put_u(out, g < w.glen.size() ? w.glen[g] : 0); out += ' ';
            put_u(out, cx(c[j])); out += ' ';
            put_u(out, s_end); out += '\n';
            fflag = 1;
        }
        i64 d1 = 0, d2 = 0;
        if (!fflag) { d1 = (i64)(cx(c[j]) - cx(c[j - 1])); d2 = (i64)(cy(c[j]) - cy(c[j - 1])); }
        out += "| ";
        put_u(out, cy(c[j])); out += ' ';
        put_u(out, cx(c[j])); out += ' ';
        put_i(out, d2); out += ' ';
        put_i(out, d1); out += ' ';
        out += cstrand(c[j]) ? '-' : '+';
        out += '\n';
        fflag = 0;
    }
}

}  // namespace

struct lnr_writer {
    Writer w; lnr_outgpu *gpu = nullptr; bool genome_on_gpu = false; char err[256] = "";
    bool genome_dev = false;                   // lnr_writer_set_genome_dev: the GPU side's copy came from device memory (the host forms have no bases)
    int sort_state = 0;                        // lnr_writer_sort_*: 0 off, 1 collecting, 2 sorted: pieces go out, 3 every piece handed out
    std::vector<u64> sort_moff;                // offsets of the members handed out so far in the run of record members (+ the end of the last)
    std::string sorted, bai;                   // what lnr_writer_sort_host / _sort_bai / _bai_host return
};

extern "C" {

lnr_status lnr_writer_create(const char *const *genome_ids, const uint64_t *genome_len, uint32_t nseq, lnr_writer **out) {
    if (!genome_ids || !genome_len || !out) return LNR_ERR_ARG;
    lnr_writer *p = new (std::nothrow) lnr_writer();
    if (!p) return LNR_ERR_NOMEM;
    for (uint32_t i = 0; i < nseq; i++) { p->w.gid.emplace_back(genome_ids[i] ? genome_ids[i] : "*"); p->w.glen.push_back(genome_len[i]); }
    *out = p;
    return LNR_OK;
}
void lnr_writer_destroy(lnr_writer *w) {
    if (w && w->gpu && lnr_outgpu_close) lnr_outgpu_close(w->gpu);
    delete w;
}

// ---- the GPU twin of lnr_writer_format: the entry points live here (host code), the work behind the weak hook of lnr_output_hook.h
const char *lnr_writer_error(const lnr_writer *w) { return w ? w->err : "null writer"; }

lnr_status lnr_writer_gpu_open(lnr_writer *wr, int32_t device) {
    if (!wr) return LNR_ERR_ARG;
    if (wr->gpu) return LNR_OK;
    if (!lnr_outgpu_open) {
        snprintf(wr->err, sizeof wr->err, "no usable device: this build of the writer has no GPU side (device %d asked for)", (int)device);
        return LNR_ERR_NO_DEVICE;
    }
    std::string blob; std::vector<u64> goff;
    for (const std::string &g : wr->w.gid) { goff.push_back(blob.size()); blob += g; blob += '\0'; }
    wr->err[0] = 0;
    return (lnr_status)lnr_outgpu_open(device, blob.data(), blob.size(), goff.data(), wr->w.glen.data(), (uint32_t)wr->w.gid.size(), &wr->gpu, wr->err, sizeof wr->err);
}

static lnr_status format_on_gpu(lnr_writer *wr, lnr_outgpu_batch &b, const char **text, uint64_t *size) {
    if (!wr->gpu) { snprintf(wr->err, sizeof wr->err, "lnr_writer_gpu_open has not been called on this writer"); return LNR_ERR_ARG; }
    if (b.what == 3 && wr->sort_state >= 2) { snprintf(wr->err, sizeof wr->err, "lnr_writer_sort_finish has been called: no BAM call before lnr_writer_sort_end"); return LNR_ERR_ARG; }
    b.thd_large_X = wr->w.thd_large_X; b.thd_DI = wr->w.thd_DI; b.thd_X = wr->w.thd_X;
    wr->err[0] = 0;
    return (lnr_status)lnr_outgpu_format(wr->gpu, &b, text, size, wr->err, sizeof wr->err);
}
lnr_status lnr_writer_format_gpu(lnr_writer *wr, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids, const uint64_t *id_off,
                                 int what, const char **text, uint64_t *size) {
    if (!wr || !cords || !read_len || !read_ids || !id_off || !text || !size || (what != 1 && what != 2)) return LNR_ERR_ARG;
    lnr_outgpu_batch b{0, cords->n_reads, cords->n_cords, cords->cord_off, cords->cords_str, cords->cords_end, read_len, read_ids, id_off, what, 0, 0, 0, nullptr};
    return format_on_gpu(wr, b, text, size);
}
lnr_status lnr_writer_format_dev(lnr_writer *wr, const lnr_cords_dev *cords, const uint64_t *d_read_off, const char *read_ids, const uint64_t *id_off,
                                 int what, const char **text, uint64_t *size) {
    if (!wr || !cords || !read_ids || !id_off || !text || !size || (what != 1 && what != 2) || (cords->n_reads && !d_read_off)) return LNR_ERR_ARG;
    lnr_outgpu_batch b{1, cords->n_reads, cords->n_cords, cords->d_cord_off, cords->d_cords_str, cords->d_cords_end, d_read_off, read_ids, id_off, what, 0, 0, 0, nullptr};
    return format_on_gpu(wr, b, text, size);
}
lnr_status lnr_writer_gpu_times(const lnr_writer *wr, double *ms5) {
    if (!wr || !ms5 || !wr->gpu) return LNR_ERR_ARG;
    lnr_outgpu_times(wr->gpu, ms5);
    return LNR_OK;
}

// The reads of a batch on `threads` host threads: thread t formats a contiguous share of them into a string of its own with read(k, out),
// and the strings are concatenated in read order into the writer's text.
extern "C++" {
template <class F> static lnr_status reads_on_threads(lnr_writer *wr, uint32_t n, uint32_t threads, const char **text, uint64_t *size, F read) {
    if (threads < 1) threads = 1;
    if (threads > n) threads = n ? n : 1;
    std::vector<std::string> part(threads);
    auto work = [&](uint32_t t) {
        uint32_t lo = (uint32_t)((u64)n * t / threads), hi = (uint32_t)((u64)n * (t + 1) / threads);
        for (uint32_t k = lo; k < hi; k++) read(k, part[t]);
    };
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < threads; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    wr->w.text.clear();
    for (auto &p : part) wr->w.text += p;
    *text = wr->w.text.data();
    *size = wr->w.text.size();
    return LNR_OK;
}
}  // extern "C++"
// what: 1 = SAM records, 2 = APF.
// reads_concat != nullptr (SAM only): read_len holds n + 1 read offsets instead of n lengths, and SEQ is printed
static lnr_status format_on_host(lnr_writer *wr, const lnr_cords *cords, const uint8_t *reads_concat, const uint64_t *read_len, const char *read_ids,
                                 const uint64_t *id_off, int what, uint32_t threads, const char **text, uint64_t *size) {
    const Writer &w = wr->w;
    return reads_on_threads(wr, cords->n_reads, threads, text, size, [&](uint32_t k, std::string &o) {
        thread_local std::vector<Rec> recs;                      // sam_read's scratch, one per thread
        u64 a = cords->cord_off[k], e = cords->cord_off[k + 1];
        const char *id = read_ids + id_off[k];
        if (reads_concat) sam_read(w, cords->cords_str + a, cords->cords_end + a, e - a, read_len[k + 1] - read_len[k], id, o, recs, reads_concat + read_len[k]);
        else if (what == 1) sam_read(w, cords->cords_str + a, cords->cords_end + a, e - a, read_len[k], id, o, recs);
        else apf_read(w, cords->cords_str + a, e - a, read_len[k], id, k > 0, o);
    });
}
lnr_status lnr_writer_format(lnr_writer *wr, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids, const uint64_t *id_off,
                             int what, uint32_t threads, const char **text, uint64_t *size) {
    if (!wr || !cords || !read_len || !read_ids || !id_off || !text || !size || (what != 1 && what != 2)) return LNR_ERR_ARG;
    return format_on_host(wr, cords, nullptr, read_len, read_ids, id_off, what, threads, text, size);
}

// ---- PAF: host threads (the yardstick), GPU with host cords, GPU with device cords (k_out_measure<Paf> / k_out_emit<Paf>)
lnr_status lnr_writer_format_paf(lnr_writer *wr, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids, const uint64_t *id_off,
                                 uint32_t threads, const char **text, uint64_t *size) {
    if (!wr || !cords || !read_len || !read_ids || !id_off || !text || !size) return LNR_ERR_ARG;
    const Writer &w = wr->w;
    return reads_on_threads(wr, cords->n_reads, threads, text, size, [&](uint32_t k, std::string &o) {
        thread_local std::vector<Rec> recs;
        const u64 a = cords->cord_off[k], e = cords->cord_off[k + 1];
        paf_read(w, cords->cords_str + a, cords->cords_end + a, e - a, read_len[k], read_ids + id_off[k], o, recs);
    });
}
lnr_status lnr_writer_format_paf_gpu(lnr_writer *wr, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids, const uint64_t *id_off,
                                     const char **text, uint64_t *size) {
    if (!wr || !cords || !read_len || !read_ids || !id_off || !text || !size) return LNR_ERR_ARG;
    lnr_outgpu_batch b{0, cords->n_reads, cords->n_cords, cords->cord_off, cords->cords_str, cords->cords_end, read_len, read_ids, id_off, 4, 0, 0, 0, nullptr};
    return format_on_gpu(wr, b, text, size);
}
lnr_status lnr_writer_format_paf_dev(lnr_writer *wr, const lnr_cords_dev *cords, const uint64_t *d_read_off, const char *read_ids, const uint64_t *id_off,
                                     const char **text, uint64_t *size) {
    if (!wr || !cords || !read_ids || !id_off || !text || !size || (cords->n_reads && !d_read_off)) return LNR_ERR_ARG;
    lnr_outgpu_batch b{1, cords->n_reads, cords->n_cords, cords->d_cord_off, cords->d_cords_str, cords->d_cords_end, d_read_off, read_ids, id_off, 4, 0, 0, 0, nullptr};
    return format_on_gpu(wr, b, text, size);
}

// ---- SAM with the SEQ column (what the reference prints with -ss 1): host, GPU with host cords, GPU with device cords
lnr_status lnr_writer_set_genome(lnr_writer *wr, const uint8_t *const *seq) {
    if (!wr) return LNR_ERR_ARG;
    wr->w.genome = seq;
    wr->genome_on_gpu = wr->genome_dev = false;        // the GPU side takes its copy in the next SEQ call
    return LNR_OK;
}
// the GPU side's copy straight from device memory (a genome lnr_genome_load_gpu holds): device to device, at once; d_seq is not kept
lnr_status lnr_writer_set_genome_dev(lnr_writer *wr, const uint8_t *const *d_seq) {
    if (!wr) return LNR_ERR_ARG;
    if (!wr->gpu) { snprintf(wr->err, sizeof wr->err, "lnr_writer_set_genome_dev: lnr_writer_gpu_open has not been called on this writer"); return LNR_ERR_ARG; }
    if (!d_seq) { wr->genome_dev = false; wr->genome_on_gpu = false; return LNR_OK; }      // off (host pointers, where set, are taken again)
    if (!lnr_outgpu_set_genome_dev) { snprintf(wr->err, sizeof wr->err, "lnr_writer_set_genome_dev: this library was linked without its device half"); return LNR_ERR_NO_DEVICE; }
    for (size_t i = 0; i < wr->w.glen.size(); i++)
        if (!d_seq[i]) { snprintf(wr->err, sizeof wr->err, "lnr_writer_set_genome_dev: null sequence pointer"); return LNR_ERR_ARG; }
    wr->err[0] = 0;
    lnr_status s = (lnr_status)lnr_outgpu_set_genome_dev(wr->gpu, d_seq, wr->w.glen.data(), (uint32_t)wr->w.glen.size(), wr->err, sizeof wr->err);
    if (s != LNR_OK) return s;
    wr->genome_dev = wr->genome_on_gpu = true;
    return LNR_OK;
}
static bool seq_ready(lnr_writer *wr, bool gpu_form = false) {
    if (wr->w.genome || (gpu_form && wr->genome_dev)) return true;
    snprintf(wr->err, sizeof wr->err, "lnr_writer_set_genome has not been called on this writer: no bases for SEQ");
    return false;
}
lnr_status lnr_writer_format_seq(lnr_writer *wr, const lnr_cords *cords, const uint8_t *reads_concat, const uint64_t *read_off, const char *read_ids,
                                 const uint64_t *id_off, uint32_t threads, const char **text, uint64_t *size) {
    if (!wr || !cords || !reads_concat || !read_off || !read_ids || !id_off || !text || !size || !seq_ready(wr)) return LNR_ERR_ARG;
    return format_on_host(wr, cords, reads_concat, read_off, read_ids, id_off, 1, threads, text, size);
}
static lnr_status format_seq_on_gpu(lnr_writer *wr, lnr_outgpu_batch &b, const char **text, uint64_t *size) {
    if (!seq_ready(wr, true)) return LNR_ERR_ARG;
    if (!wr->gpu) { snprintf(wr->err, sizeof wr->err, "lnr_writer_gpu_open has not been called on this writer"); return LNR_ERR_ARG; }
    if (!wr->genome_on_gpu) {
        wr->err[0] = 0;
        lnr_status s = (lnr_status)lnr_outgpu_set_genome(wr->gpu, wr->w.genome, wr->w.glen.data(), (uint32_t)wr->w.glen.size(), wr->err, sizeof wr->err);
        if (s != LNR_OK) return s;
        wr->genome_on_gpu = true;
    }
    return format_on_gpu(wr, b, text, size);
}
lnr_status lnr_writer_format_seq_gpu(lnr_writer *wr, const lnr_cords *cords, const uint8_t *reads_concat, const uint64_t *read_off, const char *read_ids,
                                     const uint64_t *id_off, const char **text, uint64_t *size) {
    if (!wr || !cords || !reads_concat || !read_off || !read_ids || !id_off || !text || !size) return LNR_ERR_ARG;
    lnr_outgpu_batch b{0, cords->n_reads, cords->n_cords, cords->cord_off, cords->cords_str, cords->cords_end, read_off, read_ids, id_off, 1, 0, 0, 0, reads_concat};
    return format_seq_on_gpu(wr, b, text, size);
}
lnr_status lnr_writer_format_seq_dev(lnr_writer *wr, const lnr_cords_dev *cords, const uint8_t *d_reads_concat, const uint64_t *d_read_off, const char *read_ids,
                                     const uint64_t *id_off, const char **text, uint64_t *size) {
    if (!wr || !cords || !read_ids || !id_off || !text || !size || (cords->n_reads && (!d_read_off || !d_reads_concat))) return LNR_ERR_ARG;
    lnr_outgpu_batch b{1, cords->n_reads, cords->n_cords, cords->d_cord_off, cords->d_cords_str, cords->d_cords_end, d_read_off, read_ids, id_off, 1, 0, 0, 0, d_reads_concat};
    return format_seq_on_gpu(wr, b, text, size);
}

// ---- BAM: the header on the host; the records by the shared logic of lnr_output_hd.h, here through a memory sink on host threads (the
// yardstick of the GPU forms below), there in k_out_measure<Bam> / k_out_emit<Bam>
static void put_le32(std::string &o, uint32_t v) { for (int b = 0; b < 4; b++) o += (char)(v >> (8 * b)); }
lnr_status lnr_writer_bam_header(lnr_writer *wr, const char *command_line, int pbsv, const char **data, uint64_t *size) {
    if (!wr || !data || !size) return LNR_ERR_ARG;
    const char *t; uint64_t z;
    lnr_writer_sam_header(wr, command_line, &t, &z);
    std::string text(t, z);
    if (wr->sort_state) text.insert(0, "@HD\tVN:1.6\tSO:coordinate\n");      // sort mode: the file will be coordinate-sorted
    if (pbsv) {                                        // -ot 8: "@RG\t ID:" (mapper.cpp:308-312)
        size_t p = text.find("@RG\tID:");
        if (p != std::string::npos) text.insert(p + 4, " ");
    }
    std::string &o = wr->w.text;
    o.assign("BAM\1", 4);
    put_le32(o, (uint32_t)text.size());
    o += text;
    put_le32(o, (uint32_t)wr->w.gid.size());           // (the reference writes n_ref 0 here: see include/linear_amd.h)
    for (size_t i = 0; i < wr->w.gid.size(); i++) {
        put_le32(o, (uint32_t)wr->w.gid[i].size() + 1);
        o += wr->w.gid[i]; o += '\0';
        put_le32(o, (uint32_t)wr->w.glen[i]);
    }
    *data = o.data(); *size = o.size();
    return LNR_OK;
}
namespace {
struct StrSink { std::string &s; void put(char c) { s.push_back(c); } };
}
lnr_status lnr_writer_format_bam(lnr_writer *wr, const lnr_cords *cords, const uint8_t *reads_concat, const uint64_t *read_len, const char *read_ids,
                                 const uint64_t *id_off, uint32_t threads, const char **data, uint64_t *size) {
    if (!wr || !cords || !read_len || !read_ids || !id_off || !data || !size || (reads_concat && !seq_ready(wr))) return LNR_ERR_ARG;
    const Writer &w = wr->w;
    const uint32_t nseq = (uint32_t)w.gid.size();
    std::string blob; std::vector<u64> goff;
    for (const std::string &g : w.gid) { goff.push_back(blob.size()); blob += g; blob += '\0'; }
    const lnr_out::Params P{blob.data(), goff.data(), w.glen.data(), nseq, w.thd_large_X, w.thd_DI, w.thd_X};
    return reads_on_threads(wr, cords->n_reads, threads, data, size, [&](uint32_t k, std::string &out) {
        StrSink o{out};
        const u64 a = cords->cord_off[k], nc = cords->cord_off[k + 1] - a;
        const u64 L = reads_concat ? read_len[k + 1] - read_len[k] : read_len[k];
        const lnr_out::SeqSrc q{nullptr, nullptr, w.glen.data(), nseq, reads_concat ? reads_concat + read_len[k] : nullptr, L, w.genome};      // the borrowed sequences, each where it lies
        lnr_out::bam_read(o, P, reads_concat ? &q : nullptr, cords->cords_str + a, cords->cords_end + a, nc, L, read_ids + id_off[k]);
    });
}
lnr_status lnr_writer_format_bam_gpu(lnr_writer *wr, const lnr_cords *cords, const uint8_t *reads_concat, const uint64_t *read_len, const char *read_ids,
                                     const uint64_t *id_off, const char **data, uint64_t *size) {
    if (!wr || !cords || !read_len || !read_ids || !id_off || !data || !size) return LNR_ERR_ARG;
    lnr_outgpu_batch b{0, cords->n_reads, cords->n_cords, cords->cord_off, cords->cords_str, cords->cords_end, read_len, read_ids, id_off, 3, 0, 0, 0, reads_concat};
    return reads_concat ? format_seq_on_gpu(wr, b, data, size) : format_on_gpu(wr, b, data, size);
}
lnr_status lnr_writer_format_bam_dev(lnr_writer *wr, const lnr_cords_dev *cords, const uint8_t *d_reads_concat, const uint64_t *d_read_off, const char *read_ids,
                                     const uint64_t *id_off, const char **data, uint64_t *size) {
    if (!wr || !cords || !read_ids || !id_off || !data || !size || (cords->n_reads && !d_read_off)) return LNR_ERR_ARG;
    lnr_outgpu_batch b{1, cords->n_reads, cords->n_cords, cords->d_cord_off, cords->d_cords_str, cords->d_cords_end, d_read_off, read_ids, id_off, 3, 0, 0, 0, d_reads_concat};
    return d_reads_concat ? format_seq_on_gpu(wr, b, data, size) : format_on_gpu(wr, b, data, size);
}

// ---- coordinate sort + BAI (the order and the index format: include/linear_amd.h).  The host forms walk a record stream; the GPU forms
// (lnr_output_kernels.hip behind the weak hooks) leave the same per-record arrays, so ONE function writes the index for both.
namespace {
constexpr u64 MEMBER_TEXT = 0xff00;            // bytes of the sorted stream per BGZF member
struct SRec { u64 key; uint32_t flag; i64 end; u64 off, size; };
bool walk_stream(const char *raw, u64 size, std::vector<SRec> &out, char *err, size_t err_cap) {
    const uint8_t *r = (const uint8_t *)raw;
    for (u64 p = 0; p < size;) {
        const u64 bs = p + 36 <= size ? lnr_out::le32_at(r + p) : 0;
        if (bs < 32 || p + 4 + bs > size) { snprintf(err, err_cap, "record %zu at byte %llu of the stream: block_size does not fit the %llu bytes given", out.size(), (unsigned long long)p, (unsigned long long)size); return false; }
        const lnr_out::BamKey k = lnr_out::bam_key(r + p, size - p);
        out.push_back({lnr_out::bam_sort_key(k), k.flag, k.end, p, 4 + bs});
        p += 4 + bs;
    }
    return true;
}
// n records in file order: key, flag, end; off[n + 1] their offsets in the stream
lnr_status bai_core(uint32_t n_ref, size_t n, const u64 *key, const uint32_t *flag, const i64 *end, const u64 *off, u64 first_offset, const u64 *moff, u64 n_members,
                    std::string &o, char *err, size_t err_cap) {
    struct RefIx { std::map<uint32_t, std::vector<std::pair<u64, u64> > > bins; std::vector<u64> lin; u64 first = 0, last = 0, mapped = 0, unmapped = 0; bool any = false; };
    if ((off[n] + MEMBER_TEXT - 1) / MEMBER_TEXT != n_members) { snprintf(err, err_cap, "%llu bytes of records do not make %llu members", (unsigned long long)off[n], (unsigned long long)n_members); return LNR_ERR_ARG; }
    auto voff = [&](u64 s) { return (first_offset + moff[s / MEMBER_TEXT]) << 16 | s % MEMBER_TEXT; };
    std::vector<RefIx> R(n_ref);
    u64 no_coor = 0;
    bool have_prev = false; int32_t prev_ref = 0; uint32_t prev_bin = 0;
    for (size_t i = 0; i < n; i++) {
        const int32_t ref = (int32_t)(key[i] >> 32), pos = (int32_t)(uint32_t)key[i];
        if (ref < 0) { no_coor++; have_prev = false; continue; }
        if ((uint32_t)ref >= n_ref) { snprintf(err, err_cap, "record %zu of the sorted stream has refID %d, the writer has %u sequences", i, (int)ref, n_ref); return LNR_ERR_ARG; }
        if (pos < 0 || end[i] > ((i64)1 << 29)) {
            snprintf(err, err_cap, "record %zu of the sorted stream (refID %d, pos %d, end %lld) lies outside what a BAI can index (0 .. 2^29)", i, (int)ref, (int)pos, (long long)end[i]);
            return LNR_ERR_UNSUPPORTED;
        }
        const u64 vs = voff(off[i]), ve = voff(off[i + 1]);
        const uint32_t bin = lnr_out::reg2bin((uint32_t)pos, (uint32_t)end[i]);
        RefIx &x = R[(size_t)ref];
        std::vector<std::pair<u64, u64> > &ch = x.bins[bin];
        if (have_prev && prev_ref == ref && prev_bin == bin) ch.back().second = ve; else ch.push_back({vs, ve});
        have_prev = true; prev_ref = ref; prev_bin = bin;
        if (!x.any) { x.any = true; x.first = vs; }
        x.last = ve;
        (flag[i] & 4 ? x.unmapped : x.mapped)++;
        const size_t w0 = (size_t)(pos >> 14), w1 = (size_t)((end[i] - 1) >> 14);
        if (x.lin.size() <= w1) x.lin.resize(w1 + 1, ~0ULL);
        for (size_t w = w0; w <= w1; w++) if (vs < x.lin[w]) x.lin[w] = vs;
    }
    auto put64 = [&](u64 v) { for (int b = 0; b < 8; b++) o += (char)(v >> (8 * b)); };
    auto put32 = [&](uint32_t v) { for (int b = 0; b < 4; b++) o += (char)(v >> (8 * b)); };
    o.assign("BAI\1", 4);
    put32(n_ref);
    for (RefIx &x : R) {
        put32(x.any ? (uint32_t)x.bins.size() + 1 : 0);
        for (auto &b : x.bins) {
            put32(b.first); put32((uint32_t)b.second.size());
            for (auto &c : b.second) { put64(c.first); put64(c.second); }
        }
        if (x.any) { put32(37450); put32(2); put64(x.first); put64(x.last); put64(x.mapped); put64(x.unmapped); }
        for (size_t w = x.lin.size(); w-- > 1;) if (x.lin[w - 1] == ~0ULL) x.lin[w - 1] = x.lin[w];       // (the highest window has a record)
        put32((uint32_t)x.lin.size());
        for (u64 v : x.lin) put64(v);
    }
    put64(no_coor);
    return LNR_OK;
}
bool sort_ready(lnr_writer *wr) {
    if (wr->gpu && lnr_outgpu_sort_begin) return true;
    snprintf(wr->err, sizeof wr->err, "lnr_writer_gpu_open has not been called on this writer");
    return false;
}
}  // namespace

lnr_status lnr_writer_sort_host(lnr_writer *wr, const char *records, uint64_t size, const char **sorted) {
    if (!wr || (size && !records) || !sorted) return LNR_ERR_ARG;
    std::vector<SRec> recs;
    wr->err[0] = 0;
    if (!walk_stream(records, size, recs, wr->err, sizeof wr->err)) return LNR_ERR_ARG;
    std::sort(recs.begin(), recs.end(), [](const SRec &a, const SRec &b) {
        if (a.key != b.key) return a.key < b.key;
        if ((a.flag ^ b.flag) & 16) return !(a.flag & 16);
        return a.off < b.off;
    });
    std::string o;
    o.reserve(size);
    for (const SRec &r : recs) o.append(records + r.off, r.size);
    wr->sorted.swap(o);                            // (records may be an earlier result of this call)
    *sorted = wr->sorted.data();
    return LNR_OK;
}
lnr_status lnr_writer_bai_host(lnr_writer *wr, const char *sorted_records, uint64_t size, uint64_t first_offset, const uint64_t *member_off, uint64_t n_members,
                               const char **data, uint64_t *bai_size) {
    if (!wr || (size && !sorted_records) || !member_off || !data || !bai_size) return LNR_ERR_ARG;
    std::vector<SRec> recs;
    wr->err[0] = 0;
    if (!walk_stream(sorted_records, size, recs, wr->err, sizeof wr->err)) return LNR_ERR_ARG;
    const size_t n = recs.size();
    std::vector<u64> key(n), off(n + 1); std::vector<uint32_t> flag(n); std::vector<i64> end(n);
    for (size_t i = 0; i < n; i++) { key[i] = recs[i].key; flag[i] = recs[i].flag; end[i] = recs[i].end; off[i] = recs[i].off; }
    off[n] = size;
    const lnr_status s = bai_core((uint32_t)wr->w.gid.size(), n, key.data(), flag.data(), end.data(), off.data(), first_offset, member_off, n_members, wr->bai, wr->err, sizeof wr->err);
    if (s != LNR_OK) return s;
    *data = wr->bai.data(); *bai_size = wr->bai.size();
    return LNR_OK;
}

static void sort_info_of(const lnr_writer *wr, lnr_sort_info *info) {
    lnr_outgpu_sort_info i;
    lnr_outgpu_sort_info_get(wr->gpu, &i);
    info->records = i.records; info->record_bytes = i.record_bytes; info->device_bytes = i.device_bytes; info->members = i.members;
    info->index_ms = i.index_ms; info->sort_ms = i.sort_ms; info->gather_ms = i.gather_ms; info->deflate_ms = i.deflate_ms; info->pack_ms = i.pack_ms; info->download_ms = i.download_ms;
}
lnr_status lnr_writer_sort_begin(lnr_writer *wr, uint64_t max_device_bytes) {
    if (!wr || !sort_ready(wr)) return LNR_ERR_ARG;
    if (wr->sort_state) { snprintf(wr->err, sizeof wr->err, "lnr_writer_sort_begin: the sort mode is on already (lnr_writer_sort_end leaves it)"); return LNR_ERR_ARG; }
    wr->err[0] = 0;
    const lnr_status s = (lnr_status)lnr_outgpu_sort_begin(wr->gpu, max_device_bytes, wr->err, sizeof wr->err);
    if (s == LNR_OK) { wr->sort_state = 1; wr->sort_moff.assign(1, 0); }
    return s;
}
lnr_status lnr_writer_sort_spill(lnr_writer *wr, uint64_t max_host_bytes) {
    if (!wr) return LNR_ERR_ARG;
    if (!wr->gpu || !lnr_outgpu_sort_spill) { snprintf(wr->err, sizeof wr->err, "lnr_writer_sort_spill: lnr_writer_gpu_open has not been called on this writer"); return LNR_ERR_ARG; }
    if (wr->sort_state != 1) { snprintf(wr->err, sizeof wr->err, "lnr_writer_sort_spill: valid between lnr_writer_sort_begin and lnr_writer_sort_finish"); return LNR_ERR_ARG; }
    wr->err[0] = 0;
    return (lnr_status)lnr_outgpu_sort_spill(wr->gpu, max_host_bytes, wr->err, sizeof wr->err);
}
lnr_status lnr_writer_sort_hold_info_get(const lnr_writer *wr, lnr_sort_hold_info *out) {
    if (!wr || !out || !wr->gpu || !lnr_outgpu_sort_hold_info_get || wr->sort_state < 1) return LNR_ERR_ARG;
    lnr_outgpu_hold_info i;
    lnr_outgpu_sort_hold_info_get(wr->gpu, &i);
    out->stream_bytes = i.stream_bytes; out->held_device_bytes = i.held_device_bytes; out->held_host_bytes = i.held_host_bytes;
    out->device_batches = i.device_batches; out->host_batches = i.host_batches; out->keep_ms = i.keep_ms; out->spill_ms = i.spill_ms;
    return LNR_OK;
}
lnr_status lnr_writer_sort_finish(lnr_writer *wr, uint32_t piece_members, lnr_sort_info *info) {
    if (!wr || !sort_ready(wr)) return LNR_ERR_ARG;
    if (wr->sort_state != 1) { snprintf(wr->err, sizeof wr->err, "lnr_writer_sort_finish: %s", wr->sort_state ? "called already" : "lnr_writer_sort_begin has not been called"); return LNR_ERR_ARG; }
    wr->err[0] = 0;
    const lnr_status s = (lnr_status)lnr_outgpu_sort_finish(wr->gpu, piece_members, wr->err, sizeof wr->err);
    if (s != LNR_OK) return s;
    wr->sort_state = 2;
    if (info) sort_info_of(wr, info);
    return LNR_OK;
}
lnr_status lnr_writer_sort_next(lnr_writer *wr, const char **data, uint64_t *size) {
    if (!wr || !data || !size || !sort_ready(wr)) return LNR_ERR_ARG;
    if (wr->sort_state < 2) { snprintf(wr->err, sizeof wr->err, "lnr_writer_sort_next: lnr_writer_sort_finish has not been called"); return LNR_ERR_ARG; }
    const uint64_t *moff = nullptr; uint32_t nb = 0;
    wr->err[0] = 0;
    const lnr_status s = (lnr_status)lnr_outgpu_sort_next(wr->gpu, data, size, &moff, &nb, wr->err, sizeof wr->err);
    if (s != LNR_OK) return s;
    if (!nb) { wr->sort_state = 3; return LNR_OK; }
    const u64 base = wr->sort_moff.back();
    for (uint32_t k = 1; k <= nb; k++) wr->sort_moff.push_back(base + moff[k]);
    return LNR_OK;
}
lnr_status lnr_writer_sort_bai(lnr_writer *wr, uint64_t first_offset, const char **data, uint64_t *size) {
    if (!wr || !data || !size || !sort_ready(wr)) return LNR_ERR_ARG;
    if (wr->sort_state != 3) { snprintf(wr->err, sizeof wr->err, "lnr_writer_sort_bai: valid once lnr_writer_sort_next has returned size 0"); return LNR_ERR_ARG; }
    lnr_sort_info info;
    sort_info_of(wr, &info);
    const size_t n = (size_t)info.records;
    std::vector<u64> key(n + 1), off(n + 1); std::vector<uint32_t> flag(n + 1); std::vector<i64> end(n + 1);
    wr->err[0] = 0;
    lnr_status s = (lnr_status)lnr_outgpu_sort_fetch(wr->gpu, key.data(), flag.data(), end.data(), off.data(), wr->err, sizeof wr->err);
    if (s != LNR_OK) return s;
    s = bai_core((uint32_t)wr->w.gid.size(), n, key.data(), flag.data(), end.data(), off.data(), first_offset, wr->sort_moff.data(), wr->sort_moff.size() - 1, wr->bai, wr->err, sizeof wr->err);
    if (s != LNR_OK) return s;
    *data = wr->bai.data(); *size = wr->bai.size();
    return LNR_OK;
}
lnr_status lnr_writer_sort_info_get(const lnr_writer *wr, lnr_sort_info *info) {
    if (!wr || !info || !wr->gpu || !lnr_outgpu_sort_info_get || wr->sort_state < 2) return LNR_ERR_ARG;
    sort_info_of(wr, info);
    return LNR_OK;
}
lnr_status lnr_writer_sort_end(lnr_writer *wr) {
    if (!wr || !sort_ready(wr)) return LNR_ERR_ARG;
    lnr_outgpu_sort_end(wr->gpu);
    wr->sort_state = 0;
    wr->sort_moff.clear();
    return LNR_OK;
}

// ---- BGZF output of the GPU side (the work: lnr_output_kernels.hip behind the weak hooks)
lnr_status lnr_writer_set_bgzf(lnr_writer *wr, int on) {
    if (!wr) return LNR_ERR_ARG;
    if (!wr->gpu || !lnr_outgpu_set_bgzf) { snprintf(wr->err, sizeof wr->err, "lnr_writer_gpu_open has not been called on this writer"); return LNR_ERR_ARG; }
    lnr_outgpu_set_bgzf(wr->gpu, on);
    return LNR_OK;
}
lnr_status lnr_writer_bgzf_bytes_gpu(lnr_writer *wr, const char *bytes, uint64_t size, const char **data, uint64_t *out_size) {
    if (!wr || (size && !bytes) || !data || !out_size) return LNR_ERR_ARG;
    if (!wr->gpu || !lnr_outgpu_bgzf_bytes) { snprintf(wr->err, sizeof wr->err, "lnr_writer_gpu_open has not been called on this writer"); return LNR_ERR_ARG; }
    wr->err[0] = 0;
    return (lnr_status)lnr_outgpu_bgzf_bytes(wr->gpu, bytes, size, data, out_size, wr->err, sizeof wr->err);
}
lnr_status lnr_writer_bgzf_eof(const char **data, uint64_t *size) {
    static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!data || !size) return LNR_ERR_ARG;
    *data = (const char *)eof; *size = sizeof eof;
    return LNR_OK;
}
lnr_status lnr_writer_bgzf_stats(const lnr_writer *wr, lnr_bgzf_stats *out) {
    if (!wr || !out || !wr->gpu || !lnr_outgpu_bgzf_stats_get) return LNR_ERR_ARG;
    lnr_outgpu_bgzf_stats s;
    lnr_outgpu_bgzf_stats_get(wr->gpu, &s);
    out->blocks = s.blocks; out->stored_blocks = s.stored_blocks; out->text_bytes = s.text_bytes; out->compressed_bytes = s.compressed_bytes;
    out->deflate_ms = s.deflate_ms; out->pack_ms = s.pack_ms;
    return LNR_OK;
}

// SAM header as `linear filter` writes it: @SQ per reference sequence, then @RG and @PG (no @HD)
lnr_status lnr_writer_sam_header(lnr_writer *wr, const char *command_line, const char **text, uint64_t *size) {
    if (!wr || !text || !size) return LNR_ERR_ARG;
    std::string &o = wr->w.text;
    o.clear();
    for (size_t i = 0; i < wr->w.gid.size(); i++) { o += "@SQ\tSN:"; o += wr->w.gid[i]; o += "\tLN:"; put_u(o, wr->w.glen[i]); o += '\n'; }
    o += "@RG\tID:"; o += wr->w.rg; o += "\tSM:"; o += wr->w.sn; o += "\n@PG\tID:M1-3\tPN:Linear\tCL:";
    o += command_line ? command_line : "";
    o += '\n';
    *text = o.data(); *size = o.size();
    return LNR_OK;
}

lnr_status lnr_writer_set_preset(lnr_writer *wr, uint32_t preset) {
    if (!wr || preset > 2) return LNR_ERR_ARG;
    if (preset == 1) { wr->w.thd_DI = 80; wr->w.thd_X = 200; }                     // mapper.cpp:181-186
    else { wr->w.thd_DI = ((i64)1 << 60) - 1; wr->w.thd_X = ((i64)1 << 60) - 1; }  // FIOParms::FIOParms f_io.cpp:14-22
    return LNR_OK;
}
lnr_status lnr_writer_set_read_group(lnr_writer *wr, const char *read_group, const char *sample_name) {
    if (!wr) return LNR_ERR_ARG;
    wr->w.rg = read_group ? read_group : ""; wr->w.sn = sample_name ? sample_name : "";
    return LNR_OK;
}

}  // extern "C"
