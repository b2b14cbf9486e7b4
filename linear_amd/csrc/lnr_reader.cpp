// lnr_reader.cpp -- input side of the hot path: FASTA / FASTQ records, plain or gzip, decoded straight into the
// byte layout the C ABI takes (SeqAn Dna5 ordinals, reads back to back + offsets), so that a front-end fills a pinned block
// (lnr_host_alloc) and hands it to lnr_filter_submit without another copy.  Host code, no GPU involved.
//
// Replaces, for the filter path, what the reference's fetcher does per block (src/parallel_io.cpp:433-485: SeqAn
// readRecords(ids, reads, SeqFileIn, n) into StringSet<String<Dna5>>):
//   * format by the first record character: '>' FASTA, '@' FASTQ (seqan/seq_io/fasta_fastq.h); gzip detected by zlib;
//   * the id is the whole header line without its marker (reads keep it whole, mapper.cpp / base.cpp:188-195 cut genome ids at
//     the first blank -- lnr_reader_next_ids returns the whole line, the caller cuts);
//   * sequence characters convert as SeqAn's char -> Dna5 table does (basic/alphabet_residue_tabs.h:107-140): A/a 0, C/c 1,
//     G/g 2, T/t/U/u 3, everything else N = 4; blanks and line ends inside a record are skipped; multi-line FASTA and
//     multi-line FASTQ (quality length = sequence length) are accepted.
#include "../../include/linear_amd.h"
#include "lnr_reader_hook.h"
#include "lnr_inflate_hd.h"
#include "lnr_bam_hd.h"
#include "lnr_gunzip_hd.h"
#include "lnr_window_hd.h"

// Plain (not gzip) files take a PARALLEL path (f4's reason to exist: feed a GPU that filters 2 M reads/s): the file is mapped, one pass of
// memchr finds the record boundaries of the next block (a FASTA record ends before the next '>' at a line start; a FASTQ record is taken as four
// lines -- anything else, e.g. multi-line FASTQ, hands the rest of the file to the serial parser below), then `threads` host threads count and
// convert the bases of their share of the records straight into the caller's (pinned) block.  Same records, same ordinals, same ids as the serial
// parser (tests/test_reader_cpu.py runs both on every fixture).  A gzip file is one inflate stream and stays serial.
//
// A BGZF file (blocked gzip: every member carries its size in a 'BC' extra subfield, lnr_inf::bgzf_member) is mapped too, for
// lnr_reader_next_dev alone: its blocks go up compressed and are inflated on the device (k_bgzf_inflate).  lnr_reader_next reads it
// through gzread like any gzip file; bgzf_to_stream() is the one place where the two meet.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

enum Src { SRC_STREAM, SRC_MAP, SRC_BGZF, SRC_GZIP };       // who gives lnr_reader_next_dev its text: gzread, the mapped file, the BGZF chain, the gzip rounds
struct DevText { uint64_t keep_from = 0, carry = 0; };      // device text [keep_from, keep_from + carry) is what the last window left (SRC_BGZF, SRC_GZIP)

struct lnr_reader {
    // ---- the reader: what the file is, the last block's ids, the totals
    std::string path, err; bool started = false;
    int format = 0;              // 0 unknown, 1 FASTA, 2 FASTQ, 3 BAM (by content: the first four inflated bytes)
    Src src = SRC_STREAM;        // (lnr_reader_next knows SRC_MAP alone: it reads every other file through the stream)
    std::vector<char> ids; std::vector<uint64_t> id_off;             // ids of the last block, '\0' separated
    uint64_t records = 0, bases = 0; unsigned char tab[256];
    // ---- the stream: gzread through buf; a record that did not fit the last block any more (a gzip stream cannot be rewound) is the first of the next
    gzFile f = nullptr; std::vector<unsigned char> buf; size_t pos = 0, end = 0;
    bool eof = false, gz_done = false;                                // of fill(); of the GPU twin's own gzread into the staging buffer
    uint64_t gz_bytes = 0;                                            // text bytes that came out of gzread
    std::vector<uint8_t> spill; std::vector<char> spill_id; bool have_spill = false;
    // ---- the mapped file: SRC_MAP parses it in place (plain files only); SRC_BGZF and SRC_GZIP upload its compressed bytes
    const unsigned char *map = nullptr; size_t map_len = 0, mpos = 0; unsigned threads = 8;
    // ---- the BGZF chain (device inflate), walked one window at a time from bpos on; `chain` = the blocks whose text lies on the device and
    // is not used up, byte 0 of the device text = byte bskip of chain[0]'s text.  bend: the chain reached the end of the file; bstop: the
    // member at bpos is not BGZF
    bool bend = false, bstop = false, bfailed = false; int bfd = -1; uint64_t bpos = 0, bskip = 0;
    std::vector<lnr_win::Block> chain;
    lnr_inflate_counts ist_last{}, ist_total{};
    // ---- the gzip member (lnr_reader_gpu_gzip: gzp), inflated in rounds from the mapped file.  text_made = text bytes the device has
    // inflated so far (BGZF blocks included), so text_made - dtext.carry is the offset in the uncompressed stream at which a gzread stream
    // would go on
    bool gzp = false, gz_failed = false; lnr_gz::Member gzm; uint64_t text_made = 0;
    lnr_rdgpu_gz_counts gzs_last{}, gzs_total{};
    // ---- BAM: the header has been passed; a record was refused (the reader can only be closed); the header's n_ref; records passed so far
    // (skipped ones included) and the offset of the next one in the uncompressed stream -- what an error message names
    bool bam_hdr = false, bam_failed = false; int32_t bam_nref = 0; uint64_t bam_ord = 0, bam_off = 0;
    std::vector<unsigned char> bam_tmp;
    lnr_bam_counts bam_last{}, bam_total{};
    // ---- the GPU twin (lnr_reader_gpu_open / lnr_reader_next_dev): its device side, the slot of the next block, "the serial parser has
    // taken over", the text on the device, the host block the serial parser's records pass through on their way up
    lnr_rdgpu *gpu = nullptr; uint32_t gslots = 0, gslot = 0; bool gpu_serial = false;
    DevText dtext; std::unique_ptr<uint8_t[]> hblock; uint64_t hblock_cap = 0;
    const uint8_t *last_block = nullptr; uint64_t last_bases = 0;     // the block lnr_reader_next_dev delivered last (lnr_reader_keep_block)
    uint64_t g_text = 0, g_recs = 0;     // text bytes and records the windows have used up so far: sizes the next window
    std::vector<uint64_t> span_off; std::vector<uint32_t> span_len;   // the names of a window of host text (names_of_spans)
    char gerr[256] = "";

    bool fill() {
        if (eof) return false;
        if (pos < end) return true;
        int n = gzread(f, buf.data(), (unsigned)buf.size());
        if (n < 0) { int e; err = gzerror(f, &e); eof = true; return false; }
        if (n == 0) { eof = true; return false; }
        gz_bytes += (uint64_t)n;
        pos = 0; end = (size_t)n;
        return true;
    }
    int peek() { return fill() ? buf[pos] : -1; }
    // the next n bytes of the stream -> dst (dropped when dst is null); returns how many there were
    uint64_t bytes(unsigned char *dst, uint64_t n) {
        uint64_t got = 0;
        while (got < n && fill()) {
            const uint64_t k = end - pos < n - got ? end - pos : n - got;
            if (dst) memcpy(dst + got, buf.data() + pos, k);
            pos += k; got += k;
        }
        return got;
    }
    int get() { return fill() ? buf[pos++] : -1; }
    // appends the rest of the current line (without CR / LF) to s (or drops it when s is null); returns false at end of file with nothing read
    bool line(std::vector<char> *s) {
        bool any = false;
        while (fill()) {
            any = true;
            unsigned char *p = buf.data() + pos, *e = buf.data() + end;
            unsigned char *nl = (unsigned char *)memchr(p, '\n', (size_t)(e - p));
            unsigned char *stop = nl ? nl : e;
            if (s) s->insert(s->end(), (char *)p, (char *)stop);
            pos = (size_t)(stop - buf.data());
            if (nl) { pos++; break; }
        }
        if (s) while (!s->empty() && s->back() == '\r') s->pop_back();
        return any;
    }
};

// "Continue the serial stream at the first text byte the device path has not used up": block chain[0] (or the member at bpos), bskip bytes
// in.  Every BGZF block is a complete gzip member, so a fresh inflate stream may start at its file offset (lseek + gzdopen of a duplicated
// descriptor; gzseek would inflate the file from its start again).  From here on the reader treats the file as any gzip file.
static bool bgzf_to_stream(lnr_reader *r) {
    const uint64_t off = r->chain.empty() ? r->bpos : r->chain[0].off;
    uint64_t skip = r->chain.empty() ? 0 : r->bskip;
    r->src = SRC_STREAM; r->chain.clear(); r->bskip = 0; r->dtext = DevText{};
    int fd = dup(r->bfd);
    gzFile nf = nullptr;
    if (fd < 0 || lseek(fd, (off_t)off, SEEK_SET) < 0 || !(nf = gzdopen(fd, "rb"))) {
        if (fd >= 0) close(fd);
        r->err = "cannot reopen the file at BGZF block offset " + std::to_string(off);
        return false;
    }
    if (r->f) gzclose(r->f);
    r->f = nf;
    gzbuffer(r->f, 1u << 20);
    r->pos = r->end = 0; r->eof = false; r->gz_done = false;
    while (skip) {
        const unsigned ask = skip < r->buf.size() ? (unsigned)skip : (unsigned)r->buf.size();
        int got = gzread(r->f, r->buf.data(), ask);
        if (got <= 0) { int e; r->err = "BGZF block at file offset " + std::to_string(off) + ": " + (got < 0 ? gzerror(r->f, &e) : "unexpected end of file"); return false; }
        skip -= (uint64_t)got; r->gz_bytes += (uint64_t)got;
    }
    return true;
}

// ---- plain gzip rounds (lnr_reader_gpu_gzip).  "Continue the serial stream at the first text byte the device path has not used up": a
// member cannot be entered in its middle by zlib without its history, so a fresh gzread stream is opened and moved to the text offset with
// gzseek -- which inflates the file once more from its start.  Accepted: the hand-over is rare (a FASTQ that leaves the four-line form, a
// lnr_reader_next behind lnr_reader_next_dev).
static bool gz_to_stream(lnr_reader *r) {
    const uint64_t at = r->text_made - r->dtext.carry;
    r->src = SRC_STREAM; r->dtext = DevText{};
    gzFile nf = gzopen(r->path.c_str(), "rb");
    if (!nf) { r->err = "cannot reopen " + r->path; return false; }
    gzbuffer(nf, 1u << 20);
    if (at && gzseek(nf, (z_off_t)at, SEEK_SET) < 0) { int e; r->err = std::string("moving the gzip stream to text offset ") + std::to_string(at) + ": " + gzerror(nf, &e); gzclose(nf); return false; }
    if (r->f) gzclose(r->f);
    r->f = nf;
    r->pos = r->end = 0; r->eof = false; r->gz_done = false;
    return true;
}
static lnr_status gz_fail(lnr_reader *r, uint32_t status, uint64_t off) {
    snprintf(r->gerr, sizeof r->gerr, "gzip data at file offset %llu: %s", (unsigned long long)off, lnr_gz::status_text(status));
    r->err = r->gerr; r->gz_failed = true;
    return LNR_ERR_ARG;
}
// the member at gzm.pos, or the end of the file's members.  LNR_OK, or the header's error
static lnr_status gz_next_member(lnr_reader *r) {
    const uint32_t st = lnr_gz::member_enter(r->gzm, r->map, r->map_len);
    return st ? gz_fail(r, st, r->gzm.pos) : LNR_OK;
}
// ---- BAM (format 3; every decision from lnr_bam_hd.h).  The records come through the gzread stream one after the other.
static lnr_status bam_fail(lnr_reader *r, uint64_t ord, uint64_t off, const char *why) {
    char m[200];
    snprintf(m, sizeof m, "BAM record %llu at offset %llu of the uncompressed stream: %s", (unsigned long long)ord, (unsigned long long)off, why);
    r->err = m; r->bam_failed = true;
    return LNR_ERR_ARG;
}
static const char *const BAM_INVALID = "not a valid record", *const BAM_CUT = "the file ends inside it";
// the header, from the stream
static lnr_status bam_header(lnr_reader *r) {
    std::vector<unsigned char> hb;
    for (;;) {
        const lnr_bam::Header h = lnr_bam::header_span(hb.data(), hb.size());
        if (h.status < 0) { r->err = "not a BAM header"; r->bam_failed = true; return LNR_ERR_ARG; }
        if (h.status == 0) { r->bam_hdr = true; r->bam_nref = h.n_ref; r->bam_off = h.first; return LNR_OK; }
        const size_t have = hb.size();
        hb.resize(h.need);
        if (r->bytes(hb.data() + have, h.need - have) < h.need - have) { r->err = "the file ends inside the BAM header"; r->bam_failed = true; return LNR_ERR_ARG; }
    }
}
static lnr_status bam_next(lnr_reader *r, uint8_t *dst, uint64_t dst_cap, uint64_t *off, uint32_t max_reads, uint32_t *n_out, uint32_t n, uint64_t used) {
    using namespace lnr_bam;
    if (r->bam_failed) return LNR_ERR_ARG;
    if (!r->bam_hdr) if (lnr_status s = bam_header(r)) return s;
    while (n < max_reads) {
        unsigned char h[HEAD + 256];
        const uint64_t at = r->bam_off;
        const uint64_t got = r->bytes(h, HEAD);
        if (!got) break;
        if (got < HEAD) return bam_fail(r, r->bam_ord, at, BAM_CUT);
        const Fields f = rec_fields(h);
        if (!rec_valid(f, r->bam_nref, h, HEAD)) return bam_fail(r, r->bam_ord, at, BAM_INVALID);
        if (r->bytes(h + HEAD, f.l_read_name) < f.l_read_name) return bam_fail(r, r->bam_ord, at, BAM_CUT);
        if (!rec_valid(f, r->bam_nref, h, HEAD + f.l_read_name)) return bam_fail(r, r->bam_ord, at, BAM_INVALID);
        const uint64_t cig = 4ULL * f.n_cigar_op, packed = ((uint64_t)f.l_seq + 1) / 2, l = (uint64_t)f.l_seq;
        uint64_t rest = (uint64_t)f.block_size - 32 - f.l_read_name - cig;
        if (r->bytes(nullptr, cig) < cig) return bam_fail(r, r->bam_ord, at, BAM_CUT);
        const bool want = delivered(f.flag);
        if (want) {
            if (r->bam_tmp.size() < packed) r->bam_tmp.resize(packed);
            if (r->bytes(r->bam_tmp.data(), packed) < packed) return bam_fail(r, r->bam_ord, at, BAM_CUT);
            rest -= packed;
        }
        if (r->bytes(nullptr, rest) < rest) return bam_fail(r, r->bam_ord, at, BAM_CUT);
        r->bam_ord++; r->bam_off += 4 + (uint64_t)f.block_size;
        if (!want) continue;
        const uint32_t len1 = (uint32_t)l;
        const Take t = take(&len1, 1, dst_cap - used, max_reads - n, n == 0);
        const bool rev = reversed(f.flag);
        r->records++; r->bases += l;
        if (!t.n) {                                                // keep it for the next block
            r->spill.resize(l);
            for (uint64_t j = 0; j < l; j++) r->spill[j] = base_at(r->bam_tmp.data(), l, j, rev);
            r->spill_id.assign((const char *)h + HEAD, (const char *)h + HEAD + f.l_read_name);
            r->have_spill = true;
            if (t.too_big) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
            break;
        }
        for (uint64_t j = 0; j < l; j++) dst[used + j] = base_at(r->bam_tmp.data(), l, j, rev);
        used += l;
        r->ids.insert(r->ids.end(), (const char *)h + HEAD, (const char *)h + HEAD + f.l_read_name);
        n++;
        off[n] = used;
        r->id_off.push_back(r->ids.size());
    }
    *n_out = n;
    return LNR_OK;
}

// t += c for the counts structs of the public header: NU counts, then ND times (lnr_rdgpu_gz_add is the third of the kind)
template <int NU, int ND, class C> static void counts_add_n(C &t, const C &c) {
    static_assert(sizeof(C) == 8 * (NU + ND), "NU 64-bit counts and ND doubles");
    uint64_t *tu = (uint64_t *)&t; const uint64_t *cu = (const uint64_t *)&c;
    for (int i = 0; i < NU; i++) tu[i] += cu[i];
    double *td = (double *)(tu + NU); const double *cd = (const double *)(cu + NU);
    for (int i = 0; i < ND; i++) td[i] += cd[i];
}
static_assert(offsetof(lnr_inflate_counts, inflate_ms) == 8 * 4 && offsetof(lnr_bam_counts, find_ms) == 8 * 5, "where the times begin");
static void counts_add(lnr_inflate_counts &t, const lnr_inflate_counts &c) { counts_add_n<4, 2>(t, c); }
static void counts_add(lnr_bam_counts &t, const lnr_bam_counts &c) { counts_add_n<5, 3>(t, c); }

// ---- the GPU twin's loop (lnr_reader_next_dev): size the window, ask the source for it, parse it, account for it, tell the
// source what was used, decide (lnr_win::decide).  One call's state, what a source hands to the parse, what the parse leaves behind:
struct Call { lnr_reader *r; uint32_t slot; uint32_t n = 0; uint64_t used = 0, grow = 1; };   // n records and `used` bases in the block; the window's factor
struct Window {
    lnr_rdgpu_window w{};            // the limits; host text: w.text / w.len, byte 0 starts a record
    lnr_rdgpu_bgzf job{};            // device text: what the last window left and the blocks to inflate behind it
    std::vector<lnr_rdgpu_bgzf_blk> tab;
    size_t chain0 = 0;               // SRC_BGZF: tab[k] is chain[chain0 + k]
    uint64_t len = 0;                // lnr_win::Seen::len
    bool ended = false, stuck = false;
};
struct Parsed {
    lnr_rdgpu_result res{};
    lnr_rdgpu_names names{};
    uint64_t lead = 0, passed = 0;   // device text used up in front of the parsed text; records in front of res.consumed (BAM: skipped ones included)
    bool parsed = false, handover = false;
};
enum Got { GOT_WINDOW, GOT_AGAIN, GOT_END, GOT_ERROR };     // (GOT_ERROR: *st and r->err are set)
static Got fail(lnr_reader *r, lnr_status *st, lnr_status s, const char *why) { r->err = why; *st = s; return GOT_ERROR; }
static Got gfail(lnr_reader *r, lnr_status *st, int s) { return fail(r, st, (lnr_status)s, r->gerr); }
static Got bam_header_fail(lnr_reader *r, lnr_status *st, const char *why) { r->bam_failed = true; return fail(r, st, LNR_ERR_ARG, why); }
static const char *const TOO_LONG = "a record is longer than the reader's window";
static bool is_ws(unsigned char c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t'; }
static void put_back(lnr_reader *r, const uint8_t *p, uint64_t left) {       // what a window of the stream did not use goes back in front of the stream
    if (r->buf.size() < left) r->buf.resize(left);
    memcpy(r->buf.data(), p, left);
    r->pos = 0; r->end = left;
}

// SRC_GZIP: rounds of the member inflated on the device behind what the last window left, until the device text holds `want` bytes
static Got gzip_window(Call &c, uint64_t want, Window &W, lnr_status *st) {
    lnr_reader *r = c.r;
    lnr_gz::Member &m = r->gzm;
    auto failed = [&]() { return c.n ? GOT_END : gfail(r, st, LNR_ERR_ARG); };      // bad data: the records in front of it are delivered first
    if (r->gz_failed || gz_next_member(r)) return failed();
    const uint64_t chunk = lnr_gz::env_bytes("LNR_READER_GZ_CHUNK", 128ULL << 10, 1024, 1ULL << 30), round = lnr_gz::env_bytes("LNR_READER_GZ_ROUND", 64ULL << 20, 1024, 1ULL << 31);
    constexpr uint64_t TEXT_MAX = lnr_win::WINDOW_MAX - 65536;
    uint64_t &carry = r->dtext.carry;
    while (!m.end && !r->gz_failed && carry < want && !W.stuck) {
        const uint64_t rb = m.start_bit >> 3;
        if (rb >= r->map_len) { gz_fail(r, lnr_inf::E_INPUT_END, r->map_len); break; }      // the file ends behind a member's header
        if (carry >= TEXT_MAX) { W.stuck = true; break; }
        uint64_t base = want - carry + 2 * chunk;                     // text is seldom smaller than its compressed bytes: no more of them than text is wanted
        if (base > round) base = round;
        const uint64_t rsize = lnr_gz::member_round_size(m, base), clen = r->map_len - rb < rsize ? r->map_len - rb : rsize;
        lnr_rdgpu_gzip job{};
        job.comp = r->map + rb; job.comp_len = clen; job.start_bit = (uint32_t)(m.start_bit & 7); job.hist = m.hist; job.chunk = chunk;
        job.keep_from = r->dtext.keep_from; job.carry = carry; job.text_cap = TEXT_MAX - carry; job.threads = r->threads;
        lnr_rdgpu_gzip_result gr{};
        if (int s = lnr_rdgpu_gzip_round(r->gpu, &job, &gr, r->gerr, sizeof r->gerr)) { r->gz_failed = true; return gfail(r, st, s); }
        lnr_gz::Round R = lnr_gz::empty_round(rb * 8 + gr.end_bit);   // the round as the walker takes it: in the file's coordinates
        R.status = gr.status; R.stop = gr.stop; R.pieces = gr.pieces; R.text = gr.text; R.bad_bit = (rb + gr.bad_off) * 8;
        lnr_rdgpu_gz_counts cn = gr.counts;
        bool grown, final; uint64_t bad = 0;
        uint32_t v = lnr_gz::round_verdict(m, R, rb + clen, r->map_len, rsize, grown, &bad);
        if (!gr.status && v == lnr_gz::E_TEXT_CAP) { W.stuck = true; v = 0; }               // the device text is full: what it holds is parsed first
        if (!gr.status && !gr.pieces) cn.grown_rounds = 1;            // no block completed
        if (v || !gr.pieces) {
            lnr_rdgpu_gz_add(&r->gzs_last, &cn);
            if (!gr.status && v == lnr_gz::E_LIMIT) return fail(r, st, LNR_ERR_LIMIT, "a DEFLATE block is longer than the reader's staging limit");
            if (v) { gz_fail(r, v, bad); break; }
            continue;                                                 // (the same round doubled; stuck: the loop ends)
        }
        r->dtext.keep_from = 0; carry += gr.text; r->text_made += gr.text;
        v = lnr_gz::member_fold(m, r->map, r->map_len, R, gr.crc, &final, &bad);
        cn.compressed_bytes = ((m.start_bit + 7) >> 3) - rb;
        cn.members = final;
        lnr_rdgpu_gz_add(&r->gzs_last, &cn);
        if (v) { gz_fail(r, v, bad); break; }                         // (the text in front of a bad trailer is delivered, as gzread delivers it)
        if (final && gz_next_member(r)) break;
    }
    W.ended = m.end || r->gz_failed;
    if (!carry) {
        if (r->gz_failed) return failed();
        return m.end ? GOT_END : fail(r, st, LNR_ERR_LIMIT, TOO_LONG);
    }
    W.job.keep_from = r->dtext.keep_from; W.job.carry = W.len = carry;      // no block to inflate: the parse of the device text
    return GOT_WINDOW;
}

// A member that is not BGZF: with lnr_reader_gpu_gzip the gzip rounds take over there (text only), where gzread takes over without it -- at
// the first byte the device has not used up (the rounds: r->dtext stays as it is)
static bool bgzf_give_way(lnr_reader *r) {
    if (!r->gzp || r->format == 3) return bgzf_to_stream(r);
    r->src = SRC_GZIP; r->chain.clear(); r->bskip = 0;
    r->gzm = lnr_gz::Member{}; r->gzm.pos = r->bpos;
    return true;
}
// SRC_BGZF: a run of whole BGZF blocks, to be inflated on the device behind what the last window left
static Got bgzf_window(Call &c, uint64_t want, Window &W, lnr_status *st) {
    lnr_reader *r = c.r;
    if (r->bfailed) return gfail(r, st, LNR_ERR_ARG);
    const uint64_t c0 = r->bpos;
    uint64_t fresh = 0, tl = r->dtext.carry;
    W.chain0 = r->chain.size();
    while (!r->bend && !r->bstop && tl < want && tl + 65536 <= lnr_win::WINDOW_MAX && r->bpos - c0 < (1ULL << 30)) {
        if (r->bpos >= r->map_len) { r->bend = true; break; }
        uint32_t doff = 0;
        const unsigned char *m = r->map + r->bpos;
        const uint32_t size = lnr_inf::bgzf_member(m, r->map_len - r->bpos, doff);
        auto le32 = [](const unsigned char *q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); };
        const uint32_t isize = size ? le32(m + size - 4) : 0;
        if (!size || isize > 65536) { r->bstop = true; break; }     // not a BGZF member (or the chain leaves the file): gzread goes on here
        if (isize) {
            W.tab.push_back(lnr_rdgpu_bgzf_blk{r->bpos + doff - c0, fresh, size - doff - 8, isize, le32(m + size - 8), 0});
            r->chain.push_back(lnr_win::Block{r->bpos, size, isize});
            fresh += isize; tl += isize;
        }
        r->bpos += size;
    }
    if (!r->bend && !r->bstop && r->bpos >= r->map_len) r->bend = true;
    if (!tl) {
        if (r->bend) return GOT_END;
        if (r->bstop) return bgzf_give_way(r) ? GOT_AGAIN : (*st = LNR_ERR_ARG, GOT_ERROR);
    }
    // (a chain that stops short of `want` because the window is at its largest is parsed like any other: it may well hold whole records --
    // a genome's windows do, once one chromosome has doubled them -- and lnr_win::decide reports TOO_LONG where it holds none)
    W.job.comp = r->map + c0; W.job.comp_len = r->bpos - c0; W.job.blk = W.tab.data(); W.job.nblk = (uint32_t)W.tab.size();
    W.job.keep_from = r->dtext.keep_from; W.job.carry = r->dtext.carry; W.job.new_text = fresh;
    W.len = tl; W.ended = r->bend;
    return GOT_WINDOW;
}

// SRC_MAP: the next bytes of the mapped file
static Got map_window(Call &c, uint64_t want, Window &W, lnr_status *) {
    lnr_reader *r = c.r;
    while (r->mpos < r->map_len && is_ws(r->map[r->mpos])) r->mpos++;
    if (r->mpos >= r->map_len) return GOT_END;
    W.w.text = r->map + r->mpos; W.w.len = W.len = r->map_len - r->mpos < want ? r->map_len - r->mpos : want;
    W.ended = r->mpos + W.len == r->map_len;
    return GOT_WINDOW;
}

// SRC_STREAM: an inflate stream (or any file the reader does not map), gzread into a pinned buffer.  BAM: the header is passed here, the
// records go up as they are
static Got stream_window(Call &c, uint64_t want, Window &W, lnr_status *st) {
    lnr_reader *r = c.r;
    const uint64_t have = r->end - r->pos;
    if (want < have + 16) want = have + 16;
    uint8_t *S = lnr_rdgpu_stage(r->gpu, want);
    if (!S) return fail(r, st, LNR_ERR_NOMEM, "pinned host allocation failed");
    memcpy(S, r->buf.data() + r->pos, have);
    r->pos = r->end = 0;
    uint64_t len = have, lead = 0;
    while (!r->gz_done && len < want) {
        const uint64_t ask = want - len < (1u << 30) ? want - len : (1u << 30);
        int got = gzread(r->f, S + len, (unsigned)ask);
        if (got < 0) { int e; return fail(r, st, LNR_ERR_ARG, gzerror(r->f, &e)); }
        if (got == 0) r->gz_done = true;
        len += (uint64_t)got; r->gz_bytes += (uint64_t)got;
    }
    const bool eof = W.ended = r->gz_done;
    if (r->format == 0 && lnr_bam::is_magic(S, len)) r->format = 3;
    if (r->format == 3 && !r->bam_hdr) {
        const lnr_bam::Header h = lnr_bam::header_span(S, len);
        if (h.status < 0) return bam_header_fail(r, st, "not a BAM header");
        if (h.status == 1) {
            if (eof) return bam_header_fail(r, st, "the file ends inside the BAM header");
            if (len >= lnr_win::WINDOW_MAX) return fail(r, st, LNR_ERR_LIMIT, "the BAM header is longer than the reader's window");
            put_back(r, S, len); c.grow *= 2;
            return GOT_AGAIN;
        }
        r->bam_hdr = true; r->bam_nref = h.n_ref; r->bam_off = h.first; lead = h.first;
    }
    if (r->format != 3) while (lead < len && is_ws(S[lead])) lead++;
    if (len == lead) return eof ? GOT_END : GOT_AGAIN;
    W.w.text = S + lead; W.w.len = len - lead; W.w.pinned = 1; W.len = r->format == 3 ? len : len - lead;
    return GOT_WINDOW;
}

// the names of a window of host text in the form the gather gives them: the header spans over the text itself, trailing '\r' dropped
static void names_of_spans(lnr_reader *r, const unsigned char *text, const uint64_t *hdr, uint64_t n, lnr_rdgpu_names *out) {
    r->span_off.resize(n); r->span_len.resize(n);
    for (uint64_t k = 0; k < n; k++) {
        uint64_t hb = hdr[2 * k], he = hdr[2 * k + 1];
        while (he > hb && text[he - 1] == '\r') he--;
        r->span_off[k] = hb; r->span_len[k] = (uint32_t)(he - hb);
    }
    *out = lnr_rdgpu_names{(const char *)text, r->span_off.data(), r->span_len.data()};
}

// the parse of a window: device text (blocks inflated first) or host text, text records or BAM.  GOT_AGAIN: nothing was parsed, the file
// turned out to be a BAM and the source has been told
static Got parse_window(Call &c, Window &W, Parsed &P, lnr_status *st) {
    lnr_reader *r = c.r;
    const bool dev = r->src == SRC_BGZF || r->src == SRC_GZIP;
    lnr_rdgpu_bam_result bb{};
    if (dev) {
        bool &failed = r->src == SRC_GZIP ? r->gz_failed : r->bfailed;
        lnr_rdgpu_bgzf_result br{};
        const lnr_rdgpu_bam_in in{r->bam_hdr ? 1 : 0, r->bam_nref};
        W.w.fmt = r->format;
        // BAM records, not text: the same inflate, then find / stitch / take / emit
        if (int s = r->format == 3 ? lnr_rdgpu_parse_bam(r->gpu, &W.job, &W.w, &in, &P.res, &bb, r->gerr, sizeof r->gerr)
                                   : lnr_rdgpu_parse_bgzf(r->gpu, &W.job, &W.w, &P.res, &br, r->gerr, sizeof r->gerr)) { failed = true; return gfail(r, st, s); }
        const lnr_rdgpu_badblk bad = r->format == 3 ? bb.bad_block : br.bad_block;
        if (bad.status) {                                             // a call that meets a bad block delivers no block
            snprintf(r->gerr, sizeof r->gerr, "BGZF block at file offset %llu: %s", (unsigned long long)r->chain[W.chain0 + bad.blk].off, lnr_inf::status_text(bad.status));
            return r->bfailed = true, gfail(r, st, LNR_ERR_ARG);
        }
        r->ist_last.blocks += W.tab.size(); r->ist_last.compressed_bytes += W.job.comp_len; r->ist_last.text_bytes += W.job.new_text;
        if (r->format == 3) {
            if (bb.hdr_state == 2) return bam_header_fail(r, st, "not a BAM header");
            if (bb.hdr_state == 1 && r->bend) return bam_header_fail(r, st, "the file ends inside the BAM header");
            if (bb.hdr_state == 0 && !r->bam_hdr) { r->bam_hdr = true; r->bam_nref = bb.n_ref; r->bam_off = bb.lead; }
            P.lead = bb.lead;                                         // (the header was moved out of the device text)
        } else {
            r->text_made += W.job.new_text;
            if (r->format == 0 && W.w.fmt == 3) {                     // "BAM\1"
                if (r->src == SRC_GZIP) return gz_to_stream(r) ? GOT_AGAIN : (*st = LNR_ERR_ARG, GOT_ERROR);     // in a plain gzip file: read through gzread, as without the switch
                r->format = 3; r->dtext = DevText{0, W.len};          // the text stays on the device whole, the next pass reads it as records
                return GOT_AGAIN;
            }
            if (r->format == 0 && br.first >= 0) r->format = W.w.fmt;
            P.parsed = br.parsed; P.lead = br.lead; P.names = br.names; P.passed = P.res.n;
            P.handover = br.parsed ? P.res.handover != 0 : br.first >= 0;      // not a record start: the serial parser reports it
        }
    } else if (r->format == 3) {
        const lnr_rdgpu_bam_in in{1, r->bam_nref};
        W.w.fmt = 3;
        if (int s = lnr_rdgpu_parse_bam(r->gpu, nullptr, &W.w, &in, &P.res, &bb, r->gerr, sizeof r->gerr)) return gfail(r, st, s);
    } else {
        const unsigned char *text = W.w.text;
        if (r->format == 0) r->format = text[0] == '>' ? 1 : (text[0] == '@' ? 2 : -1);
        P.handover = r->format < 0 || text[0] != (r->format == 1 ? '>' : '@');       // (the serial parser reports it)
        if (!P.handover) {
            W.w.fmt = r->format;
            if (int s = lnr_rdgpu_parse(r->gpu, &W.w, &P.res, r->gerr, sizeof r->gerr)) return gfail(r, st, s);
            names_of_spans(r, text, P.res.hdr, P.res.n, &P.names);     // (no gather here: it would cost a launch and a download per window)
            P.parsed = true; P.passed = P.res.n; P.handover = P.res.handover != 0;
        }
    }
    if (r->format == 3) {                                             // the error the host reader would meet here, the position in the stream, the counts
        if (bb.bad) { *st = bam_fail(r, r->bam_ord + bb.bad_ord, r->bam_off + bb.bad_off, bb.bad == 1 ? BAM_INVALID : BAM_CUT); return GOT_ERROR; }
        r->bam_ord += bb.passed; r->bam_off += P.res.consumed;
        const lnr_bam_counts wc{P.res.n, bb.skipped, bb.reverse, bb.tiles, bb.repaired, bb.find_ms, bb.stitch_ms, bb.emit_ms};
        counts_add(r->bam_last, wc);
        P.parsed = true; P.passed = bb.passed; P.names = bb.names;
    }
    return GOT_WINDOW;
}

// a window was parsed: its names, its records and bases join the block and the totals
static void window_parsed(Call &c, const Parsed &P) {
    lnr_reader *r = c.r;
    for (uint64_t k = 0; k < P.res.n; k++) {
        const char *id = P.names.ids + P.names.id_off[k];
        r->ids.insert(r->ids.end(), id, id + P.names.id_len[k]);
        r->ids.push_back('\0'); r->id_off.push_back(r->ids.size());
    }
    c.n += (uint32_t)P.res.n; c.used += P.res.bases; r->records += P.res.n; r->bases += P.res.bases;
    r->g_recs += P.passed; r->g_text += P.res.consumed;
}

// the source learns what the window used up (`lead` bytes in front of the parsed text, `consumed` of it); the rest stays for the next
// window.  Returns the bytes that stay; false: a source that had to give way could not
static bool window_used(Call &c, const Window &W, const Parsed &P, uint64_t *left) {
    lnr_reader *r = c.r;
    const uint64_t consumed = P.parsed ? P.res.consumed : 0, adv = P.lead + consumed;
    switch (r->src) {
    case SRC_GZIP: case SRC_BGZF:
        r->dtext.keep_from = P.parsed ? consumed : P.lead;            // (a parse moves its text to the front of the device text)
        r->dtext.carry = *left = W.len - adv;
        if (r->src == SRC_BGZF) {
            lnr_win::chain_advance(r->chain, r->bskip, adv);
            if (r->bstop && !P.handover) return bgzf_give_way(r);     // (a hand-over ends the chain by itself)
        }
        break;
    case SRC_MAP: r->mpos += consumed; *left = W.w.len - consumed; break;
    case SRC_STREAM: put_back(r, W.w.text + consumed, *left = W.w.len - consumed); break;
    }
    return true;
}

// the serial parser takes the rest of the file: the stream goes on at the first byte the device has not used up
static bool to_serial(lnr_reader *r) {
    if (r->src == SRC_GZIP) return gz_to_stream(r);
    if (r->src == SRC_BGZF) return bgzf_to_stream(r);
    if (r->src == SRC_MAP) { r->src = SRC_STREAM; gzseek(r->f, (z_off_t)r->mpos, SEEK_SET); r->pos = r->end = 0; r->eof = false; }
    return true;
}

extern "C" {

lnr_status lnr_reader_open(const char *path, lnr_reader **out) {
    if (!path || !out) return LNR_ERR_ARG;
    *out = nullptr;
    lnr_reader *r = new (std::nothrow) lnr_reader();
    if (!r) return LNR_ERR_NOMEM;
    r->f = gzopen(path, "rb");
    if (!r->f) { delete r; return LNR_ERR_ARG; }
    gzbuffer(r->f, 1u << 20);
    r->buf.resize(4u << 20);
    r->path = path;
    if (!getenv("LNR_READER_SERIAL")) {
        int fd = open(path, O_RDONLY);
        struct stat st;
        unsigned char magic[2] = {0, 0};
        if (fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 2 && pread(fd, magic, 2, 0) == 2 && !(magic[0] == 0x1f && magic[1] == 0x8b)) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) { r->map = (const unsigned char *)m; r->map_len = (size_t)st.st_size; r->src = SRC_MAP; (void)madvise(m, r->map_len, MADV_SEQUENTIAL); }
        } else if (fd >= 0 && magic[0] == 0x1f && magic[1] == 0x8b && S_ISREG(st.st_mode) && st.st_size >= 18 && !(getenv("LNR_READER_BGZF") && atoi(getenv("LNR_READER_BGZF")) == 0)) {
            // gzip: BGZF when the first member says so (the walk of the other members waits for the windows that need them)
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            uint32_t doff = 0;
            if (m != MAP_FAILED && lnr_inf::bgzf_member((const uint8_t *)m, (uint64_t)st.st_size, doff)) {
                r->map = (const unsigned char *)m; r->map_len = (size_t)st.st_size; (void)madvise(m, r->map_len, MADV_SEQUENTIAL);
                r->src = SRC_BGZF; r->bfd = fd; fd = -1;                 // (the serial and host paths still read through r->f)
            } else if (m != MAP_FAILED) munmap(m, (size_t)st.st_size);
        }
        if (fd >= 0) close(fd);
        unsigned hw = std::thread::hardware_concurrency();
        r->threads = hw ? (hw < 16 ? hw : 16) : 4;
        if (const char *e = getenv("LNR_READER_THREADS")) { int v = atoi(e); if (v >= 1 && v <= 256) r->threads = (unsigned)v; }
    }
    memset(r->tab, 4, sizeof r->tab);
    r->tab['A'] = r->tab['a'] = 0; r->tab['C'] = r->tab['c'] = 1; r->tab['G'] = r->tab['g'] = 2;
    r->tab['T'] = r->tab['t'] = r->tab['U'] = r->tab['u'] = 3;
    *out = r;
    return LNR_OK;
}

void lnr_reader_close(lnr_reader *r) {
    if (!r) return;
    if (r->gpu && lnr_rdgpu_close) lnr_rdgpu_close(r->gpu);
    if (r->f) gzclose(r->f);
    if (r->bfd >= 0) close(r->bfd);
    if (r->map) munmap((void *)r->map, r->map_len);
    delete r;
}

const char *lnr_reader_error(const lnr_reader *r) { return r ? r->err.c_str() : "null reader"; }

// 3 when the file is a BAM (looked up in the stream's first bytes where nothing was read yet), else the format decided so far
int lnr_reader_format(lnr_reader *r) {
    if (!r) return 0;
    if (r->format == 0 && r->src != SRC_MAP && r->fill() && lnr_bam::is_magic(r->buf.data() + r->pos, r->end - r->pos)) r->format = 3;
    return r->format;
}

// Next block of records: at most max_reads records and never more than dst_cap bases (a record that does not fit any more is left
// for the next call; one that could never fit is LNR_ERR_LIMIT).  off[0] = 0 .. off[*n_out] written.  *n_out == 0 at end of file.
// (the body of lnr_reader_next: the block holds n records / `used` bases already when the GPU twin hands the rest of a block to the serial parser)
static lnr_status next_from(lnr_reader *r, uint8_t *dst, uint64_t dst_cap, uint64_t *off, uint32_t max_reads, uint32_t *n_out, uint32_t n, uint64_t used,
                            bool serial_only) {
    if (r->have_spill) {
        if (r->spill.size() > dst_cap) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
        memcpy(dst, r->spill.data(), r->spill.size());
        used = r->spill.size();
        r->ids.insert(r->ids.end(), r->spill_id.begin(), r->spill_id.end());
        n = 1; off[1] = used; r->id_off.push_back(r->ids.size());
        r->have_spill = false; r->spill.clear(); r->spill_id.clear();
    }
    if (r->src == SRC_MAP && !r->have_spill && !serial_only) {
        struct Rec { size_t hdr, hdr_end, seq, seq_end; uint64_t nb; };
        std::vector<Rec> recs;
        const unsigned char *M = r->map;
        const size_t ML = r->map_len;
        auto is_ws = [](unsigned char c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t'; };
        size_t pos = r->mpos, fallback_at = (size_t)-1;
        uint64_t cum = 0;
        while (n + recs.size() < max_reads) {
            while (pos < ML && is_ws(M[pos])) pos++;
            if (pos >= ML) break;
            if (r->format == 0) r->format = M[pos] == '>' ? 1 : (M[pos] == '@' ? 2 : -1);
            if (r->format < 0 || M[pos] != (r->format == 1 ? '>' : '@')) { fallback_at = pos; break; }     // (the serial parser reports it)
            Rec q;
            q.hdr = pos + 1;
            const unsigned char *nl = (const unsigned char *)memchr(M + q.hdr, '\n', ML - q.hdr);
            q.hdr_end = nl ? (size_t)(nl - M) : ML;
            q.seq = q.hdr_end < ML ? q.hdr_end + 1 : ML;
            size_t next;
            if (r->format == 1) {
                size_t p = q.seq;
                for (;;) {
                    const unsigned char *g = p < ML ? (const unsigned char *)memchr(M + p, '>', ML - p) : nullptr;
                    if (!g) { q.seq_end = ML; break; }
                    if ((size_t)(g - M) == q.seq || g[-1] == '\n') { q.seq_end = (size_t)(g - M); break; }
                    p = (size_t)(g - M) + 1;
                }
                next = q.seq_end;
            } else {
                const unsigned char *e2 = q.seq < ML ? (const unsigned char *)memchr(M + q.seq, '\n', ML - q.seq) : nullptr;
                if (!e2 || (size_t)(e2 - M) + 1 >= ML || e2[1] != '+') { fallback_at = pos; break; }             // not the four-line form
                const unsigned char *e3 = (const unsigned char *)memchr(e2 + 1, '\n', ML - (size_t)(e2 + 1 - M));
                if (!e3) { fallback_at = pos; break; }
                const unsigned char *qs = e3 + 1;
                const unsigned char *e4 = (size_t)(qs - M) < ML ? (const unsigned char *)memchr(qs, '\n', ML - (size_t)(qs - M)) : nullptr;
                const unsigned char *qe = e4 ? e4 : M + ML;
                size_t sl = (size_t)(e2 - (M + q.seq)), ql = (size_t)(qe - qs);
                while (sl && M[q.seq + sl - 1] == '\r') sl--;
                while (ql && qs[ql - 1] == '\r') ql--;
                bool clean = sl == ql;
                for (size_t i = 0; clean && i < sl; i++) clean = !is_ws(M[q.seq + i]);
                for (size_t i = 0; clean && i < ql; i++) clean = !is_ws(qs[i]);
                if (!clean) { fallback_at = pos; break; }
                q.seq_end = q.seq + sl;
                next = (size_t)(qe - M);
            }
            uint64_t span = q.seq_end - q.seq;
            if (used + cum + span > dst_cap) {                       // the block may be full: decide by the record's exact number of bases
                uint64_t nb = 0;
                for (size_t i = q.seq; i < q.seq_end; i++) nb += !is_ws(M[i]);
                if (used + cum + nb > dst_cap) {
                    if (n + recs.size() == 0) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
                    break;
                }
            }
            cum += span;
            recs.push_back(q);
            pos = next;
        }
        const size_t R = recs.size();
        if (R) {
            unsigned T = r->threads < R ? r->threads : (unsigned)R;
            if (cum < (1u << 20)) T = 1;
            auto share = [&](unsigned t, size_t &a, size_t &b) { a = R * t / T; b = R * (t + 1) / T; };
            auto run = [&](auto fn) {
                std::vector<std::thread> th;
                for (unsigned t = 1; t < T; t++) th.emplace_back(fn, t);
                fn(0u);
                for (auto &x : th) x.join();
            };
            run([&](unsigned t) {                                     // pass 1: bases per record
                size_t a, b; share(t, a, b);
                for (size_t k = a; k < b; k++) {
                    uint64_t nb = 0;
                    const unsigned char *p = M + recs[k].seq, *e = M + recs[k].seq_end;
                    if (r->format == 2) nb = (uint64_t)(e - p);       // (a clean single line)
                    else for (; p < e; p++) nb += !is_ws(*p);
                    recs[k].nb = nb;
                }
            });
            for (size_t k = 0; k < R; k++) { off[n + k + 1] = off[n + k] + recs[k].nb; }
            if (off[n + R] > dst_cap) { r->err = "internal: block accounting"; return LNR_ERR_INTERNAL; }
            const unsigned char *tab = r->tab;
            run([&](unsigned t) {                                     // pass 2: convert into the caller's block
                size_t a, b; share(t, a, b);
                for (size_t k = a; k < b; k++) {
                    uint8_t *d = dst + off[n + k];
                    const unsigned char *p = M + recs[k].seq, *e = M + recs[k].seq_end;
                    if (r->format == 2) { for (; p < e; p++) *d++ = tab[*p]; }
                    else for (; p < e; p++) { unsigned char ch = *p; if (!is_ws(ch)) *d++ = tab[ch]; }
                }
            });
            for (size_t k = 0; k < R; k++) {
                size_t he = recs[k].hdr_end;
                while (he > recs[k].hdr && M[he - 1] == '\r') he--;
                r->ids.insert(r->ids.end(), (const char *)M + recs[k].hdr, (const char *)M + he);
                r->ids.push_back('\0');
                r->id_off.push_back(r->ids.size());
                r->bases += recs[k].nb;
            }
            r->records += R;
            n += (uint32_t)R;
            used = off[n];
        }
        r->mpos = pos;
        if (fallback_at != (size_t)-1) {                              // the serial parser takes over from this record on
            r->src = SRC_STREAM;
            gzseek(r->f, (z_off_t)fallback_at, SEEK_SET);
            r->pos = r->end = 0; r->eof = false;
        } else { *n_out = n; return LNR_OK; }
    }
    if (r->format == 0 && r->fill() && lnr_bam::is_magic(r->buf.data() + r->pos, r->end - r->pos)) r->format = 3;
    if (r->format == 3) return bam_next(r, dst, dst_cap, off, max_reads, n_out, n, used);
    while (n < max_reads) {
        int c;
        while ((c = r->peek()) == '\n' || c == '\r' || c == ' ' || c == '\t') r->pos++;     // blank lines between records
        if (c < 0) break;
        if (r->format == 0) r->format = c == '>' ? 1 : (c == '@' ? 2 : -1);
        if (r->format < 0 || c != (r->format == 1 ? '>' : '@')) { r->err = "record does not start with '>' / '@'"; return LNR_ERR_ARG; }
        r->pos++;
        size_t id_start = r->ids.size();
        r->line(&r->ids);
        r->ids.push_back('\0');
        uint64_t start = used, len = 0;
        bool spilling = false;
        // bases of one line (or what is left of it) -> dst, or -> the spill buffer once the block is full
        auto seq_line = [&]() {
            while (r->fill()) {
                unsigned char *p = r->buf.data() + r->pos, *e = r->buf.data() + r->end;
                bool eol = false;
                for (; p < e; p++) {
                    unsigned char ch = *p;
                    if (ch == '\n') { eol = true; p++; break; }
                    if (ch == '\r' || ch == ' ' || ch == '\t') continue;
                    if (!spilling && used < dst_cap) dst[used++] = r->tab[ch];
                    else {
                        if (!spilling) { r->spill.assign(dst + start, dst + used); used = start; spilling = true; }
                        r->spill.push_back(r->tab[ch]);
                    }
                    len++;
                }
                r->pos = (size_t)(p - r->buf.data());
                if (eol) break;
            }
        };
        if (r->format == 1) {
            while ((c = r->peek()) >= 0 && c != '>') seq_line();
        } else {
            while ((c = r->peek()) >= 0 && c != '+') seq_line();   // sequence lines up to the '+' line ...
            if (c == '+') r->line(nullptr);
            uint64_t got = 0;                                      // ... then as many quality characters as there were bases
            while (got < len && r->fill()) {
                unsigned char ch = r->buf[r->pos++];
                if (ch == '\n' || ch == '\r' || ch == ' ' || ch == '\t') continue;
                got++;
            }
            if (got < len) { r->err = "FASTQ record with fewer qualities than bases"; return LNR_ERR_ARG; }
            if (len) r->line(nullptr);                             // rest of the last quality line
        }
        r->records++;
        r->bases += len;
        if (spilling) {                                            // keep it for the next block
            r->spill_id.assign(r->ids.begin() + (long)id_start, r->ids.end());
            r->ids.resize(id_start);
            r->have_spill = true;
            if (n == 0 && r->spill.size() > dst_cap) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
            break;
        }
        n++;
        off[n] = used;
        r->id_off.push_back(r->ids.size());
    }
    *n_out = n;
    return LNR_OK;
}

lnr_status lnr_reader_next(lnr_reader *r, uint8_t *dst, uint64_t dst_cap, uint64_t *off, uint32_t max_reads, uint32_t *n_out) {
    if (!r || !dst || !off || !n_out) return LNR_ERR_ARG;
    *n_out = 0;
    off[0] = 0;
    r->ids.clear(); r->id_off.assign(1, 0);
    r->started = true;
    if (r->src == SRC_GZIP) {
        if (r->gz_failed) { r->err = r->gerr; return LNR_ERR_ARG; }
        if (r->text_made == 0) r->src = SRC_STREAM;                   // nothing was read on the device: r->f stands at the start of the file
        else if (!gz_to_stream(r)) return LNR_ERR_ARG;
    }
    if (r->src == SRC_BGZF) {
        if (r->bpos == 0 && r->chain.empty()) r->src = SRC_STREAM;   // nothing was read on the device: r->f stands at the start of the file, as ever
        else if (!bgzf_to_stream(r)) return LNR_ERR_ARG;              // next_dev has read ahead on the device: the stream goes on where it stopped
    }
    const uint64_t gz0 = r->gz_bytes;
    const lnr_status s = next_from(r, dst, dst_cap, off, max_reads, n_out, 0, 0, false);
    if (r->gzp) r->gzs_total.gzread_bytes += r->gz_bytes - gz0;      // (the total counts what this entry point read through gzread, too)
    return s;
}

// ---- the GPU twin: the same blocks, parsed on the device into device memory (lnr_reader_kernels.hip behind lnr_reader_hook.h)
lnr_status lnr_reader_gpu_open(lnr_reader *r, int32_t device, uint32_t slots) {
    if (!r) return LNR_ERR_ARG;
    if (slots < 1 || slots > 8) { r->err = "lnr_reader_gpu_open: slots must be 1..8"; return LNR_ERR_ARG; }
    if (r->gpu) { r->err = "lnr_reader_gpu_open: the reader has a GPU side already"; return LNR_ERR_ARG; }
    if (!lnr_rdgpu_open) {
        snprintf(r->gerr, sizeof r->gerr, "no usable device %d: this library was linked without its device half", (int)device);
        r->err = r->gerr;
        return LNR_ERR_NO_DEVICE;
    }
    lnr_status s = (lnr_status)lnr_rdgpu_open(device, slots, &r->gpu, r->gerr, sizeof r->gerr);
    if (s != LNR_OK) { r->err = r->gerr; return s; }
    r->gslots = slots; r->gslot = 0;
    return LNR_OK;
}

// for lnr_genome.cpp (declared in lnr_reader_hook.h): a copy of the block delivered last, in device memory of its own; the records passed so far
int lnr_reader_keep_block(lnr_reader *r, uint64_t bytes, uint8_t **d_out, int32_t *device) {
    if (!r || !d_out || !device) return LNR_ERR_ARG;
    if (!r->gpu || !r->last_block || bytes > r->last_bases) { r->err = "lnr_reader_keep_block: no delivered block of that size"; return LNR_ERR_ARG; }
    if (!lnr_rdgpu_keep || !lnr_rdgpu_device) { r->err = "this library was linked without its device half"; return LNR_ERR_NO_DEVICE; }
    if (int s = lnr_rdgpu_keep(r->gpu, r->last_block, bytes, d_out, r->gerr, sizeof r->gerr)) { r->err = r->gerr; return s; }
    *device = lnr_rdgpu_device(r->gpu);
    return LNR_OK;
}
uint64_t lnr_reader_records(const lnr_reader *r) { return r ? r->records : 0; }

uint32_t lnr_reader_gpu_tile(void) { return lnr_rdgpu_tile ? lnr_rdgpu_tile() : 0; }
uint32_t lnr_reader_gpu_bam_tile(void) { return lnr_rdgpu_bam_tile ? lnr_rdgpu_bam_tile() : 0; }

lnr_status lnr_reader_gpu_bam_stats(const lnr_reader *r, lnr_bam_stats *out) {
    if (!r || !out || !r->gpu) return LNR_ERR_ARG;
    out->last = r->bam_last; out->total = r->bam_total;
    return LNR_OK;
}

lnr_status lnr_reader_gpu_times(const lnr_reader *r, double *ms5) {
    if (!r || !ms5 || !r->gpu) return LNR_ERR_ARG;
    lnr_rdgpu_times(r->gpu, ms5);
    return LNR_OK;
}

lnr_status lnr_reader_gpu_inflate_stats(const lnr_reader *r, lnr_inflate_stats *out) {
    if (!r || !out || !r->gpu) return LNR_ERR_ARG;
    out->last = r->ist_last; out->total = r->ist_total;
    return LNR_OK;
}

static_assert(sizeof(lnr_gzip_counts) == sizeof(lnr_rdgpu_gz_counts), "lnr_rdgpu_gz_counts has the layout of lnr_gzip_counts");
static void gz_counts_out(lnr_gzip_counts &o, const lnr_rdgpu_gz_counts &c) { memcpy(&o, &c, sizeof o); }

lnr_status lnr_reader_gpu_gzip(lnr_reader *r, int on) {
    if (!r) return LNR_ERR_ARG;
    if (!r->gpu) { r->err = "lnr_reader_gpu_gzip: lnr_reader_gpu_open has not been called on this reader"; return LNR_ERR_ARG; }
    if (r->started) { r->err = "lnr_reader_gpu_gzip: the reader has been read from"; return LNR_ERR_ARG; }
    if (!lnr_rdgpu_gzip_round) { r->err = "lnr_reader_gpu_gzip: this library was linked without its device half"; return LNR_ERR_NO_DEVICE; }
    if (!on) {
        if (r->src == SRC_GZIP) { r->src = SRC_STREAM; if (r->map) munmap((void *)r->map, r->map_len); r->map = nullptr; r->map_len = 0; }
        r->gzp = false;
        return LNR_OK;
    }
    if (r->gzp) return LNR_OK;
    if (getenv("LNR_READER_SERIAL") || (getenv("LNR_READER_BGZF") && atoi(getenv("LNR_READER_BGZF")) == 0)) return LNR_OK;   // the file is read as any gzip file
    r->gzp = true;
    if (r->src != SRC_STREAM || r->map) return LNR_OK;              // BGZF keeps precedence (the rounds take over at a member that is not BGZF); plain text
    int fd = open(r->path.c_str(), O_RDONLY);
    struct stat st;
    unsigned char magic[2] = {0, 0};
    if (fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 10 && (uint64_t)st.st_size <= (1ULL << 40) && pread(fd, magic, 2, 0) == 2 &&
        magic[0] == 0x1f && magic[1] == 0x8b) {
        void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) {
            r->map = (const unsigned char *)m; r->map_len = (size_t)st.st_size; (void)madvise(m, r->map_len, MADV_SEQUENTIAL);
            r->src = SRC_GZIP;
        }
    }
    if (fd >= 0) close(fd);
    return LNR_OK;
}

lnr_status lnr_reader_gpu_gzip_stats(const lnr_reader *r, lnr_gzip_stats *out) {
    if (!r || !out || !r->gpu) return LNR_ERR_ARG;
    gz_counts_out(out->last, r->gzs_last); gz_counts_out(out->total, r->gzs_total);
    return LNR_OK;
}

// plain gzip over a host buffer: the stages of the reader's gzip rounds, no parse
lnr_status lnr_gunzip_gpu(int32_t device, const uint8_t *gz, uint64_t size, uint8_t *text, uint64_t text_cap, uint64_t *text_size, lnr_gzip_stats *stats,
                          char *err, size_t err_cap) {
    char local[256] = "";
    if (!err || !err_cap) { err = local; err_cap = sizeof local; }
    err[0] = 0;
    if ((!gz && size) || (!text && text_cap) || !text_size) { snprintf(err, err_cap, "lnr_gunzip_gpu: null argument"); return LNR_ERR_ARG; }
    *text_size = 0;
    if (stats) *stats = lnr_gzip_stats{};
    if (!lnr_rdgpu_gunzip) { snprintf(err, err_cap, "no usable device %d: this library was linked without its device half", (int)device); return LNR_ERR_NO_DEVICE; }
    lnr_rdgpu_gz_counts last{}, total{};
    uint64_t bad_off = 0;
    uint32_t bad = 0;
    const int s = lnr_rdgpu_gunzip(device, gz, size, text, text_cap, text_size, &last, &total, &bad_off, &bad, err, err_cap);
    if (stats) { gz_counts_out(stats->last, last); gz_counts_out(stats->total, total); }
    if (s) return (lnr_status)s;
    if (bad) { snprintf(err, err_cap, "gzip data at file offset %llu: %s", (unsigned long long)bad_off, lnr_gz::status_text(bad)); return LNR_ERR_ARG; }
    return LNR_OK;
}

// Windows of text go to the device until the block is full, the file ends or the four-line FASTQ form breaks (hand-over: the serial parser
// takes the rest of the file, its records are uploaded).  LNR_READER_GPU_WINDOW = bytes of text per window (default 256 MiB; a window that
// holds no whole record is doubled): block boundaries do not depend on it.
lnr_status lnr_reader_next_dev(lnr_reader *r, uint64_t dst_cap, uint32_t max_reads, const uint8_t **d_reads_concat, const uint64_t **d_off,
                               const uint64_t **off, uint32_t *n_out) {
    if (!r || !d_reads_concat || !d_off || !off || !n_out) return LNR_ERR_ARG;
    *n_out = 0;
    if (!r->gpu) { r->err = "lnr_reader_gpu_open has not been called on this reader"; return LNR_ERR_ARG; }
    Call c{r, r->gslot};
    r->last_block = nullptr; r->last_bases = 0;
    uint8_t *dr; uint64_t *dof, *ho;
    if (int s = lnr_rdgpu_block(r->gpu, c.slot, dst_cap, max_reads, &dr, &dof, &ho, r->gerr, sizeof r->gerr)) { r->err = r->gerr; return (lnr_status)s; }
    r->gslot = (c.slot + 1) % r->gslots;
    lnr_rdgpu_times_reset(r->gpu);
    r->ids.clear(); r->id_off.assign(1, 0);
    r->ist_last = lnr_inflate_counts{};
    r->bam_last = lnr_bam_counts{};
    r->gzs_last = lnr_rdgpu_gz_counts{};
    r->started = true;
    if (r->bam_failed) return LNR_ERR_ARG;
    struct StatsAtExit {                                          // the counts of this call join the totals however it ends
        lnr_reader *r; uint64_t gz0;
        ~StatsAtExit() {
            double ms2[2] = {0, 0}, ms5[5] = {0, 0, 0, 0, 0};
            if (lnr_rdgpu_inflate_times) lnr_rdgpu_inflate_times(r->gpu, ms2);
            r->ist_last.gzread_bytes = r->gz_bytes - gz0; r->ist_last.inflate_ms = ms2[0]; r->ist_last.gather_ms = ms2[1];
            counts_add(r->ist_total, r->ist_last);
            counts_add(r->bam_total, r->bam_last);
            if (!r->gzp) return;
            lnr_rdgpu_times(r->gpu, ms5);
            r->gzs_last.gzread_bytes = r->gz_bytes - gz0; r->gzs_last.parse_ms = ms5[1] + ms5[2] + ms5[3]; r->gzs_last.download_ms = ms5[4];
            lnr_rdgpu_gz_add(&r->gzs_total, &r->gzs_last);
        }
    } stats_at_exit{r, r->gz_bytes};
    uint64_t wcap = lnr_win::WINDOW_CAP;
    if (const char *e = getenv("LNR_READER_GPU_WINDOW")) { long long v = atoll(e); if (v >= 16) wcap = (uint64_t)v; }
    if (wcap > lnr_win::WINDOW_MAX) wcap = lnr_win::WINDOW_MAX;
    bool full = false, more = true;
    while (more && !r->gpu_serial && !r->have_spill && c.n < max_reads) {
        Window W;
        W.w.slot = c.slot; W.w.threads = r->threads;
        W.w.rec_base = c.n; W.w.base_base = c.used; W.w.allowed = max_reads - c.n; W.w.free = dst_cap - c.used;
        const uint64_t want = lnr_win::window_size(W.w.free, W.w.allowed, r->format == 1, r->g_text, r->g_recs, wcap, c.grow);
        const Src src = r->src;
        lnr_status st = LNR_OK;
        Got got = src == SRC_GZIP ? gzip_window(c, want, W, &st) : src == SRC_BGZF ? bgzf_window(c, want, W, &st) : src == SRC_MAP ? map_window(c, want, W, &st) : stream_window(c, want, W, &st);
        Parsed P;
        W.w.eof = W.ended;
        if (got == GOT_WINDOW) got = parse_window(c, W, P, &st);
        if (got == GOT_AGAIN) continue;
        if (got != GOT_WINDOW) { if (got == GOT_ERROR) return st; break; }
        const bool bam = r->format == 3;
        window_parsed(c, P);
        lnr_win::Seen s{};
        if (!window_used(c, W, P, &s.left)) return LNR_ERR_ARG;
        s.site = src == SRC_GZIP ? lnr_win::GZIP_TEXT : src == SRC_BGZF ? (bam ? lnr_win::BGZF_BAM : lnr_win::BGZF_TEXT) : bam ? lnr_win::STREAM_BAM : lnr_win::HOST_TEXT;
        s.handover = P.handover; s.too_big = P.res.too_big; s.full = P.res.full; s.n_block = c.n;
        s.parsed = P.parsed; s.taken = P.res.n; s.consumed = P.res.consumed; s.len = W.len;
        s.ended = W.ended; s.live = r->src == src; s.stuck = W.stuck; s.failed = src == SRC_GZIP && r->gz_failed;
        switch (lnr_win::decide(s)) {
        case lnr_win::HAND_OVER: if (!to_serial(r)) return LNR_ERR_ARG; r->gpu_serial = true; break;
        case lnr_win::BLOCK_FULL: full = true; more = false; break;
        case lnr_win::SOURCE_END: more = false; break;
        case lnr_win::GROW_WINDOW: c.grow *= 2; break;
        case lnr_win::NEXT_WINDOW: break;
        case lnr_win::ERR_BLOCK: r->err = "a record is longer than the block"; return LNR_ERR_LIMIT;
        case lnr_win::ERR_WINDOW: r->err = TOO_LONG; return LNR_ERR_LIMIT;
        case lnr_win::ERR_SOURCE: r->err = r->gerr; return LNR_ERR_ARG;
        }
    }
    uint32_t n = c.n;
    if ((r->gpu_serial || r->have_spill) && !full && n < max_reads) {   // the serial parser's share of the block, through a host block
        if (r->hblock_cap < dst_cap) {
            r->hblock.reset(new (std::nothrow) uint8_t[dst_cap ? dst_cap : 1]);
            if (!r->hblock) { r->hblock_cap = 0; r->err = "host allocation failed"; return LNR_ERR_NOMEM; }
            r->hblock_cap = dst_cap;
        }
        uint32_t n2 = n;
        lnr_status s = next_from(r, r->hblock.get(), dst_cap, ho, max_reads, &n2, n, c.used, true);
        if (s != LNR_OK) return s;
        if (int s2 = lnr_rdgpu_append(r->gpu, c.slot, c.used, r->hblock.get() + c.used, ho[n2] - c.used, n, ho + n, n2 - n, r->gerr, sizeof r->gerr)) { r->err = r->gerr; return (lnr_status)s2; }
        n = n2;
    }
    *d_reads_concat = dr; *d_off = dof; *off = ho; *n_out = n;
    r->last_block = dr; r->last_bases = ho[n];
    return LNR_OK;
}

// ids of the last block: *ids = '\0'-separated header lines, id_off[k] = start of id k (n + 1 entries)
lnr_status lnr_reader_ids(const lnr_reader *r, const char **ids, const uint64_t **id_off) {
    if (!r || !ids || !id_off) return LNR_ERR_ARG;
    *ids = r->ids.data();
    *id_off = r->id_off.data();
    return LNR_OK;
}

}  // extern "C"
