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

struct lnr_reader {
    gzFile f = nullptr;
    std::vector<unsigned char> buf;
    size_t pos = 0, end = 0;
    bool eof = false;
    int format = 0;              // 0 unknown, 1 FASTA, 2 FASTQ, 3 BAM (by content: the first four inflated bytes)
    std::string err;
    std::vector<char> ids;       // ids of the last block, '\0' separated
    std::vector<uint8_t> spill;  // a record that did not fit the last block any more (a gzip stream cannot be rewound): first record of the next
    std::vector<char> spill_id;
    bool have_spill = false;
    std::vector<uint64_t> id_off;
    uint64_t records = 0, bases = 0;
    unsigned char tab[256];
    // the mapped file of the parallel path (plain files only)
    const unsigned char *map = nullptr; size_t map_len = 0, mpos = 0; bool use_map = false; unsigned threads = 8;
    // the GPU twin (lnr_reader_gpu_open / lnr_reader_next_dev): its device side, the slot of the next block, "the serial parser has taken over",
    // "the inflate stream has ended", and the host block the serial parser's records pass through on their way up
    lnr_rdgpu *gpu = nullptr; uint32_t gslots = 0, gslot = 0; bool gpu_serial = false, gz_done = false;
    std::unique_ptr<uint8_t[]> hblock; uint64_t hblock_cap = 0;
    uint64_t g_text = 0, g_recs = 0;     // text bytes and records the windows have used up so far: sizes the next window
    char gerr[256] = "";
    // BGZF (device inflate): the file is mapped at `map` with use_map false.  The chain is walked one window at a time from bpos on;
    // `chain` = the blocks whose text lies on the device and is not used up, byte 0 of the device text = byte bskip of chain[0]'s text
    struct BBlk { uint64_t off; uint32_t size, isize; };
    bool bgzf = false, bend = false, bstop = false, bfailed = false;   // live; the chain reached the end of the file; the member at bpos is not BGZF
    int bfd = -1;
    uint64_t bpos = 0, bskip = 0, bkeep_from = 0, bcarry = 0;         // device text [bkeep_from, bkeep_from + bcarry) is what the last window left
    std::vector<BBlk> chain;
    lnr_inflate_counts ist_last{}, ist_total{};
    uint64_t gz_bytes = 0;                                            // text bytes that came out of gzread
    // BAM: the header has been passed; a record was refused (the reader can only be closed); the header's n_ref; records passed so far
    // (skipped ones included) and the offset of the next one in the uncompressed stream -- what an error message names
    bool bam_hdr = false, bam_failed = false;
    int32_t bam_nref = 0;
    uint64_t bam_ord = 0, bam_off = 0;
    std::vector<unsigned char> bam_tmp;
    lnr_bam_counts bam_last{}, bam_total{};
    // plain gzip on the device (lnr_reader_gpu_gzip): the file is mapped at `map` with use_map false, as for BGZF.  gz_live: the rounds
    // read the file from gz_pos (a member's header) or, inside a member, from bit gz_bit of the file.  The device text
    // [gkeep_from, gkeep_from + gcarry) is what the last window left; text_made = text bytes the device has inflated so far (BGZF blocks
    // included), so text_made - gcarry is the offset in the uncompressed stream at which a gzread stream would go on
    std::string path;
    bool started = false, gzp = false, gz_live = false, gz_in_member = false, gz_end = false, gz_failed = false;
    uint64_t gz_pos = 0, gz_bit = 0, gz_mtext = 0, gkeep_from = 0, gcarry = 0, text_made = 0, gz_grow = 1;
    uint32_t gz_hist = 0, gz_crc = 0;
    lnr_rdgpu_gz_counts gzs_last{}, gzs_total{};

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
    r->bgzf = false; r->chain.clear(); r->bskip = r->bcarry = r->bkeep_from = 0;
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
    const uint64_t at = r->text_made - r->gcarry;
    r->gz_live = false; r->gcarry = r->gkeep_from = 0;
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
// the member at gz_pos, or the end of the file's members.  LNR_OK, or the header's error
static lnr_status gz_next_member(lnr_reader *r) {
    while (!r->gz_in_member && !r->gz_end) {
        if (r->gz_pos >= r->map_len) { r->gz_end = true; break; }
        uint64_t data = 0;
        const uint32_t st = lnr_gz::member_at(r->map, r->map_len, r->gz_pos, r->gz_pos == 0, &data);
        if (st == lnr_gz::PASS_OVER) { r->gz_end = true; break; }
        if (st) return gz_fail(r, st, r->gz_pos);
        r->gz_bit = data * 8; r->gz_in_member = true; r->gz_hist = 0; r->gz_crc = 0; r->gz_mtext = 0;
    }
    return LNR_OK;
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
            if (m != MAP_FAILED) { r->map = (const unsigned char *)m; r->map_len = (size_t)st.st_size; r->use_map = true; (void)madvise(m, r->map_len, MADV_SEQUENTIAL); }
        } else if (fd >= 0 && magic[0] == 0x1f && magic[1] == 0x8b && S_ISREG(st.st_mode) && st.st_size >= 18 && !(getenv("LNR_READER_BGZF") && atoi(getenv("LNR_READER_BGZF")) == 0)) {
            // gzip: BGZF when the first member says so (the walk of the other members waits for the windows that need them)
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            uint32_t doff = 0;
            if (m != MAP_FAILED && lnr_inf::bgzf_member((const uint8_t *)m, (uint64_t)st.st_size, doff)) {
                r->map = (const unsigned char *)m; r->map_len = (size_t)st.st_size; (void)madvise(m, r->map_len, MADV_SEQUENTIAL);
                r->bgzf = true; r->bfd = fd; fd = -1;                 // (the serial and host paths still read through r->f)
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
    if (r->format == 0 && !r->use_map && r->fill() && lnr_bam::is_magic(r->buf.data() + r->pos, r->end - r->pos)) r->format = 3;
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
    if (r->use_map && !r->have_spill && !serial_only) {
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
            r->use_map = false;
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
    if (r->gz_live) {
        if (r->gz_failed) { r->err = r->gerr; return LNR_ERR_ARG; }
        if (r->text_made == 0) r->gz_live = false;                    // nothing was read on the device: r->f stands at the start of the file
        else if (!gz_to_stream(r)) return LNR_ERR_ARG;
    }
    if (r->bgzf) {
        if (r->bpos == 0 && r->chain.empty()) r->bgzf = false;       // nothing was read on the device: r->f stands at the start of the file, as ever
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
        if (r->gz_live) { r->gz_live = false; if (r->map) munmap((void *)r->map, r->map_len); r->map = nullptr; r->map_len = 0; }
        r->gzp = false;
        return LNR_OK;
    }
    if (r->gzp) return LNR_OK;
    if (getenv("LNR_READER_SERIAL") || (getenv("LNR_READER_BGZF") && atoi(getenv("LNR_READER_BGZF")) == 0)) return LNR_OK;   // the file is read as any gzip file
    r->gzp = true;
    if (r->bgzf || r->use_map || r->map) return LNR_OK;              // BGZF keeps precedence (the rounds take over at a member that is not BGZF); plain text
    int fd = open(r->path.c_str(), O_RDONLY);
    struct stat st;
    unsigned char magic[2] = {0, 0};
    if (fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 10 && (uint64_t)st.st_size <= (1ULL << 40) && pread(fd, magic, 2, 0) == 2 &&
        magic[0] == 0x1f && magic[1] == 0x8b) {
        void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) {
            r->map = (const unsigned char *)m; r->map_len = (size_t)st.st_size; (void)madvise(m, r->map_len, MADV_SEQUENTIAL);
            r->gz_live = true; r->gz_pos = 0;
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
    auto gfail = [&](int s) { r->err = r->gerr; return (lnr_status)s; };
    const uint32_t slot = r->gslot;
    uint8_t *dr; uint64_t *dof, *ho;
    if (int s = lnr_rdgpu_block(r->gpu, slot, dst_cap, max_reads, &dr, &dof, &ho, r->gerr, sizeof r->gerr)) return gfail(s);
    r->gslot = (slot + 1) % r->gslots;
    lnr_rdgpu_times_reset(r->gpu);
    r->ids.clear(); r->id_off.assign(1, 0);
    r->ist_last = lnr_inflate_counts{};
    r->bam_last = lnr_bam_counts{};
    r->gzs_last = lnr_rdgpu_gz_counts{};
    r->started = true;
    if (r->bam_failed) return LNR_ERR_ARG;
    const uint64_t gz0 = r->gz_bytes;
    struct StatsAtExit {                                          // the counts of this call join the totals however it ends
        lnr_reader *r; uint64_t gz0;
        ~StatsAtExit() {
            lnr_inflate_counts &l = r->ist_last, &t = r->ist_total;
            double ms2[2] = {0, 0};
            if (lnr_rdgpu_inflate_times) lnr_rdgpu_inflate_times(r->gpu, ms2);
            l.gzread_bytes = r->gz_bytes - gz0; l.inflate_ms = ms2[0]; l.gather_ms = ms2[1];
            t.blocks += l.blocks; t.compressed_bytes += l.compressed_bytes; t.text_bytes += l.text_bytes; t.gzread_bytes += l.gzread_bytes;
            t.inflate_ms += l.inflate_ms; t.gather_ms += l.gather_ms;
            lnr_bam_counts &bl = r->bam_last, &bt = r->bam_total;
            bt.records += bl.records; bt.skipped += bl.skipped; bt.reverse += bl.reverse; bt.tiles += bl.tiles; bt.repaired_tiles += bl.repaired_tiles;
            bt.find_ms += bl.find_ms; bt.stitch_ms += bl.stitch_ms; bt.emit_ms += bl.emit_ms;
            if (r->gzp) {
                double ms5[5] = {0, 0, 0, 0, 0};
                lnr_rdgpu_times(r->gpu, ms5);
                r->gzs_last.gzread_bytes = r->gz_bytes - gz0; r->gzs_last.parse_ms = ms5[1] + ms5[2] + ms5[3]; r->gzs_last.download_ms = ms5[4];
                lnr_rdgpu_gz_add(&r->gzs_total, &r->gzs_last);
            }
        }
    } stats_at_exit{r, gz0};
    uint64_t wcap = 256ULL << 20, grow = 1, used = 0;
    if (const char *e = getenv("LNR_READER_GPU_WINDOW")) { long long v = atoll(e); if (v >= 16) wcap = (uint64_t)v; }
    if (wcap > (1ULL << 30)) wcap = 1ULL << 30;
    uint32_t n = 0;
    bool full = false;
    auto is_ws = [](unsigned char c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t'; };
    // BAM: what a window's parse leaves behind it -- the error the host reader would meet here, the position in the stream, the counts, the names
    auto bam_done = [&](const lnr_rdgpu_result &res, const lnr_rdgpu_bam_result &bb) -> lnr_status {
        if (bb.bad) return bam_fail(r, r->bam_ord + bb.bad_ord, r->bam_off + bb.bad_off, bb.bad == 1 ? BAM_INVALID : BAM_CUT);
        r->bam_ord += bb.passed; r->bam_off += res.consumed;
        lnr_bam_counts &c = r->bam_last;
        c.records += res.n; c.skipped += bb.skipped; c.reverse += bb.reverse; c.tiles += bb.tiles; c.repaired_tiles += bb.repaired;
        c.find_ms += bb.find_ms; c.stitch_ms += bb.stitch_ms; c.emit_ms += bb.emit_ms;
        for (uint64_t k = 0; k < res.n; k++) {
            r->ids.insert(r->ids.end(), bb.ids + bb.id_off[k], bb.ids + bb.id_off[k] + bb.id_len[k]);
            r->ids.push_back('\0');
            r->id_off.push_back(r->ids.size());
        }
        return LNR_OK;
    };
    auto bam_header_fail = [&](const char *why) { r->err = why; r->bam_failed = true; return LNR_ERR_ARG; };
    while (!r->gpu_serial && !r->have_spill && n < max_reads) {
        const uint64_t freeb = dst_cap - used, allowed = max_reads - n;
        // the window: what the free bases can take as text, but no more than the records still allowed will probably need -- by the bytes
        // per record seen so far (a first window guesses 1 KiB per record; a window that runs out is followed by the next one)
        uint64_t want = freeb * (r->format == 1 ? 1 : 2) + freeb / 50 + allowed * 128 + 65536;
        const uint64_t per_rec = r->g_recs ? r->g_text / r->g_recs + 1 : 1024;
        const uint64_t by_recs = allowed * (per_rec + per_rec / 8) + 65536;
        if (want > by_recs) want = by_recs;
        if (want > wcap) want = wcap;
        want *= grow;
        if (want > (1ULL << 30)) want = 1ULL << 30;
        lnr_rdgpu_window w{};
        const unsigned char *text = nullptr;
        uint64_t len = 0, lead = 0;
        bool eof = false;
        if (r->gz_live) {                                         // plain gzip: rounds of the member inflated on the device behind what the last window left
            if (r->gz_failed) { if (n) break; r->err = r->gerr; return LNR_ERR_ARG; }
            const uint64_t chunk = lnr_gz::env_bytes("LNR_READER_GZ_CHUNK", 128ULL << 10, 1024, 1ULL << 30), round = lnr_gz::env_bytes("LNR_READER_GZ_ROUND", 64ULL << 20, 1024, 1ULL << 31);
            constexpr uint64_t TEXT_MAX = (1ULL << 30) - 65536;
            bool stuck = false;
            if (lnr_status s = gz_next_member(r)) { if (n) break; return s; }
            while (!r->gz_end && !r->gz_failed && r->gcarry < want && !stuck) {
                const uint64_t rb = r->gz_bit >> 3;
                if (rb >= r->map_len) { gz_fail(r, lnr_inf::E_INPUT_END, r->map_len); break; }      // the file ends behind a member's header
                if (r->gcarry >= TEXT_MAX) { stuck = true; break; }
                uint64_t rsize = want - r->gcarry + 2 * chunk;            // text is seldom smaller than its compressed bytes: no more of them than text is wanted
                if (rsize > round) rsize = round;
                if (rsize > (1ULL << 31) / r->gz_grow) rsize = 1ULL << 31; else rsize *= r->gz_grow;
                const uint64_t clen = r->map_len - rb < rsize ? r->map_len - rb : rsize;
                lnr_rdgpu_gzip job{};
                job.comp = r->map + rb; job.comp_len = clen; job.start_bit = (uint32_t)(r->gz_bit & 7); job.hist = r->gz_hist; job.chunk = chunk;
                job.keep_from = r->gkeep_from; job.carry = r->gcarry; job.text_cap = TEXT_MAX - r->gcarry; job.threads = r->threads;
                lnr_rdgpu_gzip_result gr{};
                if (int s = lnr_rdgpu_gzip_round(r->gpu, &job, &gr, r->gerr, sizeof r->gerr)) { r->gz_failed = true; return gfail(s); }
                lnr_rdgpu_gz_counts c = gr.counts;
                if (gr.status) { lnr_rdgpu_gz_add(&r->gzs_last, &c); gz_fail(r, gr.status, rb + gr.bad_off); break; }
                if (!gr.pieces) {                                 // no block completed
                    c.grown_rounds = 1;
                    lnr_rdgpu_gz_add(&r->gzs_last, &c);
                    if (gr.stop == lnr_gz::AT_BUDGET) { stuck = true; break; }                     // the device text is full: what it holds is parsed first
                    if (rb + clen >= r->map_len) { gz_fail(r, lnr_inf::E_INPUT_END, rb); break; }
                    if (rsize >= (1ULL << 31)) { r->err = "a DEFLATE block is longer than the reader's staging limit"; return LNR_ERR_LIMIT; }
                    r->gz_grow *= 2;
                    continue;
                }
                r->gz_grow = 1;
                r->gkeep_from = 0; r->gcarry += gr.text; r->text_made += gr.text;
                r->gz_bit = rb * 8 + gr.end_bit;
                r->gz_crc = lnr_inf::crc_combine(r->gz_crc, gr.crc, gr.text);
                r->gz_hist = r->gz_hist + gr.text > lnr_gz::WIN ? lnr_gz::WIN : (uint32_t)(r->gz_hist + gr.text);
                r->gz_mtext += gr.text;
                c.compressed_bytes = ((r->gz_bit + 7) >> 3) - rb;
                if (gr.stop == lnr_gz::AT_FINAL) {                // the trailer; then the next member, or the end of the file
                    uint64_t next = 0;
                    const uint32_t st = lnr_gz::check_trailer(r->map, r->map_len, r->gz_bit, r->gz_crc, r->gz_mtext, &next);
                    if (st) { lnr_rdgpu_gz_add(&r->gzs_last, &c); gz_fail(r, st, (r->gz_bit + 7) >> 3); break; }   // (the text in front of it is delivered, as gzread delivers it)
                    c.members = 1;
                    r->gz_in_member = false; r->gz_pos = next;
                    lnr_rdgpu_gz_add(&r->gzs_last, &c);
                    if (gz_next_member(r)) break;
                    continue;
                }
                lnr_rdgpu_gz_add(&r->gzs_last, &c);
                if (gr.stop == lnr_gz::AT_BUDGET) { stuck = true; break; }
            }
            const uint64_t tl = r->gcarry;
            const bool gend = r->gz_end || r->gz_failed;
            if (!tl) {
                if (r->gz_failed) { if (n) break; r->err = r->gerr; return LNR_ERR_ARG; }
                if (r->gz_end) break;
                r->err = "a record is longer than the reader's window"; return LNR_ERR_LIMIT;
            }
            lnr_rdgpu_bgzf job{};                                 // no block to inflate: the parse of the device text
            job.keep_from = r->gkeep_from; job.carry = tl;
            lnr_rdgpu_window w{};
            w.fmt = r->format; w.eof = gend; w.slot = slot; w.threads = r->threads;
            w.rec_base = n; w.base_base = used; w.allowed = allowed; w.free = freeb;
            lnr_rdgpu_result res{};
            lnr_rdgpu_bgzf_result br{};
            if (int s = lnr_rdgpu_parse_bgzf(r->gpu, &job, &w, &res, &br, r->gerr, sizeof r->gerr)) { r->gz_failed = true; return gfail(s); }
            if (r->format == 0 && w.fmt == 3) {                   // "BAM\1" in a plain gzip file: read through gzread, as without the switch
                r->gkeep_from = 0;
                if (!gz_to_stream(r)) return LNR_ERR_ARG;
                continue;
            }
            if (r->format == 0 && br.first >= 0) r->format = w.fmt;
            bool handover = br.first >= 0 && !br.parsed;
            if (br.parsed) {
                for (uint64_t k = 0; k < res.n; k++) {
                    r->ids.insert(r->ids.end(), br.ids + br.id_off[k], br.ids + br.id_off[k] + br.id_len[k]);
                    r->ids.push_back('\0');
                    r->id_off.push_back(r->ids.size());
                }
                n += (uint32_t)res.n; used += res.bases;
                r->records += res.n; r->bases += res.bases;
                r->g_recs += res.n; r->g_text += res.consumed;
                handover = res.handover != 0;
            }
            const uint64_t adv = br.lead + (br.parsed ? res.consumed : 0);
            r->gkeep_from = br.parsed ? res.consumed : br.lead;
            r->gcarry = tl - adv;
            if (handover) {
                if (r->gz_failed) { r->err = r->gerr; return LNR_ERR_ARG; }
                if (!gz_to_stream(r)) return LNR_ERR_ARG;
                r->gpu_serial = true;
                break;
            }
            if (res.too_big && n == 0) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
            if (res.full) { full = true; break; }
            if (gend && r->gcarry == 0) { if (r->gz_failed && !n) { r->err = r->gerr; return LNR_ERR_ARG; } break; }
            if (br.parsed && res.n == 0) {
                if (stuck || gend) {
                    if (r->gz_failed) { r->err = r->gerr; return LNR_ERR_ARG; }
                    r->err = "a record is longer than the reader's window"; return LNR_ERR_LIMIT;
                }
                grow *= 2;
            }
            continue;
        }
        if (r->bgzf) {                                            // a run of whole BGZF blocks, inflated on the device behind what the last window left
            if (r->bfailed) { r->err = r->gerr; return LNR_ERR_ARG; }
            std::vector<lnr_rdgpu_bgzf_blk> tab;
            const uint64_t c0 = r->bpos, chain0 = r->chain.size();
            uint64_t fresh = 0, tl = r->bcarry;
            while (!r->bend && !r->bstop && tl < want && tl + 65536 <= (1ULL << 30) && r->bpos - c0 < (1ULL << 30)) {
                if (r->bpos >= r->map_len) { r->bend = true; break; }
                uint32_t doff = 0;
                const unsigned char *m = r->map + r->bpos;
                const uint32_t size = lnr_inf::bgzf_member(m, r->map_len - r->bpos, doff);
                auto le32 = [](const unsigned char *q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); };
                const uint32_t isize = size ? le32(m + size - 4) : 0;
                if (!size || isize > 65536) { r->bstop = true; break; }     // not a BGZF member (or the chain leaves the file): gzread goes on here
                if (isize) {
                    tab.push_back(lnr_rdgpu_bgzf_blk{r->bpos + doff - c0, fresh, size - doff - 8, isize, le32(m + size - 8), 0});
                    r->chain.push_back(lnr_reader::BBlk{r->bpos, size, isize});
                    fresh += isize; tl += isize;
                }
                r->bpos += size;
            }
            if (!r->bend && !r->bstop && r->bpos >= r->map_len) r->bend = true;
            // with lnr_reader_gpu_gzip the gzip rounds take over at a member that is not BGZF, where gzread takes over without it
            auto to_rounds = [&]() {
                r->bgzf = false; r->chain.clear(); r->bskip = 0;
                r->gz_live = true; r->gz_pos = r->bpos; r->gz_in_member = false; r->gz_end = false;
                r->gkeep_from = r->bkeep_from; r->gcarry = r->bcarry; r->bkeep_from = r->bcarry = 0;
            };
            if (!tl) {
                if (r->bend) break;
                if (r->bstop) {
                    if (r->gzp && r->format != 3) { to_rounds(); continue; }
                    if (!bgzf_to_stream(r)) return LNR_ERR_ARG;
                    continue;
                }
            }
            if (tl + 65536 > (1ULL << 30) && tl < want) { r->err = "a record is longer than the reader's window"; return LNR_ERR_LIMIT; }
            lnr_rdgpu_bgzf job{};
            job.comp = r->map + c0; job.comp_len = r->bpos - c0; job.blk = tab.data(); job.nblk = (uint32_t)tab.size();
            job.keep_from = r->bkeep_from; job.carry = r->bcarry; job.new_text = fresh;
            lnr_rdgpu_window w{};
            w.fmt = r->format; w.eof = r->bend; w.slot = slot; w.threads = r->threads;
            w.rec_base = n; w.base_base = used; w.allowed = allowed; w.free = freeb;
            lnr_rdgpu_result res{};
            // a call that meets a bad block delivers no block
            auto bad_block = [&](uint32_t blk, uint32_t status) {
                snprintf(r->gerr, sizeof r->gerr, "BGZF block at file offset %llu: %s", (unsigned long long)r->chain[chain0 + blk].off, lnr_inf::status_text(status));
                r->bfailed = true;
                return gfail(LNR_ERR_ARG);
            };
            // what the window used up (`lead` bytes in front of the parsed text, `consumed` of it) leaves the chain; the rest stays on the
            // device for the next window, `keep_from` = where it starts in the device text
            auto advance = [&](uint64_t lead, uint64_t consumed, uint64_t keep_from) {
                const uint64_t adv = lead + consumed;
                r->bkeep_from = keep_from;
                r->bcarry = tl - adv;
                r->bskip += adv;
                size_t gone = 0;
                while (gone < r->chain.size() && r->bskip >= r->chain[gone].isize) r->bskip -= r->chain[gone++].isize;
                r->chain.erase(r->chain.begin(), r->chain.begin() + (long)gone);
            };
            // a window without a whole record is doubled
            auto grow_window = [&]() -> bool {
                if (tl + 65536 > (1ULL << 30)) { r->err = "a record is longer than the reader's window"; return false; }
                grow *= 2;
                return true;
            };
            if (r->format == 3) {                                 // BAM records, not text: the same inflate, then find / stitch / take / emit
                lnr_rdgpu_bam_result bb{};
                const lnr_rdgpu_bam_in in{r->bam_hdr ? 1 : 0, r->bam_nref};
                if (int s = lnr_rdgpu_parse_bam(r->gpu, &job, &w, &in, &res, &bb, r->gerr, sizeof r->gerr)) { r->bfailed = true; return gfail(s); }
                if (bb.bad_status) return bad_block(bb.bad_blk, bb.bad_status);
                r->ist_last.blocks += tab.size(); r->ist_last.compressed_bytes += job.comp_len; r->ist_last.text_bytes += fresh;
                if (bb.hdr_state == 2) return bam_header_fail("not a BAM header");
                if (bb.hdr_state == 1 && r->bend) return bam_header_fail("the file ends inside the BAM header");
                if (bb.hdr_state == 0 && !r->bam_hdr) { r->bam_hdr = true; r->bam_nref = bb.n_ref; r->bam_off = bb.lead; }
                if (lnr_status s = bam_done(res, bb)) return s;
                n += (uint32_t)res.n; used += res.bases;
                r->records += res.n; r->bases += res.bases;
                r->g_recs += bb.passed; r->g_text += res.consumed;
                advance(bb.lead, res.consumed, res.consumed);     // (the header was moved out of the device text)
                if (r->bstop) { if (!bgzf_to_stream(r)) return LNR_ERR_ARG; }     // a member that is not BGZF: gzread goes on, inside the header too
                if (res.too_big && n == 0) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
                if (res.full) { full = true; break; }
                if (r->bend && r->bcarry == 0) break;
                if (res.n == 0 && res.consumed == 0 && r->bgzf && !grow_window()) return LNR_ERR_LIMIT;
                continue;
            }
            lnr_rdgpu_bgzf_result br{};
            if (int s = lnr_rdgpu_parse_bgzf(r->gpu, &job, &w, &res, &br, r->gerr, sizeof r->gerr)) { r->bfailed = true; return gfail(s); }
            if (br.bad_status) return bad_block(br.bad_blk, br.bad_status);
            r->ist_last.blocks += tab.size(); r->ist_last.compressed_bytes += job.comp_len; r->ist_last.text_bytes += fresh;
            r->text_made += fresh;
            if (r->format == 0 && w.fmt == 3) {                   // "BAM\1": the text stays on the device whole, the next pass reads it as records
                r->format = 3; r->bkeep_from = 0; r->bcarry = tl;
                continue;
            }
            if (r->format == 0 && br.first >= 0) r->format = w.fmt;
            bool handover = br.first >= 0 && !br.parsed;          // not a record start: the serial parser reports it
            if (br.parsed) {
                for (uint64_t k = 0; k < res.n; k++) {
                    r->ids.insert(r->ids.end(), br.ids + br.id_off[k], br.ids + br.id_off[k] + br.id_len[k]);
                    r->ids.push_back('\0');
                    r->id_off.push_back(r->ids.size());
                }
                n += (uint32_t)res.n; used += res.bases;
                r->records += res.n; r->bases += res.bases;
                r->g_recs += res.n; r->g_text += res.consumed;
                handover = res.handover != 0;
            }
            advance(br.lead, br.parsed ? res.consumed : 0, br.parsed ? res.consumed : br.lead);
            if (r->bstop && !handover && r->gzp) to_rounds();
            else if (handover || r->bstop) {                      // the stream goes on at the first byte the device has not used up
                if (!bgzf_to_stream(r)) return LNR_ERR_ARG;
                if (handover) { r->gpu_serial = true; break; }
            }
            if (res.too_big && n == 0) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
            if (res.full) { full = true; break; }
            if (r->bend && r->bcarry == 0) break;
            if (br.parsed && res.n == 0 && r->bgzf && !grow_window()) return LNR_ERR_LIMIT;
            continue;
        }
        if (r->use_map) {
            while (r->mpos < r->map_len && is_ws(r->map[r->mpos])) r->mpos++;
            if (r->mpos >= r->map_len) break;
            text = r->map + r->mpos;
            len = r->map_len - r->mpos < want ? r->map_len - r->mpos : want;
            eof = r->mpos + len == r->map_len;
        } else {                                                  // an inflate stream (or any file the reader does not map): gzread into a pinned buffer
            const uint64_t have = r->end - r->pos;
            if (want < have + 16) want = have + 16;
            uint8_t *S = lnr_rdgpu_stage(r->gpu, want);
            if (!S) { r->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
            memcpy(S, r->buf.data() + r->pos, have);
            r->pos = r->end = 0;
            len = have;
            while (!r->gz_done && len < want) {
                const uint64_t ask = want - len < (1u << 30) ? want - len : (1u << 30);
                int got = gzread(r->f, S + len, (unsigned)ask);
                if (got < 0) { int e; r->err = gzerror(r->f, &e); return LNR_ERR_ARG; }
                if (got == 0) r->gz_done = true;
                len += (uint64_t)got; r->gz_bytes += (uint64_t)got;
            }
            eof = r->gz_done;
            if (r->format == 0 && lnr_bam::is_magic(S, len)) r->format = 3;
            if (r->format == 3) {                                 // BAM through gzread: the header is passed here, the records go up as they are
                auto put_back = [&](const uint8_t *p, uint64_t left) {
                    if (r->buf.size() < left) r->buf.resize(left);
                    memcpy(r->buf.data(), p, left);
                    r->pos = 0; r->end = left;
                };
                if (!r->bam_hdr) {
                    const lnr_bam::Header h = lnr_bam::header_span(S, len);
                    if (h.status < 0) return bam_header_fail("not a BAM header");
                    if (h.status == 1) {
                        if (eof) return bam_header_fail("the file ends inside the BAM header");
                        if (len >= (1ULL << 30)) { r->err = "the BAM header is longer than the reader's window"; return LNR_ERR_LIMIT; }
                        put_back(S, len); grow *= 2;
                        continue;
                    }
                    r->bam_hdr = true; r->bam_nref = h.n_ref; r->bam_off = h.first; lead = h.first;
                }
                if (len == lead) { if (eof) break; continue; }
                w.fmt = 3; w.eof = eof; w.text = S + lead; w.len = len - lead; w.pinned = 1; w.slot = slot; w.threads = r->threads;
                w.rec_base = n; w.base_base = used; w.allowed = allowed; w.free = freeb;
                const lnr_rdgpu_bam_in in{1, r->bam_nref};
                lnr_rdgpu_result res{};
                lnr_rdgpu_bam_result bb{};
                if (int s = lnr_rdgpu_parse_bam(r->gpu, nullptr, &w, &in, &res, &bb, r->gerr, sizeof r->gerr)) return gfail(s);
                if (lnr_status s = bam_done(res, bb)) return s;
                n += (uint32_t)res.n; used += res.bases;
                r->records += res.n; r->bases += res.bases;
                r->g_recs += bb.passed; r->g_text += res.consumed;
                put_back(S + lead + res.consumed, w.len - res.consumed);
                if (res.too_big && n == 0) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
                if (res.full) { full = true; break; }
                if (eof && res.consumed == w.len) break;
                if (res.n == 0 && res.consumed == 0) {
                    if (len >= (1ULL << 30)) { r->err = "a record is longer than the reader's window"; return LNR_ERR_LIMIT; }
                    grow *= 2;
                }
                continue;
            }
            while (lead < len && is_ws(S[lead])) lead++;
            text = S + lead; len -= lead;
            w.pinned = 1;
            if (!len) { if (eof) break; continue; }
        }
        if (r->format == 0) r->format = text[0] == '>' ? 1 : (text[0] == '@' ? 2 : -1);
        uint64_t consumed = 0;
        bool handover = r->format < 0 || text[0] != (r->format == 1 ? '>' : '@');       // (the serial parser reports it)
        lnr_rdgpu_result res{};
        if (!handover) {
            w.fmt = r->format; w.eof = eof; w.text = text; w.len = len; w.slot = slot; w.threads = r->threads;
            w.rec_base = n; w.base_base = used; w.allowed = allowed; w.free = freeb;
            if (int s = lnr_rdgpu_parse(r->gpu, &w, &res, r->gerr, sizeof r->gerr)) return gfail(s);
            for (uint64_t k = 0; k < res.n; k++) {
                uint64_t hb = res.hdr[2 * k], he = res.hdr[2 * k + 1];
                while (he > hb && text[he - 1] == '\r') he--;
                r->ids.insert(r->ids.end(), (const char *)text + hb, (const char *)text + he);
                r->ids.push_back('\0');
                r->id_off.push_back(r->ids.size());
            }
            n += (uint32_t)res.n; used += res.bases; consumed = res.consumed;
            r->records += res.n; r->bases += res.bases;
            r->g_recs += res.n; r->g_text += res.consumed;
            handover = res.handover != 0;
        }
        if (r->use_map) r->mpos += consumed;
        else {                                                    // what the window did not use goes back in front of the stream
            const uint64_t left = len - consumed;
            if (r->buf.size() < left) r->buf.resize(left);
            memcpy(r->buf.data(), text + consumed, left);
            r->pos = 0; r->end = left;
        }
        if (handover) {
            if (r->use_map) { r->use_map = false; gzseek(r->f, (z_off_t)r->mpos, SEEK_SET); r->pos = r->end = 0; r->eof = false; }
            r->gpu_serial = true;
            break;
        }
        if (res.too_big && n == 0) { r->err = "a record is longer than the block"; return LNR_ERR_LIMIT; }
        if (res.full) { full = true; break; }
        if (eof && consumed == len) break;
        if (res.n == 0) {
            if (len >= (1ULL << 30)) { r->err = "a record is longer than the reader's window"; return LNR_ERR_LIMIT; }
            grow *= 2;
        }
    }
    if ((r->gpu_serial || r->have_spill) && !full && n < max_reads) {   // the serial parser's share of the block, through a host block
        if (r->hblock_cap < dst_cap) {
            r->hblock.reset(new (std::nothrow) uint8_t[dst_cap ? dst_cap : 1]);
            if (!r->hblock) { r->hblock_cap = 0; r->err = "host allocation failed"; return LNR_ERR_NOMEM; }
            r->hblock_cap = dst_cap;
        }
        uint32_t n2 = n;
        lnr_status s = next_from(r, r->hblock.get(), dst_cap, ho, max_reads, &n2, n, used, true);
        if (s != LNR_OK) return s;
        if (int s2 = lnr_rdgpu_append(r->gpu, slot, used, r->hblock.get() + used, ho[n2] - used, n, ho + n, n2 - n, r->gerr, sizeof r->gerr)) return gfail(s2);
        n = n2;
    }
    *d_reads_concat = dr; *d_off = dof; *off = ho; *n_out = n;
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
