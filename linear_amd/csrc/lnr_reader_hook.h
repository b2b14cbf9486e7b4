// lnr_reader_hook.h -- the seam between the reader's C ABI (lnr_reader.cpp, host code by g++) and its GPU side (lnr_reader_kernels.hip).
// lnr_reader.cpp is also linked WITHOUT the device half (the front-end's test double, tests/stub_abi.cpp), so it refers to these symbols
// weakly: where they are absent lnr_reader_gpu_open answers LNR_ERR_NO_DEVICE.  Plain data only crosses here.  Return values are lnr_status.
#pragma once
#include <stddef.h>
#include <stdint.h>

extern "C" {
struct lnr_rdgpu;
struct lnr_rdgpu_window {
    int fmt;                         // 1 FASTA, 2 FASTQ, 3 BAM (lnr_rdgpu_parse_bam)
    int eof;                         // the window ends at the end of the file
    int pinned;                      // text lies in a staging buffer of lnr_rdgpu_stage: copied up as it is
    const uint8_t *text; uint64_t len;               // host text; byte 0 starts a record
    uint32_t slot, threads;          // device block to append to; host threads that fill the staging buffers
    uint64_t rec_base, base_base;    // records and bases already in the block
    uint64_t allowed, free;          // records still allowed, bases still free
};
struct lnr_rdgpu_result {
    uint64_t n, bases, consumed;     // records taken, their bases, text bytes used up
    uint32_t handover, full, too_big;                // the serial parser goes on at `consumed`; the next record does not fit; ... and it is the first
    const uint64_t *hdr;             // n pairs (begin, end) of header spans, window offsets (pinned host memory, valid until the next parse)
};
struct lnr_rdgpu_names { const char *ids; const uint64_t *id_off; const uint32_t *id_len; };     // header line / name of taken record k: id_len[k] bytes at ids + id_off[k], no trailing '\r'
struct lnr_rdgpu_badblk { uint32_t blk, status; };   // status != 0: block blk of the window did not inflate (lnr_inf::Status); nothing else of the result is valid
// ---- BGZF input: the blocks of a window are inflated on the device, behind the text the last window left over
struct lnr_rdgpu_bgzf_blk { uint64_t coff, ooff; uint32_t clen, isize, crc, pad; };   // DEFLATE data at comp + coff; text at (new text) + ooff
struct lnr_rdgpu_bgzf {
    const uint8_t *comp; uint64_t comp_len;          // the compressed bytes of the window's blocks (pageable host memory: the mapped file)
    const lnr_rdgpu_bgzf_blk *blk; uint32_t nblk;    // blocks with ISIZE > 0
    uint64_t keep_from, carry;                       // device text [keep_from, keep_from + carry) of the last window moves to the front
    uint64_t new_text;                               // sum of ISIZE: the window's text is carry + new_text bytes
};
struct lnr_rdgpu_bgzf_result {
    lnr_rdgpu_badblk bad_block;
    uint64_t lead;                                   // white space skipped at the front of the text (the parse saw the text behind it)
    int first;                                       // first byte behind it, -1: the text is white space up to `lead`
    uint32_t parsed;                                 // 0: no parse ran (format unknown / not a record start: hand-over, or nothing but blanks)
    lnr_rdgpu_names names;                           // of the taken records (pinned, valid until the next parse)
};
// stage these compressed bytes, inflate these blocks behind `carry` bytes, then measure / scan / emit over the device text.  w->text is
// not used, w->len is set here; w->fmt == 0: decided by the first byte.
int lnr_rdgpu_parse_bgzf(lnr_rdgpu *g, const lnr_rdgpu_bgzf *job, lnr_rdgpu_window *w, lnr_rdgpu_result *r, lnr_rdgpu_bgzf_result *br,
                         char *err, size_t err_cap) __attribute__((weak));
// ---- BAM input: the window's bytes are BAM records behind `lead` header bytes.  job != null: BGZF blocks are inflated first, as in
// lnr_rdgpu_parse_bgzf (which sets w->fmt = 3 and parses nothing when an undecided file starts with "BAM\1"); job == null: w->text / w->len
// is the staged stream and byte 0 starts a record.  Then find / stitch / meta on the device, the take on the host from the per-record
// metadata (lnr_bam::take), emit and the gather of the names.
struct lnr_rdgpu_bam_in { int hdr_done; int32_t n_ref; };
struct lnr_rdgpu_bam_result {
    lnr_rdgpu_badblk bad_block;
    uint32_t hdr_state;                              // 0 passed; 1 the window is too short for the header (nothing was parsed); 2 not a BAM header
    int32_t n_ref; uint64_t lead;                    // set when the header was passed by this call: its n_ref and its bytes
    uint32_t bad;                                    // the record the host reader would read next: 1 fails rec_valid, 2 the file ends inside it
    uint64_t bad_ord, bad_off;                       // ... records of the window in front of it, its window offset (behind lead)
    uint64_t passed;                                 // records in front of `consumed`, skipped ones included
    uint64_t skipped, reverse, tiles, repaired;      // among the passed; of the window
    double find_ms, stitch_ms, emit_ms;
    lnr_rdgpu_names names;                           // of the taken records (pinned, valid until the next parse)
};
int lnr_rdgpu_parse_bam(lnr_rdgpu *g, const lnr_rdgpu_bgzf *job, lnr_rdgpu_window *w, const lnr_rdgpu_bam_in *in, lnr_rdgpu_result *r,
                        lnr_rdgpu_bam_result *br, char *err, size_t err_cap) __attribute__((weak));
uint32_t lnr_rdgpu_bam_tile(void) __attribute__((weak));
// ---- plain gzip input (lnr_gunzip_hd.h): counts of one round / of a call, in the layout of lnr_gzip_counts
struct lnr_rdgpu_gz_counts {
    uint64_t rounds, members, chunks, candidates, true_pieces, false_candidates, deflate_blocks, compressed_bytes, text_bytes, window_symbols, gzread_bytes, grown_rounds;
    double find_ms, measure_ms, stitch_ms, emit_ms, chain_ms, resolve_ms, parse_ms, upload_ms, download_ms;
};
// one round for the reader: comp = the mapped file from the byte that holds the member's next bit (start_bit 0..7 into it), comp_len bytes
// of it; hist bytes of history exist in the window the device keeps (0: a member starts); the device text [keep_from, keep_from + carry) is
// what the last window left.  status != 0: the data is bad at comp + bad_off.  pieces == 0: no block completed (stop 2: the bytes end inside
// a block; 3: the block's text is more than text_cap) and nothing has changed; else moved = 1: the device text is now [0, carry + text),
// end_bit = the next bit of the member (from comp), stop 1 = a final block was passed, crc = CRC32 of the round's text.
struct lnr_rdgpu_gzip { const uint8_t *comp; uint64_t comp_len; uint32_t start_bit, hist; uint64_t chunk, keep_from, carry, text_cap; uint32_t threads, pad; };
struct lnr_rdgpu_gzip_result { uint32_t status, stop, pieces, crc, moved, pad; uint64_t bad_off, end_bit, text; lnr_rdgpu_gz_counts counts; };
int lnr_rdgpu_gzip_round(lnr_rdgpu *g, const lnr_rdgpu_gzip *job, lnr_rdgpu_gzip_result *out, char *err, size_t err_cap) __attribute__((weak));
static inline void lnr_rdgpu_gz_add(lnr_rdgpu_gz_counts *t, const lnr_rdgpu_gz_counts *c) {      // the one place that knows the fields: 12 counts, 9 times
    uint64_t *tu = &t->rounds; const uint64_t *cu = &c->rounds;
    for (int i = 0; i < 12; i++) tu[i] += cu[i];
    double *td = &t->find_ms; const double *cd = &c->find_ms;
    for (int i = 0; i < 9; i++) td[i] += cd[i];
}
// every member of gz[0, size) -> text (host buffers).  0 with *bad_status != 0: the stream is bad at compressed offset *bad_off
// (lnr_gz::status_text), *text_size = the text of the rounds before it
int lnr_rdgpu_gunzip(int32_t device, const uint8_t *gz, uint64_t size, uint8_t *text, uint64_t text_cap, uint64_t *text_size, lnr_rdgpu_gz_counts *last,
                     lnr_rdgpu_gz_counts *total, uint64_t *bad_off, uint32_t *bad_status, char *err, size_t err_cap) __attribute__((weak));
void lnr_rdgpu_inflate_times(const lnr_rdgpu *g, double *ms2) __attribute__((weak));   // last block: inflate kernel, header gather (HIP events)
int lnr_rdgpu_open(int32_t device, uint32_t slots, lnr_rdgpu **out, char *err, size_t err_cap) __attribute__((weak));
// makes block `slot` hold dst_cap bases and max_reads + 1 offsets; hands out its device arrays and the host copy of the offsets
int lnr_rdgpu_block(lnr_rdgpu *g, uint32_t slot, uint64_t dst_cap, uint32_t max_reads, uint8_t **d_reads, uint64_t **d_off, uint64_t **h_off,
                    char *err, size_t err_cap) __attribute__((weak));
uint8_t *lnr_rdgpu_stage(lnr_rdgpu *g, uint64_t bytes) __attribute__((weak));   // the pinned buffer a stream is inflated into (contents are not kept when it grows)
int lnr_rdgpu_parse(lnr_rdgpu *g, const lnr_rdgpu_window *w, lnr_rdgpu_result *r, char *err, size_t err_cap) __attribute__((weak));
// records of the serial parser: nb bases behind base_base, offsets off[0 .. n] (block coordinates) at rec_base
int lnr_rdgpu_append(lnr_rdgpu *g, uint32_t slot, uint64_t base_base, const uint8_t *bases, uint64_t nb, uint64_t rec_base, const uint64_t *off, uint64_t n,
                     char *err, size_t err_cap) __attribute__((weak));
void lnr_rdgpu_times(const lnr_rdgpu *g, double *ms5) __attribute__((weak));   // last block: stage + upload, measure, scan, emit, download
void lnr_rdgpu_times_reset(lnr_rdgpu *g) __attribute__((weak));
uint32_t lnr_rdgpu_tile(void) __attribute__((weak));
void lnr_rdgpu_close(lnr_rdgpu *g) __attribute__((weak));
// ---- a genome held on the device (lnr_genome.cpp): the first `bytes` bases of a delivered block copied, device to device on the reader's
// stream, into an allocation of their own (*d_out, never null, 16 spare bytes behind the bases); complete on return.  The allocation
// belongs to no reader: _free and _download name the device (lnr_rdgpu_device: the ordinal the reader's GPU side resolved to).
int lnr_rdgpu_keep(lnr_rdgpu *g, const uint8_t *d_src, uint64_t bytes, uint8_t **d_out, char *err, size_t err_cap) __attribute__((weak));
int lnr_rdgpu_keep_download(int32_t device, const uint8_t *d_src, uint8_t *dst, uint64_t bytes, char *err, size_t err_cap) __attribute__((weak));
void lnr_rdgpu_keep_free(int32_t device, uint8_t *d) __attribute__((weak));
int32_t lnr_rdgpu_device(const lnr_rdgpu *g) __attribute__((weak));
}

// ---- the other direction: what lnr_reader.cpp itself offers to lnr_genome.cpp (host code, not part of the public header; the reader's GPU
// side stays the reader's).  lnr_reader_keep_block: the first `bytes` bases of the block the last lnr_reader_next_dev delivered, through
// lnr_rdgpu_keep; *device = the ordinal the allocation lies on.  A lnr_status; the reason in lnr_reader_error.  lnr_reader_records: records
// the reader has passed so far, those of a call that ended in an error included -- the ordinal in the file of the record such a call stopped at.
struct lnr_reader;
extern "C" {
int lnr_reader_keep_block(lnr_reader *r, uint64_t bytes, uint8_t **d_out, int32_t *device);
uint64_t lnr_reader_records(const lnr_reader *r);
}
