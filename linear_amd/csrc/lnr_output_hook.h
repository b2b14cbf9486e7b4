// lnr_output_hook.h -- the seam between the writer's C ABI (lnr_output.cpp, host code by g++) and its GPU side (lnr_output_kernels.hip).
// lnr_output.cpp is also linked WITHOUT the device half (the front-end's test double, tests/stub_abi.cpp), so it refers to these symbols
// weakly: where they are absent lnr_writer_gpu_open answers LNR_ERR_NO_DEVICE.  Plain data only crosses here.  Return values are lnr_status.
#pragma once
#include <stddef.h>
#include <stdint.h>

extern "C" {
struct lnr_outgpu;
struct lnr_outgpu_batch {
    int dev_form;                    // 0: the arrays below are host memory and get uploaded; 1: device memory, used in place
    uint32_t n_reads; uint64_t n_cords;
    const uint64_t *cord_off, *cords_str, *cords_end;
    const uint64_t *read_len;        // dev_form 0: n lengths (host); dev_form 1: n + 1 read offsets (device), length k = off[k + 1] - off[k]
    const char *read_ids; const uint64_t *id_off;      // host, id_off[k] = start of id k; the blob ends with the '\0' of the last id
    int what;                        // 1 SAM, 2 APF, 3 BAM records, 4 PAF lines (lnr_writer_format_paf_gpu / _dev: k_out_measure<Paf> / k_out_emit<Paf>;
                                     // reads stays NULL, read_len as for SAM without SEQ)
    uint64_t thd_large_X; int64_t thd_DI, thd_X;
    const uint8_t *reads;            // SAM with SEQ: the reads' bases back to back (host or device as dev_form says), and read_len then holds n + 1
                                     // read offsets in both forms; NULL: SEQ prints as '*' (BAM: l_seq 0)
};
int lnr_outgpu_open(int32_t device, const char *gblob, uint64_t gblob_bytes, const uint64_t *goff, const uint64_t *glen, uint32_t nseq,
                    lnr_outgpu **out, char *err, size_t err_cap) __attribute__((weak));
int lnr_outgpu_format(lnr_outgpu *g, const lnr_outgpu_batch *b, const char **text, uint64_t *size, char *err, size_t err_cap) __attribute__((weak));
// the GPU side's own copy of the genome for SEQ: nseq host sequences, one Dna5 ordinal per byte; replaces an earlier copy
int lnr_outgpu_set_genome(lnr_outgpu *g, const uint8_t *const *seq, const uint64_t *glen, uint32_t nseq, char *err, size_t err_cap) __attribute__((weak));
// the same copy from nseq sequences in the memory of the writer's device (device-to-device copies on the writer's stream, no host hop)
int lnr_outgpu_set_genome_dev(lnr_outgpu *g, const uint8_t *const *d_seq, const uint64_t *glen, uint32_t nseq, char *err, size_t err_cap) __attribute__((weak));
void lnr_outgpu_times(const lnr_outgpu *g, double *ms5) __attribute__((weak));   // last call: upload, measure, scan, emit, download
void lnr_outgpu_close(lnr_outgpu *g) __attribute__((weak));
// BGZF output (lnr_writer_set_bgzf): on != 0, lnr_outgpu_format compresses its text on the device (k_bgzf_deflate, one BGZF member per
// 0xff00 text bytes) and hands out the members instead; lnr_outgpu_bgzf_bytes does the same to any host bytes.  Stats: the last call.
struct lnr_outgpu_bgzf_stats { uint64_t blocks, stored_blocks, text_bytes, compressed_bytes; double deflate_ms, pack_ms; };
void lnr_outgpu_set_bgzf(lnr_outgpu *g, int on) __attribute__((weak));
int lnr_outgpu_bgzf_bytes(lnr_outgpu *g, const char *bytes, uint64_t size, const char **data, uint64_t *out_size, char *err, size_t err_cap) __attribute__((weak));
void lnr_outgpu_bgzf_stats_get(const lnr_outgpu *g, lnr_outgpu_bgzf_stats *out) __attribute__((weak));
// Sort mode (lnr_writer_sort_*): between _begin and _finish, lnr_outgpu_format with what == 3 keeps the batch's records in device segments
// and returns size 0.  _finish sorts; _next hands out the BGZF members of the next piece of the sorted stream with their offsets inside the
// piece (moff[0 .. nb], host memory valid until the next call; nb == 0 and size 0: done); _fetch downloads the sorted per-record arrays
// (records each: key = (u32)refID << 32 | (u32)pos, flag, reference end; off: records + 1 offsets in the sorted stream) for the index.
struct lnr_outgpu_sort_info { uint64_t records, record_bytes, device_bytes, members; double index_ms, sort_ms, gather_ms, deflate_ms, pack_ms, download_ms; };
// The hold (lnr_sort_hold_info): records are held without their quality spans; _sort_spill (while collecting; 0 switches it off) lets
// batches that do not fit on the device go to pinned host segments, max_host_bytes of them at most.
struct lnr_outgpu_hold_info { uint64_t stream_bytes, held_device_bytes, held_host_bytes, device_batches, host_batches; double keep_ms, spill_ms; };
int lnr_outgpu_sort_spill(lnr_outgpu *g, uint64_t max_host_bytes, char *err, size_t err_cap) __attribute__((weak));
void lnr_outgpu_sort_hold_info_get(const lnr_outgpu *g, lnr_outgpu_hold_info *out) __attribute__((weak));
int lnr_outgpu_sort_begin(lnr_outgpu *g, uint64_t max_bytes, char *err, size_t err_cap) __attribute__((weak));
int lnr_outgpu_sort_finish(lnr_outgpu *g, uint32_t piece_members, char *err, size_t err_cap) __attribute__((weak));
int lnr_outgpu_sort_next(lnr_outgpu *g, const char **data, uint64_t *size, const uint64_t **moff, uint32_t *nb, char *err, size_t err_cap) __attribute__((weak));
int lnr_outgpu_sort_fetch(lnr_outgpu *g, uint64_t *key, uint32_t *flag, int64_t *end, uint64_t *off, char *err, size_t err_cap) __attribute__((weak));
void lnr_outgpu_sort_info_get(const lnr_outgpu *g, lnr_outgpu_sort_info *out) __attribute__((weak));
void lnr_outgpu_sort_end(lnr_outgpu *g) __attribute__((weak));
}
