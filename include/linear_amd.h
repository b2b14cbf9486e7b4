/* linear_amd.h -- C ABI of the MI355X-native `linear filter` hot path.
 *
 * Drop-in boundary for the compute path of xp3i4/linear's `Mapper` (reference paths are
 * relative to the reference root):
 *
 *   reference entry point                                     replaced by
 *   --------------------------------------------------------  --------------------------
 *   createFeatures(genomes, f2, type, T)  pmpfinder.h:196-197  \
 *   Mapper::createIndex -> createIndexDynamic(seqs, index,      } lnr_index_build
 *       gstr, gend, threads, efficient)   index_util.h:297-302 /
 *   body of the `for j` loop in Mapper::p_calRecords            lnr_filter_batch
 *       (mapper.cpp:438-462): _compltRvseStr + createFeatures
 *       (read) x2 + apxMap(...)           pmpfinder.h:213-225
 *   getDIndexMatchAll (stage a7)          pmpfinder.cpp:1856    lnr_seed_lookup_batch
 *
 * Sequences are SeqAn `Dna5` ordinals, one byte per base (A,C,G,T,N = 0..4): exactly the
 * storage of `String<Dna5>` (begin pointer + length), so `&read[0]` / `length(read)` bind
 * directly.  Results are the reference's 64-bit cord words
 * (main[63] recd[62] strand[61] blockEnd[60] id[50..59] x[20..49] y[0..19], cords.h:24-39),
 * `cords_str[j]` and `cords_end[j]` of every read in CSR form.
 *
 * Plain C: pointers and sizes only.  No exceptions cross this boundary; every call returns
 * LNR_OK (0) or a negative lnr_status.  A context is single-threaded and owns one GPU; use
 * one context per GPU / per process (reads shard across contexts, the index is identical).
 * The library has no CPU execution path: without a HIP device lnr_create fails with
 * LNR_ERR_NO_DEVICE.
 */
#ifndef LINEAR_AMD_H
#define LINEAR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lnr_ctx lnr_ctx;

typedef enum lnr_status {
    LNR_OK = 0,
    LNR_ERR_ARG = -1,         /* bad argument (null pointer, offsets not monotone, >= 1024 sequences, ...).  Base ordinals above 4 are not an
                                 error: they are read as N (4), in reads and in reference sequences alike */
    LNR_ERR_NO_DEVICE = -2,   /* no usable HIP device */
    LNR_ERR_HIP = -3,         /* a HIP runtime call failed; see lnr_last_error */
    LNR_ERR_NOMEM = -4,       /* device or host allocation failed */
    LNR_ERR_NO_INDEX = -5,    /* filter/seed call before lnr_index_build / lnr_index_adopt */
    LNR_ERR_LIMIT = -6,       /* input exceeds a format limit (read >= 2^20, sequence >= 2^30 - 2^20; cords.cpp:13-15) */
    LNR_ERR_UNSUPPORTED = -7, /* option outside this build (index_type not 1 or 2, feature_type != 2, dup > 1) */
    LNR_ERR_INTERNAL = -8     /* device-side capacity overflow that retries could not resolve */
} lnr_status;

/* Options = the subset of the reference's `Options` (base.cpp:26-54) that reaches this path. */
typedef struct lnr_opts {
    int32_t device;            /* HIP device ordinal; -1 = current device */
    uint32_t index_type;       /* -i : 1 = DIndex (reference default), 2 = HIndex (index_util.cpp:2593-2610: shape 17/9, one sample per 8 bases) */
    uint32_t feature_type;     /* -f : 2 = 2-mer/48 window features (reference default) */
    uint32_t preset;           /* -p : 1 (reference default: chain stop ratio 0) or 2 (the same computation; only the writer's CIGAR thresholds differ,
                                  lnr_writer_set_preset).  -p 0 (stop ratio 0.7 in the anchor traceback) is not built: LNR_ERR_UNSUPPORTED */
    uint32_t gap_len;          /* -g : 0 = apxMap only; > 0 = the cords go through the gap re-mapper (mapGaps + reformCords, gap.cpp:407-576) with this
                                  minimum gap length, mapped as the reference does: 1 -> 50, 2..9 -> 10 (mapper.cpp:207-231) */
    uint32_t dup;              /* -dup : 0 | 1, the duplication add-on of the gap re-mapper (gap.cpp:303-362) */
    uint64_t scratch_budget;   /* max bytes of per-read device scratch in flight (0 = default 64 GiB of the 288 GB) */
} lnr_opts;

typedef struct lnr_index_info {
    uint32_t nseq;
    uint32_t layout_threads;   /* the reference's -t the index layout reproduces */
    uint64_t genome_bytes;     /* padded device copy of the sequences */
    uint64_t dir_len;          /* int32 entries (4^13 + 1); -i 2: 4^9 + 1 entries of a derived table (head of the block of X, -1 = none) */
    uint64_t hs_len;           /* uint64 entries; -i 2: the words of ysa, the reference's block array (the parity surface of that index) */
    uint64_t f2_len;           /* 16-byte feature entries over all sequences */
    uint64_t n_samples;        /* genome minimizer samples examined */
    double build_ms;           /* device time of the last build */
} lnr_index_info;

/* CSR result of a batch.  Host arrays owned by the context, valid until the next
 * lnr_filter_batch / lnr_seed_lookup_batch on the same context or lnr_destroy. */
typedef struct lnr_cords {
    uint32_t n_reads;
    uint64_t n_cords;
    const uint64_t *cord_off;   /* n_reads + 1 */
    const uint64_t *cords_str;  /* n_cords */
    const uint64_t *cords_end;  /* n_cords */
} lnr_cords;

/* Same, device resident (for callers that keep results on the GPU, and for benchmarking). */
typedef struct lnr_cords_dev {
    uint32_t n_reads;
    uint64_t n_cords;
    const uint64_t *d_cord_off;
    const uint64_t *d_cords_str;
    const uint64_t *d_cords_end;
} lnr_cords_dev;

typedef struct lnr_anchors {    /* stage a7 output: raw anchors per read, each list led by the dummy 0 */
    uint32_t n_reads;
    uint64_t n_anchors;
    const uint64_t *anchor_off; /* n_reads + 1 */
    const uint64_t *anchors;
} lnr_anchors;

/* Counters and device timings of the last batch call (deterministic functions of index + reads,
 * except the *_ms fields).  seed_bytes is SURVEY.md 8(d)'s algorithmic byte count
 * sum(ceil(L/4)) + lookups*8 + bucket_entries*8 + anchors*8. */
typedef struct lnr_stats {
    uint64_t reads, bases, jobs, samples, lookups, bucket_entries, anchors, remap_reads, cords;
    uint64_t seed_bytes;
    double prep_ms, seed_count_ms, seed_gather_ms, job_ms, tail_ms, total_ms;
    uint32_t seed_count_launches, seed_gather_launches, job_launches;
    uint32_t gap_second_pass;  /* reads of the gap re-mapper that a 16-wave team of the first stage did: ranked heavy, or handed over by a single wave (arena, cord slot, a sort or chain DP too long for one wave) */
    double gap_ms;             /* device time of the gap re-mapper (-g > 0) */
    uint32_t gap_last_launch;  /* reads the first stage left flagged and the last launch did (a team per read with the largest arena) */
    uint32_t groups_heavy, groups_mid, groups_wave1;   /* job groups (the jobs of one read in one round) that ran on 16 waves, on 4 or 2 waves and on a
                                                          single wave, both rounds together: which job kernel the batch's reads took */
} lnr_stats;

void lnr_opts_default(lnr_opts *o);
lnr_status lnr_create(const lnr_opts *opts, lnr_ctx **out);
void lnr_destroy(lnr_ctx *ctx);
const char *lnr_strerror(lnr_status s);
const char *lnr_last_error(const lnr_ctx *ctx);   /* detail of the last failure on this context */

/* Index + genome features from the reference sequences.  seq[i] may point to host memory (`&genome[i][0]` of the
 * StringSet<String<Dna5>>) or to device memory (a genome already resident in HBM); the pointer array itself is a host array.
 * layout_threads = the reference's -t whose DIndex layout is to be reproduced (index content depends on it:
 * index_util.cpp:1652-1700). */
lnr_status lnr_index_build(lnr_ctx *ctx, const uint8_t *const *seq, const uint64_t *len, uint32_t nseq, uint32_t layout_threads);
lnr_status lnr_index_info_get(const lnr_ctx *ctx, lnr_index_info *info);
/* Copy the index to host arrays (any pointer may be NULL).  f2 is written as 3 x int32 per entry. */
lnr_status lnr_index_export(lnr_ctx *ctx, int32_t *dir, uint64_t *hs, int32_t *f2, uint64_t *f2_off /* nseq+1 */);

/* Multi-GPU: the packed index is built on one rank and broadcast (RCCL) to the others.
 * lnr_index_blob_* expose the device buffers that make up the index so the host framework can
 * broadcast them in place: rank 0 calls lnr_index_build, every rank exchanges lnr_index_info +
 * the sequence lengths, the receiving ranks call lnr_index_alloc, then all ranks broadcast each
 * blob (ptr, bytes) and the receivers finish with lnr_index_adopt. */
#define LNR_INDEX_BLOBS 4       /* genome bytes, dir, hs, f2 */
lnr_status lnr_index_alloc(lnr_ctx *ctx, const lnr_index_info *info, const uint64_t *seq_len /* nseq */);
lnr_status lnr_index_blob(lnr_ctx *ctx, uint32_t which, void **d_ptr, uint64_t *bytes);
lnr_status lnr_index_adopt(lnr_ctx *ctx);
/* One process driving several GPUs (the C++ front-end: one host thread + one context per GPU): moves the index of ctxs[root] into
 * every other context (created with the same options, no index yet) through lnr_index_alloc / _blob / _adopt.  Contexts on distinct devices:
 * ncclBroadcast of the four device buffers in place over RCCL / xGMI (librccl is loaded on first use; nothing else in the library needs it);
 * a context that shares its device with another one gets device-to-device copies.  *seconds (optional): wall time of the exchange, the
 * receivers' derived tables included.  What a front-end compares it with: lnr_index_build on every context ("every GPU builds its own"). */
lnr_status lnr_index_broadcast(lnr_ctx *const *ctxs, uint32_t n, uint32_t root, double *seconds);

/* The hot path.  reads_concat = bases of all reads back to back, off[n+1] = start offsets.
 * Host-buffer form (copies in and out over PCIe): */
lnr_status lnr_filter_batch(lnr_ctx *ctx, const uint8_t *reads_concat, const uint64_t *off, uint32_t n, lnr_cords *out);
/* The same in two halves, so that one context overlaps transfers and compute: lnr_filter_submit starts the upload of a batch on a copy
 * stream and returns; lnr_filter_wait hands out the cords of the oldest submitted batch.  Up to THREE batches may be in flight, and with
 * the pattern   submit(0); submit(1); loop { submit(k + 2); wait(k); }   the GPU never idles: lnr_filter_wait(k) starts the download of
 * batch k's cords (batch k was computed during the previous wait) and computes batch k + 1 while they travel; the upload of batch k + 2
 * runs under those kernels.  (submit(k + 1); wait(k) works as well: upload overlapped, download not.)  The read buffer must stay untouched
 * until the lnr_filter_wait that RETURNS its batch has returned; the host arrays of a result stay valid until the SECOND next result of the
 * context (two result slots taken in turn: another thread may format batch k while the context runs on).  lnr_last_stats reports the batch
 * handed out last.  lnr_gap_stream(set >= 0) and lnr_set_gap need an idle context (nothing in flight).
 * Two lanes (gap_len == 0; LNR_LANES=1 in the environment of lnr_create switches them off): the submitted batches are dealt in turn to
 * two lanes of the context that COMPUTE side by side -- each lane has a worker thread of the library that runs a batch as soon as it is
 * uploaded, so lnr_filter_wait only waits for the oldest batch, downloads and returns it.  The re-map round of batch k (a few long reads,
 * the chip nearly empty) then runs under the seed lookup and the first job round of batch k + 1.  Lane 0 is the context itself; lane 1 is
 * made when a second batch is first in flight, shares the index (views, no copy) and owns a second set of per-batch buffers (about what
 * one batch needs; the bench process peaks at 162 GiB instead of 103); where that memory cannot be had -- at creation, for the input, or
 * LNR_ERR_NOMEM inside a batch on lane 1 -- that batch is run again on lane 0 and the context goes on with one lane, no error reported.  Everything above
 * holds unchanged: submission order, three in flight, lifetimes, errors reported by the lnr_filter_wait of the batch they belong to.  The
 * event-timed stage times in lnr_stats (seed_count_ms, job_ms, total_ms ...) of a batch then include time in which the chip was shared
 * with the neighbouring batch: they add up to more than the step time.  With gap_len > 0 batches run one at a time in submission order
 * (the gap re-mapper's stream state goes from batch to batch), computed inside lnr_filter_wait as before.  While batches are in flight the
 * index calls, lnr_filter_batch*, lnr_seed_lookup_batch*, lnr_last_gaps and lnr_cords_to_host return LNR_ERR_ARG; lnr_destroy gives
 * the batches in flight up and returns.
 * A read buffer in pinned host memory (lnr_host_alloc, or the caller's own hipHostMalloc / hipHostRegister) is uploaded by one
 * DMA at link rate; a pageable one goes through the context's pinned staging buffers first. */
lnr_status lnr_filter_submit(lnr_ctx *ctx, const uint8_t *reads_concat, const uint64_t *off, uint32_t n);
lnr_status lnr_filter_wait(lnr_ctx *ctx, lnr_cords *out);
void *lnr_host_alloc(size_t bytes);   /* pinned host memory for read blocks (NULL on failure) */
void lnr_host_free(void *p);
/* Device-buffer form: d_reads_concat / d_off already in HBM; results stay in HBM.  Streams: the library works on private
 * streams.  The device inputs must be complete before the call (the caller synchronises the stream that produced them) and
 * the results are complete when the call returns.  Every entry point leaves the caller's current HIP device as it found it. */
lnr_status lnr_filter_batch_dev(lnr_ctx *ctx, const uint8_t *d_reads_concat, const uint64_t *d_off, uint32_t n, lnr_cords_dev *out);
/* The device-buffer form in two halves: the same pipeline as lnr_filter_submit / lnr_filter_wait -- the same lanes, tickets and rules -- for
 * input that lies in HBM already and results that stay there.
 * lnr_filter_submit_dev takes what lnr_filter_batch_dev takes and returns at once.  Nothing is copied: the batch's input slot records the two
 * device pointers.  The device inputs must be complete before the call (as for lnr_filter_batch_dev) and stay untouched until the wait that
 * RETURNS their batch has returned.  h_off_or_null: the same n + 1 offsets on the host (lnr_reader_next_dev returns them); they are copied
 * during the call and save the library its synchronous read-back of d_off at the start of the batch.  With NULL that read-back happens.
 * lnr_filter_wait_dev hands out the oldest batch in flight as device arrays, without a download.
 * The halves combine freely: the submit says where the input is, the wait where the result goes.  A batch submitted by either submit may be
 * taken by either wait; lnr_filter_wait on a device-submitted batch downloads its cords as for any other.
 * Everything said above lnr_filter_submit holds for every combination: three batches in flight (a fourth submit: LNR_ERR_ARG), submission
 * order, a batch's error (LNR_ERR_LIMIT for a read of 2^20 bases included) reported by the wait that takes it with the batches around it
 * intact, two lanes with gap_len == 0 and the fall-back to one, one batch at a time with LNR_LANES=1 or gap_len > 0, what is refused while
 * batches are in flight, lnr_destroy, lnr_last_stats.  A wait with nothing in flight returns LNR_ERR_ARG.
 * Lifetime of a device result: its three arrays stay valid until the SECOND next wait on the context -- lnr_filter_wait or
 * lnr_filter_wait_dev, whichever -- is CALLED (not: has returned), which mirrors the rule for the host arrays: a writer may format batch k
 * on the device while the caller already sits in wait(k + 1).  The reason: lnr_filter_wait_dev does not leave the arrays in the lane's
 * result set, where the lane's next batch but one would be computed over them; it takes the set's buffers out of the lane and gives the lane
 * the buffers of the result that expires in exchange (pointer swaps under the context's lock, no copy, no allocation once they are grown).
 * So the lane's set is free when the call returns, exactly as after the download in lnr_filter_wait, and a lane never waits for the caller:
 * a scheme that kept the set itself occupied until the second next wait would stop the one-lane fall-back, where a batch of lane 1 needs a
 * set of lane 0 before that wait comes.  Every wait begins by retiring the result handed out by the wait before the last.  In one-lane
 * mode lnr_filter_wait_dev computes its batch inside the call and nothing ahead (there is no download to compute under), so it never
 * computes into arrays that are handed out.  After lnr_filter_wait_dev, lnr_cords_to_host has no batch to copy (LNR_ERR_ARG when the
 * buffers in place are too small) until the next lnr_filter_batch_dev. */
lnr_status lnr_filter_submit_dev(lnr_ctx *ctx, const uint8_t *d_reads_concat, const uint64_t *d_off /* n+1, device */,
                                 const uint64_t *h_off_or_null /* the same n+1 values on the host */, uint32_t n);
lnr_status lnr_filter_wait_dev(lnr_ctx *ctx, lnr_cords_dev *out);
/* apx_gaps of the last filter call -- apxMap's second output (include/pmpfinder.h:213-225), the input of the reference's gap
 * re-mapper mapGaps (src/mapper.cpp:448-453; not part of this library): per read, the uncovered stretches of the read as pairs of
 * cord words (first, second), as gather_gaps_y_ leaves them before the re-map loop (src/pmpfinder.cpp:2744).  CSR over the reads of
 * the batch; host arrays owned by the context, valid until the next call. */
typedef struct lnr_gaps {
    uint32_t n_reads;
    uint64_t n_gaps;
    const uint64_t *gap_off;    /* n_reads + 1 */
    const uint64_t *gaps;       /* 2 * n_gaps: first, second */
} lnr_gaps;
lnr_status lnr_last_gaps(lnr_ctx *ctx, lnr_gaps *out);
/* Copy the last device result to the context's host arrays. */
lnr_status lnr_cords_to_host(lnr_ctx *ctx, lnr_cords *out);

/* Stage a7 only (seed lookup on [0, L) with sampling step 15), for parity tests and the roofline measurement. */
lnr_status lnr_seed_lookup_batch(lnr_ctx *ctx, const uint8_t *reads_concat, const uint64_t *off, uint32_t n, lnr_anchors *out);
lnr_status lnr_seed_lookup_batch_dev(lnr_ctx *ctx, const uint8_t *d_reads_concat, const uint64_t *d_off, uint32_t n);

lnr_status lnr_last_stats(const lnr_ctx *ctx, lnr_stats *st);

/* The read stream's state of the gap re-mapper (gap_len > 0).  The reference keeps ONE GapParms per calculator thread for the whole run
 * (Mapper::loadOptions mapper.cpp:233-237, used in p_calRecords :447) and mapExtend / mapExtends leave it modified (gap_util.cpp:4046-4071,
 * 4088-4119).  Of the fields left behind only thd_cts_major_limit is read before it is written again (chainTiles :1188 under mapGeneric):
 * 1 until the first mapExtend / mapExtends of the thread's stream, 3 for every read after it.  A context therefore IS one read stream:
 * batches are taken in submission order, reads in batch order, exactly as `linear filter -t 1` meets them (with more threads the reference
 * itself is not reproducible: what a read sees depends on which reads its thread met before).  The state lives in the context across
 * batches.  set < 0: query only; set = 0: start a new stream (a new read file); set = 1: the stream has extended already -- what a
 * front-end that deals the batches of one file over several contexts / GPUs sets on the others once the first context reports 1.
 * *state (optional) receives the state after the call. */
lnr_status lnr_gap_stream(lnr_ctx *ctx, int set, int *state);
/* Change -g / -dup of an existing context (the index does not depend on them); starts a new read stream. */
lnr_status lnr_set_gap(lnr_ctx *ctx, uint32_t gap_len, uint32_t dup);

/* Input side (host code; replaces, for this path, the fetcher's SeqAn readRecords of src/parallel_io.cpp:433-485): FASTA or
 * FASTQ records, plain or gzip, or BAM records (an extension, see below), decoded into the layout lnr_filter_batch / lnr_filter_submit take.  Characters convert as SeqAn's
 * char -> Dna5 table does (A/a 0, C/c 1, G/g 2, T/t/U/u 3, anything else N = 4).  lnr_reader_next fills dst (e.g. a block from
 * lnr_host_alloc) with up to max_reads records and at most dst_cap bases, writes off[0 .. *n_out]; *n_out == 0 at end of file.
 * A record that no longer fits is delivered first by the next call.  lnr_reader_ids: header lines of the last block (without the
 * '>' / '@'), '\0'-separated, id_off[k] = start of id k. */
typedef struct lnr_reader lnr_reader;
typedef struct lnr_writer lnr_writer;
lnr_status lnr_reader_open(const char *path, lnr_reader **out);
lnr_status lnr_reader_next(lnr_reader *r, uint8_t *dst, uint64_t dst_cap, uint64_t *off, uint32_t max_reads, uint32_t *n_out);
lnr_status lnr_reader_ids(const lnr_reader *r, const char **ids, const uint64_t **id_off);
const char *lnr_reader_error(const lnr_reader *r);
void lnr_reader_close(lnr_reader *r);
/* GPU twin of lnr_reader_next: the text goes to `device` (a mapped file through two pinned staging buffers, a gzip file inflated straight into
 * pinned memory) and is parsed there -- classify, prefix sum, compact -- into device blocks the reader owns, in the layout lnr_filter_batch_dev and
 * lnr_writer_format_dev / _seq_dev take.  lnr_reader_next_dev delivers the blocks lnr_reader_next would deliver for the same dst_cap / max_reads
 * on the same file: the same n per call, the same offsets (*d_off on the device, *off the host's copy, n + 1 each), the same ordinals, the same
 * ids through lnr_reader_ids; no base comes back to the host.  The block is complete on return and stays valid until `slots` further calls.
 * The reader owns a stream and its buffers, is independent of any lnr_ctx and is used by one thread at a time; every entry leaves the caller's
 * current device as it found it; lnr_reader_close releases the GPU side.  Where a FASTQ file leaves the four-line form the serial parser takes
 * over, exactly where the mapped parser hands over, and its records are uploaded.  lnr_reader_next and lnr_reader_next_dev may be mixed on one
 * reader: both advance the same file position.  Errors: before lnr_reader_gpu_open LNR_ERR_ARG; slots outside 1..8 LNR_ERR_ARG; no usable device,
 * or a library linked without its device half, LNR_ERR_NO_DEVICE; a record that alone exceeds dst_cap LNR_ERR_LIMIT (lnr_reader_error says so).
 * lnr_reader_gpu_times: milliseconds of the last lnr_reader_next_dev, summed over its windows -- stage + upload (wall), measure, scan, emit (HIP
 * events), download of offsets and header spans (wall).  lnr_reader_gpu_tile: bytes of text per workgroup of the kernels (0 without the device
 * half).  LNR_READER_GPU_WINDOW in the environment: bytes of text per window (default 256 MiB, at most 1 GiB; a window without a whole record is
 * doubled); block boundaries do not depend on it.
 *
 * BGZF input (the blocked gzip of bgzip / htslib) is inflated on the device: only compressed bytes go up, no text byte crosses the bus.  A file
 * counts as BGZF when its first member has the magic 1f 8b, CM 8, FLG = FEXTRA and, among the subfields of its extra field, one 'B','C' of
 * length 2 (BSIZE), and lies inside the file.  Its blocks are walked one window at a time; each non-empty block is inflated by k_bgzf_inflate
 * behind the text the last window did not use, which stays on the device.  The gzread stream takes over -- at that member's offset, through a
 * fresh inflate stream opened there, never by re-reading the file -- at a member that is not BGZF, where the chain would leave the file or BSIZE
 * is too small for header and footer, where a FASTQ leaves the four-line form, and at the first lnr_reader_next on the reader.  A block whose
 * DEFLATE data is invalid, whose text is not ISIZE bytes or whose CRC32 differs from the footer makes the call return LNR_ERR_ARG and deliver
 * no block; lnr_reader_error names the block's file offset and the reason; the reader can only be closed after that.  LNR_READER_BGZF=0 in
 * the environment at lnr_reader_open: BGZF files are read like any gzip file (gzread into the pinned staging buffer).  lnr_reader_next
 * always reads gzip files through gzread.  lnr_reader_gpu_inflate_stats: counts of the last lnr_reader_next_dev and of all calls so far. */
typedef struct {
    uint64_t blocks;                 /* BGZF blocks inflated on the device */
    uint64_t compressed_bytes;       /* bytes of the file uploaded for them */
    uint64_t text_bytes;             /* text bytes produced on the device */
    uint64_t gzread_bytes;           /* text bytes that came through gzread instead */
    double inflate_ms, gather_ms;    /* k_bgzf_inflate and the gather of the header lines (HIP events) */
} lnr_inflate_counts;
typedef struct { lnr_inflate_counts last, total; } lnr_inflate_stats;
lnr_status lnr_reader_gpu_inflate_stats(const lnr_reader *r, lnr_inflate_stats *out);
lnr_status lnr_reader_gpu_open(lnr_reader *r, int32_t device, uint32_t slots /* 1..8 */);
lnr_status lnr_reader_next_dev(lnr_reader *r, uint64_t dst_cap, uint32_t max_reads, const uint8_t **d_reads_concat, const uint64_t **d_off /* n+1, device */,
                               const uint64_t **off /* n+1, host */, uint32_t *n_out);
lnr_status lnr_reader_gpu_times(const lnr_reader *r, double *ms5);
uint32_t lnr_reader_gpu_tile(void);
/* Plain gzip input (one member or several, as gzip / pigz write them) inflated on the device -- opt-in.  A single member is inflated in parallel
 * from DEFLATE block starts: the compressed bytes are read in rounds (LNR_READER_GZ_ROUND bytes, default 64 MiB) cut into chunks
 * (LNR_READER_GZ_CHUNK bytes, default 128 KiB, at least 1 KiB); every chunk is searched for a non-final dynamic-Huffman block start and decoded
 * from it with the 32 KiB history unknown; the pieces are chained in order -- a piece counts only where the decode of the piece before it ended
 * exactly on its start -- and the history is filled in afterwards.  The result never rests on a guess; a stream of fixed or stored blocks only
 * is decoded by one wave per round (slow, correct).  CRC32 and ISIZE of every member's trailer are checked; bytes behind the last member that
 * start no member are passed over, as gzread passes over them.
 * lnr_reader_gpu_gzip(r, 1): after lnr_reader_gpu_open and before the first read (else LNR_ERR_ARG).  A regular file that starts with a gzip
 * member that is not BGZF is then mapped and lnr_reader_next_dev reads it by rounds, the text staying on the device; at a member that is not
 * BGZF inside a BGZF file the gzip rounds take over where gzread takes over without the switch, and keep the file to its end.  Without the
 * switch nothing changes.  The host takes the stream over -- for a FASTQ that leaves the four-line form, and at a lnr_reader_next after
 * lnr_reader_next_dev -- through a fresh gzread stream moved to the text offset with gzseek, which inflates the file once more from its start.
 * A corrupt or cut stream: LNR_ERR_ARG, lnr_reader_error names the compressed file offset of the piece or trailer and the reason; blocks
 * delivered before it stay delivered; the reader can only be closed after that.  The text inflated in front of the failure is parsed as
 * the end of the file: where the stream breaks inside a record, the cut record may be delivered as a record (as lnr_reader_next delivers it
 * when gzread fails) before the next call reports the error.  lnr_reader_gpu_gzip_stats: counts of the last
 * lnr_reader_next_dev and of all calls so far.
 * lnr_gunzip_gpu: the same stages over a host buffer, no parse: gz[0, size) -> text[0, *text_size), size <= 2^31.  Text beyond text_cap, and a
 * corrupt stream: LNR_ERR_ARG with the reason and the compressed offset in err (text_size = the bytes of the rounds before it); no usable
 * device, or a library without its device half: LNR_ERR_NO_DEVICE.  stats may be NULL; its `last` is the last round. */
typedef struct {
    uint64_t rounds, members;        /* rounds that delivered text; members whose trailer was checked */
    uint64_t chunks, candidates;     /* chunks of those rounds; block-start candidates the chain came to (on them or past them) */
    uint64_t true_pieces;            /* pieces the chain landed on, the rounds' first pieces included */
    uint64_t false_candidates;       /* candidates a true piece's decode passed: true_pieces + false_candidates = candidates + rounds */
    uint64_t deflate_blocks;         /* DEFLATE blocks decoded */
    uint64_t compressed_bytes, text_bytes;
    uint64_t window_symbols;         /* text bytes that were references into the history of their piece */
    uint64_t gzread_bytes;           /* text bytes that came through gzread instead (the reader only; total: lnr_reader_next's too) */
    uint64_t grown_rounds;           /* rounds in which no block completed: run again with twice the bytes */
    double find_ms, measure_ms, stitch_ms, emit_ms, chain_ms, resolve_ms;   /* the six kernels (HIP events) */
    double parse_ms, upload_ms, download_ms;                                 /* measure + scan + emit of the reader (events); copies (wall) */
} lnr_gzip_counts;
typedef struct { lnr_gzip_counts last, total; } lnr_gzip_stats;
lnr_status lnr_reader_gpu_gzip(lnr_reader *r, int on);
lnr_status lnr_reader_gpu_gzip_stats(const lnr_reader *r, lnr_gzip_stats *out);
lnr_status lnr_gunzip_gpu(int32_t device, const uint8_t *gz, uint64_t size, uint8_t *text, uint64_t text_cap, uint64_t *text_size, lnr_gzip_stats *stats,
                          char *err, size_t err_cap);
/* BAM input (an extension: the reference reads FASTA / FASTQ).  A read file whose first four inflated bytes are "BAM\1" is read as BAM, aligned
 * or unaligned, whatever its name; lnr_reader_next reads it through gzread, lnr_reader_next_dev in both ways it reads BGZF text (device inflate,
 * or gzread into the pinned staging buffer under LNR_READER_BGZF=0) and delivers the blocks lnr_reader_next delivers.  A record is a read as
 * `samtools fastq` prints it: records with flag 0x100 or 0x800 (secondary, supplementary) are skipped; a record with flag 0x10 is delivered
 * reverse-complemented; the id is read_name without its NUL; the 4-bit codes A C G T become 0 1 2 3 and every other code N = 4; l_seq == 0 is a
 * read of length 0.  Qualities, CIGAR and aux tags are not carried anywhere.  A header-only BAM gives *n_out == 0.  A record that fails the
 * conditions every real record meets (l_read_name >= 1, l_seq >= 0, its parts fit block_size, block_size below 2^29, -1 <= refID, next_refID <
 * n_ref, pos, next_pos >= -1, the name ends in NUL), or that the file ends inside, makes the call return LNR_ERR_ARG and deliver no block;
 * lnr_reader_error names the record's ordinal in the file (from 0, skipped records counted) and its offset in the uncompressed stream, the same
 * from both entry points; the reader can only be closed after that.  On the device the record starts of a window are found tile by tile
 * (lnr_reader_gpu_bam_tile bytes each, 0 without the device half): every tile guesses its first start and walks on from it, one pass verifies
 * the guesses in order and walks a tile again where its guess was not the true position.  lnr_reader_gpu_bam_stats: counts of the
 * last lnr_reader_next_dev and of all calls so far.  lnr_reader_gpu_times keeps its five slots: find -> measure, stitch + take -> scan, emit -> emit. */
typedef struct {
    uint64_t records;                /* records delivered in blocks */
    uint64_t skipped;                /* secondary / supplementary records passed over */
    uint64_t reverse;                /* delivered records that were reverse-complemented (flag 0x10) */
    uint64_t tiles;                  /* tiles k_bam_find looked at */
    uint64_t repaired_tiles;         /* tiles whose guess did not stand: walked again from the true position, or lying inside a record */
    double find_ms, stitch_ms, emit_ms;      /* k_bam_find; k_bam_stitch + k_bam_meta; k_bam_emit (HIP events) */
} lnr_bam_counts;
typedef struct { lnr_bam_counts last, total; } lnr_bam_stats;
lnr_status lnr_reader_gpu_bam_stats(const lnr_reader *r, lnr_bam_stats *out);
/* The format of the file: 3 BAM, else what the reads so far have shown: 1 FASTA, 2 FASTQ, 0 not decided yet, -1 neither.  Not a pure
 * query: where nothing was read yet it reads the first buffer of the inflate stream (the bytes stay in front of the next read) and, on
 * "BAM\1", sets the reader's format.  A plain file that is not gzip (mapped at open) is never a BAM: there it does not look and returns 0
 * until a read has decided.  The front-end uses it to refuse a BAM genome. */
int lnr_reader_format(lnr_reader *r);
uint32_t lnr_reader_gpu_bam_tile(void);

/* The reference genome, from files to sequences resident on `device` (replaces, for a front-end, loading it through lnr_reader_next with
 * max_reads = 1 and uploading it from the host).  lnr_genome_load_gpu runs, per file, lnr_reader_open + lnr_reader_gpu_open(r, device, 1) and
 * lnr_reader_next_dev(r, block_bases, ...) until it delivers nothing: FASTA / FASTQ text is parsed on the device, BGZF is inflated there, plain
 * gzip goes through gzread unless LNR_GENOME_GPU_GZIP asks for the device inflate (lnr_reader_gpu_gzip(r, 1)).  Every delivered block is copied
 * device to device, on the reader's stream, into an allocation the genome owns (one per block); no base crosses the bus.  The object holds
 * the sequences the lnr_reader_next(max_reads = 1) loop over the same files delivers, in the same order (files in order, records in file
 * order): the same lengths, the same Dna5 ordinals, the same header lines (whole; a front-end cuts them at the first blank itself).
 * block_bases: bases per block, 0 = 2^30 (no record the reader delivers is longer: its text limit is 2^30 bytes); the sequences do not
 * depend on it.  lnr_genome_info: any out pointer may be NULL; len[nseq], id_off[nseq + 1] and the array d_seq[nseq] are host arrays owned
 * by the object, ids = the header lines '\0'-separated, d_seq[i] = device address of sequence i (never NULL, also where len[i] == 0; what
 * lnr_index_build and lnr_writer_set_genome_dev take) -- *d_seq is NULL after lnr_genome_drop_dev.  lnr_genome_to_host: one download into
 * host memory of the object, kept until lnr_genome_free; repeated calls return the same pointers; after lnr_genome_drop_dev only where it
 * was called before (else LNR_ERR_ARG).  lnr_genome_drop_dev frees the device copy (lengths, ids and a host copy stay).  Every entry leaves
 * the caller's current device as it found it.
 * Errors of lnr_genome_load_gpu (*out is NULL, nothing stays allocated, lnr_genome_error(NULL) = the message of this thread's last failed
 * load): a file that is a BAM: LNR_ERR_ARG naming the file; a file that cannot be opened: the reader's status; a record longer than
 * block_bases or whose text exceeds the reader's limit: LNR_ERR_LIMIT naming the file and the record's ordinal in it (from 0); a corrupt
 * compressed block: the reader's LNR_ERR_ARG text with its file offset; no usable device, or a library linked without its device half:
 * LNR_ERR_NO_DEVICE.  Files without any sequence: LNR_OK and nseq == 0. */
typedef struct lnr_genome lnr_genome;
#define LNR_GENOME_GPU_GZIP 1u   /* plain (non-BGZF) gzip members inflated on the device, as lnr_reader_gpu_gzip(r, 1) */
lnr_status lnr_genome_load_gpu(const char *const *paths, uint32_t npaths, int32_t device, uint32_t flags, uint64_t block_bases /* 0 = default */, lnr_genome **out);
lnr_status lnr_genome_info(const lnr_genome *g, uint32_t *nseq, const uint64_t **len /* nseq, host */, const char **ids /* NUL-terminated, whole header lines */,
                           const uint64_t **id_off /* nseq+1 */, const uint8_t *const **d_seq /* nseq device pointers, host array; NULL after drop_dev */);
lnr_status lnr_genome_to_host(lnr_genome *g, const uint8_t *const **seq);
lnr_status lnr_genome_drop_dev(lnr_genome *g);
const char *lnr_genome_error(const lnr_genome *g);
void lnr_genome_free(lnr_genome *g);

/* Output side (host threads, and a GPU twin below; replaces, for this path, the calculator's tail cords2BamLink + fillBamRecords, src/mapper.cpp:463-470,
 * src/f_io.cpp:758-1011, src/align_util.cpp:301-343,452-744, and the printer's writeSam / print_cords_apf, src/f_io.cpp:100-207,
 * 313-412): the cords of a batch as SAM records (what = 1) or APF text (what = 2), byte for byte what the reference prints for
 * the same cords with -g 0 (MAPQ 255, flag 16 / 2048, SA:Z of the read's other lines; APF: a blank line before every '@' record
 * of a read that is not the first of the call, as the reference does per block).  read_ids = header lines, '\0'-separated,
 * id_off[k] = start of id k (the layout lnr_reader_ids returns); read_len[k] = bases of read k.  The text is owned by the writer
 * and valid until its next call.  lnr_writer_sam_header: @SQ per sequence, @RG ID: SM:, @PG ID:M1-3 PN:Linear CL:<command_line>. */
lnr_status lnr_writer_create(const char *const *genome_ids, const uint64_t *genome_len, uint32_t nseq, lnr_writer **out);
lnr_status lnr_writer_format(lnr_writer *w, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids, const uint64_t *id_off,
                             int what, uint32_t threads, const char **text, uint64_t *size);
lnr_status lnr_writer_sam_header(lnr_writer *w, const char *command_line, const char **text, uint64_t *size);
/* -p (mapper.cpp:173-196): preset 1 splits large diagonal shifts of a CIGAR (thd_DI 80, thd_X 200); presets 0 and 2 leave the reference's
 * defaults (2^60 - 1: never).  -rg / -sn: the @RG line's ID / SM (mapper.cpp:288-324); both empty by default. */
lnr_status lnr_writer_set_preset(lnr_writer *w, uint32_t preset);
lnr_status lnr_writer_set_read_group(lnr_writer *w, const char *read_group, const char *sample_name);
void lnr_writer_destroy(lnr_writer *w);
/* GPU twin of lnr_writer_format: the same bytes, formatted on `device`.  A writer with a GPU side owns a stream and its buffers there, is
 * independent of any lnr_ctx (may run while a context computes on the same device) and is used by one thread at a time.  The text lands in
 * pinned host memory owned by the writer, valid until the writer's next format call; lnr_writer_set_preset applies to both sides.
 * lnr_writer_format_dev takes what lnr_filter_batch_dev hands out (the caller has waited for that call) and the batch's d_off;
 * lnr_writer_format_gpu uploads host cords and goes the same way.  Before lnr_writer_gpu_open both return LNR_ERR_ARG;
 * lnr_writer_destroy releases the GPU side.  Every entry leaves the caller's current device as it found it.  lnr_writer_error: detail of
 * the writer's last failure.  lnr_writer_gpu_times: wall / device milliseconds of the last GPU format call -- upload (wall), measure, scan,
 * emit (HIP events), download (wall). */
lnr_status lnr_writer_gpu_open(lnr_writer *w, int32_t device);              /* LNR_ERR_NO_DEVICE without a usable device */
lnr_status lnr_writer_format_gpu(lnr_writer *w, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids,
                                 const uint64_t *id_off, int what, const char **text, uint64_t *size);   /* host cords in (uploaded), host text out */
lnr_status lnr_writer_format_dev(lnr_writer *w, const lnr_cords_dev *cords, const uint64_t *d_read_off /* n + 1, the batch's d_off */,
                                 const char *read_ids, const uint64_t *id_off, int what, const char **text, uint64_t *size);
lnr_status lnr_writer_gpu_times(const lnr_writer *w, double *ms5);
const char *lnr_writer_error(const lnr_writer *w);
/* SAM with the SEQ column, as the reference prints it with -ss 1 (fillBamRecordLinkRecords align_util.cpp:745-808, cigar2SamSeq :1434-1500):
 * the record's CIGAR is walked with the genome at (RNAME, POS) and the read at its first base (flag 16: at the first base of its reverse
 * complement); S and I print the read's bases, '=' prints the GENOME's, X prints the read's base where it differs from the genome's and N
 * where it does not, D prints nothing; an empty SEQ prints '*'.  Every other byte of the line is that of lnr_writer_format(what = 1).
 * A source position outside its sequence (undefined behaviour in the reference) reads as ordinal 0 ('A'), ordinals above 4 read as N.
 * lnr_writer_set_genome: nseq host pointers (Dna5 ordinals, lengths as given to lnr_writer_create), borrowed until lnr_writer_destroy or the
 * next call; NULL = off.  Without it the three format calls return LNR_ERR_ARG (lnr_writer_error says so); the two GPU forms also before
 * lnr_writer_gpu_open.  The GPU side uploads ITS OWN byte-per-base copy of the genome in the first SEQ call after set_genome + gpu_open
 * (either order) and again only after another set_genome: 3.1 GB of HBM for a human genome, next to whatever a lnr_ctx holds -- the
 * writer stays independent of any context.  reads_concat / read_off[n + 1]: the layout lnr_filter_batch takes (device memory for _dev).
 * Text lifetime, current device and lnr_writer_gpu_times as for the calls above. */
lnr_status lnr_writer_set_genome(lnr_writer *w, const uint8_t *const *seq);
/* The GPU side's copy taken from device memory instead: d_seq = nseq device pointers on the writer's device (a host array, e.g. lnr_genome_info's),
 * copied device to device on the writer's stream before the call returns; nothing is borrowed.  After lnr_writer_gpu_open (before it: LNR_ERR_ARG).
 * The GPU SEQ / BAM forms then work as after lnr_writer_set_genome; the host forms keep returning "no bases for SEQ" unless host pointers are
 * set as well.  A later lnr_writer_set_genome replaces the copy (the next GPU SEQ call uploads the host sequences); NULL = off.
 * Nothing about d_seq is checked beyond NULL entries: sequence i is read for the genome_len[i] bytes given to lnr_writer_create, whatever
 * the genome behind the pointers was loaded with (shorter sequences: bytes behind them are read), and pointers into another device's memory
 * are not refused: the copy then fails with LNR_ERR_HIP, or goes over the peer link where peer access is on. */
lnr_status lnr_writer_set_genome_dev(lnr_writer *w, const uint8_t *const *d_seq);
lnr_status lnr_writer_format_seq(lnr_writer *w, const lnr_cords *cords, const uint8_t *reads_concat, const uint64_t *read_off,
                                 const char *read_ids, const uint64_t *id_off, uint32_t threads, const char **text, uint64_t *size);
lnr_status lnr_writer_format_seq_gpu(lnr_writer *w, const lnr_cords *cords, const uint8_t *reads_concat, const uint64_t *read_off,
                                     const char *read_ids, const uint64_t *id_off, const char **text, uint64_t *size);
lnr_status lnr_writer_format_seq_dev(lnr_writer *w, const lnr_cords_dev *cords, const uint8_t *d_reads_concat, const uint64_t *d_read_off,
                                     const char *read_ids, const uint64_t *id_off, const char **text, uint64_t *size);
/* BGZF output of the GPU writer.  on != 0: lnr_writer_format_gpu / _dev / _seq_gpu / _seq_dev return, in *text / *size, whole BGZF members
 * whose inflated concatenation is byte for byte the text the same call returns with it off; block k holds text [k*0xff00, ...); an empty
 * text gives zero bytes; no EOF marker is added.  Before lnr_writer_gpu_open: LNR_ERR_ARG.  lnr_writer_format / _format_seq are not affected.
 * The text is compressed where it was formatted (one dynamic-Huffman DEFLATE block per member, a stored block where that is not smaller:
 * a member is at most its text + 31 bytes) and only the members are downloaded: with the switch on, download_ms of lnr_writer_gpu_times
 * times that download.  The bytes are a function of the text alone.  Lifetime of the returned bytes: until the writer's next format or
 * lnr_writer_bgzf_bytes_gpu call. */
lnr_status lnr_writer_set_bgzf(lnr_writer *w, int on);
/* Any host bytes (the SAM header) compressed the same way on the writer's device; size 0 gives zero bytes. */
lnr_status lnr_writer_bgzf_bytes_gpu(lnr_writer *w, const char *bytes, uint64_t size, const char **data, uint64_t *out_size);
/* The 28-byte empty member that ends a BGZF file (host constant; needs no device). */
lnr_status lnr_writer_bgzf_eof(const char **data, uint64_t *size);
typedef struct { uint64_t blocks, stored_blocks, text_bytes, compressed_bytes; double deflate_ms, pack_ms; } lnr_bgzf_stats;   /* last GPU call */
lnr_status lnr_writer_bgzf_stats(const lnr_writer *w, lnr_bgzf_stats *out);

/* BAM output (what the reference writes with -ot 4 / 8).  A record is the plain re-encoding of the SAM line the calls above print for the same
 * cords, little endian: block_size, refID (index of RNAME among the writer's sequences, -1 for '*'), pos = POS - 1, l_read_name, mapq 255,
 * bin = reg2bin(pos, pos + reference bases of the CIGAR), n_cigar_op, flag, l_seq, next_refID -1, next_pos -1, tlen 0, QNAME and a NUL, one
 * word count << 4 | op per CIGAR element (MIDNSHP=X = 0..8), SEQ at two bases per byte (high nibble first, =ACMGRSVTWYHKDBN = 0..15; an
 * odd tail gets a low nibble of 0), l_seq bytes 0xff, and where the line has SA:Z: the bytes 'S' 'A' 'Z', the tag's text and a NUL -- byte
 * for byte the records of the reference's .bam (tests/golden/cli_bam_<case>.npz).  Fields narrower than their value take its low bits, as
 * the reference's (SeqAn's) casts do: a QNAME of 255 or more characters and more than 65535 CIGAR elements give records no reader can
 * walk; both are outside the tested ground.
 * lnr_writer_bam_header (host only): "BAM\1", l_text, the text of lnr_writer_sam_header (pbsv != 0: the -ot 8 form, whose @RG line reads
 * "@RG\t ID:" with a blank before ID), then the reference list: n_ref = the writer's nseq sequences, each l_name (with the NUL), the name,
 * a NUL and l_ref.  THE ONE DELIBERATE DEVIATION FROM THE REFERENCE: it writes n_ref = 0 (an empty context, f_io.cpp:509-523) while its
 * records carry refID >= 0, a file htslib refuses; with the list the same records open in samtools, pbsv and IGV.
 * lnr_writer_format_bam (host threads; the in-library yardstick of the GPU forms): the records of a batch back to back.  ONE function
 * for both forms: reads_concat == NULL -- no SEQ (l_seq 0) and read_len_or_off is read_len[n]; otherwise SEQ as lnr_writer_format_seq prints
 * it, lnr_writer_set_genome is required (else LNR_ERR_ARG) and read_len_or_off is read_off[n + 1].  lnr_writer_format_bam_gpu takes the
 * same arguments (host memory) and formats on the GPU (k_out_measure<Bam> / k_out_scan / k_out_emit<Bam>); lnr_writer_format_bam_dev takes
 * what lnr_filter_batch_dev hands out, the batch's d_off and its device bases d_reads_concat or NULL.  With lnr_writer_set_bgzf off
 * the two return the raw record bytes, with it on BGZF members of them, compressed where they lie.  A .bam file = the members of
 * lnr_writer_bgzf_bytes_gpu(the header), of every batch, and lnr_writer_bgzf_eof.  No record: zero bytes.  Before lnr_writer_gpu_open:
 * LNR_ERR_ARG; no device: LNR_ERR_NO_DEVICE (from lnr_writer_gpu_open).  Lifetime of the bytes, errors, current device,
 * lnr_writer_gpu_times and lnr_writer_bgzf_stats as for the SAM calls. */
lnr_status lnr_writer_bam_header(lnr_writer *w, const char *command_line, int pbsv, const char **data, uint64_t *size);
lnr_status lnr_writer_format_bam(lnr_writer *w, const lnr_cords *cords, const uint8_t *reads_concat_or_null, const uint64_t *read_len_or_off,
                                 const char *read_ids, const uint64_t *id_off, uint32_t threads, const char **data, uint64_t *size);
lnr_status lnr_writer_format_bam_gpu(lnr_writer *w, const lnr_cords *cords, const uint8_t *reads_concat_or_null, const uint64_t *read_len_or_off,
                                     const char *read_ids, const uint64_t *id_off, const char **data, uint64_t *size);
lnr_status lnr_writer_format_bam_dev(lnr_writer *w, const lnr_cords_dev *cords, const uint8_t *d_reads_concat_or_null, const uint64_t *d_read_off,
                                     const char *read_ids, const uint64_t *id_off, const char **data, uint64_t *size);

/* PAF output (an extension: the reference writes none).  What the filter computes is an approximate mapping, and PAF is the format general
 * long-read tools read for one: twelve tab-separated columns and tags, one line per mapping, no header.  One line per SAM record of a read,
 * in the order lnr_writer_format(what = 1) prints them -- the same segmentation under the writer's preset.  For the record whose first cord
 * is lo and whose last cord is hi, with the elements of its CIGAR* (S I D = X):
 *    1  query name      the QNAME of the SAM line
 *    2  query length    L = read_len[k]
 *    3, 4  query start, end   0-based, on the ORIGINAL read strand.  lead = y(cords_str[lo]); trail = max(0, (int)(L - y(cords_end[hi]))) -- the
 *                       two numbers the S elements of the CIGAR* hold.  Forward: lead, L - trail.  Flag 16: trail, L - lead.
 *    5  strand          '+' or '-' (the strand bit of cords_str[lo])
 *    6  target name     the RNAME of the SAM line: '*' for a sequence id at or beyond nseq
 *    7  target length   genome_len[id]; 0 for '*'
 *    8, 9  target start, end  x(cords_str[lo]) (= POS - 1), and that plus the sum of the = X D counts (no max(1, .) as in the sort key)
 *    10 matches         the sum of the '=' counts
 *    11 block length    the sum of the = X I D counts
 *    12 mapping quality 255
 *    cg:Z:              the record's merged elements without the S elements, count then op; the tag and its tab are left out when none remains
 * Numbers are decimal without padding, the line ends with '\n'.  A read without cords gives no line (no PAF for unmapped reads); nothing
 * is sorted.  lnr_writer_format_paf: on `threads` host threads, the in-library yardstick.  lnr_writer_format_paf_gpu (host cords in) and
 * lnr_writer_format_paf_dev (what lnr_filter_batch_dev hands out and the batch's d_off) format on the GPU (k_out_measure<Paf> / k_out_scan /
 * k_out_emit<Paf>) and return the same bytes -- with lnr_writer_set_bgzf on, BGZF members of them (an empty text: zero bytes).  Before
 * lnr_writer_gpu_open the two return LNR_ERR_ARG.  Text lifetime, errors, current device and lnr_writer_gpu_times as for lnr_writer_format_gpu
 * / _dev. */
lnr_status lnr_writer_format_paf(lnr_writer *w, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids, const uint64_t *id_off,
                                 uint32_t threads, const char **text, uint64_t *size);
lnr_status lnr_writer_format_paf_gpu(lnr_writer *w, const lnr_cords *cords, const uint64_t *read_len, const char *read_ids,
                                     const uint64_t *id_off, const char **text, uint64_t *size);
lnr_status lnr_writer_format_paf_dev(lnr_writer *w, const lnr_cords_dev *cords, const uint64_t *d_read_off /* n + 1, the batch's d_off */,
                                     const char *read_ids, const uint64_t *id_off, const char **text, uint64_t *size);

/* Coordinate-sorted BAM with a BAI index (an extension: the reference tells its users to run `samtools sort` / `samtools index`).
 * A sort mode of the GPU writer.  Between lnr_writer_sort_begin and lnr_writer_sort_finish, lnr_writer_format_bam_gpu / _dev keep the
 * batch's raw records (copied by k_sort_keep into segments the GPU side owns: at least 256 MiB each -- less where max_device_bytes leaves
 * less --, a batch contiguous in one) and return *size = 0; lnr_writer_bam_header puts "@HD\tVN:1.6\tSO:coordinate\n" in front of its text;
 * every other call is unchanged.
 * THE HOLD IS COMPACT: this writer has no qualities, every record with SEQ carries l_seq bytes of 0xff, and those are not held; the gather
 * writes them again, so the sorted stream and every size reported about it are those of the full records.  Held per read: about 0.8 KB
 * without SEQ, 5.8 KB of the 15.8 KB record of a 10 kb read with it.  max_device_bytes bounds the bytes HELD on the device (0: no bound of
 * its own; without SEQ held and record bytes are the same number).
 * THE TIERS: a batch goes to the device if it fits under max_device_bytes and its segment can be allocated.  Otherwise, once
 * lnr_writer_sort_spill(max_host_bytes) has been called in this round (while collecting; 0 switches it off again), it goes to the host tier
 * if held_host_bytes + batch <= max_host_bytes and its segment can be allocated: pinned host memory the GPU reads in place (hipHostMalloc;
 * segments of 64 MiB, less where max_host_bytes leaves less, never less than the batch; no managed memory, no XNACK), written by one
 * device-to-host copy per batch and read by k_sort_gather over the bus when the pieces are made.  Otherwise the BAM call returns
 * LNR_ERR_NOMEM (lnr_writer_error names the bytes held -- on both tiers where the host tier is on -- and asked for) and leaves the batches
 * added before intact.  A batch is whole in one segment of one tier.  Everything is held until lnr_writer_sort_end, which also ends the
 * spill setting: it belongs to the round.  lnr_writer_sort_hold_info_get (any time between begin and end): what is held where.
 * THE ORDER: (uint32)refID (so -1 sorts last), (uint32)pos, the reverse-strand bit (flag & 0x10, forward first), then the record's byte
 * offset in the stream of records as they were added (batches in call order, records as the BAM calls emit them).  The order is total: the
 * output is a function of the input alone.  Whether samtools breaks (refID, pos) ties by strand has not been verified here.
 * lnr_writer_sort_finish sorts on the device (k_sort_index per batch, rocPRIM's stable radix sort, a scan of the sorted sizes).  The sorted
 * stream S is then handed out by lnr_writer_sort_next in pieces of piece_members (0: 4096) BGZF members: k_sort_gather writes S[a, b) of
 * the piece, k_bgzf_deflate / k_bgzf_pack compress it; member k holds S[k * 0xff00, ...) whatever piece_members is, so the file's bytes do
 * not depend on it.  *size == 0: no piece is left.  A file = the members of the header, the pieces, lnr_writer_bgzf_eof.
 * lnr_writer_sort_bai (valid once lnr_writer_sort_next has returned size 0): the .bai of that file, first_offset = file bytes in front of
 * the first record member (the header's members).  Layout: "BAI\1", n_ref = nseq, per reference n_bin, per bin (ascending) bin, n_chunk,
 * chunks (beg, end), n_intv, ioffset[]; n_no_coor.  Virtual offset of stream offset s: (first_offset + member_off[s / 0xff00]) << 16 |
 * s % 0xff00.  Bin = reg2bin(pos, end), end = pos + max(1, reference bases of the CIGAR); a bin's chunks in file order, a record whose
 * predecessor in the file has the same refID and bin extends that chunk, no other merging; pseudo-bin 37450 last (first start .. last end;
 * records without / with flag 4); ioffset[w] = smallest start of the records over 16 KiB window w, an empty window takes the next higher
 * one's value; a reference without records has n_bin 0 and n_intv 0; refID < 0 counts in n_no_coor.  A record with refID >= 0 and pos < 0
 * or end > 2^29 cannot be indexed: LNR_ERR_UNSUPPORTED naming the record (the sorted BAM stays valid).  Byte equality with `samtools index`
 * is not claimed (htslib merges chunks further).  Bytes returned live until the writer's next call.
 * Errors: before lnr_writer_gpu_open, and calls out of order (begin twice, spill before begin or after finish, next before finish, bai before the last piece): LNR_ERR_ARG with
 * the reason in lnr_writer_error.  lnr_writer_sort_end frees the segments and leaves the mode; lnr_writer_destroy does so too.
 * lnr_writer_sort_host / lnr_writer_bai_host: the same order and the same index on the host, no device needed (the in-library yardsticks). */
typedef struct {
    uint64_t records, record_bytes;  /* kept records and their bytes (the length of S) */
    uint64_t device_bytes;           /* device memory the sort holds: segments and per-record arrays */
    uint64_t members;                /* BGZF members of S */
    double index_ms, sort_ms;        /* k_sort_index summed over the batches; the sort with its gathers and scan (HIP events) */
    double gather_ms, deflate_ms, pack_ms, download_ms;   /* summed over the pieces handed out so far */
} lnr_sort_info;
typedef struct {
    uint64_t stream_bytes;                 /* length of S so far */
    uint64_t held_device_bytes, held_host_bytes;   /* record bytes held per tier (compact) */
    uint64_t device_batches, host_batches; /* batches that went to each tier */
    double keep_ms, spill_ms;              /* k_sort_keep summed; device->host copies summed */
} lnr_sort_hold_info;
lnr_status lnr_writer_sort_begin(lnr_writer *w, uint64_t max_device_bytes);
lnr_status lnr_writer_sort_spill(lnr_writer *w, uint64_t max_host_bytes);   /* while collecting; 0 switches it off again */
lnr_status lnr_writer_sort_hold_info_get(const lnr_writer *w, lnr_sort_hold_info *out);  /* any time between begin and end */
lnr_status lnr_writer_sort_finish(lnr_writer *w, uint32_t piece_members, lnr_sort_info *info /* optional; piece times still 0 */);
lnr_status lnr_writer_sort_next(lnr_writer *w, const char **data, uint64_t *size);
lnr_status lnr_writer_sort_bai(lnr_writer *w, uint64_t first_offset, const char **data, uint64_t *size);
lnr_status lnr_writer_sort_info_get(const lnr_writer *w, lnr_sort_info *info);      /* any time between finish and end: the sums so far */
lnr_status lnr_writer_sort_end(lnr_writer *w);
lnr_status lnr_writer_sort_host(lnr_writer *w, const char *records, uint64_t size, const char **sorted);
lnr_status lnr_writer_bai_host(lnr_writer *w, const char *sorted_records, uint64_t size, uint64_t first_offset, const uint64_t *member_off /* n_members + 1 */,
                               uint64_t n_members, const char **data, uint64_t *bai_size);

#ifdef __cplusplus
}
#endif
#endif
