// linear_filter_main.cpp -- the `linear filter` front-end over the C ABI (include/linear_amd.h).  Plain C++ host code: everything it does goes
// through the ABI, so it doubles as the integration example.  It mirrors the reference's program around the hot path:
//   command line   src/args_parser.cpp:14-343 -- `filter` word optional, bare -g / -r / -ss mean 1 (:42-71), every option of the table at :150-270 by
//                  its short and long name, several read files and the `x` separator (:297-319), E[01] / E[02] / E[05] / E[06] (mapper.cpp:143-160)
//   defaults       Options::Options src/base.cpp:26-50 -- -t 16, -ot 2 (.sam only), -g 1 (= gaps of 50), -p 1, -i 1, -f 2
//   output naming  Mapper::p_printResults src/mapper.cpp:478-509 -- without -o one output per read file, named by the file's name up to its first '.';
//                  with -o one output for all read files
//   pipeline       process3 / p_ThreadProcess src/linear.cpp:68-91, src/parallel_io.cpp:372-608 -- ONE fetcher, calculators, ONE printer, output in
//                  input order -- here: a reader thread (FASTA / FASTQ(.gz) / BAM -> pinned blocks), one calculator thread + one lnr_ctx PER GPU (blocks dealt in
//                  order, three blocks in flight per GPU: upload, kernels and download of consecutive blocks overlap), a writer thread that restores
//                  the file order and formats on -t host threads.
//   several GPUs   --gpus N (extension): the index is built once on the first GPU and moved to the others with RCCL (lnr_index_broadcast, north_star;
//                  --index-mode build = every GPU builds its own instead; both times are printed).  Reads shard, nothing else is exchanged.
//   gap stream     with -g > 0 the reference's result depends on the order reads meet a thread's GapParms (lnr_gap_stream in the header): the blocks
//                  are taken strictly in file order until a block reports the stream "extended"; from then on every GPU runs freely with that state.
//                  The result is the reference's `-t 1` result whatever --gpus is.
//   device chain   --gpu-reader (extension): the reader thread parses the read files on the first GPU (lnr_reader_next_dev, five device blocks), the
//                  calculator hands them to lnr_filter_submit_dev, up to three ahead, and the text comes from lnr_filter_wait + the host writer or,
//                  with --gpu-writer, from lnr_filter_wait_dev and lnr_writer_format_dev / _seq_dev on the same device buffers: no read base crosses
//                  PCIe, and the context's two lanes compute the next blocks while the text of one is made.  One GPU; the same bytes as the
//                  default path.  LNR_CLI_DEV_HALVES=0 in the environment: one lnr_filter_batch_dev at a time on three blocks, as a library
//                  without the halves gets it.
//   BGZF output    --bgzf (extension, needs --gpu-writer): the text is compressed on the GPU it was formatted on (lnr_writer_set_bgzf) and the
//                  outputs are PREFIX.sam.gz / PREFIX.apf.gz: the SAM header through lnr_writer_bgzf_bytes_gpu, every block's members as
//                  returned, the EOF marker at close.  bgzip -d, zcat and samtools read them.
//   BAM output     -ot 4 (PREFIX.bam) / -ot 8 (PREFIX_pbsv.bam), in any combination with 1 and 2; needs --gpu-writer: the records are encoded
//                  on the GPU (lnr_writer_format_bam_gpu / _dev) and compressed where they lie, whether --bgzf is given or not.  Each file: the
//                  members of the header (lnr_writer_bam_header through lnr_writer_bgzf_bytes_gpu; -ot 8: the "@RG\t ID:" form), of every
//                  block, and the EOF marker.  --sam-seq puts SEQ into the records as it does into the .sam.  The header lists the genome
//                  (the reference writes n_ref 0: include/linear_amd.h).
//   sorted BAM     --sort (extension, needs -ot with 4 or 8 and --gpu-writer): the records of an output file stay on the GPU (lnr_writer_sort_begin
//                  before the file's first block), and when the file ends they are sorted by coordinate there: the header's members (with
//                  @HD SO:coordinate), the pieces of lnr_writer_sort_next as they come, the EOF marker, then PREFIX.bam.bai / PREFIX_pbsv.bam.bai
//                  from lnr_writer_sort_bai(bytes of that file's header).  The .sam / .apf next to it stay in read order.  All records of
//                  a file are held until it ends, without their 0xff quality runs: in HBM, --sort-device-mem SIZE of it at most
//                  (lnr_writer_sort_begin's max_device_bytes), and with --sort-host-mem SIZE what does not fit there in pinned host memory
//                  (lnr_writer_sort_spill right after every begin).
//   SEQ column     --sam-seq (extension): the .sam carries the read sequences the reference prints with -ss 1 (lnr_writer_format_seq / _seq_gpu); the
//                  option -ss itself stays refused.
//   PAF output     --paf (extension): PREFIX.paf next to whatever -ot asks for, one line per record of the .sam (twelve columns and cg:Z:, the line's
//                  definition: include/linear_amd.h), named, split over read files and ordered as the .sam is.  Host writer by default
//                  (lnr_writer_format_paf), lnr_writer_format_paf_gpu with --gpu-writer, lnr_writer_format_paf_dev in the device chain; with --bgzf
//                  PREFIX.paf.gz (BGZF members and the EOF marker).  --sort does not touch it.
//   genome on GPU  --gpu-genome (extension): the genome files are loaded by lnr_genome_load_gpu on the first GPU (text parsed there, BGZF inflated
//                  there, plain gzip too with --gpu-gunzip), the index is built from the device pointers, a GPU writer with --sam-seq takes its
//                  copy device to device (lnr_writer_set_genome_dev), then the loader's copy is dropped.  What needs host bases (a host writer
//                  with --sam-seq, --index-mode build on the other GPUs) takes one download (lnr_genome_to_host).  The same bytes as without it.
//   BAM input      (extension) a read file may be a BAM, aligned or unaligned: found by its content (the first four inflated bytes are "BAM\1"), never
//                  by its name, with the default host reader and under --gpu-reader (record starts found on the GPU: DESIGN 6h).  Its reads are
//                  what `samtools fastq` prints: secondary / supplementary records (flag 0x100 / 0x800) are skipped, reverse-strand records
//                  (0x10) reverse-complemented, the id is read_name; qualities and tags are dropped.  A record that is not valid BAM, or that
//                  the file ends inside, ends the run with the record's ordinal and offset in the uncompressed stream.  Output naming is
//                  unchanged.  A genome file that is a BAM is refused.
// Not built (exit 1 with a message, never a silently different result): BAM output (-ot 4 / 8) without --gpu-writer, -ss 1 (use --sam-seq), -c 0, -f 1, -r 1, -p 0, -b 0
// (the reference's -b 0 path writes a header-only SAM: SURVEY App. C.7).
#include "../../include/linear_amd.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

// entry points only --gpu-reader uses: referred to weakly, so that the front-end still links against a library without them (the test double)
extern "C" {
lnr_status lnr_filter_batch_dev(lnr_ctx *, const uint8_t *, const uint64_t *, uint32_t, lnr_cords_dev *) __attribute__((weak));
lnr_status lnr_cords_to_host(lnr_ctx *, lnr_cords *) __attribute__((weak));
lnr_status lnr_filter_submit_dev(lnr_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, uint32_t) __attribute__((weak));   // (a library without the
lnr_status lnr_filter_wait_dev(lnr_ctx *, lnr_cords_dev *) __attribute__((weak));                                                  //  halves: one batch at a time)
lnr_status lnr_writer_format_dev(lnr_writer *, const lnr_cords_dev *, const uint64_t *, const char *, const uint64_t *, int, const char **, uint64_t *) __attribute__((weak));
lnr_status lnr_writer_format_seq_dev(lnr_writer *, const lnr_cords_dev *, const uint8_t *, const uint64_t *, const char *, const uint64_t *, const char **, uint64_t *) __attribute__((weak));
lnr_status lnr_writer_format_bam_dev(lnr_writer *, const lnr_cords_dev *, const uint8_t *, const uint64_t *, const char *, const uint64_t *, const char **, uint64_t *) __attribute__((weak));
lnr_status lnr_reader_gpu_open(lnr_reader *, int32_t, uint32_t) __attribute__((weak));
lnr_status lnr_reader_next_dev(lnr_reader *, uint64_t, uint32_t, const uint8_t **, const uint64_t **, const uint64_t **, uint32_t *) __attribute__((weak));
int lnr_reader_format(lnr_reader *) __attribute__((weak));
lnr_status lnr_reader_gpu_gzip(lnr_reader *, int) __attribute__((weak));                // --gpu-gunzip
// entry points only --sort uses
lnr_status lnr_writer_sort_begin(lnr_writer *, uint64_t) __attribute__((weak));
lnr_status lnr_writer_sort_finish(lnr_writer *, uint32_t, lnr_sort_info *) __attribute__((weak));
lnr_status lnr_writer_sort_next(lnr_writer *, const char **, uint64_t *) __attribute__((weak));
lnr_status lnr_writer_sort_bai(lnr_writer *, uint64_t, const char **, uint64_t *) __attribute__((weak));
lnr_status lnr_writer_sort_end(lnr_writer *) __attribute__((weak));
lnr_status lnr_writer_sort_spill(lnr_writer *, uint64_t) __attribute__((weak));        // (--sort-host-mem alone)
// entry points only --paf uses
lnr_status lnr_writer_format_paf(lnr_writer *, const lnr_cords *, const uint64_t *, const char *, const uint64_t *, uint32_t, const char **, uint64_t *) __attribute__((weak));
lnr_status lnr_writer_format_paf_gpu(lnr_writer *, const lnr_cords *, const uint64_t *, const char *, const uint64_t *, const char **, uint64_t *) __attribute__((weak));
lnr_status lnr_writer_format_paf_dev(lnr_writer *, const lnr_cords_dev *, const uint64_t *, const char *, const uint64_t *, const char **, uint64_t *) __attribute__((weak));
// entry points only --gpu-genome uses
lnr_status lnr_genome_load_gpu(const char *const *, uint32_t, int32_t, uint32_t, uint64_t, lnr_genome **) __attribute__((weak));
lnr_status lnr_genome_info(const lnr_genome *, uint32_t *, const uint64_t **, const char **, const uint64_t **, const uint8_t *const **) __attribute__((weak));
lnr_status lnr_genome_to_host(lnr_genome *, const uint8_t *const **) __attribute__((weak));
lnr_status lnr_genome_drop_dev(lnr_genome *) __attribute__((weak));
const char *lnr_genome_error(const lnr_genome *) __attribute__((weak));
void lnr_genome_free(lnr_genome *) __attribute__((weak));
lnr_status lnr_writer_set_genome_dev(lnr_writer *, const uint8_t *const *) __attribute__((weak));
}

// the device chain's calculator submits ahead through the halves of the device form unless LNR_CLI_DEV_HALVES says otherwise (README: the A/B)
static const bool DEV_HALVES_DEFAULT = true;

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Options {
    std::vector<std::string> r_paths, g_paths;
    std::string oPath, read_group, sample_name;
    unsigned gap_len = 1, apx_chain_flag = 1, reform_ccs = 0, bal_flag = 1, f_output_type = 2, f_dup = 0, sensitivity = 1, thread = 16;
    int index_t = 1, feature_t = 2, sequence_sam = 0;
    // extensions of this front-end
    unsigned gpus = 1, block_reads = 65536, index_build_each = 0, gpu_writer = 0, sam_seq = 0, gpu_reader = 0, bgzf = 0, sort = 0, gpu_gunzip = 0, gpu_genome = 0, paf = 0;
    uint64_t sort_device_mem = 0, sort_host_mem = 0;      // --sort-device-mem / --sort-host-mem in bytes
    bool has_sort_device_mem = false, has_sort_host_mem = false;
    std::vector<int> devices;
};

static bool is_number(const std::string &s) { if (s.empty()) return false; for (char c : s) if (c < '0' || c > '9') return false; return true; }

// SIZE: digits with an optional K, M or G (powers of 1024)
static bool parse_size(const std::string &s, uint64_t &out) {
    size_t n = s.size();
    unsigned shift = 0;
    if (n && (s[n - 1] == 'K' || s[n - 1] == 'M' || s[n - 1] == 'G')) { shift = s[n - 1] == 'K' ? 10 : s[n - 1] == 'M' ? 20 : 30; n--; }
    if (n == 0 || n > 18 || !is_number(s.substr(0, n))) return false;
    const uint64_t v = strtoull(s.substr(0, n).c_str(), nullptr, 10);
    if (v > (~0ULL >> shift)) return false;
    out = v << shift;
    return true;
}
// --sort: a round of the writer's sort mode begins, with the limits of --sort-device-mem / --sort-host-mem
static bool sort_round_begin(lnr_writer *wr, uint64_t device_mem, bool spill, uint64_t host_mem) {
    if (lnr_writer_sort_begin(wr, device_mem) != LNR_OK) return false;
    return !spill || lnr_writer_sort_spill(wr, host_mem) == LNR_OK;
}
// what a failed BAM call of a sorted run adds to its message
static std::string sort_hint(const Options &o, lnr_status s) {
    return o.sort && s == LNR_ERR_NOMEM ? " (--sort holds every record of a file: --sort-device-mem SIZE bounds the GPU memory, --sort-host-mem SIZE lets the rest go to pinned host memory)" : "";
}

static void usage() {
    fprintf(stderr,
            "linear filter - options and arguments.\n\nSYNOPSIS\n    linear filter [OPTIONS] read.fa/fastq(.gz)|reads.bam genome.fa(.gz)\n    linear filter [OPTIONS] reads_1 reads_2 ... x genome_1 genome_2 ...\n\n"
            "    a read file may be a BAM (aligned or unaligned; found by content): secondary / supplementary records are skipped, reverse-strand records\n"
            "    reverse-complemented, as `samtools fastq` prints them; the genome is FASTA / FASTQ only\n\n"
            "Basic options\n    -o,  --output STR          prefix of the output (default: the read file's name up to its first '.')\n"
            "    -ot, --output_type INT     1 .apf, 2 .sam {DEFAULT}, 4 .bam, 8 _pbsv.bam, or a sum of them (BAM needs --gpu-writer)\n    -t,  --thread INT          threads: the index layout of the reference's -t and the host threads of the writer {16}\n"
            "    -g,  --gap_len INT         minimal length of gaps to re-map; -g 0 off; bare -g or 1 = 50 {DEFAULT}\n    -rg, --read_group STR      @RG ID\n    -sn, --sample_name STR     @RG SM\n"
            "    -ss, --sequence_sam INT    0 {DEFAULT} (1 not built here: --sam-seq prints what the reference prints with -ss 1)\nMore options\n    -dup, --duplication INT    0 {DEFAULT} | 1\n    -b,  --bal_flag INT        1 {DEFAULT}\n"
            "    -p,  --preset INT          1 {DEFAULT} | 2   (0 not built here)\n    -i,  --index_type INT      1 {DEFAULT} | 2\n    -c,  --apx_c_flag INT      1 {DEFAULT}\n    -f,  --feature_type INT    2 {DEFAULT}\n"
            "    -r,  --reform_ccs_cigar_flag INT   0 {DEFAULT}\nMI355X front-end\n    --gpus INT                 GPUs to use {1}\n    --devices LIST             their HIP ordinals, e.g. 0,1,2,3\n"
            "    --block-reads INT          reads per block {65536}\n    --index-mode bcast|build   several GPUs: RCCL broadcast of the index {DEFAULT} or every GPU builds its own\n"
            "    --gpu-writer               format .sam / .apf text and encode .bam records on the first GPU in use instead of the writer's host threads {off}\n"
            "    --gpu-reader               parse the read files on the first GPU in use and keep the reads there: reader -> filter -> writer on device buffers {off}\n"
            "                               (one GPU; with --sam-seq it needs --gpu-writer: the read bases are not on the host)\n"
            "    --gpu-gunzip               --gpu-reader: inflate plain gzip read files (.fastq.gz / .fa.gz, not BGZF) on the GPU, in parallel from DEFLATE\n"
            "                               block starts, instead of through zlib on the host; needs --gpu-reader or --gpu-genome (then the genome\n"
            "                               files are inflated that way, too) {off}\n"
            "    --gpu-genome               load the genome files on the first GPU in use (text parsed, BGZF inflated there) and build the index from\n"
            "                               the device copy instead of parsing on one host thread and uploading {off}\n"
            "    --sam-seq                  print the SEQ column of the .sam as the reference does with -ss 1 {off}\n"
            "    --paf                      write PREFIX.paf next to the -ot outputs: one PAF line (12 columns and cg:Z:) per record of the .sam, in its\n"
            "                               order; with --bgzf PREFIX.paf.gz; not sorted by --sort {off}\n"
            "    --bgzf                     compress the text on the GPU and write PREFIX.sam.gz / PREFIX.apf.gz (BGZF); needs --gpu-writer {off}\n"
            "    --sort                     sort the .bam / _pbsv.bam by coordinate on the GPU and write PREFIX.bam.bai next to it; needs -ot with 4 or 8 and\n"
            "                               --gpu-writer; every record of a file stays in GPU memory until the file ends (about 0.8 KB per read, with\n"
            "                               --sam-seq 6 KB per 10 kb read; what does not fit goes to host memory with --sort-host-mem) {off}\n"
            "    --sort-device-mem SIZE     --sort: GPU memory the held records may take, digits with an optional K, M or G {no bound of its own}\n"
            "    --sort-host-mem SIZE       --sort: records that do not fit into GPU memory are held in pinned host memory, SIZE of it at most {off}\n");
}

// returns 0 ok, 1 error, 2 help shown
static int parse_command_line(int argc, char **argv, Options &o) {
    std::vector<std::string> a;
    for (int i = 0; i < argc; i++) {
        if (i == 1 && strcmp(argv[1], "filter") == 0) continue;                                  // args_parser.cpp:31-40
        a.push_back(argv[i]);
        std::string s = argv[i];
        if ((s == "-a" || s == "-g" || s == "-os" || s == "-oa" || s == "-r" || s == "-ss") && (i + 1 >= argc || !is_number(argv[i + 1]))) a.push_back("1");   // :42-71
    }
    if (a.size() < 3) { usage(); return 2; }                                                      // :73-77 (-h appended)
    struct Opt { const char *sh, *lg; int kind; };   // kind 0 string, 1 integer
    static const Opt table[] = {{"o", "output", 0}, {"ot", "output_type", 1}, {"t", "thread", 1}, {"g", "gap_len", 1}, {"rg", "read_group", 0}, {"sn", "sample_name", 0},
                                {"ss", "sequence_sam", 1}, {"dup", "duplication", 1}, {"b", "bal_flag", 1}, {"p", "preset", 1}, {"i", "index_type", 1}, {"c", "apx_c_flag", 1},
                                {"f", "feature_type", 1}, {"r", "reform_ccs_cigar_flag", 1}, {"gpus", "gpus", 1}, {"devices", "devices", 0}, {"blk", "block-reads", 1}, {"ix", "index-mode", 0}};
    std::vector<std::string> pos;
    for (size_t i = 1; i < a.size(); i++) {
        const std::string &s = a[i];
        if (s == "-h" || s == "--help") { usage(); return 2; }
        if (s == "--version") { fprintf(stderr, "linear filter (MI355X path) 1.8.2\n"); return 2; }
        if (s.size() < 2 || s[0] != '-' || is_number(s.substr(1))) { pos.push_back(s); continue; }
        std::string name = s.substr(s[1] == '-' ? 2 : 1), val;
        bool has_val = false;
        if (name == "gpu-writer") { o.gpu_writer = 1; continue; }                                  // a switch: takes no value
        if (name == "sam-seq") { o.sam_seq = 1; continue; }
        if (name == "gpu-reader") { o.gpu_reader = 1; continue; }
        if (name == "gpu-gunzip") { o.gpu_gunzip = 1; continue; }
        if (name == "gpu-genome") { o.gpu_genome = 1; continue; }
        if (name == "bgzf") { o.bgzf = 1; continue; }
        if (name == "sort") { o.sort = 1; continue; }
        if (name == "paf") { o.paf = 1; continue; }
        size_t eq = name.find('=');
        if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
        if (name == "sort-device-mem" || name == "sort-host-mem") {
            if (!has_val) { if (i + 1 >= a.size()) { fprintf(stderr, "linear filter: option requires an argument -- %s\n", name.c_str()); return 1; } val = a[++i]; }
            uint64_t v = 0;
            if (!parse_size(val, v)) { fprintf(stderr, "linear filter: --%s SIZE: '%s' is not digits with an optional K, M or G\n", name.c_str(), val.c_str()); return 1; }
            if (name == "sort-device-mem") { o.sort_device_mem = v; o.has_sort_device_mem = true; } else { o.sort_host_mem = v; o.has_sort_host_mem = true; }
            continue;
        }
        const Opt *op = nullptr;
        for (const Opt &t : table) if (name == t.sh || name == t.lg) op = &t;
        if (!op) { fprintf(stderr, "linear filter: illegal option -- %s\n", name.c_str()); return 1; }
        if (!has_val) { if (i + 1 >= a.size()) { fprintf(stderr, "linear filter: option requires an argument -- %s\n", name.c_str()); return 1; } val = a[++i]; }
        if (op->kind == 1 && !is_number(val)) { fprintf(stderr, "linear filter: the given value '%s' cannot be casted to integer\n", val.c_str()); return 1; }
        unsigned v = op->kind == 1 ? (unsigned)strtoul(val.c_str(), nullptr, 10) : 0;
        std::string k = op->lg;
        if (k == "output") o.oPath = val; else if (k == "output_type") o.f_output_type = v; else if (k == "thread") o.thread = v; else if (k == "gap_len") o.gap_len = v;
        else if (k == "read_group") o.read_group = val; else if (k == "sample_name") o.sample_name = val; else if (k == "sequence_sam") o.sequence_sam = (int)v;
        else if (k == "duplication") o.f_dup = v; else if (k == "bal_flag") o.bal_flag = v; else if (k == "preset") o.sensitivity = v; else if (k == "index_type") o.index_t = (int)v;
        else if (k == "apx_c_flag") o.apx_chain_flag = v; else if (k == "feature_type") o.feature_t = (int)v; else if (k == "reform_ccs_cigar_flag") o.reform_ccs = v;
        else if (k == "gpus") o.gpus = v; else if (k == "block-reads") o.block_reads = v;
        else if (k == "devices") { size_t p = 0; while (p <= val.size()) { size_t q = val.find(',', p); if (q == std::string::npos) q = val.size(); if (q > p) o.devices.push_back(atoi(val.substr(p, q - p).c_str())); p = q + 1; } }
        else if (k == "index-mode") { if (val == "build") o.index_build_each = 1; else if (val != "bcast") { fprintf(stderr, "linear filter: --index-mode bcast|build\n"); return 1; } }
    }
    if (pos.size() < 2) { fprintf(stderr, "\033[1;31mE[01]:\033[0m: Please specify the files of reads and genomes\n"); return 1; }   // :291-296
    if (pos.size() == 2) { o.r_paths.push_back(pos[0]); o.g_paths.push_back(pos[1]); }
    else {                                                                                                                        // :297-319
        bool cart = false;
        for (const std::string &p : pos) { if (p == "x") cart = true; else (cart ? o.g_paths : o.r_paths).push_back(p); }
        if (!cart) { fprintf(stderr, "\033[1;31mE[02]:\033[0mPlease add '\033[1;31mx\033[0m' between files of reads and genomes.\n"); return 1; }
    }
    return 0;
}

static std::string output_prefix_of(const std::string &path) {        // getFileName(path, "/", ~0) then getFileName(.., ".", 0) (mapper.cpp:481-482)
    size_t s = path.rfind('/');
    std::string base = s == std::string::npos ? path : path.substr(s + 1);
    size_t d = base.find('.');
    return d == std::string::npos ? base : base.substr(0, d);
}

// ---- pipeline plumbing
struct Block {
    uint8_t *bases = nullptr; uint64_t cap = 0;
    std::vector<uint64_t> off, len, id_off;
    std::vector<char> ids;
    uint32_t n = 0;
    uint64_t seq = 0;          // position in the read stream
    int file = 0;              // index of the read file it came from
    lnr_cords cords{};         // host arrays of the context's result slot (valid until the worker's second next result)
    int worker = -1;
};
template <class T> struct Queue {
    std::mutex m; std::condition_variable cv; std::deque<T> q; bool closed = false;
    void push(T v) { { std::lock_guard<std::mutex> l(m); q.push_back(v); } cv.notify_one(); }
    bool pop(T &v) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !q.empty() || closed; }); if (q.empty()) return false; v = q.front(); q.pop_front(); return true; }
    bool try_pop(T &v) { std::lock_guard<std::mutex> l(m); if (q.empty()) return false; v = q.front(); q.pop_front(); return true; }
    void close() { { std::lock_guard<std::mutex> l(m); closed = true; } cv.notify_all(); }
};
struct Shared {
    Queue<Block *> free_blocks, ready;
    std::mutex m; std::condition_variable cv;
    std::map<uint64_t, Block *> done;        // finished blocks waiting for their turn at the writer
    bool workers_done = false;
    // the gap stream (see the header of this file)
    int ext = 0; uint64_t turn = 0;
    // result-slot hand-back: per worker, the sequence numbers of the blocks whose text has been written
    std::vector<uint64_t> written_upto;      // per worker: number of its blocks the writer is through with
    std::atomic<int> failed{0};
    std::string err;
    void fail(const std::string &e) { std::lock_guard<std::mutex> l(m); if (!failed) { err = e; failed = 1; } cv.notify_all(); }
};

struct Headers { std::string sam, bam, pbsv; };      // what opens a .sam, a .bam and a _pbsv.bam (compressed where the file is)
// the output files of the printer (Mapper::p_printResults mapper.cpp:478-509): a new pair when the prefix changes, or once with -o
struct Outputs {
    FILE *fsam = nullptr, *fapf = nullptr, *fbam = nullptr, *fpbsv = nullptr, *fpaf = nullptr;
    std::string cur_prefix; bool any_open = false; int cur_file = -1;
    bool bgzf = false;                       // --bgzf: .gz names, the SAM header comes compressed, the EOF marker ends every file
    lnr_writer *sort_wr = nullptr;           // --sort: the writer that holds the records of the files in work; close() sorts and writes them
    uint64_t sort_device_mem = 0, sort_host_mem = 0; bool sort_spill = false;      // the limits every round of it begins with
    uint64_t head_bam = 0, head_pbsv = 0;    // bytes of the headers' members: where the record members start
    std::string sort_err;                    // why close() could not finish the sorted files
    // makes the files of read file `file` current; h = the headers as they go into the files.  false: the files cannot be written (err says which)
    bool turn_to(const Options &o, int file, const Headers &h, std::string &err) {
        if (file == cur_file) return true;
        cur_file = file;
        std::string prefix = o.oPath.empty() ? output_prefix_of(o.r_paths[(size_t)file]) : o.oPath;
        if (any_open && !(o.oPath.empty() && prefix != cur_prefix)) return true;
        close();
        if (!sort_err.empty()) { err = sort_err; return false; }
        bgzf = o.bgzf != 0;
        fsam = (o.f_output_type & 2) ? fopen((prefix + (bgzf ? ".sam.gz" : ".sam")).c_str(), "wb") : nullptr;
        fapf = (o.f_output_type & 1) ? fopen((prefix + (bgzf ? ".apf.gz" : ".apf")).c_str(), "wb") : nullptr;
        fbam = (o.f_output_type & 4) ? fopen((prefix + ".bam").c_str(), "wb") : nullptr;
        fpbsv = (o.f_output_type & 8) ? fopen((prefix + "_pbsv.bam").c_str(), "wb") : nullptr;
        fpaf = o.paf ? fopen((prefix + (bgzf ? ".paf.gz" : ".paf")).c_str(), "wb") : nullptr;
        if ((o.paf && !fpaf) || ((o.f_output_type & 2) && !fsam) || ((o.f_output_type & 1) && !fapf) || ((o.f_output_type & 4) && !fbam) || ((o.f_output_type & 8) && !fpbsv)) {
            err = "can't write output files with prefix " + prefix;
            return false;
        }
        if (fsam) fwrite(h.sam.data(), 1, h.sam.size(), fsam);
        if (fbam) fwrite(h.bam.data(), 1, h.bam.size(), fbam);
        if (fpbsv) fwrite(h.pbsv.data(), 1, h.pbsv.size(), fpbsv);
        cur_prefix = prefix; any_open = true;
        head_bam = h.bam.size(); head_pbsv = h.pbsv.size();
        return true;
    }
    // --sort: the kept records of the files in work, sorted: their members into both files; after the EOF markers the indexes; a new round begins
    bool sorted_records() {
        const char *d; uint64_t z;
        if (lnr_writer_sort_finish(sort_wr, 0, nullptr) != LNR_OK) return false;
        for (;;) {
            if (lnr_writer_sort_next(sort_wr, &d, &z) != LNR_OK) return false;
            if (!z) return true;
            if ((fbam && fwrite(d, 1, z, fbam) != z) || (fpbsv && fwrite(d, 1, z, fpbsv) != z)) { sort_err = "write error (.bam)"; return false; }
        }
    }
    bool sorted_index(const std::string &path, uint64_t head) {
        const char *d; uint64_t z;
        if (lnr_writer_sort_bai(sort_wr, head, &d, &z) != LNR_OK) return false;
        FILE *f = fopen(path.c_str(), "wb");
        const bool ok = f && fwrite(d, 1, z, f) == z;
        if (f) fclose(f);
        if (!ok) sort_err = "can't write " + path;
        return ok;
    }
    void close() {
        const bool sorting = sort_wr && (fbam || fpbsv);
        const bool had_bam = fbam != nullptr, had_pbsv = fpbsv != nullptr;
        bool sorted = sorting && sorted_records();
        close_files();
        if (sorted) sorted = (!had_bam || sorted_index(cur_prefix + ".bam.bai", head_bam)) && (!had_pbsv || sorted_index(cur_prefix + "_pbsv.bam.bai", head_pbsv));
        if (sorting) {
            if (!sorted && sort_err.empty()) sort_err = std::string("--sort: ") + lnr_writer_error(sort_wr);
            lnr_writer_sort_end(sort_wr);
            if (!sort_round_begin(sort_wr, sort_device_mem, sort_spill, sort_host_mem) && sort_err.empty()) sort_err = std::string("--sort: ") + lnr_writer_error(sort_wr);      // the next file's round
        }
    }
    void close_files() {
        const char *eof = nullptr; uint64_t n = 0;
        if (bgzf && (fsam || fapf || fpaf)) lnr_writer_bgzf_eof(&eof, &n);
        if (fsam) { if (n) fwrite(eof, 1, n, fsam); fclose(fsam); }
        if (fapf) { if (n) fwrite(eof, 1, n, fapf); fclose(fapf); }
        if (fpaf) { if (n) fwrite(eof, 1, n, fpaf); fclose(fpaf); }
        if (fbam || fpbsv) lnr_writer_bgzf_eof(&eof, &n);                                // a .bam is BGZF whatever --bgzf says
        if (fbam) { fwrite(eof, 1, n, fbam); fclose(fbam); }
        if (fpbsv) { fwrite(eof, 1, n, fpbsv); fclose(fpbsv); }
        fsam = fapf = fbam = fpbsv = fpaf = nullptr;
    }
};

int main(int argc, char **argv) {
    double t_start = now();
    Options o;
    int pr = parse_command_line(argc, argv, o);
    if (pr) return pr == 2 ? 0 : 1;
    fprintf(stderr, "Linear: Extensible Long-read Algorithms Framework (MI355X filter path)\n");
    for (const std::string &p : o.r_paths) if (access(p.c_str(), F_OK) == -1) { fprintf(stderr, "\033[1;31mE[05]:\033[0mCan't open file %s\n", p.c_str()); return 1; }
    for (const std::string &p : o.g_paths) if (access(p.c_str(), F_OK) == -1) { fprintf(stderr, "\033[1;31mE[06]:\033[0mCan't open file %s\n", p.c_str()); return 1; }
    // what the MI355X path does not build: say so instead of writing something else
    const char *nb = nullptr;
    if (!(o.f_output_type & 15)) nb = "-ot without 1 (.apf), 2 (.sam), 4 (.bam) or 8 (_pbsv.bam)";
    else if (o.sequence_sam) nb = "-ss 1 (read sequences in the SAM)"; else if (!o.apx_chain_flag) nb = "-c 0"; else if (o.feature_t != 2) nb = "-f other than 2";
    else if (o.reform_ccs) nb = "-r 1"; else if (o.sensitivity != 1 && o.sensitivity != 2) nb = "-p other than 1 or 2"; else if (!o.bal_flag) nb = "-b 0 (the reference's -b 0 path writes a header-only SAM)";
    else if (o.index_t != 1 && o.index_t != 2) nb = "-i other than 1 or 2";
    if (nb) { fprintf(stderr, "\033[1;31mE[m02G]:\033[0m %s is not built in the MI355X filter path\n", nb); return 1; }
    if (!o.sort && (o.has_sort_device_mem || o.has_sort_host_mem)) {
        fprintf(stderr, "\033[1;31mE:\033[0m %s bounds what --sort holds: it needs --sort\n", o.has_sort_device_mem ? "--sort-device-mem" : "--sort-host-mem");
        return 1;
    }
    if (o.sort && !o.gpu_writer) { fprintf(stderr, "\033[1;31mE:\033[0m --sort sorts the BAM records on the GPU that encodes them: it needs --gpu-writer\n"); return 1; }
    if (o.sort && !(o.f_output_type & 12)) { fprintf(stderr, "\033[1;31mE:\033[0m --sort sorts BAM output: it needs -ot with 4 (.bam) or 8 (_pbsv.bam)\n"); return 1; }
    if (o.sort && (!lnr_writer_sort_begin || !lnr_writer_sort_finish || !lnr_writer_sort_next || !lnr_writer_sort_bai || !lnr_writer_sort_end)) {
        fprintf(stderr, "\033[1;31mE:\033[0m --sort: this library has no sort mode of the writer\n");
        return 1;
    }
    if (o.has_sort_host_mem && !lnr_writer_sort_spill) { fprintf(stderr, "\033[1;31mE:\033[0m --sort-host-mem: this library has no host tier in the sort mode of the writer\n"); return 1; }
    if ((o.f_output_type & 12) && !o.gpu_writer) {
        fprintf(stderr, "\033[1;31mE:\033[0m -ot 4 / 8 (BAM output) is encoded and compressed on the GPU: it needs --gpu-writer (BAM on the writer's host threads is not built)\n");
        return 1;
    }
    if (o.gpu_gunzip && !o.gpu_reader && !o.gpu_genome) { fprintf(stderr, "\033[1;31mE:\033[0m --gpu-gunzip inflates files on the GPU that parses them: it needs --gpu-reader or --gpu-genome\n"); return 1; }
    if (o.gpu_genome && (!lnr_genome_load_gpu || !lnr_genome_info || !lnr_genome_to_host || !lnr_genome_drop_dev || !lnr_genome_error || !lnr_genome_free || !lnr_writer_set_genome_dev)) {
        fprintf(stderr, "\033[1;31mE:\033[0m --gpu-genome: this library has no genome loader on the GPU\n");
        return 1;
    }
    if (o.paf && (!lnr_writer_format_paf || !lnr_writer_format_paf_gpu || !lnr_writer_format_paf_dev)) {
        fprintf(stderr, "\033[1;31mE:\033[0m --paf: this library has no PAF form of the writer\n");
        return 1;
    }
    if (o.bgzf && !o.gpu_writer) { fprintf(stderr, "\033[1;31mE:\033[0m --bgzf compresses the text on the GPU that formats it: it needs --gpu-writer\n"); return 1; }
    if (o.thread < 1) o.thread = 1;
    if (o.gpus < 1) o.gpus = 1;
    if (o.block_reads < 1) o.block_reads = 1;
    if (o.devices.empty()) for (unsigned g = 0; g < o.gpus; g++) o.devices.push_back((int)g);
    o.gpus = (unsigned)o.devices.size();

    // ---- genomes (loadRecords over every genome file, ids cut at the first blank: base.cpp:188-195)
    // --gpu-genome: the files go to the first GPU and are parsed there (lnr_genome_load_gpu); the index is built from the device copy
    std::vector<std::vector<uint8_t> > genome;
    std::vector<std::string> gid;
    std::vector<const uint8_t *> gp; std::vector<uint64_t> gl;      // what lnr_index_build takes: host pointers, or the device pointers of gg
    lnr_genome *gg = nullptr;
    const double t_genome0 = now();
    if (o.gpu_genome) {
        std::vector<const char *> paths;
        for (const std::string &gpath : o.g_paths) paths.push_back(gpath.c_str());
        const lnr_status s = lnr_genome_load_gpu(paths.data(), (uint32_t)paths.size(), o.devices[0], o.gpu_gunzip ? LNR_GENOME_GPU_GZIP : 0u, 0, &gg);
        if (s != LNR_OK) {
            fprintf(stderr, "\033[1;31mE:\033[0m --gpu-genome: %s%s\n", lnr_genome_error(nullptr),
                    s == LNR_ERR_LIMIT ? " -- the genome can be loaded without --gpu-genome" : "");
            return 1;
        }
        uint32_t nseq = 0; const uint64_t *len = nullptr, *io = nullptr; const char *ids = nullptr; const uint8_t *const *d_seq = nullptr;
        lnr_genome_info(gg, &nseq, &len, &ids, &io, &d_seq);
        for (uint32_t i = 0; i < nseq; i++) {
            std::string id(ids + io[i]);
            gid.push_back(id.substr(0, id.find(' ')));
            gp.push_back(d_seq[i]); gl.push_back(len[i]);
        }
    } else {
        std::vector<uint8_t> buf((size_t)1 << 30);
        std::vector<uint64_t> off(2);
        for (const std::string &gpath : o.g_paths) {
            lnr_reader *gr = nullptr;
            if (lnr_reader_open(gpath.c_str(), &gr) != LNR_OK) { fprintf(stderr, "\033[1;31mE[06]:\033[0mCan't open file %s\n", gpath.c_str()); return 1; }
            if (lnr_reader_format && lnr_reader_format(gr) == 3) { fprintf(stderr, "\033[1;31mE:\033[0m genome %s is a BAM file: a genome is read from FASTA / FASTQ only\n", gpath.c_str()); return 1; }
            for (;;) {
                uint32_t n = 0;
                if (lnr_reader_next(gr, buf.data(), buf.size(), off.data(), 1, &n) != LNR_OK) { fprintf(stderr, "E: genome %s: %s\n", gpath.c_str(), lnr_reader_error(gr)); return 1; }
                if (!n) break;
                genome.emplace_back(buf.begin(), buf.begin() + (long)off[1]);
                const char *ids; const uint64_t *io;
                lnr_reader_ids(gr, &ids, &io);
                std::string id(ids);
                gid.push_back(id.substr(0, id.find(' ')));
            }
            lnr_reader_close(gr);
        }
        for (const std::vector<uint8_t> &g : genome) { gp.push_back(g.data()); gl.push_back(g.size()); }
    }
    const double t_genome = now() - t_genome0;
    if (gp.size() >= 1024) { fprintf(stderr, "\033[1;31mE[m01G]:\033[0m Too many reference genoemes <=1024\n"); return 1; }   // linear.cpp:107-113
    if (gp.empty()) { fprintf(stderr, "E: no reference sequence in the genome files\n"); return 1; }

    // ---- contexts (one per GPU) + index
    const unsigned G = o.gpus;
    std::vector<lnr_ctx *> ctx(G, nullptr);
    for (unsigned g = 0; g < G; g++) {
        lnr_opts lo;
        lnr_opts_default(&lo);
        lo.device = o.devices[g]; lo.index_type = (uint32_t)o.index_t; lo.preset = o.sensitivity; lo.gap_len = o.gap_len; lo.dup = o.f_dup ? 1 : 0;
        lnr_status s = lnr_create(&lo, &ctx[g]);
        if (s != LNR_OK) { fprintf(stderr, "E: GPU %d: %s\n", o.devices[g], lnr_strerror(s)); return 1; }
    }
    std::vector<const char *> gn;
    for (const std::string &id : gid) gn.push_back(id.c_str());
    // --gpu-genome: the host copy of the genome (one download, owned by gg), for what cannot take the device pointers
    const uint8_t *const *g_host = nullptr;
    auto genome_on_host = [&]() -> const uint8_t *const * {
        if (!gg) return gp.data();
        if (!g_host && lnr_genome_to_host(gg, &g_host) != LNR_OK) { fprintf(stderr, "\033[1;31mE:\033[0m --gpu-genome: %s\n", lnr_genome_error(gg)); exit(1); }
        return g_host;
    };
    {
        double t0 = now();
        lnr_status s = lnr_index_build(ctx[0], gp.data(), gl.data(), (uint32_t)gp.size(), o.thread);
        if (s != LNR_OK) { fprintf(stderr, "E: index: %s (%s)\n", lnr_strerror(s), lnr_last_error(ctx[0])); return 1; }
        double t_build = now() - t0;
        if (G > 1) {
            t0 = now();
            if (o.index_build_each) {
                const uint8_t *const *hp = genome_on_host();          // (another GPU cannot read the first one's copy without peer access)
                std::vector<std::thread> th; std::vector<lnr_status> st(G, LNR_OK);
                for (unsigned g = 1; g < G; g++) th.emplace_back([&, g] { st[g] = lnr_index_build(ctx[g], hp, gl.data(), (uint32_t)gp.size(), o.thread); });
                for (auto &t : th) t.join();
                for (unsigned g = 1; g < G; g++) if (st[g] != LNR_OK) { fprintf(stderr, "E: index on GPU %d: %s (%s)\n", o.devices[g], lnr_strerror(st[g]), lnr_last_error(ctx[g])); return 1; }
                fprintf(stderr, "  Index on %u more GPUs: every GPU built its own in %.3f s (the first took %.3f s)\n", G - 1, now() - t0, t_build);
            } else {
                double sec = 0;
                lnr_status sb = lnr_index_broadcast(ctx.data(), G, 0, &sec);
                if (sb != LNR_OK) { fprintf(stderr, "E: index broadcast: %s (%s)\n", lnr_strerror(sb), lnr_last_error(ctx[0])); return 1; }
                fprintf(stderr, "  Index on %u more GPUs: RCCL broadcast + derived tables in %.3f s (building it took %.3f s; --index-mode build lets every GPU build its own)\n", G - 1, sec, t_build);
            }
        }
        fprintf(stderr, "  Genome loaded in %.3f s (%s), index built in %.3f s\n", t_genome, o.gpu_genome ? "--gpu-genome: parsed on the GPU" : "host reader, one record at a time", t_build);
        fprintf(stderr, "  End creating index Elapsed time[s] %.2f\n", now() - t_start);
    }
    lnr_writer *wr = nullptr;
    if (lnr_writer_create(gn.data(), gl.data(), (uint32_t)gn.size(), &wr) != LNR_OK) { fprintf(stderr, "E: writer\n"); return 1; }
    lnr_writer_set_preset(wr, o.sensitivity);
    lnr_writer_set_read_group(wr, o.read_group.c_str(), o.sample_name.c_str());
    if (o.sam_seq && !(gg && o.gpu_writer)) lnr_writer_set_genome(wr, genome_on_host());         // (the genome vectors / gg's host copy outlive the writer)
    if (o.gpu_writer && lnr_writer_gpu_open(wr, o.devices[0]) != LNR_OK) {                       // before any output file is opened
        fprintf(stderr, "\033[1;31mE:\033[0m --gpu-writer: %s\n", lnr_writer_error(wr));
        lnr_writer_destroy(wr);
        for (auto *c : ctx) lnr_destroy(c);
        return 1;
    }
    if (gg) {
        // the GPU writer takes its copy device to device; then the index and the writer hold their own: the loader's copy goes
        if (o.sam_seq && o.gpu_writer && lnr_writer_set_genome_dev(wr, gp.data()) != LNR_OK) {
            fprintf(stderr, "\033[1;31mE:\033[0m --gpu-genome: %s\n", lnr_writer_error(wr));
            lnr_writer_destroy(wr);
            for (auto *c : ctx) lnr_destroy(c);
            return 1;
        }
        lnr_genome_drop_dev(gg);
        gp.clear();                                            // (device addresses that are gone)
    }
    // --bgzf: the SAM header goes through the writer's device as well, the BAM headers always; false with a message when that fails
    const bool want_bam = (o.f_output_type & 12) != 0;
    auto header_of = [&](Headers &h) {
        const char *t; uint64_t z;
        lnr_writer_sam_header(wr, "", &t, &z);
        h.sam.assign(t, z);
        if (o.bgzf) {
            const std::string plain = h.sam;
            if (lnr_writer_bgzf_bytes_gpu(wr, plain.data(), plain.size(), &t, &z) != LNR_OK) return false;
            h.sam.assign(t, z);
        }
        for (int pbsv = 0; pbsv < 2; pbsv++) {
            if (!(o.f_output_type & (pbsv ? 8u : 4u))) continue;
            lnr_writer_bam_header(wr, "", pbsv, &t, &z);
            const std::string plain(t, z);
            if (lnr_writer_bgzf_bytes_gpu(wr, plain.data(), plain.size(), &t, &z) != LNR_OK) return false;
            (pbsv ? h.pbsv : h.bam).assign(t, z);
        }
        return true;
    };
    // the BAM records of a block come compressed whatever --bgzf says: the switch is on for that call alone
    auto bam_call = [&](auto &&call) {
        lnr_status s = lnr_writer_set_bgzf(wr, 1);                // (a failure here must not let raw record bytes into the file)
        if (s == LNR_OK) s = call();
        const lnr_status back = lnr_writer_set_bgzf(wr, o.bgzf ? 1 : 0);
        return s != LNR_OK ? s : back;
    };
    if (o.bgzf && lnr_writer_set_bgzf(wr, 1) != LNR_OK) {
        fprintf(stderr, "\033[1;31mE:\033[0m --bgzf: %s\n", lnr_writer_error(wr));
        lnr_writer_destroy(wr);
        for (auto *c : ctx) lnr_destroy(c);
        return 1;
    }
    // --sort: the mode is on before the headers are made (they carry @HD SO:coordinate); Outputs::close ends a file's round and begins the next
    if (o.sort && !sort_round_begin(wr, o.sort_device_mem, o.has_sort_host_mem, o.sort_host_mem)) {
        fprintf(stderr, "\033[1;31mE:\033[0m --sort: %s\n", lnr_writer_error(wr));
        lnr_writer_destroy(wr);
        for (auto *c : ctx) lnr_destroy(c);
        return 1;
    }
    if (o.gpu_reader) {                                                                          // before any output file is opened, too
        std::string why;
        if (!lnr_filter_batch_dev || !lnr_cords_to_host || !lnr_writer_format_dev || !lnr_writer_format_seq_dev || !lnr_writer_format_bam_dev || !lnr_reader_gpu_open || !lnr_reader_next_dev)
            why = "no usable device: this library has no device form of the filter";
        else if (o.gpu_gunzip && !lnr_reader_gpu_gzip) why = "--gpu-gunzip: this library has no device inflate of plain gzip";
        else if (G != 1) why = "the device chain runs on one GPU (--gpus 1)";
        else if (o.sam_seq && !o.gpu_writer) why = "with --sam-seq the reads stay on the device: add --gpu-writer";
        else {
            lnr_reader *probe = nullptr;
            if (lnr_reader_open(o.r_paths[0].c_str(), &probe) != LNR_OK) why = "can't open read file " + o.r_paths[0];
            else { if (lnr_reader_gpu_open(probe, o.devices[0], 3) != LNR_OK) why = lnr_reader_error(probe); lnr_reader_close(probe); }
        }
        if (!why.empty()) {
            fprintf(stderr, "\033[1;31mE:\033[0m --gpu-reader: %s\n", why.c_str());
            lnr_writer_destroy(wr);
            for (auto *c : ctx) lnr_destroy(c);
            return 1;
        }
        // reader thread -> calculator -> writer thread over the reader's device blocks
        struct DBlock {
            const uint8_t *d_reads = nullptr; const uint64_t *d_off = nullptr;
            std::vector<uint64_t> off, len, id_off, coff, cs, ce;
            std::vector<char> ids;
            std::string sam, apf, bam, paf;
            uint32_t n = 0; int file = 0;
        };
        Queue<DBlock *> freeq, readyq, doneq;
        std::mutex em; std::string err; std::atomic<int> failed{0};
        auto fail = [&](const std::string &e) { { std::lock_guard<std::mutex> l(em); if (!failed) { err = e; failed = 1; } } freeq.close(); readyq.close(); doneq.close(); };
        Headers sam_header;                                      // (taken here: the calculator thread is the writer's only user under --gpu-writer)
        if (!header_of(sam_header)) {
            fprintf(stderr, "\033[1;31mE:\033[0m %s: %s\n", want_bam ? "BAM / BGZF header" : "--bgzf", lnr_writer_error(wr));
            lnr_writer_destroy(wr);
            for (auto *c : ctx) lnr_destroy(c);
            return 1;
        }
        // The halves of the device form (lnr_filter_submit_dev / _wait_dev) let the calculator submit ahead; LNR_CLI_DEV_HALVES=0|1 in the
        // environment chooses between that and one lnr_filter_batch_dev at a time (an A/B switch, not an option).
        // Blocks: one being read, up to three in the context, one whose text is being made or written -- five; three for the old loop (one
        // being read, one in the context, one being written).  The reader's device blocks are as many: a block goes back to the reader only
        // after its batch's wait has returned and its text has been written.
        bool halves = lnr_filter_submit_dev && lnr_filter_wait_dev && DEV_HALVES_DEFAULT;
        if (const char *e = getenv("LNR_CLI_DEV_HALVES")) halves = lnr_filter_submit_dev && lnr_filter_wait_dev && atoi(e) != 0;
        const unsigned NDB = halves ? 5 : 3;
        std::vector<DBlock> dblocks(NDB);
        for (auto &b : dblocks) freeq.push(&b);
        // --sort with one output per read file: the writer thread ends a file's sort round (lnr_writer_sort_finish .. _begin on `wr`) while this
        // thread would add the next file's records to it.  A fence block (n == 0) goes through the queue in front of the first block of a new
        // output; the calculator waits until the writer thread has turned to the new files.
        DBlock fence; std::mutex fm; std::condition_variable fcv; uint64_t fences_passed = 0, fences_sent = 0;
        std::string calc_prefix; bool calc_has_prefix = false;
        uint64_t cap = (uint64_t)o.block_reads * 12000 + (1u << 20);
        if (cap > ((uint64_t)3 << 30)) cap = (uint64_t)3 << 30;
        lnr_reader *cur = nullptr;                               // the reader of the file in work: its device blocks live until the file's last block is written
        std::atomic<uint64_t> total_reads{0}, us_reader{0}, us_gpu{0}, us_writer{0};
        const double t_reads0 = now();
        std::thread reader([&] {
            for (size_t f = 0; f < o.r_paths.size() && !failed; f++) {
                if (lnr_reader_open(o.r_paths[f].c_str(), &cur) != LNR_OK) { cur = nullptr; fail("can't open read file " + o.r_paths[f]); break; }
                if (lnr_reader_gpu_open(cur, o.devices[0], NDB) != LNR_OK) { fail(std::string("--gpu-reader: ") + lnr_reader_error(cur)); break; }
                if (o.gpu_gunzip && lnr_reader_gpu_gzip(cur, 1) != LNR_OK) { fail(std::string("--gpu-gunzip: ") + lnr_reader_error(cur)); break; }
                for (;;) {
                    DBlock *b = nullptr;
                    if (!freeq.pop(b) || failed) break;
                    const uint64_t *ho = nullptr;
                    double tr0 = now();
                    lnr_status rs_ = lnr_reader_next_dev(cur, cap, o.block_reads, &b->d_reads, &b->d_off, &ho, &b->n);
                    us_reader += (uint64_t)((now() - tr0) * 1e6);
                    if (rs_ != LNR_OK) { fail(std::string("reads: ") + lnr_reader_error(cur)); break; }
                    if (!b->n) { freeq.push(b); break; }
                    const char *ids; const uint64_t *io;
                    lnr_reader_ids(cur, &ids, &io);
                    b->off.assign(ho, ho + b->n + 1);
                    b->id_off.assign(io, io + b->n + 1);
                    b->ids.assign(ids, ids + io[b->n]);
                    b->len.resize(b->n);
                    for (uint32_t i = 0; i < b->n; i++) b->len[i] = b->off[i + 1] - b->off[i];
                    b->file = (int)f;
                    readyq.push(b);
                }
                // the file is read: once its blocks are back the reader goes, with its device blocks and staging buffers
                std::vector<DBlock *> back(NDB); size_t nb = 0;
                while (nb < NDB && !failed && freeq.pop(back[nb])) nb++;
                if (nb < NDB) break;
                lnr_reader_close(cur); cur = nullptr;
                for (DBlock *b : back) freeq.push(b);
            }
            readyq.close();
        });
        // (calculator thread) --sort with one output per read file: before the first block of a new output goes to the writer `wr`, the fence.
        // False: the run has failed.
        auto pass_fence = [&](DBlock *b) {
            if (!(o.sort && o.oPath.empty())) return true;
            const std::string prefix = output_prefix_of(o.r_paths[(size_t)b->file]);
            if (calc_has_prefix && prefix != calc_prefix) {
                fence.n = 0; fence.file = b->file;
                fences_sent++;
                doneq.push(&fence);
                std::unique_lock<std::mutex> l(fm);
                while (fences_passed != fences_sent && !failed) fcv.wait_for(l, std::chrono::milliseconds(50));      // (a failure elsewhere does not signal here)
                if (failed) return false;
            }
            calc_prefix = prefix; calc_has_prefix = true;
            return true;
        };
        auto needs_fence = [&](const DBlock *b) { return o.sort && o.oPath.empty() && calc_has_prefix && output_prefix_of(o.r_paths[(size_t)b->file]) != calc_prefix; };
        // (calculator thread, --gpu-writer) the text of block b from its device buffers and its cords `dev`
        auto text_of = [&](DBlock *b, const lnr_cords_dev &dev) {
            const char *text; uint64_t size;
            lnr_status s;
            b->sam.clear(); b->apf.clear(); b->bam.clear(); b->paf.clear();
            if (o.f_output_type & 2) {
                s = o.sam_seq ? lnr_writer_format_seq_dev(wr, &dev, b->d_reads, b->d_off, b->ids.data(), b->id_off.data(), &text, &size)
                              : lnr_writer_format_dev(wr, &dev, b->d_off, b->ids.data(), b->id_off.data(), 1, &text, &size);
                if (s != LNR_OK) { fail(std::string("writer (.sam): ") + lnr_writer_error(wr)); return false; }
                b->sam.assign(text, size);
            }
            if (o.f_output_type & 1) {
                s = lnr_writer_format_dev(wr, &dev, b->d_off, b->ids.data(), b->id_off.data(), 2, &text, &size);
                if (s != LNR_OK) { fail(std::string("writer (.apf): ") + lnr_writer_error(wr)); return false; }
                b->apf.assign(text, size);
            }
            if (o.paf) {
                s = lnr_writer_format_paf_dev(wr, &dev, b->d_off, b->ids.data(), b->id_off.data(), &text, &size);
                if (s != LNR_OK) { fail(std::string("writer (.paf): ") + lnr_writer_error(wr)); return false; }
                b->paf.assign(text, size);
            }
            if (want_bam) {
                s = bam_call([&] { return lnr_writer_format_bam_dev(wr, &dev, o.sam_seq ? b->d_reads : nullptr, b->d_off, b->ids.data(), b->id_off.data(), &text, &size); });
                if (s != LNR_OK) { fail(std::string("writer (.bam): ") + lnr_writer_error(wr) + sort_hint(o, s)); return false; }
                b->bam.assign(text, size);
            }
            return true;
        };
        auto keep_cords = [](DBlock *b, const lnr_cords &c) {
            b->coff.assign(c.cord_off, c.cord_off + c.n_reads + 1);
            b->cs.assign(c.cords_str, c.cords_str + c.n_cords);
            b->ce.assign(c.cords_end, c.cords_end + c.n_cords);
        };
        std::thread calc([&] {
            DBlock *b = nullptr;
            if (halves) {
                // submit(0); submit(1); loop { submit(k + 2); wait(k); text of k }: the lanes compute blocks k + 1 and k + 2 while this thread makes
                // the text of block k.  A block that would need a fence is held back until everything before it has gone to the writer thread.
                std::deque<DBlock *> fl;             // submitted, not handed out yet
                DBlock *held = nullptr;
                bool eof = false;
                while (!failed) {
                    while (!eof && !held && fl.size() < 3) {
                        DBlock *nb = nullptr;
                        if (fl.empty()) { if (!readyq.pop(nb)) { eof = true; break; } }
                        else if (!readyq.try_pop(nb)) break;
                        if (needs_fence(nb)) { held = nb; break; }
                        if (!pass_fence(nb)) break;        // (no fence here: it notes the output the block belongs to)
                        lnr_status s = lnr_filter_submit_dev(ctx[0], nb->d_reads, nb->d_off, nb->off.data(), nb->n);
                        if (s != LNR_OK) { fail(std::string("filter: ") + lnr_strerror(s) + " (" + lnr_last_error(ctx[0]) + ")"); break; }
                        fl.push_back(nb);
                    }
                    if (failed) break;
                    if (fl.empty()) {
                        if (!held) { if (eof) break; continue; }
                        if (!pass_fence(held)) break;      // the pipeline is drained: the fence goes out, then the held block starts the new output
                        lnr_status s = lnr_filter_submit_dev(ctx[0], held->d_reads, held->d_off, held->off.data(), held->n);
                        if (s != LNR_OK) { fail(std::string("filter: ") + lnr_strerror(s) + " (" + lnr_last_error(ctx[0]) + ")"); break; }
                        fl.push_back(held); held = nullptr;
                        continue;
                    }
                    b = fl.front(); fl.pop_front();
                    double tg0 = now();
                    if (o.gpu_writer) {
                        lnr_cords_dev dev{};
                        lnr_status s = lnr_filter_wait_dev(ctx[0], &dev);
                        if (s != LNR_OK) { fail(std::string("filter: ") + lnr_strerror(s) + " (" + lnr_last_error(ctx[0]) + ")"); break; }
                        if (!text_of(b, dev)) break;
                    } else {
                        lnr_cords c{};
                        lnr_status s = lnr_filter_wait(ctx[0], &c);
                        if (s != LNR_OK) { fail(std::string("filter: ") + lnr_strerror(s) + " (" + lnr_last_error(ctx[0]) + ")"); break; }
                        keep_cords(b, c);
                    }
                    us_gpu += (uint64_t)((now() - tg0) * 1e6);
                    doneq.push(b);
                }
                // (after a failure: the lanes still read the device blocks of what is in flight, and the reader frees them next)
                for (size_t k = fl.size(); k--;) { lnr_cords_dev d{}; (void)lnr_filter_wait_dev(ctx[0], &d); }
                doneq.close();
                return;
            }
            while (readyq.pop(b) && !failed) {
                double tg0 = now();
                lnr_cords_dev dev{};
                lnr_status s = lnr_filter_batch_dev(ctx[0], b->d_reads, b->d_off, b->n, &dev);
                if (s != LNR_OK) { fail(std::string("filter: ") + lnr_strerror(s) + " (" + lnr_last_error(ctx[0]) + ")"); break; }
                if (!pass_fence(b)) break;
                if (o.gpu_writer) {                                  // the text of the block, from the device buffers
                    if (!text_of(b, dev)) break;
                } else {
                    lnr_cords c{};
                    s = lnr_cords_to_host(ctx[0], &c);
                    if (s != LNR_OK) { fail(std::string("cords: ") + lnr_last_error(ctx[0])); break; }
                    keep_cords(b, c);
                }
                us_gpu += (uint64_t)((now() - tg0) * 1e6);
                doneq.push(b);
            }
            doneq.close();
        });
        std::thread writer([&] {
            Outputs out;
            FILE *&fsam = out.fsam, *&fapf = out.fapf;
            const char *text; uint64_t size;
            DBlock *b = nullptr;
            if (o.sort) { out.sort_wr = wr; out.sort_device_mem = o.sort_device_mem; out.sort_host_mem = o.sort_host_mem; out.sort_spill = o.has_sort_host_mem; }
            while (doneq.pop(b) && !failed) {
                std::string oe;
                if (!out.turn_to(o, b->file, sam_header, oe)) { fail(oe); fcv.notify_all(); break; }
                if (!b->n) { { std::lock_guard<std::mutex> l(fm); fences_passed++; } fcv.notify_all(); continue; }      // a fence: the files are turned
                double tw0 = now();
                bool ok = true;
                if (o.gpu_writer) {
                    if (fsam) ok = fwrite(b->sam.data(), 1, b->sam.size(), fsam) == b->sam.size();
                    if (ok && fapf) ok = fwrite(b->apf.data(), 1, b->apf.size(), fapf) == b->apf.size();
                    if (ok && out.fpaf) ok = fwrite(b->paf.data(), 1, b->paf.size(), out.fpaf) == b->paf.size();
                    if (ok && out.fbam) ok = fwrite(b->bam.data(), 1, b->bam.size(), out.fbam) == b->bam.size();
                    if (ok && out.fpbsv) ok = fwrite(b->bam.data(), 1, b->bam.size(), out.fpbsv) == b->bam.size();
                    if (!ok) { fail("write error"); break; }
                } else {
                    lnr_cords c{b->n, (uint64_t)b->cs.size(), b->coff.data(), b->cs.data(), b->ce.data()};
                    if (fsam) { if (lnr_writer_format(wr, &c, b->len.data(), b->ids.data(), b->id_off.data(), 1, o.thread, &text, &size) != LNR_OK) { fail(std::string("writer (.sam): ") + lnr_writer_error(wr)); break; } if (fwrite(text, 1, size, fsam) != size) { fail("write error (.sam)"); break; } }
                    if (fapf) { if (lnr_writer_format(wr, &c, b->len.data(), b->ids.data(), b->id_off.data(), 2, o.thread, &text, &size) != LNR_OK) { fail(std::string("writer (.apf): ") + lnr_writer_error(wr)); break; } if (fwrite(text, 1, size, fapf) != size) { fail("write error (.apf)"); break; } }
                    if (out.fpaf) { if (lnr_writer_format_paf(wr, &c, b->len.data(), b->ids.data(), b->id_off.data(), o.thread, &text, &size) != LNR_OK) { fail(std::string("writer (.paf): ") + lnr_writer_error(wr)); break; } if (fwrite(text, 1, size, out.fpaf) != size) { fail("write error (.paf)"); break; } }
                }
                us_writer += (uint64_t)((now() - tw0) * 1e6);
                total_reads += b->n;
                freeq.push(b);
            }
            if (failed) out.sort_wr = nullptr;                       // (the calculator may still be at the writer: nothing is sorted after a failure)
            out.close();
            if (!out.sort_err.empty()) fail(out.sort_err);
            fcv.notify_all();
        });
        calc.join();
        writer.join();
        freeq.close();
        reader.join();
        if (cur) lnr_reader_close(cur);
        lnr_writer_destroy(wr);
        for (auto *c : ctx) lnr_destroy(c);
        if (gg) lnr_genome_free(gg);
        if (failed) { fprintf(stderr, "\033[1;31mE:\033[0m %s\n", err.c_str()); return 1; }
        const double t_reads = now() - t_reads0;
        fprintf(stderr, "  Processed: %llu reads on 1 GPU (device chain); read files in -> output files out: %.3f s = %.0f reads/s\n", (unsigned long long)total_reads.load(), t_reads,
                total_reads.load() / (t_reads > 0 ? t_reads : 1));
        fprintf(stderr, "  Stage busy time[s]: reader %.3f, GPU (kernels%s) %.3f, writer %.3f\n", us_reader.load() / 1e6, o.gpu_writer ? " + text" : " + download", us_gpu.load() / 1e6, us_writer.load() / 1e6);
        fprintf(stderr, "Time in sum[s] %.2f      \n", now() - t_start);
        return 0;
    }

    // ---- the pipeline
    Shared sh;
    sh.written_upto.assign(G, 0);
    const unsigned NB = 4 * G + 2;
    std::vector<Block> blocks(NB);
    for (auto &b : blocks) {
        b.cap = (uint64_t)o.block_reads * 12000 + (1u << 20);
        if (b.cap > ((uint64_t)3 << 30)) b.cap = (uint64_t)3 << 30;
        b.bases = (uint8_t *)lnr_host_alloc(b.cap);
        b.off.resize((size_t)o.block_reads + 1);
        if (!b.bases) { fprintf(stderr, "E: pinned host allocation of %llu bytes failed\n", (unsigned long long)b.cap); return 1; }
        sh.free_blocks.push(&b);
    }
    std::atomic<uint64_t> total_reads{0};
    std::atomic<uint64_t> us_reader{0}, us_gpu{0}, us_writer{0};        // busy time of the three stages (microseconds), printed at the end
    const double t_reads0 = now();
    // reader: the one fetcher (parallel_io.cpp:433-485)
    std::thread reader([&] {
        uint64_t seq = 0;
        for (size_t f = 0; f < o.r_paths.size() && !sh.failed; f++) {
            lnr_reader *rr = nullptr;
            if (lnr_reader_open(o.r_paths[f].c_str(), &rr) != LNR_OK) { sh.fail("can't open read file " + o.r_paths[f]); break; }
            for (;;) {
                Block *b = nullptr;
                if (!sh.free_blocks.pop(b) || sh.failed) break;
                double tr0 = now();
                lnr_status rs_ = lnr_reader_next(rr, b->bases, b->cap, b->off.data(), o.block_reads, &b->n);
                us_reader += (uint64_t)((now() - tr0) * 1e6);
                if (rs_ != LNR_OK) { sh.fail(std::string("reads: ") + lnr_reader_error(rr)); sh.free_blocks.push(b); break; }
                if (!b->n) { sh.free_blocks.push(b); break; }
                const char *ids; const uint64_t *io;
                lnr_reader_ids(rr, &ids, &io);
                b->id_off.assign(io, io + b->n + 1);
                b->ids.assign(ids, ids + io[b->n]);
                b->len.resize(b->n);
                for (uint32_t i = 0; i < b->n; i++) b->len[i] = b->off[i + 1] - b->off[i];
                b->seq = seq++; b->file = (int)f;
                sh.ready.push(b);
            }
            lnr_reader_close(rr);
        }
        sh.ready.close();
    });
    // calculators: one per GPU.  Free-running (no gap re-mapper, or the read stream has "extended"): three blocks in flight -- lnr_filter_wait hands
    // out block k while it computes k + 1 and the upload of k + 2 runs.  Before that (-g > 0, stream not extended yet): one block at a time, strictly
    // in file order across all GPUs, each starting from the state the block before left.
    std::vector<std::thread> workers;
    for (unsigned g = 0; g < G; g++) workers.emplace_back([&, g] {
        std::deque<Block *> fl;                 // submitted, not handed out yet
        uint64_t count = 0;                     // results this context has handed out
        bool eof = false, free_run = o.gap_len == 0;
        while (!sh.failed) {
            size_t depth = free_run ? 3 : 1;
            while (!eof && fl.size() < depth) {
                Block *b = nullptr;
                if (fl.empty()) { if (!sh.ready.pop(b)) { eof = true; break; } }
                else if (!sh.ready.try_pop(b)) break;
                if (!free_run) {                 // (the context is idle here: depth 1)
                    std::unique_lock<std::mutex> l(sh.m);
                    sh.cv.wait(l, [&] { return sh.failed || sh.ext || sh.turn == b->seq; });
                    if (sh.failed) return;
                    if (sh.ext) free_run = true;
                    l.unlock();
                    if (lnr_gap_stream(ctx[g], free_run ? 1 : 0, nullptr) != LNR_OK) { sh.fail(std::string("gap stream: ") + lnr_last_error(ctx[g])); return; }
                }
                if (lnr_filter_submit(ctx[g], b->bases, b->off.data(), b->n) != LNR_OK) { sh.fail(std::string("submit: ") + lnr_last_error(ctx[g])); return; }
                fl.push_back(b);
            }
            if (fl.empty()) break;
            Block *b = fl.front();
            fl.pop_front();
            // the result slot this wait fills was handed out two results ago: the writer must be through with that block
            { std::unique_lock<std::mutex> l(sh.m); sh.cv.wait(l, [&] { return sh.failed || count < 2 || sh.written_upto[g] + 2 > count; }); if (sh.failed) return; }
            double tg0 = now();
            lnr_status s = lnr_filter_wait(ctx[g], &b->cords);
            us_gpu += (uint64_t)((now() - tg0) * 1e6);
            if (s != LNR_OK) { sh.fail(std::string("filter: ") + lnr_strerror(s) + " (" + lnr_last_error(ctx[g]) + ")"); return; }
            count++;
            if (!free_run) {
                int st = 0;
                lnr_gap_stream(ctx[g], -1, &st);
                std::lock_guard<std::mutex> l(sh.m);
                if (st) { sh.ext = 1; free_run = true; }
                sh.turn = b->seq + 1;
            }
            b->worker = (int)g;
            { std::lock_guard<std::mutex> l(sh.m); sh.done[b->seq] = b; }
            sh.cv.notify_all();
        }
    });
    // writer: the one printer, in file order (parallel_io.cpp:522-569)
    std::thread writer([&] {
        Outputs out;
        FILE *&fsam = out.fsam, *&fapf = out.fapf;
        // `@PG ... CL:` stays empty: the reference's Options constructor fills cmd_line only `if (length(argv) < 1)` (base.cpp:64-72), i.e. never
        Headers sam_header;
        uint64_t want = 0;
        const char *text; uint64_t size;
        if (o.sort) { out.sort_wr = wr; out.sort_device_mem = o.sort_device_mem; out.sort_host_mem = o.sort_host_mem; out.sort_spill = o.has_sort_host_mem; }
        if (!header_of(sam_header)) sh.fail(std::string(want_bam ? "BAM / BGZF header: " : "--bgzf: ") + lnr_writer_error(wr));
        for (;;) {
            Block *b = nullptr;
            {
                std::unique_lock<std::mutex> l(sh.m);
                sh.cv.wait(l, [&] { return sh.failed || sh.done.count(want) || (sh.workers_done && sh.done.empty()); });
                if (sh.failed) break;
                auto it = sh.done.find(want);
                if (it == sh.done.end()) break;
                b = it->second; sh.done.erase(it);
            }
            { std::string oe; if (!out.turn_to(o, b->file, sam_header, oe)) { sh.fail(oe); break; } }
            double tw0 = now();
            auto format = [&](int what) {
                if (what == 1 && o.sam_seq)                              // the block's bases are alive: it is recycled below, after the writer is through
                    return o.gpu_writer ? lnr_writer_format_seq_gpu(wr, &b->cords, b->bases, b->off.data(), b->ids.data(), b->id_off.data(), &text, &size)
                                        : lnr_writer_format_seq(wr, &b->cords, b->bases, b->off.data(), b->ids.data(), b->id_off.data(), o.thread, &text, &size);
                return o.gpu_writer ? lnr_writer_format_gpu(wr, &b->cords, b->len.data(), b->ids.data(), b->id_off.data(), what, &text, &size)
                                    : lnr_writer_format(wr, &b->cords, b->len.data(), b->ids.data(), b->id_off.data(), what, o.thread, &text, &size);
            };
            if (fsam) { if (format(1) != LNR_OK) { sh.fail(std::string("writer (.sam): ") + lnr_writer_error(wr)); break; } if (fwrite(text, 1, size, fsam) != size) { sh.fail("write error (.sam)"); break; } }
            if (fapf) { if (format(2) != LNR_OK) { sh.fail(std::string("writer (.apf): ") + lnr_writer_error(wr)); break; } if (fwrite(text, 1, size, fapf) != size) { sh.fail("write error (.apf)"); break; } }
            if (out.fpaf) {
                const lnr_status s = o.gpu_writer ? lnr_writer_format_paf_gpu(wr, &b->cords, b->len.data(), b->ids.data(), b->id_off.data(), &text, &size)
                                                  : lnr_writer_format_paf(wr, &b->cords, b->len.data(), b->ids.data(), b->id_off.data(), o.thread, &text, &size);
                if (s != LNR_OK) { sh.fail(std::string("writer (.paf): ") + lnr_writer_error(wr)); break; }
                if (fwrite(text, 1, size, out.fpaf) != size) { sh.fail("write error (.paf)"); break; }
            }
            if (out.fbam || out.fpbsv) {                                 // one encoding serves both files: they differ in their headers alone
                lnr_status s = bam_call([&] { return o.sam_seq ? lnr_writer_format_bam_gpu(wr, &b->cords, b->bases, b->off.data(), b->ids.data(), b->id_off.data(), &text, &size)
                                                               : lnr_writer_format_bam_gpu(wr, &b->cords, nullptr, b->len.data(), b->ids.data(), b->id_off.data(), &text, &size); });
                if (s != LNR_OK) { sh.fail(std::string("writer (.bam): ") + lnr_writer_error(wr) + sort_hint(o, s)); break; }
                if ((out.fbam && fwrite(text, 1, size, out.fbam) != size) || (out.fpbsv && fwrite(text, 1, size, out.fpbsv) != size)) { sh.fail("write error (.bam)"); break; }
            }
            us_writer += (uint64_t)((now() - tw0) * 1e6);
            total_reads += b->n;
            { std::lock_guard<std::mutex> l(sh.m); sh.written_upto[(size_t)b->worker]++; }
            sh.cv.notify_all();
            sh.free_blocks.push(b);
            want++;
        }
        if (sh.failed) out.sort_wr = nullptr;
        out.close();
        if (!out.sort_err.empty()) sh.fail(out.sort_err);
    });
    for (auto &t : workers) t.join();
    { std::lock_guard<std::mutex> l(sh.m); sh.workers_done = true; }
    sh.cv.notify_all();
    if (sh.failed) { sh.free_blocks.close(); sh.ready.close(); }
    writer.join();
    sh.free_blocks.close();
    reader.join();
    for (auto &b : blocks) lnr_host_free(b.bases);
    lnr_writer_destroy(wr);
    for (auto *c : ctx) lnr_destroy(c);
    if (gg) lnr_genome_free(gg);
    if (sh.failed) { fprintf(stderr, "\033[1;31mE:\033[0m %s\n", sh.err.c_str()); return 1; }
    double dt = now() - t_start;
    const double t_reads = now() - t_reads0;
    fprintf(stderr, "  Processed: %llu reads on %u GPU%s; read files in -> output files out: %.3f s = %.0f reads/s\n", (unsigned long long)total_reads.load(), G, G > 1 ? "s" : "", t_reads,
            total_reads.load() / (t_reads > 0 ? t_reads : 1));
    fprintf(stderr, "  Stage busy time[s]: reader %.3f, GPU (upload wait + kernels + download, all calculators) %.3f, writer %.3f\n", us_reader.load() / 1e6, us_gpu.load() / 1e6, us_writer.load() / 1e6);
    fprintf(stderr, "Time in sum[s] %.2f      \n", dt);
    return 0;
}
