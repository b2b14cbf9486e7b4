// lnr_genome.cpp -- the reference genome, from files to sequences resident on the device (include/linear_amd.h: lnr_genome_*).  Host code:
// the files are read by the GPU reader (lnr_reader_open + lnr_reader_gpu_open + lnr_reader_next_dev: FASTA text parsed on the device, BGZF
// and -- on request -- plain gzip inflated there), and every delivered block is copied, device to device on the reader's stream, into an
// allocation the genome owns (lnr_reader_keep_block -> lnr_rdgpu_keep behind lnr_reader_hook.h).  No base crosses the bus unless lnr_genome_to_host asks for it.
//
// Replaces, for a front-end, the loop that loads a genome through lnr_reader_next(max_reads = 1): the same sequences in the same order
// (files in order, records in file order), the same lengths, ordinals and header lines.
#include "../../include/linear_amd.h"
#include "lnr_reader_hook.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace {
constexpr uint64_t BLOCK_BASES = 1ULL << 30;    // default block: no record the reader can deliver is longer (its text limit is 2^30 bytes)
constexpr uint32_t BLOCK_RECORDS = 1024;        // records per block at most (a genome of short contigs takes several blocks)
struct Block { uint8_t *d = nullptr, *h = nullptr; uint64_t bytes = 0; };
thread_local std::string load_err;              // why the last lnr_genome_load_gpu of this thread failed (there is no object to ask)
}  // namespace

struct lnr_genome {
    int32_t device = 0;
    std::vector<uint64_t> len, id_off{0};
    std::vector<char> ids;
    std::vector<Block> blocks;                  // one device allocation per delivered block
    std::vector<uint32_t> blk_of; std::vector<uint64_t> off_in;     // sequence i lies in blocks[blk_of[i]] at off_in[i]
    std::vector<const uint8_t *> d_seq, h_seq;
    bool on_dev = true, on_host = false;
    std::string err;
};

namespace {
void free_dev(lnr_genome *g) {
    for (Block &b : g->blocks) { if (b.d && lnr_rdgpu_keep_free) lnr_rdgpu_keep_free(g->device, b.d); b.d = nullptr; }
    g->on_dev = false;
}
lnr_status load_fail(lnr_genome *g, lnr_reader *r, lnr_status s, const std::string &why) {
    load_err = why;
    if (r) lnr_reader_close(r);
    if (g) lnr_genome_free(g);
    return s;
}
}  // namespace

extern "C" {

lnr_status lnr_genome_load_gpu(const char *const *paths, uint32_t npaths, int32_t device, uint32_t flags, uint64_t block_bases, lnr_genome **out) {
    if (out) *out = nullptr;
    load_err.clear();
    if (!out || (!paths && npaths)) return load_fail(nullptr, nullptr, LNR_ERR_ARG, "lnr_genome_load_gpu: null argument");
    if (flags & ~LNR_GENOME_GPU_GZIP) return load_fail(nullptr, nullptr, LNR_ERR_ARG, "lnr_genome_load_gpu: unknown flag");
    if (!lnr_rdgpu_keep || !lnr_rdgpu_keep_free || !lnr_rdgpu_keep_download)
        return load_fail(nullptr, nullptr, LNR_ERR_NO_DEVICE, "no usable device " + std::to_string(device) + ": this library was linked without its device half");
    const uint64_t bb = block_bases ? block_bases : BLOCK_BASES;
    lnr_genome *g = new (std::nothrow) lnr_genome();
    if (!g) return load_fail(nullptr, nullptr, LNR_ERR_NOMEM, "host allocation failed");
    g->device = device;
    for (uint32_t f = 0; f < npaths; f++) {
        const std::string path = paths[f] ? paths[f] : "";
        lnr_reader *r = nullptr;
        lnr_status s = lnr_reader_open(path.c_str(), &r);
        if (s != LNR_OK) return load_fail(g, nullptr, s, "can't open genome file " + path);
        if (lnr_reader_format(r) == 3) return load_fail(g, r, LNR_ERR_ARG, "genome " + path + " is a BAM file: a genome is read from FASTA / FASTQ only");
        if ((s = lnr_reader_gpu_open(r, device, 1)) != LNR_OK) return load_fail(g, r, s, "genome " + path + ": " + lnr_reader_error(r));
        if ((flags & LNR_GENOME_GPU_GZIP) && (s = lnr_reader_gpu_gzip(r, 1)) != LNR_OK) return load_fail(g, r, s, "genome " + path + ": " + lnr_reader_error(r));
        for (;;) {
            const uint8_t *d_reads; const uint64_t *d_off, *off; uint32_t n = 0;
            s = lnr_reader_next_dev(r, bb, BLOCK_RECORDS, &d_reads, &d_off, &off, &n);
            if (s == LNR_ERR_LIMIT)             // the record the call stopped at: the reader's own count, records of this call's unfinished block included
                return load_fail(g, r, s, "genome " + path + ": record " + std::to_string(lnr_reader_records(r)) + ": " + lnr_reader_error(r) + " (blocks of " + std::to_string(bb) + " bases)");
            if (s != LNR_OK) return load_fail(g, r, s, "genome " + path + ": " + lnr_reader_error(r));
            if (!n) break;
            Block b;
            b.bytes = off[n];
            if (int ks = lnr_reader_keep_block(r, b.bytes, &b.d, &g->device)) return load_fail(g, r, (lnr_status)ks, "genome " + path + ": " + lnr_reader_error(r));      // (device < 0: the one the reader resolved it to)
            g->blocks.push_back(b);
            const char *ids; const uint64_t *io;
            lnr_reader_ids(r, &ids, &io);
            g->ids.insert(g->ids.end(), ids, ids + io[n]);
            for (uint32_t k = 0; k < n; k++) {
                g->len.push_back(off[k + 1] - off[k]);
                g->blk_of.push_back((uint32_t)g->blocks.size() - 1);
                g->off_in.push_back(off[k]);
                g->d_seq.push_back(b.d + off[k]);
                g->id_off.push_back(g->id_off.back() + (io[k + 1] - io[k]));
            }
        }
        lnr_reader_close(r);
    }
    *out = g;
    return LNR_OK;
}

lnr_status lnr_genome_info(const lnr_genome *g, uint32_t *nseq, const uint64_t **len, const char **ids, const uint64_t **id_off, const uint8_t *const **d_seq) {
    if (!g) return LNR_ERR_ARG;
    if (nseq) *nseq = (uint32_t)g->len.size();
    if (len) *len = g->len.data();
    if (ids) *ids = g->ids.data();
    if (id_off) *id_off = g->id_off.data();
    if (d_seq) *d_seq = g->on_dev ? g->d_seq.data() : nullptr;
    return LNR_OK;
}

lnr_status lnr_genome_to_host(lnr_genome *g, const uint8_t *const **seq) {
    if (!g || !seq) return LNR_ERR_ARG;
    *seq = nullptr;
    if (!g->on_host) {
        if (!g->on_dev) { g->err = "lnr_genome_to_host: the device copy has been dropped and no host copy was taken before"; return LNR_ERR_ARG; }
        char e[256] = "";
        for (Block &b : g->blocks) {
            if (!b.h && !(b.h = (uint8_t *)malloc(b.bytes ? b.bytes : 1))) { g->err = "host allocation failed"; return LNR_ERR_NOMEM; }
            if (int s = lnr_rdgpu_keep_download(g->device, b.d, b.h, b.bytes, e, sizeof e)) { g->err = e; return (lnr_status)s; }
        }
        g->h_seq.clear();
        for (size_t i = 0; i < g->len.size(); i++) g->h_seq.push_back(g->blocks[g->blk_of[i]].h + g->off_in[i]);
        g->on_host = true;
    }
    *seq = g->h_seq.data();
    return LNR_OK;
}

lnr_status lnr_genome_drop_dev(lnr_genome *g) {
    if (!g) return LNR_ERR_ARG;
    free_dev(g);
    return LNR_OK;
}

const char *lnr_genome_error(const lnr_genome *g) { return g ? g->err.c_str() : load_err.c_str(); }

void lnr_genome_free(lnr_genome *g) {
    if (!g) return;
    free_dev(g);
    for (Block &b : g->blocks) free(b.h);
    delete g;
}

}  // extern "C"
