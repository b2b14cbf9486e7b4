// qual_span_main.cpp -- the quality span of a raw BAM record (lnr_out::bam_qual_span, linear_amd/csrc/lnr_output_hd.h) as a stand-alone
// program for the address and undefined-behaviour sanitizers (tests/test_output_qual_span_cpu.py).  Input file: u64 n_bytes, the record
// stream, then per record two i64: qoff, l_seq.  Every record is copied into a heap block of exactly its size at each of the four byte
// alignments, so a read before or past the record is an error; the span must be the expected one, hold 0xff alone, and the record without
// it, with l_seq bytes of 0xff put back at qoff, must be the record.  Cut short by one byte and down to its core, the record is looked at
// within what is left of it.  Prints "ok <records>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../linear_amd/csrc/lnr_output_hd.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t nbytes = 0;
    if (fread(&nbytes, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> raw(nbytes);
    if (nbytes && fread(raw.data(), 1, nbytes, f) != nbytes) return 2;
    uint64_t p = 0, n = 0;
    while (p < nbytes) {
        int64_t want[2];
        if (fread(want, 8, 2, f) != 2) { fprintf(stderr, "record %llu: no expectation\n", (unsigned long long)n); return 1; }
        const uint64_t size = 4ULL + lnr_out::le32_at(raw.data() + p);
        if (size < 36 || p + size > nbytes) { fprintf(stderr, "record %llu does not fit\n", (unsigned long long)n); return 1; }
        for (unsigned shift = 0; shift < 4; shift++) {
            uint8_t *block = (uint8_t *)malloc(size + shift);        // the record ends where the block ends
            memcpy(block + shift, raw.data() + p, size);
            const uint8_t *rec = block + shift;
            const lnr_out::BamQual q = lnr_out::bam_qual_span(rec, size);
            bool ok = q.qoff == (uint64_t)want[0] && q.l_seq == (uint64_t)want[1] && (uint64_t)q.qoff + q.l_seq <= size;
            if (ok) {
                for (uint32_t i = 0; i < q.l_seq; i++) ok = ok && rec[q.qoff + i] == 0xff;
                std::vector<uint8_t> held(rec, rec + q.qoff);         // what the sort mode holds ...
                held.insert(held.end(), rec + q.qoff + q.l_seq, rec + size);
                std::vector<uint8_t> back(held.begin(), held.begin() + q.qoff);       // ... and what its gather writes
                back.insert(back.end(), q.l_seq, 0xff);
                back.insert(back.end(), held.begin() + q.qoff, held.end());
                ok = ok && back.size() == size && memcmp(back.data(), rec, size) == 0;
            }
            free(block);
            if (!ok) { fprintf(stderr, "record %llu at alignment %u: span %u + %u\n", (unsigned long long)n, shift, q.qoff, q.l_seq); return 1; }
        }
        for (uint64_t cut_size : {size - 1, (uint64_t)36}) {
            uint8_t *cut = (uint8_t *)malloc(cut_size);
            memcpy(cut, raw.data() + p, cut_size);
            const lnr_out::BamQual q = lnr_out::bam_qual_span(cut, cut_size);
            free(cut);
            if ((uint64_t)q.qoff + q.l_seq > cut_size) return 1;
        }
        p += size; n++;
    }
    fclose(f);
    printf("ok %llu\n", (unsigned long long)n);
    return 0;
}
