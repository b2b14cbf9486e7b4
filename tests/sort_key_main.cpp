// sort_key_main.cpp -- the key extraction of the coordinate sort (lnr_out::bam_key, linear_amd/csrc/lnr_output_hd.h) as a stand-alone
// program for the address and undefined-behaviour sanitizers (tests/test_output_sort_cpu.py).  Input file: u64 n_bytes, the record stream,
// then per record five i64: refID, pos, flag, block_size, end.  Every record is copied into a heap block of exactly its size at each of the
// four byte alignments, so a read before or past the record is an error, and the key must be the expected one.  Prints "ok <records>".
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
        int64_t want[5];
        if (fread(want, 8, 5, f) != 5) { fprintf(stderr, "record %llu: no expectation\n", (unsigned long long)n); return 1; }
        const uint64_t size = 4ULL + lnr_out::le32_at(raw.data() + p);
        if (size < 36 || p + size > nbytes) { fprintf(stderr, "record %llu does not fit\n", (unsigned long long)n); return 1; }
        for (unsigned shift = 0; shift < 4; shift++) {
            uint8_t *block = (uint8_t *)malloc(size + shift);        // the record ends where the block ends
            memcpy(block + shift, raw.data() + p, size);
            const lnr_out::BamKey k = lnr_out::bam_key(block + shift, size);
            const int64_t got[5] = {k.ref, k.pos, (int64_t)k.flag, (int64_t)k.block_size, k.end};
            free(block);
            if (memcmp(got, want, sizeof got)) {
                fprintf(stderr, "record %llu at alignment %u: got %lld %lld %lld %lld %lld\n", (unsigned long long)n, shift, (long long)got[0], (long long)got[1], (long long)got[2], (long long)got[3], (long long)got[4]);
                return 1;
            }
            const uint64_t key = lnr_out::bam_sort_key(k);
            if (key != ((uint64_t)(uint32_t)want[0] << 32 | (uint32_t)want[1])) return 1;
        }
        // a record cut short after its core: the CIGAR words that are not there are not read
        uint8_t *cut = (uint8_t *)malloc(36);
        memcpy(cut, raw.data() + p, 36);
        (void)lnr_out::bam_key(cut, 36);
        free(cut);
        p += size; n++;
    }
    fclose(f);
    printf("ok %llu\n", (unsigned long long)n);
    return 0;
}
