// reader_bam_asan_main.cpp -- a stand-alone program for the sanitizer run of tests/test_reader_bam_cpu.py: host code only, its own main.
// Linked with linear_amd/csrc/lnr_reader.cpp (without the device half) and zlib.  Per file of the command line it runs the host decode
// (lnr_reader_next, blocks of 5000 bases / 7 records) and the host model of the device scheme (bh_scheme of the shim) at the given tile
// size, and prints one line:
//   <file> status <s> blocks <b> records <r> bases <n> | chain <records> repaired <t> flag <f>
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/linear_amd.h"
#include "reader_bam_hd_shim.cpp"

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s tile file...\n", argv[0]); return 2; }
    const u32 tile = (u32)atoi(argv[1]);
    for (int a = 2; a < argc; a++) {
        lnr_reader *r = nullptr;
        if (lnr_reader_open(argv[a], &r) != LNR_OK) { fprintf(stderr, "cannot open %s\n", argv[a]); return 1; }
        std::vector<uint8_t> dst(5000);
        std::vector<uint64_t> off(8);
        uint64_t blocks = 0, records = 0, bases = 0;
        lnr_status s;
        for (;;) {
            uint32_t n = 0;
            s = lnr_reader_next(r, dst.data(), dst.size(), off.data(), 7, &n);
            if (s != LNR_OK || !n) break;
            blocks++; records += n; bases += off[n];
            const char *ids; const uint64_t *io;
            lnr_reader_ids(r, &ids, &io);
            uint64_t sum = 0;
            for (uint64_t i = 0; i < io[n]; i++) sum += (unsigned char)ids[i];        // every byte of the block is read once
            for (uint64_t i = 0; i < off[n]; i++) sum += dst[i];
            if (sum == ~0ULL) return 3;
        }
        lnr_reader_close(r);
        std::vector<u8> st;
        gzFile f = gzopen(argv[a], "rb");
        if (!f) return 1;
        u8 buf[65536];
        for (int got; (got = gzread(f, buf, sizeof buf)) > 0;) st.insert(st.end(), buf, buf + got);
        gzclose(f);
        const Header h = header_span(st.data(), st.size());
        uint64_t info[5] = {0, 0, 0, 0, 0};
        if (h.status == 0 && st.size() > h.first) {
            std::vector<uint64_t> offs(st.size() / MIN_REC + 1);
            bh_scheme(st.data() + h.first, st.size() - h.first, h.n_ref, tile, offs.data(), offs.size(), info);
        }
        printf("%s status %d blocks %llu records %llu bases %llu | chain %llu repaired %llu flag %llu\n", argv[a], (int)s, (unsigned long long)blocks, (unsigned long long)records,
               (unsigned long long)bases, (unsigned long long)info[0], (unsigned long long)info[1], (unsigned long long)info[2]);
    }
    return 0;
}
