// The per-block logic of the writer's device deflate (linear_amd/csrc/lnr_deflate_hd.h) compiled for the host as a team of one lane: one
// block of text into one BGZF member (tests/test_deflate_hd_cpu.py).  With -DDEF_MAIN a stand-alone program for the sanitizers: it reads
// records "u32 n, n bytes" from a file, compresses every record block by block into arrays of exactly the size a member may take, inflates
// each member again with lnr_inf::inflate_block and prints "members bytes stored fnv status" per record.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../linear_amd/csrc/lnr_deflate_hd.h"

using namespace lnr_def;

// the size a member of n text bytes may take, rounded up to the 4-byte words the image is built in
extern "C" unsigned def_slot_bytes(unsigned n) { return (n + 31 + 3) & ~3u; }

// out: def_slot_bytes(n) bytes, 4-byte aligned.  Returns the member's size.
extern "C" unsigned def_member(const unsigned char *txt, unsigned n, unsigned char *out, unsigned *stored) {
    if (n > BLOCK_TEXT) return 0;
    static thread_local Work W;
    std::vector<u32> tab(HASH_SIZE), tok(n + 1);
    HostTeam T;
    return deflate_member(T, W, txt, n, tab.data(), tok.data(), out, stored);
}

// the whole text as the writer cuts it: block k = text [k * 0xff00, ...), members back to back.  out: total + 31 * blocks bytes at least.
// Returns the bytes written; *n_stored = members that hold a stored block.
extern "C" unsigned long long def_text(const unsigned char *txt, unsigned long long total, unsigned char *out, unsigned long long *n_stored) {
    unsigned long long at = 0;
    *n_stored = 0;
    std::vector<u32> img(MEMBER_CAP / 4);
    for (unsigned long long o = 0; o < total; o += BLOCK_TEXT) {
        const unsigned n = (unsigned)(total - o < BLOCK_TEXT ? total - o : BLOCK_TEXT);
        unsigned st = 0;
        const unsigned m = def_member(txt + o, n, (unsigned char *)img.data(), &st);
        memcpy(out + at, img.data(), m);
        at += m; *n_stored += st;
    }
    return at;
}

extern "C" const unsigned char *def_eof(unsigned *size) { *size = sizeof EOF_MEMBER; return EOF_MEMBER; }

#ifdef DEF_MAIN
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 n;
    while (fread(&n, 4, 1, f) == 1) {
        std::vector<unsigned char> txt(n);                 // exact sizes: the address sanitizer sees every byte outside them
        if (n && fread(txt.data(), 1, n, f) != n) return 2;
        unsigned long long members = 0, bytes = 0, stored = 0, fnv = 1469598103934665603ULL;
        unsigned status = 0;
        for (u32 o = 0; o < n; o += BLOCK_TEXT) {
            const u32 k = n - o < BLOCK_TEXT ? n - o : BLOCK_TEXT;
            std::vector<u32> img(def_slot_bytes(k) / 4);
            unsigned st = 0;
            const unsigned m = def_member(txt.data() + o, k, (unsigned char *)img.data(), &st);
            const unsigned char *p = (const unsigned char *)img.data();
            for (unsigned i = 0; i < m; i++) fnv = (fnv ^ p[i]) * 1099511628211ULL;
            u32 data_off = 0;
            std::vector<unsigned char> back(k);
            lnr_inf::Tables tabs;
            lnr_inf::HostSink sink{back.data()};
            if (lnr_inf::bgzf_member(p, m, data_off) != m) status = 101;
            else {
                const u32 s = lnr_inf::inflate_block(p + data_off, m - data_off - 8, sink, k, tabs);
                if (s) status = s;
                else if (memcmp(back.data(), txt.data() + o, k)) status = 102;
                else if (lnr_inf::crc_of(back.data(), k) != ((u32)p[m - 8] | (u32)p[m - 7] << 8 | (u32)p[m - 6] << 16 | (u32)p[m - 5] << 24)) status = lnr_inf::E_CRC;
            }
            members++; bytes += m; stored += st;
        }
        printf("%llu %llu %llu %llu %u\n", members, bytes, stored, fnv, status);
    }
    fclose(f);
    return 0;
}
#endif
