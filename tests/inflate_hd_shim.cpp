// The decode logic of the reader's device inflate (linear_amd/csrc/lnr_inflate_hd.h) compiled for the host: one BGZF block's raw DEFLATE
// into an array with guard bytes around it (tests/test_inflate_hd_cpu.py).  With -DINF_MAIN a stand-alone program for the sanitizers:
// it reads records "u32 clen, u32 isize, u32 crc, clen bytes" from a file and prints one status per record.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../linear_amd/csrc/lnr_inflate_hd.h"

using namespace lnr_inf;

// out has isize bytes.  Returns the status; *crc_out = CRC32 of the text by 64 slices combined as the device does, *blocks = DEFLATE blocks seen
extern "C" unsigned inf_block(const unsigned char *c, unsigned clen, unsigned char *out, unsigned isize, unsigned crc, unsigned *crc_out, unsigned *blocks) {
    Tables T;
    HostSink o{out};
    *blocks = 0; *crc_out = 0;
    u32 st = inflate_block(c, clen, o, isize, T, blocks);
    if (st != OK) return st;
    const u32 S = (isize + 63) / 64;
    u32 x = 0;
    for (u32 lane = 0; lane < 64; lane++) {
        const u32 a = lane * S < isize ? lane * S : isize, b = a + S < isize ? a + S : isize;
        x ^= crc_shift(crc_of(out + a, b - a), isize - b);
    }
    *crc_out = x;
    if (x != crc_of(out, isize)) return 100;              // the slices do not combine to the CRC of the whole
    return x == crc ? (u32)OK : (u32)E_CRC;
}
extern "C" unsigned inf_member(const unsigned char *p, unsigned long long avail, unsigned *data_off) { return bgzf_member(p, avail, *data_off); }
extern "C" const char *inf_status_text(unsigned s) { return status_text(s); }

#ifdef INF_MAIN
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 h[3];
    while (fread(h, 4, 3, f) == 3) {
        std::vector<unsigned char> c(h[0]), out(h[1]);     // exact sizes: the address sanitizer sees every byte outside them
        if (h[0] && fread(c.data(), 1, h[0], f) != h[0]) return 2;
        unsigned crc = 0, blocks = 0;
        unsigned st = inf_block(c.data(), h[0], out.data(), h[1], h[2], &crc, &blocks);
        printf("%u\n", st);
    }
    fclose(f);
    return 0;
}
#endif
