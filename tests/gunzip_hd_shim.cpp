// The parallel gzip inflate of the reader's device path (linear_amd/csrc/lnr_gunzip_hd.h) compiled for the host: the host driver over a
// whole file, the finder's test at every bit offset, and zlib's own block starts by inflate(Z_BLOCK) (tests/test_gunzip_hd_cpu.py).
// With -DGZ_MAIN a stand-alone program for the sanitizers: it reads records "u64 size, u64 text cap, u64 chunk, u64 round, size bytes" from
// a file and prints "status text-size crc32-of-text false-candidates" per record.  Link with -lz.
#include <cstdio>
#include <cstring>
#include <vector>
#include <zlib.h>

#include "../linear_amd/csrc/lnr_gunzip_hd.h"

using namespace lnr_gz;

// stats: rounds, members, chunks, candidates, pieces, falses, blocks, comp_bytes, text_bytes, win_syms, grown
extern "C" unsigned gz_gunzip(const unsigned char *gz, unsigned long long size, unsigned char *out, unsigned long long cap, unsigned long long *text_size,
                              unsigned long long chunk, unsigned long long round, unsigned long long *stats, unsigned long long *bad_off) {
    Stats S{};
    u64 ts = 0, bo = 0;
    const u32 st = gunzip_host(gz, size, out, cap, &ts, chunk, round, S, &bo);
    *text_size = ts; *bad_off = bo;
    const u64 v[11] = {S.rounds, S.members, S.chunks, S.candidates, S.pieces, S.falses, S.blocks, S.comp_bytes, S.text_bytes, S.win_syms, S.grown};
    for (int i = 0; i < 11; i++) stats[i] = v[i];
    return st;
}
extern "C" const char *gz_status_text(unsigned s) { return status_text(s); }
extern "C" unsigned gz_member_header(const unsigned char *p, unsigned long long avail, unsigned long long *data_off) {
    u64 d = 0;
    const u32 st = member_header(p, avail, &d);
    *data_off = d;
    return st;
}
// every bit offset in [from_bit, 8 * size) that passes the finder's test
extern "C" unsigned long long gz_find_all(const unsigned char *gz, unsigned long long size, unsigned long long from_bit, unsigned long long *bits, unsigned long long cap) {
    u64 n = 0;
    for (u64 b = from_bit; b < size * 8; b++)
        if (is_dynamic_start(gz, size, b)) { if (n < cap) bits[n] = b; n++; }
    return n;
}
// zlib's block boundaries of the first member: the bit offset behind the header and behind every block
extern "C" long long gz_zlib_boundaries(const unsigned char *gz, unsigned long long size, unsigned long long *bits, unsigned long long cap) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 31) != Z_OK) return -1;
    std::vector<unsigned char> buf(1 << 16);
    z.next_in = const_cast<unsigned char *>(gz); z.avail_in = (uInt)size;
    long long n = 0;
    for (;;) {
        z.next_out = buf.data(); z.avail_out = (uInt)buf.size();
        const int r = inflate(&z, Z_BLOCK);
        if (r != Z_OK && r != Z_STREAM_END && r != Z_BUF_ERROR) { inflateEnd(&z); return -2; }
        if (r == Z_STREAM_END) break;
        if (z.data_type & 128) { if ((u64)n < cap) bits[n] = (u64)z.total_in * 8 - (u64)(z.data_type & 63); n++; }
        if (r == Z_BUF_ERROR && z.avail_in == 0) break;
    }
    inflateEnd(&z);
    return n;
}

#ifdef GZ_MAIN
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned long long h[4];
    while (fread(h, 8, 4, f) == 4) {
        std::vector<unsigned char> gz(h[0]), out(h[1]);      // exact sizes: the address sanitizer sees every byte outside them
        if (h[0] && fread(gz.data(), 1, h[0], f) != h[0]) return 2;
        unsigned long long ts = 0, bo = 0, st[11];
        const unsigned s = gz_gunzip(gz.data(), h[0], out.data(), h[1], &ts, h[2], h[3], st, &bo);
        printf("%u %llu %lu %llu\n", s, ts, s ? 0ul : crc32(0L, out.data(), (uInt)ts), st[5]);
    }
    fclose(f);
    return 0;
}
#endif
