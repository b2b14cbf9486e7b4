// TEST-ONLY, stand-alone (built with -fsanitize=address,undefined by tests/test_output_paf_cpu.py, never loaded into Python): paf_read of
// linear_amd/csrc/lnr_output_hd.h over the batches of a file, every read measured with the counting sink and then emitted into a heap block
// of EXACTLY the measured size, every input array in a heap block of exactly its size -- a byte written past the text or a word read past
// the cords is the sanitizer's finding.  Prints "ok <reads> <bytes> <fnv1a of all text>".
//
// File: batches back to back, each of little-endian u64 words  nseq, n_reads, n_cords, gblob_bytes, id_bytes, preset,  then goff[nseq],
// glen[nseq], cord_off[n_reads + 1], cords_str[n_cords], cords_end[n_cords], read_len[n_reads], id_off[n_reads], then gblob and the read
// ids ('\0'-separated), each padded with zero bytes to a multiple of 8.
#include "../linear_amd/csrc/lnr_output_hd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace lnr_out;

template <class T> static T *take(FILE *f, u64 count) {          // exactly count elements on the heap (count 0: one byte nobody may touch)
    T *p = (T *)malloc(count ? count * sizeof(T) : 1);
    if (!p || (count && fread(p, sizeof(T), count, f) != count)) { fprintf(stderr, "short file\n"); exit(2); }
    return p;
}
static char *take_bytes(FILE *f, u64 bytes) {
    char *p = take<char>(f, bytes);
    char pad[8];
    const u64 rest = (8 - bytes % 8) % 8;
    if (rest && fread(pad, 1, rest, f) != rest) { fprintf(stderr, "short file\n"); exit(2); }
    return p;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: output_paf_main BATCHES\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    u64 reads = 0, bytes = 0, h = 1469598103934665603ULL, head[6];
    while (fread(head, 8, 6, f) == 6) {
        const u64 nseq = head[0], n = head[1], nc = head[2];
        u64 *goff = take<u64>(f, nseq), *glen = take<u64>(f, nseq), *coff = take<u64>(f, n + 1), *cs = take<u64>(f, nc), *ce = take<u64>(f, nc);
        u64 *len = take<u64>(f, n), *idoff = take<u64>(f, n);
        char *gblob = take_bytes(f, head[3]), *ids = take_bytes(f, head[4]);
        Params P{gblob, goff, glen, (u32)nseq, 8000, 80, 200};
        if (head[5] != 1) { P.thd_DI = ((i64)1 << 60) - 1; P.thd_X = ((i64)1 << 60) - 1; }
        for (u64 k = 0; k < n; k++) {
            const u64 a = coff[k], m = coff[k + 1] - a;
            CountSink c;
            paf_read(c, P, cs + a, ce + a, m, len[k], ids + idoff[k]);
            char *text = (char *)malloc(c.n ? c.n : 1);
            ByteSink b{text};
            paf_read(b, P, cs + a, ce + a, m, len[k], ids + idoff[k]);
            if ((u64)(b.p - text) != c.n) { fprintf(stderr, "read %llu: measured %llu bytes, emitted %llu\n", (unsigned long long)k, (unsigned long long)c.n, (unsigned long long)(b.p - text)); return 1; }
            if (c.n && text[c.n - 1] != '\n') { fprintf(stderr, "read %llu: the text does not end with a line end\n", (unsigned long long)k); return 1; }
            for (u64 i = 0; i < c.n; i++) h = (h ^ (unsigned char)text[i]) * 1099511628211ULL;
            free(text);
            reads++; bytes += c.n;
        }
        free(goff); free(glen); free(coff); free(cs); free(ce); free(len); free(idoff); free(gblob); free(ids);
    }
    fclose(f);
    printf("ok %llu %llu %016llx\n", (unsigned long long)reads, (unsigned long long)bytes, (unsigned long long)h);
    return 0;
}
