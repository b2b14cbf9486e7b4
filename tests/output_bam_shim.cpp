// TEST-ONLY: the BAM form of linear_amd/csrc/lnr_output_hd.h (bam_read: head, packed SEQ, the 0xff run, tag) compiled for the host
// (tests/test_output_bam_cpu.py).  With -DOBS_MAIN a stand-alone program for the sanitizers: it reads one batch from a file written by the
// test (the arrays of `In`, each as a u64 byte count and its bytes, then the expected record bytes), measures, emits into an array of exactly
// the measured size and compares.
#include "../linear_amd/csrc/lnr_output_hd.h"

using namespace lnr_out;

struct In {
    const char *gblob; const u64 *goff, *glen; u32 nseq, preset;
    const uint8_t *genome; const u64 *gstart;
    const u64 *coff, *cs, *ce; u32 n;
    const uint8_t *reads; const u64 *rlen;      // seq != 0: rlen holds n + 1 read offsets into reads; else n read lengths (seq == 2: see one())
    const char *ids; const u64 *idoff;
    u32 seq;
};
template <class S> static void one(S &s, const In &in, u32 k) {
    Params P{in.gblob, in.goff, in.glen, in.nseq, 8000, 80, 200};
    if (in.preset != 1) { P.thd_DI = ((i64)1 << 60) - 1; P.thd_X = ((i64)1 << 60) - 1; }
    const u64 L = in.seq ? in.rlen[k + 1] - in.rlen[k] : in.rlen[k];
    SeqSrc q{in.genome, in.gstart, in.glen, in.nseq, in.seq ? in.reads + in.rlen[k] : nullptr, L};
    const uint8_t *table[16];                       // seq == 2: the sequences through a pointer table, as the host writer holds them
    if (in.seq == 2 && in.nseq <= 16) { for (u32 g = 0; g < in.nseq; g++) table[g] = in.genome + in.gstart[g]; q.genome = nullptr; q.gstart = nullptr; q.gseq = table; }
    u64 a = in.coff[k];
    bam_read(s, P, in.seq ? &q : nullptr, in.cs + a, in.ce + a, in.coff[k + 1] - a, L, in.ids + in.idoff[k]);
}

extern "C" {
u64 obs_measure(const In *in, u64 *sizes) {
    u64 total = 0;
    for (u32 k = 0; k < in->n; k++) { CountSink c; one(c, *in, k); sizes[k] = c.n; total += c.n; }
    return total;
}
u64 obs_emit(const In *in, char *out, u64 *emitted) {
    ByteSink b{out};
    for (u32 k = 0; k < in->n; k++) { char *p0 = b.p; one(b, *in, k); emitted[k] = (u64)(b.p - p0); }
    return (u64)(b.p - out);
}
}

#ifdef OBS_MAIN
#include <cstdio>
#include <cstring>
#include <vector>
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<std::vector<unsigned char>> a;     // exact sizes: the address sanitizer sees every byte outside them
    for (;;) {
        u64 n;
        if (fread(&n, 8, 1, f) != 1) break;
        a.emplace_back(n);
        if (n && fread(a.back().data(), 1, n, f) != n) return 2;
    }
    fclose(f);
    if (a.size() != 14) return 2;
    auto u = [&](int i) { return (const u64 *)a[i].data(); };
    const u64 *sc = u(0);                           // nseq, preset, n, seq
    In in{(const char *)a[1].data(), u(2), u(3), (u32)sc[0], (u32)sc[1], a[4].data(), u(5), u(6), u(7), u(8), (u32)sc[2], a[9].data(), u(10),
          (const char *)a[11].data(), u(12), (u32)sc[3]};
    std::vector<u64> sizes(in.n + 1), emitted(in.n + 1);
    const u64 total = obs_measure(&in, sizes.data());
    std::vector<char> out(total);
    if (obs_emit(&in, out.data(), emitted.data()) != total || sizes != emitted) { fprintf(stderr, "measured and emitted sizes differ\n"); return 1; }
    if (total != a[13].size() || (total && memcmp(out.data(), a[13].data(), total))) { fprintf(stderr, "bytes differ from the expected records\n"); return 1; }
    printf("ok %llu\n", (unsigned long long)total);
    return 0;
}
#endif
