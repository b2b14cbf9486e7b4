// TEST-ONLY: the PAF part of linear_amd/csrc/lnr_output_hd.h (paf_read, the body of k_out_measure<Paf> / k_out_emit<Paf>) compiled for the host:
// "measure" and "emit" of a batch, as tests/output_shim.cpp does for SAM and APF.
#include "../linear_amd/csrc/lnr_output_hd.h"

using namespace lnr_out;

static Params mk(const char *gblob, const u64 *goff, const u64 *glen, u32 nseq, u32 preset) {
    Params P{gblob, goff, glen, nseq, 8000, 80, 200};
    if (preset != 1) { P.thd_DI = ((i64)1 << 60) - 1; P.thd_X = ((i64)1 << 60) - 1; }
    return P;
}

extern "C" {
// bytes per read with the counting sink; returns their sum
u64 ps_measure(const char *gblob, const u64 *goff, const u64 *glen, u32 nseq, u32 preset, const u64 *coff, const u64 *cs, const u64 *ce, u32 n, const u64 *len,
               const char *ids, const u64 *idoff, u64 *sizes) {
    Params P = mk(gblob, goff, glen, nseq, preset);
    u64 total = 0;
    for (u32 k = 0; k < n; k++) {
        CountSink c;
        paf_read(c, P, cs + coff[k], ce + coff[k], coff[k + 1] - coff[k], len[k], ids + idoff[k]);
        sizes[k] = c.n; total += c.n;
    }
    return total;
}
// text with the byte sink into out (the caller sized it from ps_measure); emitted[k] = bytes read k wrote; returns the total
u64 ps_emit(const char *gblob, const u64 *goff, const u64 *glen, u32 nseq, u32 preset, const u64 *coff, const u64 *cs, const u64 *ce, u32 n, const u64 *len,
            const char *ids, const u64 *idoff, char *out, u64 *emitted) {
    Params P = mk(gblob, goff, glen, nseq, preset);
    ByteSink b{out};
    for (u32 k = 0; k < n; k++) {
        char *p0 = b.p;
        paf_read(b, P, cs + coff[k], ce + coff[k], coff[k + 1] - coff[k], len[k], ids + idoff[k]);
        emitted[k] = (u64)(b.p - p0);
    }
    return (u64)(b.p - out);
}
}
