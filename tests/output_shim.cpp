// TEST-ONLY: linear_amd/csrc/lnr_output_hd.h (the body of the writer's kernels) compiled for the host: "measure" and "emit" of a batch.
#include "../linear_amd/csrc/lnr_output_hd.h"

using namespace lnr_out;

static Params mk(const char *gblob, const u64 *goff, const u64 *glen, u32 nseq, u32 preset) {
    Params P{gblob, goff, glen, nseq, 8000, 80, 200};
    if (preset != 1) { P.thd_DI = ((i64)1 << 60) - 1; P.thd_X = ((i64)1 << 60) - 1; }
    return P;
}
template <class S> static void one(S &s, const Params &P, const u64 *coff, const u64 *cs, const u64 *ce, const u64 *len, const char *ids, const u64 *idoff, int what, u32 k) {
    u64 a = coff[k], n = coff[k + 1] - a;
    if (what == 1) sam_read(s, P, cs + a, ce + a, n, len[k], ids + idoff[k]);
    else apf_read(s, P, cs + a, n, len[k], ids + idoff[k], k > 0);
}

extern "C" {
// bytes per read with the counting sink; returns their sum
u64 os_measure(const char *gblob, const u64 *goff, const u64 *glen, u32 nseq, u32 preset, const u64 *coff, const u64 *cs, const u64 *ce, u32 n, const u64 *len,
               const char *ids, const u64 *idoff, int what, u64 *sizes) {
    Params P = mk(gblob, goff, glen, nseq, preset);
    u64 total = 0;
    for (u32 k = 0; k < n; k++) { CountSink c; one(c, P, coff, cs, ce, len, ids, idoff, what, k); sizes[k] = c.n; total += c.n; }
    return total;
}
// text with the byte sink into out (the caller sized it from os_measure); emitted[k] = bytes read k wrote; returns the total
u64 os_emit(const char *gblob, const u64 *goff, const u64 *glen, u32 nseq, u32 preset, const u64 *coff, const u64 *cs, const u64 *ce, u32 n, const u64 *len,
            const char *ids, const u64 *idoff, int what, char *out, u64 *emitted) {
    Params P = mk(gblob, goff, glen, nseq, preset);
    ByteSink b{out};
    for (u32 k = 0; k < n; k++) { char *p0 = b.p; one(b, P, coff, cs, ce, len, ids, idoff, what, k); emitted[k] = (u64)(b.p - p0); }
    return (u64)(b.p - out);
}
}
