// TEST-ONLY: the SEQ form of linear_amd/csrc/lnr_output_hd.h (sam_read_seq: head, segments, tail) compiled for the host.
#include "../linear_amd/csrc/lnr_output_hd.h"

using namespace lnr_out;

struct In {
    const char *gblob; const u64 *goff, *glen; u32 nseq, preset;
    const uint8_t *genome; const u64 *gstart;
    const u64 *coff, *cs, *ce; u32 n;
    const uint8_t *reads; const u64 *roff;
    const char *ids; const u64 *idoff;
};
template <class S> static void one(S &s, const In &in, u32 k) {
    Params P{in.gblob, in.goff, in.glen, in.nseq, 8000, 80, 200};
    if (in.preset != 1) { P.thd_DI = ((i64)1 << 60) - 1; P.thd_X = ((i64)1 << 60) - 1; }
    SeqSrc q{in.genome, in.gstart, in.glen, in.nseq, in.reads + in.roff[k], in.roff[k + 1] - in.roff[k]};
    u64 a = in.coff[k];
    sam_read_seq(s, P, q, in.cs + a, in.ce + a, in.coff[k + 1] - a, in.ids + in.idoff[k]);
}

extern "C" {
u64 oss_measure(const In *in, u64 *sizes) {
    u64 total = 0;
    for (u32 k = 0; k < in->n; k++) { CountSink c; one(c, *in, k); sizes[k] = c.n; total += c.n; }
    return total;
}
u64 oss_emit(const In *in, char *out, u64 *emitted) {
    ByteSink b{out};
    for (u32 k = 0; k < in->n; k++) { char *p0 = b.p; one(b, *in, k); emitted[k] = (u64)(b.p - p0); }
    return (u64)(b.p - out);
}
}
