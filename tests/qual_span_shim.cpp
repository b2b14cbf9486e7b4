// TEST-ONLY: bam_qual_span of linear_amd/csrc/lnr_output_hd.h compiled for the host (tests/test_output_qual_span_cpu.py; compiled the way
// tests/shimlib.py compiles its shim).  The same function the sort mode's kernels call on the device.
#include <cstdint>

#include "../linear_amd/csrc/lnr_output_hd.h"

extern "C" {
// rec: one raw record of `size` = 4 + block_size bytes; out[0] = qoff, out[1] = l_seq of its quality span ({0, 0}: the record is kept whole)
void qs_span(const uint8_t *rec, uint64_t size, uint32_t *out) {
    const lnr_out::BamQual q = lnr_out::bam_qual_span(rec, size);
    out[0] = q.qoff; out[1] = q.l_seq;
}
}
