// reader_bam_hd_shim.cpp -- linear_amd/csrc/lnr_bam_hd.h compiled by g++ behind a C ABI for tests/test_reader_bam_cpu.py: the header span,
// rec_valid / rec_plausible, nib2ord, the take, and the speculate / verify / repair scheme of k_bam_find + k_bam_stitch run on the host,
// tile after tile, at any tile size.  The same text the kernels call.
#include <cstdint>
#include <vector>

#include "../linear_amd/csrc/lnr_bam_hd.h"

using namespace lnr_bam;

extern "C" {

// 0 ok (first, n_ref set), 1 need more (need set), -1 not a BAM header
int bh_header_span(const u8 *b, u64 len, u64 *first, u64 *need, int *n_ref) {
    const Header h = header_span(b, len);
    *first = h.first; *need = h.need; *n_ref = h.n_ref;
    return h.status;
}
int bh_rec_valid(const u8 *rec, u64 avail, int n_ref) { return avail >= HEAD && rec_valid(rec_fields(rec), n_ref, rec, avail); }
int bh_rec_plausible(const u8 *rec, u64 avail, int n_ref) { return avail >= HEAD && rec_plausible(rec_fields(rec), n_ref, rec, avail); }
int bh_nib2ord(int nib) { return nib2ord((u32)nib); }
int bh_max_block(void) { return MAX_BLOCK; }
void bh_rec_fields(const u8 *rec, int64_t *out9) {
    const Fields f = rec_fields(rec);
    out9[0] = f.block_size; out9[1] = f.refID; out9[2] = f.pos; out9[3] = f.l_read_name; out9[4] = f.n_cigar_op; out9[5] = f.flag; out9[6] = f.l_seq;
    out9[7] = f.next_refID; out9[8] = f.next_pos;
}
void bh_take(const u32 *len, u64 count, u64 free_, u64 allowed, int block_empty, u64 *out4) {
    const Take t = take(len, count, free_, allowed, block_empty != 0);
    out4[0] = t.n; out4[1] = t.bases; out4[2] = t.full; out4[3] = t.too_big;
}
// the first plausible offset of every tile (NONE: none) -> first[nt]
void bh_guesses(const u8 *text, u64 len, int n_ref, u32 tile, u32 *first) {
    const u64 nt = (len + tile - 1) / tile;
    for (u64 t = 0; t < nt; t++) { const u64 t0 = t * tile, tend = t0 + tile < len ? t0 + tile : len; first[t] = find_first(text, len, n_ref, t0, tend); }
}
// the scheme over text = the stream behind the header: record starts in order -> offs (at most cap); info = {records, repaired tiles, flag of
// the stop (CH_OK / CH_BAD / CH_CUT), offset of the first byte no whole record covers, tiles}
void bh_scheme(const u8 *text, u64 len, int n_ref, u32 tile, u64 *offs, u64 cap, u64 *info) {
    const u64 nt = (len + tile - 1) / tile;
    const u32 sc = slice_cap(tile);
    std::vector<u32> list(nt * sc), cnt(nt, 0);
    std::vector<Tile> tiles(nt);
    for (u64 t = 0; t < nt; t++) {                                   // k_bam_find: every tile on its own
        const u64 t0 = t * tile, tend = t0 + tile < len ? t0 + tile : len;
        tiles[t] = speculate(text, len, n_ref, t0, tend, find_first(text, len, n_ref, t0, tend), list.data() + t * sc, sc, true);
    }
    u64 p = 0, nrec = 0, next = 0;                                   // k_bam_stitch: the true position through the tiles in order
    u32 flag = CH_OK, repaired = 0;
    while (p < len && flag == CH_OK) {
        const u64 t = p / tile, t0 = t * tile, tend = t0 + tile < len ? t0 + tile : len;
        repaired += (u32)(t - next);
        u32 count = 0;
        flag = stitch_tile(text, len, n_ref, p, t0, tend, tiles[t], list.data() + t * sc, sc, count, repaired, true);
        cnt[t] = count; nrec += count; next = t + 1;
        if (flag == CH_OK && p < tend) break;
    }
    u64 k = 0;
    for (u64 t = 0; t < nt; t++) for (u32 j = 0; j < cnt[t]; j++, k++) if (k < cap) offs[k] = list[t * sc + j];
    info[0] = nrec; info[1] = repaired; info[2] = flag; info[3] = p; info[4] = nt;
}

}  // extern "C"
