// TEST-ONLY: the reader's GPU logic (linear_amd/csrc/lnr_reader_hd.h) compiled for the host.  rs_parse runs what the three kernels of
// lnr_reader_kernels.hip run -- measure per tile, scan of the tile summaries + the decision, emit per tile -- with the group masks made by
// a loop instead of wave ballots, at any tile size.  With -DRS_MAIN it is a stand-alone program (for the sanitizers): file, tile size.
#include "../linear_amd/csrc/lnr_reader_hd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lnr_rd;

static Masks masks_of(int fmt, const u8 *text, u64 g, u64 tend, bool measure) {
    Masks m{};
    for (u32 lane = 0; lane < 64 && g + lane < tend; lane++) {
        const u64 pos = g + lane;
        u32 b = byte_bits(fmt, text[pos], pos ? text[pos - 1] : (u8)'\n');
        if (!measure) b &= 15u;
        const u64 bit = 1ULL << lane;
        if (b & 1) m.valid |= bit;
        if (b & 2) m.nl |= bit;
        if (fmt == FASTA && (b & 4)) m.gt |= bit;
        if (b & 8) m.keep |= bit;
        if (b & 16) m.wsbad |= bit;
        if (b & 32) m.notat |= bit;
        if (b & 64) m.notplus |= bit;
    }
    return m;
}

static Sum measure_tile(int fmt, const u8 *text, u64 len, u64 t0, u64 tile) {
    const u64 tend = t0 + tile < len ? t0 + tile : len;
    const bool ls = t0 == 0 || text[t0 - 1] == '\n';
    FaState fa = fa_begin(ls, 2, 0, 0);
    FqState fq = fq_begin(ls);
    for (u64 g = t0; g < tend; g += 64) {
        const Masks m = masks_of(fmt, text, g, tend, true);
        if (fmt == FASTA) { Out o; fa_step(fa, m, g, o); } else fq_measure_step(fq, m, g);
    }
    return fmt == FASTA ? fa_sum(fa) : fq.s;
}

static Sum tree_fold(const std::vector<Sum> &v, size_t a, size_t b) {
    if (b - a == 1) return v[a];
    const size_t mid = a + (b - a) / 2;
    return sum_combine(tree_fold(v, a, mid), tree_fold(v, mid, b));
}
static bool same(const Sum &a, const Sum &b) {
    return a.kept == b.kept && a.last_rs1 == b.last_rs1 && a.last_nl1 == b.last_nl1 && a.recs == b.recs && a.nl == b.nl && a.head_kept == b.head_kept &&
           a.ls_res == b.ls_res && a.fe_has == b.fe_has && !memcmp(a.cnt, b.cnt, 16) && !memcmp(a.fe_l, b.fe_l, 16) && !memcmp(a.fe_w, b.fe_w, 16) &&
           !memcmp(a.badmin, b.badmin, 16);
}

extern "C" {

// res8: n, bases, consumed, handover, full, too_big, "left fold == balanced tree == folds of three uneven parts", tiles
// out: ordinals (cap free), off (cap allowed + 1, window coordinates), hdr (2 per record)
int rs_parse(int fmt, const u8 *text, u64 len, int eof, u64 tile, u64 allowed, u64 free_, u8 *out, u64 *off, u64 *hdr, u64 *res8) {
    if (!len || !tile) return -1;
    const u64 nt = (len + tile - 1) / tile;
    std::vector<Sum> sums(nt);
    for (u64 t = 0; t < nt; t++) sums[t] = measure_tile(fmt, text, len, t * tile, tile);
    // scan
    std::vector<Carry> carry(nt);
    Sum S = sum_identity();
    for (u64 t = 0; t < nt; t++) S = sum_combine(S, sums[t]);
    const Sum total = S;
    bool grouping_ok = same(total, tree_fold(sums, 0, nt));
    if (nt >= 3) {
        const size_t a = nt / 5 + 1, b = nt - nt / 3;
        Sum p0 = sum_identity(), p1 = sum_identity(), p2 = sum_identity();
        for (size_t t = 0; t < a; t++) p0 = sum_combine(p0, sums[t]);
        for (size_t t = a; t < b; t++) p1 = sum_combine(p1, sums[t]);
        for (size_t t = b; t < nt; t++) p2 = sum_combine(p2, sums[t]);
        grouping_ok = grouping_ok && same(total, sum_combine(p0, sum_combine(p1, p2))) && same(total, sum_combine(sum_combine(p0, p1), p2));
    }
    Limits L; L.fmt = fmt; L.eof = eof ? 1u : 0u; L.len = len; L.allowed = allowed; L.free = free_;
    const Plan P = plan_of(L, total);
    S = sum_identity();
    u64 b1 = ~0ULL, b2 = ~0ULL;
    for (u64 t = 0; t < nt; t++) {
        Carry c = carry_of(S);
        if (fmt != FASTA) c.kept = S.cnt[1];
        carry[t] = c;
        if (tile_candidate(L, P, S, sums[t])) { b2 = b1; b1 = t; }
        S = sum_combine(S, sums[t]);
    }
    Take tk; tk.n = 0; tk.bases = 0; tk.found = 0;
    for (u64 sel : {b1, b2}) {
        if (sel == ~0ULL || tk.found) continue;
        const u64 t0 = sel * tile, tend = t0 + tile < len ? t0 + tile : len;
        const Carry c = carry[sel];
        const bool ls = t0 == 0 || text[t0 - 1] == '\n';
        FaState fa = fa_begin(ls, c.st, c.kept, c.rec);
        FqEmit fq{c.kept, c.nl, ls ? 1u : 0u};
        for (u64 g = t0; g < tend; g += 64) {
            const Masks m = masks_of(fmt, text, g, tend, false);
            const u64 kept0 = fmt == FASTA ? fa.kept : fq.kept, rec0 = fa.recs;
            const u32 line0 = fq.l;
            Out o;
            if (fmt == FASTA) fa_step(fa, m, g, o); else fq_emit_step(fq, m, o);
            take_group(L, P, o, m, rec0, line0, kept0, tk);
        }
    }
    if (!tk.found) return -2;
    Result R = result_of(L, P, tk);
    off[R.n] = R.bases;
    // emit
    const u64 n = R.n, bases = R.bases;
    for (u64 t = 0; t < nt; t++) {
        const u64 t0 = t * tile, tend = t0 + tile < len ? t0 + tile : len;
        const Carry c = carry[t];
        const bool ls = t0 == 0 || text[t0 - 1] == '\n';
        FaState fa = fa_begin(ls, c.st, c.kept, c.rec);
        FqEmit fq{c.kept, c.nl, ls ? 1u : 0u};
        for (u64 g = t0; g < tend; g += 64) {
            const Masks m = masks_of(fmt, text, g, tend, false);
            const u64 kept0 = fmt == FASTA ? fa.kept : fq.kept, rec0 = fa.recs;
            const u32 line0 = fq.l;
            Out o;
            if (fmt == FASTA) fa_step(fa, m, g, o); else fq_emit_step(fq, m, o);
            for (u32 lane = 0; lane < 64 && g + lane < tend; lane++) {
                const u64 bit = 1ULL << lane, pos = g + lane;
                const u64 idx = kept0 + popc(o.base & below(lane));
                if ((o.base & bit) && idx < bases) out[idx] = ordinal(text[pos]);
                if ((o.rs | o.hdr) & bit) {
                    const u64 k = fmt == FASTA ? rec0 + popc(o.rs & (below(lane) | bit)) - 1 : (u64)(line0 + popc(m.nl & below(lane))) / 4;
                    if (o.rs & bit) {
                        if (k < n) { off[k] = idx; hdr[2 * k] = pos + 1; }
                        else if (k == n) R.consumed = pos;
                    }
                    if (k < n) {
                        if (m.nl & bit) hdr[2 * k + 1] = pos;
                        else if (pos + 1 == len) hdr[2 * k + 1] = len;
                    }
                }
            }
        }
    }
    res8[0] = R.n; res8[1] = R.bases; res8[2] = R.consumed == ~0ULL ? len : R.consumed; res8[3] = R.handover; res8[4] = R.full; res8[5] = R.too_big;
    res8[6] = grouping_ok; res8[7] = nt;
    return 0;
}

}  // extern "C"

#ifdef RS_MAIN
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<u8> text;
    u8 buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + got);
    fclose(f);
    const u64 tile = strtoull(argv[2], nullptr, 10), max_reads = 64, cap = 40000;
    const int fmt = text.size() && text[0] == '>' ? FASTA : FASTQ;
    std::vector<u8> out(cap);
    std::vector<u64> off(max_reads + 1), hdr(2 * max_reads);
    u64 pos = 0, records = 0, bases = 0, sum = 0, blocks = 0, res[8];
    while (pos < text.size()) {                       // block after block, each from one window to the end of the file
        if (rs_parse(fmt, text.data() + pos, text.size() - pos, 1, tile, max_reads, cap, out.data(), off.data(), hdr.data(), res)) return 3;
        if (!res[6]) return 4;
        for (u64 i = 0; i < res[1]; i++) sum += out[i];
        for (u64 k = 0; k < res[0]; k++) sum += hdr[2 * k + 1] - hdr[2 * k];
        records += res[0]; bases += res[1]; pos += res[2]; blocks++;
        if (res[3] || (res[0] == 0 && !res[4])) break;
        if (res[5]) return 5;
    }
    printf("%llu records %llu bases %llu blocks checksum %llu stopped at %llu of %llu\n", (unsigned long long)records, (unsigned long long)bases,
           (unsigned long long)blocks, (unsigned long long)sum, (unsigned long long)pos, (unsigned long long)text.size());
    return 0;
}
#endif
