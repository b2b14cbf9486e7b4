// lnr_reader_kernels.hip -- the GPU side of the reader (lnr_reader_next_dev): FASTA / FASTQ text -> Dna5 ordinals back to back + read
// offsets in HBM.  gfx950, wave64.  Every decision comes from lnr_reader_hd.h, the same text the CPU test pins.
//
// Three steps per window of text, on the reader's own stream:
//   k_rd_measure   one workgroup = one wave per tile of RD_TILE bytes: the tile goes to LDS by 16-byte loads, the wave walks it in groups
//                  of 64 bytes, lane = byte; the byte classes are wave ballots, the counts popcounts of them; one Sum per tile
//   k_rd_scan      one workgroup: every thread folds its share of the tile summaries, the shares are scanned, every tile gets the state at
//                  its first byte (Carry); then the take is decided on the device (lnr_rd::plan_of / take_group / result_of): the wave
//                  looks once more at the one tile that holds the last record start within the limits
//   k_rd_emit      the walk again with the carried state: a base lane stores its ordinal at (bases before it) -- position by ballot and
//                  prefix popcount, guarded by the number of bases the scan chose; a record-start lane stores off[k] and the header begin,
//                  the lane of a header's '\n' the header end.  No atomics; the only divergence is on lanes that hold a record boundary.
// The text of a mapped file is pageable: it goes up through two pinned staging buffers that host threads fill in turn, and the tiles of a
// chunk are measured while the next chunk is copied.  A gzip file is inflated straight into ONE pinned buffer by the caller, the whole window
// before its copy starts: the inflate is serial and takes over 95 % of such a call, so a second buffer would hide next to nothing.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "lnr_reader_hd.h"
#include "lnr_reader_hook.h"
#if defined(__HIP_DEVICE_COMPILE__)
#define LNR_INFLATE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))      // the decoder's state is the same in every lane
#endif
#include "lnr_inflate_hd.h"

namespace {

using namespace lnr_rd;

constexpr u32 RD_TILE = 4096;                  // bytes of text per workgroup
constexpr u32 SCAN_THREADS = 256;
constexpr u64 RD_CHUNK = 16ULL << 20;          // bytes per staging buffer (a multiple of RD_TILE)

__device__ __forceinline__ void load_tile(const u8 *text, u64 t0, u8 *lds) {        // the buffer is padded to whole tiles
    const uint4 *src = reinterpret_cast<const uint4 *>(text + t0);
    for (u32 i = threadIdx.x & 63; i < RD_TILE / 16; i += 64) reinterpret_cast<uint4 *>(lds)[i] = src[i];
    __syncthreads();
}
__device__ __forceinline__ Masks group_masks(int fmt, u32 bits) {
    Masks m;
    m.valid = __ballot(bits & 1u); m.nl = __ballot(bits & 2u); m.keep = __ballot(bits & 8u);
    m.gt = 0; m.wsbad = 0; m.notat = 0; m.notplus = 0;
    if (fmt == FASTA) m.gt = __ballot(bits & 4u);
    else { m.wsbad = __ballot(bits & 16u); m.notat = __ballot(bits & 32u); m.notplus = __ballot(bits & 64u); }
    return m;
}

__global__ __launch_bounds__(64) void k_rd_measure(const u8 *text, u64 len, int fmt, u32 tile0, Sum *sums) {
    __shared__ __attribute__((aligned(16))) u8 lds[RD_TILE];
    const u32 lane = threadIdx.x, tile = tile0 + blockIdx.x;
    const u64 t0 = (u64)tile * RD_TILE, tend = t0 + RD_TILE < len ? t0 + RD_TILE : len;
    load_tile(text, t0, lds);
    u8 prevc = t0 ? text[t0 - 1] : (u8)'\n';
    FaState fa = fa_begin(prevc == '\n', 2, 0, 0);
    FqState fq = fq_begin(prevc == '\n');
    for (u64 g = t0; g < tend; g += 64) {
        const u32 o = (u32)(g - t0) + lane;
        const u8 c = lds[o], p = lane ? lds[o - 1] : prevc;
        const Masks m = group_masks(fmt, g + lane < tend ? byte_bits(fmt, c, p) : 0u);
        if (fmt == FASTA) { Out out; fa_step(fa, m, g, out); }
        else fq_measure_step(fq, m, g);
        prevc = lds[(u32)(g - t0) + 63];
    }
    if (lane == 0) sums[tile] = fmt == FASTA ? fa_sum(fa) : fq.s;
}

struct ScanArgs { const u8 *text; const Sum *sums; Carry *carry; u32 nt; Limits L; Result *res; u64 *d_off; u64 rec_base, base_base; };

// record starts of tile `tile` against the limits (one wave)
__device__ void take_tile(const ScanArgs &A, const Plan &P, u32 tile, const Carry &c, const u8 *lds, Take &t) {
    const u32 lane = threadIdx.x & 63;
    const u64 t0 = (u64)tile * RD_TILE, tend = t0 + RD_TILE < A.L.len ? t0 + RD_TILE : A.L.len;
    const u8 prevc = t0 ? A.text[t0 - 1] : (u8)'\n';
    FaState fa = fa_begin(prevc == '\n', c.st, c.kept, c.rec);
    FqEmit fq{c.kept, c.nl, prevc == '\n' ? 1u : 0u};
    for (u64 g = t0; g < tend; g += 64) {
        const u8 ch = lds[(u32)(g - t0) + lane];
        const Masks m = group_masks(A.L.fmt, g + lane < tend ? byte_bits(A.L.fmt, ch, 0) & 15u : 0u);
        const u64 kept0 = A.L.fmt == FASTA ? fa.kept : fq.kept, rec0 = fa.recs;
        const u32 line0 = fq.l;
        Out o;
        if (A.L.fmt == FASTA) fa_step(fa, m, g, o); else fq_emit_step(fq, m, o);
        take_group(A.L, P, o, m, rec0, line0, kept0, t);
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_rd_scan(ScanArgs A) {
    __shared__ Sum part[SCAN_THREADS];
    __shared__ Sum total;
    __shared__ u32 best[SCAN_THREADS][2];
    __shared__ u32 sel[2];
    __shared__ __attribute__((aligned(16))) u8 lds[RD_TILE];
    const u32 t = threadIdx.x, chunk = (A.nt + SCAN_THREADS - 1) / SCAN_THREADS;
    const u32 lo = (u64)t * chunk < A.nt ? t * chunk : A.nt, hi = lo + chunk < A.nt ? lo + chunk : A.nt;
    Sum S = sum_identity();
    for (u32 i = lo; i < hi; i++) S = sum_combine(S, A.sums[i]);
    part[t] = S;
    __syncthreads();
    if (t == 0) {
        Sum run = sum_identity();
        for (u32 i = 0; i < SCAN_THREADS; i++) { const Sum v = part[i]; part[i] = run; run = sum_combine(run, v); }
        total = run;
    }
    __syncthreads();
    const Plan P = plan_of(A.L, total);
    S = part[t];
    u32 b1 = NONE, b2 = NONE;
    for (u32 i = lo; i < hi; i++) {
        const Sum T = A.sums[i];
        Carry c = carry_of(S);
        if (A.L.fmt != FASTA) c.kept = S.cnt[1];
        A.carry[i] = c;
        if (tile_candidate(A.L, P, S, T)) { b2 = b1; b1 = i; }
        S = sum_combine(S, T);
    }
    best[t][0] = b1; best[t][1] = b2;
    __syncthreads();
    if (t == 0) {                                    // the last two candidate tiles (shares are in tile order)
        u32 s0 = NONE, s1 = NONE;
        for (int i = SCAN_THREADS - 1; i >= 0 && s1 == NONE; i--)
            for (int k = 0; k < 2; k++) {
                const u32 v = best[i][k];
                if (v == NONE) continue;
                if (s0 == NONE) s0 = v; else if (s1 == NONE) s1 = v;
            }
        sel[0] = s0; sel[1] = s1;
    }
    __syncthreads();
    Take tk; tk.n = 0; tk.bases = 0; tk.found = 0;
    for (int k = 0; k < 2; k++) {                    // one wave looks at the text of the chosen tile (every wave keeps to the barriers)
        const u32 tile = sel[k];
        if (tile == NONE) break;
        load_tile(A.text, (u64)tile * RD_TILE, lds);
        if (t < 64 && !tk.found) take_tile(A, P, tile, A.carry[tile], lds, tk);
        __syncthreads();
    }
    if (t == 0) {
        const Result r = result_of(A.L, P, tk);
        *A.res = r;
        A.d_off[A.rec_base + r.n] = A.base_base + r.bases;
    }
}

struct EmitArgs { const u8 *text; u64 len; int fmt; const Carry *carry; Result *res; u64 rec_base, base_base; u8 *out; u64 *d_off; u64 *hdr; };

__global__ __launch_bounds__(64) void k_rd_emit(EmitArgs A) {
    __shared__ __attribute__((aligned(16))) u8 lds[RD_TILE];
    const u32 lane = threadIdx.x, tile = blockIdx.x;
    const u64 t0 = (u64)tile * RD_TILE, tend = t0 + RD_TILE < A.len ? t0 + RD_TILE : A.len;
    const u64 n = A.res->n, bases = A.res->bases;
    const Carry c = A.carry[tile];
    if (c.kept >= bases && (A.fmt == FASTA ? c.rec : c.nl / 4) > n) return;      // the whole tile lies behind the take
    load_tile(A.text, t0, lds);
    const u8 prevc = t0 ? A.text[t0 - 1] : (u8)'\n';
    FaState fa = fa_begin(prevc == '\n', c.st, c.kept, c.rec);
    FqEmit fq{c.kept, c.nl, prevc == '\n' ? 1u : 0u};
    const u64 bit = 1ULL << lane;
    for (u64 g = t0; g < tend; g += 64) {
        const u8 ch = lds[(u32)(g - t0) + lane];
        const u64 pos = g + lane;
        const Masks m = group_masks(A.fmt, pos < tend ? byte_bits(A.fmt, ch, 0) & 15u : 0u);
        const u64 kept0 = A.fmt == FASTA ? fa.kept : fq.kept, rec0 = fa.recs;
        const u32 line0 = fq.l;
        Out o;
        if (A.fmt == FASTA) fa_step(fa, m, g, o); else fq_emit_step(fq, m, o);
        const u64 idx = kept0 + popc(o.base & below(lane));
        if ((o.base & bit) && idx < bases) A.out[A.base_base + idx] = ordinal(ch);
        if ((o.rs | o.hdr) & bit) {                                              // lanes on a record boundary or in a header
            const u64 k = A.fmt == FASTA ? rec0 + popc(o.rs & (below(lane) | bit)) - 1 : (u64)(line0 + popc(m.nl & below(lane))) / 4;
            if (o.rs & bit) {
                if (k < n) { A.d_off[A.rec_base + k] = A.base_base + idx; A.hdr[2 * k] = pos + 1; }
                else if (k == n) A.res->consumed = pos;
            }
            if (k < n) {
                if (m.nl & bit) A.hdr[2 * k + 1] = pos;
                else if (pos + 1 == A.len) A.hdr[2 * k + 1] = A.len;
            }
        }
    }
}

// ---- BGZF: one wave inflates one block (lnr_inflate_hd.h) straight into the window's text in global memory.  Every lane runs the decoder
// with the same values (bit buffer, code tables in LDS); lane 0 stores literals, all lanes copy a match: byte i of it comes from byte
// (i mod distance) of the source, all of which the wave has stored before.  A workgroup-scope fence stands between those stores and the
// loads: on gfx950 it needs no vmcnt wait (a CU performs one wave's vector memory operations in issue order through its one L1, so the
// load sees the store), and it keeps the compiler from reordering them.  Then 64 slices of the text are CRC'd, one per lane, and combined.
struct WaveSink {
    u8 *out; u32 lane;
    __device__ void lit(u32 pos, u8 b) { if (lane == 0) out[pos] = b; }
    __device__ void match(u32 pos, u32 len, u32 dist) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const u8 *src = out + (pos - dist);
        for (u32 i = lane; i < len; i += 64) out[pos + i] = src[dist >= len ? i : i % dist];
    }
    __device__ void stored(u32 pos, const u8 *src, u32 n) { for (u32 i = lane; i < n; i += 64) out[pos + i] = src[i]; }
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(const u8 *comp, u64 comp_len, const lnr_rdgpu_bgzf_blk *tab, u32 nblk, u8 *text, u64 text_cap, u32 *status) {
    __shared__ lnr_inf::Tables T;
    const u32 b = blockIdx.x, lane = threadIdx.x;
    if (b >= nblk) return;
    const lnr_rdgpu_bgzf_blk B = tab[b];
    u32 st;
    if (B.coff > comp_len || B.clen > comp_len - B.coff || B.ooff > text_cap || B.isize > text_cap - B.ooff) st = lnr_inf::E_TABLE;
    else {
        WaveSink o{text + B.ooff, lane};
        st = lnr_inf::inflate_block(comp + B.coff, B.clen, o, B.isize, T);
        if (st == lnr_inf::OK) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            const u32 S = (B.isize + 63) / 64, a = lane * S < B.isize ? lane * S : B.isize, e = a + S < B.isize ? a + S : B.isize;
            u32 x = lnr_inf::crc_shift(lnr_inf::crc_of(o.out + a, e - a), B.isize - e);
            for (int d = 32; d; d >>= 1) x ^= (u32)__shfl_xor((int)x, d, 64);
            if (x != B.crc) st = lnr_inf::E_CRC;
        }
    }
    if (lane == 0) status[b] = st;
}

// header bytes of the taken records -> one run of bytes the host reads (one wave per record); trailing '\r' dropped as the host parser does
__global__ __launch_bounds__(64) void k_rd_gather(const u8 *text, u64 len, const u64 *hdr, const u64 *dst_off, u64 n, u8 *dst, u64 dst_cap, u32 *lens) {
    const u64 k = blockIdx.x;
    if (k >= n) return;
    const u32 lane = threadIdx.x;
    const u64 hb = hdr[2 * k], o = dst_off[k];
    u64 he = hdr[2 * k + 1];
    if (hb > he || he > len || o > dst_cap || he - hb > dst_cap - o) { if (lane == 0) lens[k] = ~0u; return; }
    while (he > hb && text[he - 1] == '\r') he--;
    for (u64 i = lane; i < he - hb; i += 64) dst[o + i] = text[hb + i];
    if (lane == 0) lens[k] = (u32)(he - hb);
}

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Buf { void *p = nullptr; u64 cap = 0; };
struct Pin { void *p = nullptr; u64 cap = 0; };
struct Block { Buf reads, off; Pin h_off; };

}  // namespace

struct lnr_rdgpu {
    int device = 0;
    u32 slots = 0;
    hipStream_t st = nullptr, s_copy = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> ev_m;               // pairs around the measure launches of a window
    Buf text, sums, carry, hdr, res;
    Pin up[2], stage, h_res, h_hdr;
    Block blk[8];
    double ms[5] = {0, 0, 0, 0, 0};
    // BGZF: compressed bytes, block table, status per block, a buffer for moves that overlap, the gathered headers
    Buf comp, btab, bstat, move, idoff, idbytes, idlen;
    Pin h_btab, h_bstat, h_head, h_idoff, h_idbytes, h_idlen;
    hipEvent_t ev_i[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms_inf[2] = {0, 0};
};

namespace {

struct DeviceGuard {                            // every entry leaves the caller's current device as it found it
    int prev = -1;
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define RD_CK(call, status)                                                                                              \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) { snprintf(err, err_cap, "%s: %s", #call, hipGetErrorString(e_)); return (status); } } while (0)

int dev_need(Buf &b, u64 bytes, char *err, size_t err_cap) {
    if (bytes <= b.cap) return 0;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const u64 want = bytes + bytes / 4 + 256;
    RD_CK(hipMalloc(&b.p, want), -4);
    b.cap = want;
    return 0;
}
bool pin_need(Pin &b, u64 bytes) {
    if (bytes <= b.cap) return true;
    if (b.p) { (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
    const u64 want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&b.p, want, hipHostMallocDefault) != hipSuccess) { b.p = nullptr; return false; }
    b.cap = want;
    return true;
}
void par_copy(void *dst, const void *src, u64 n, u32 threads) {
    if (threads < 2 || n < (1u << 20)) { memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    const u64 share = (n + threads - 1) / threads;
    for (u32 t = 1; t < threads; t++) {
        const u64 a = share * t < n ? share * t : n, b = a + share < n ? a + share : n;
        if (b > a) th.emplace_back([=] { memcpy((char *)dst + a, (const char *)src + a, b - a); });
    }
    memcpy(dst, src, share < n ? share : n);
    for (auto &x : th) x.join();
}
void free_all(lnr_rdgpu *g) {
    for (Buf *b : {&g->text, &g->sums, &g->carry, &g->hdr, &g->res, &g->comp, &g->btab, &g->bstat, &g->move, &g->idoff, &g->idbytes, &g->idlen}) if (b->p) (void)hipFree(b->p);
    for (Pin *b : {&g->up[0], &g->up[1], &g->stage, &g->h_res, &g->h_hdr, &g->h_btab, &g->h_bstat, &g->h_head, &g->h_idoff, &g->h_idbytes, &g->h_idlen}) if (b->p) (void)hipHostFree(b->p);
    for (hipEvent_t e : g->ev_i) if (e) (void)hipEventDestroy(e);
    for (Block &b : g->blk) { if (b.reads.p) (void)hipFree(b.reads.p); if (b.off.p) (void)hipFree(b.off.p); if (b.h_off.p) (void)hipHostFree(b.h_off.p); }
    for (hipEvent_t e : g->ev_up) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev_m) if (e) (void)hipEventDestroy(e);
    if (g->st) (void)hipStreamDestroy(g->st);
    if (g->s_copy) (void)hipStreamDestroy(g->s_copy);
}

// scan + emit over the window's text in g->text (measured already: nchunk pairs of events), results and header spans to the host
int scan_emit(lnr_rdgpu *g, const lnr_rdgpu_window *w, u32 nt, u64 nchunk, u64 max_rec, lnr_rdgpu_result *r, char *err, size_t err_cap) {
    Block &b = g->blk[w->slot];
    u8 *d_text = (u8 *)g->text.p;
    double t0;
    // ---- scan + emit
    ScanArgs SA;
    SA.text = d_text; SA.sums = (const Sum *)g->sums.p; SA.carry = (Carry *)g->carry.p; SA.nt = nt;
    SA.L.fmt = w->fmt; SA.L.eof = w->eof ? 1u : 0u; SA.L.len = w->len; SA.L.allowed = w->allowed; SA.L.free = w->free;
    SA.res = (Result *)g->res.p; SA.d_off = (u64 *)b.off.p; SA.rec_base = w->rec_base; SA.base_base = w->base_base;
    EmitArgs EA;
    EA.text = d_text; EA.len = w->len; EA.fmt = w->fmt; EA.carry = (const Carry *)g->carry.p; EA.res = (Result *)g->res.p;
    EA.rec_base = w->rec_base; EA.base_base = w->base_base; EA.out = (u8 *)b.reads.p; EA.d_off = (u64 *)b.off.p; EA.hdr = (u64 *)g->hdr.p;
    RD_CK(hipEventRecord(g->ev[0], g->st), -3);
    hipLaunchKernelGGL(k_rd_scan, dim3(1), dim3(SCAN_THREADS), 0, g->st, SA);
    RD_CK(hipEventRecord(g->ev[1], g->st), -3);
    hipLaunchKernelGGL(k_rd_emit, dim3(nt), dim3(64), 0, g->st, EA);
    RD_CK(hipEventRecord(g->ev[2], g->st), -3);
    RD_CK(hipMemcpyAsync(g->h_res.p, g->res.p, sizeof(Result), hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    RD_CK(hipGetLastError(), -3);
    t0 = wall_ms();
    const Result R = *(const Result *)g->h_res.p;
    if (R.n > max_rec || R.bases > w->free) { snprintf(err, err_cap, "internal: the scan took %llu records", (unsigned long long)R.n); return -8; }
    u64 *h_off = (u64 *)b.h_off.p;
    RD_CK(hipMemcpyAsync(h_off + w->rec_base, (u64 *)b.off.p + w->rec_base, 8 * (R.n + 1), hipMemcpyDeviceToHost, g->st), -3);
    if (R.n) RD_CK(hipMemcpyAsync(g->h_hdr.p, g->hdr.p, 16 * R.n, hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    g->ms[4] += wall_ms() - t0;
    float f = 0;
    for (u64 k = 0; k < nchunk; k++) { RD_CK(hipEventElapsedTime(&f, g->ev_m[2 * k], g->ev_m[2 * k + 1]), -3); g->ms[1] += f; }
    RD_CK(hipEventElapsedTime(&f, g->ev[0], g->ev[1]), -3); g->ms[2] += f;
    RD_CK(hipEventElapsedTime(&f, g->ev[1], g->ev[2]), -3); g->ms[3] += f;
    r->n = R.n; r->bases = R.bases; r->consumed = R.consumed == ~0ULL ? w->len : R.consumed;
    r->handover = R.handover; r->full = R.full; r->too_big = R.too_big;
    r->hdr = (const uint64_t *)g->h_hdr.p;
    return 0;
}

}  // namespace

extern "C" {

uint32_t lnr_rdgpu_tile(void) { return RD_TILE; }

int lnr_rdgpu_open(int32_t device, uint32_t slots, lnr_rdgpu **out, char *err, size_t err_cap) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { snprintf(err, err_cap, "no usable HIP device for the GPU reader"); return -2; }
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    if (device < 0) device = dg.prev < 0 ? 0 : dg.prev;
    if (device >= count) { snprintf(err, err_cap, "no usable HIP device %d for the GPU reader (%d present)", (int)device, count); return -2; }
    lnr_rdgpu *g = new (std::nothrow) lnr_rdgpu();
    if (!g) return -4;
    g->device = device; g->slots = slots;
    auto fail = [&](int s) { free_all(g); delete g; return s; };
    if (hipSetDevice(device) != hipSuccess) { snprintf(err, err_cap, "hipSetDevice(%d) failed", (int)device); return fail(-2); }
    auto step = [&]() -> int {
        RD_CK(hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking), -3);
        RD_CK(hipStreamCreateWithFlags(&g->s_copy, hipStreamNonBlocking), -3);
        for (hipEvent_t &e : g->ev_up) RD_CK(hipEventCreate(&e), -3);
        for (hipEvent_t &e : g->ev) RD_CK(hipEventCreate(&e), -3);
        for (hipEvent_t &e : g->ev_i) RD_CK(hipEventCreate(&e), -3);
        if (!pin_need(g->h_res, sizeof(Result))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
        return dev_need(g->res, sizeof(Result), err, err_cap);
    };
    if (int s = step()) return fail(s);
    *out = g;
    return 0;
}

int lnr_rdgpu_block(lnr_rdgpu *g, uint32_t slot, uint64_t dst_cap, uint32_t max_reads, uint8_t **d_reads, uint64_t **d_off, uint64_t **h_off,
                    char *err, size_t err_cap) {
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    RD_CK(hipSetDevice(g->device), -3);
    Block &b = g->blk[slot];
    int s;
    // 16 spare bytes behind the bases: lnr_filter_batch_dev reads none, the context's own upload keeps the same floor
    if ((s = dev_need(b.reads, dst_cap + 16, err, err_cap)) || (s = dev_need(b.off, 8ULL * (max_reads + 1ULL), err, err_cap))) return s;
    if (!pin_need(b.h_off, 8ULL * (max_reads + 1ULL))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    *d_reads = (uint8_t *)b.reads.p; *d_off = (uint64_t *)b.off.p; *h_off = (uint64_t *)b.h_off.p;
    (*h_off)[0] = 0;
    RD_CK(hipMemsetAsync(b.off.p, 0, 8, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    return 0;
}

uint8_t *lnr_rdgpu_stage(lnr_rdgpu *g, uint64_t bytes) {
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    if (hipSetDevice(g->device) != hipSuccess) return nullptr;
    return pin_need(g->stage, bytes) ? (uint8_t *)g->stage.p : nullptr;
}

int lnr_rdgpu_parse(lnr_rdgpu *g, const lnr_rdgpu_window *w, lnr_rdgpu_result *r, char *err, size_t err_cap) {
    if (!w->len || w->len > (1ULL << 30) || w->slot >= g->slots) { snprintf(err, err_cap, "internal: window of %llu bytes", (unsigned long long)w->len); return -8; }
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    RD_CK(hipSetDevice(g->device), -3);
    Block &b = g->blk[w->slot];
    const u32 nt = (u32)((w->len + RD_TILE - 1) / RD_TILE);
    const u64 max_rec = w->allowed < w->len / 2 + 1 ? w->allowed : w->len / 2 + 1;
    int s;
    if ((s = dev_need(g->text, (u64)nt * RD_TILE + 16, err, err_cap)) || (s = dev_need(g->sums, (u64)nt * sizeof(Sum), err, err_cap)) ||
        (s = dev_need(g->carry, (u64)nt * sizeof(Carry), err, err_cap)) || (s = dev_need(g->hdr, 16 * max_rec + 16, err, err_cap))) return s;
    if (!pin_need(g->h_hdr, 16 * max_rec + 16)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    if (w->base_base + w->free + 16 > b.reads.cap || 8 * (w->rec_base + w->allowed + 1) > b.off.cap) { snprintf(err, err_cap, "internal: block accounting"); return -8; }
    u8 *d_text = (u8 *)g->text.p;
    // ---- text up, measured chunk by chunk
    double t0 = wall_ms();
    const u64 nchunk = w->pinned ? 1 : (w->len + RD_CHUNK - 1) / RD_CHUNK;
    while (g->ev_m.size() < 2 * nchunk) { hipEvent_t e; RD_CK(hipEventCreate(&e), -3); g->ev_m.push_back(e); }
    if (!w->pinned) for (Pin &p : g->up) if (!pin_need(p, RD_CHUNK)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    for (u64 k = 0; k < nchunk; k++) {
        const u64 o = w->pinned ? 0 : k * RD_CHUNK, len = w->pinned ? w->len : (w->len - o < RD_CHUNK ? w->len - o : RD_CHUNK);
        const void *src = w->text + o;
        if (!w->pinned) {
            RD_CK(hipEventSynchronize(g->ev_up[k & 1]), -3);                  // the last copy out of this staging buffer has finished
            par_copy(g->up[k & 1].p, w->text + o, len, w->threads);
            src = g->up[k & 1].p;
        }
        RD_CK(hipMemcpyAsync(d_text + o, src, len, hipMemcpyHostToDevice, g->s_copy), -3);
        RD_CK(hipEventRecord(g->ev_up[k & 1], g->s_copy), -3);
        RD_CK(hipStreamWaitEvent(g->st, g->ev_up[k & 1], 0), -3);
        const u32 tile0 = (u32)(o / RD_TILE), tiles = (u32)((len + RD_TILE - 1) / RD_TILE);
        RD_CK(hipEventRecord(g->ev_m[2 * k], g->st), -3);
        hipLaunchKernelGGL(k_rd_measure, dim3(tiles), dim3(64), 0, g->st, (const u8 *)d_text, (u64)w->len, w->fmt, tile0, (Sum *)g->sums.p);
        RD_CK(hipEventRecord(g->ev_m[2 * k + 1], g->st), -3);
    }
    RD_CK(hipStreamSynchronize(g->s_copy), -3);
    g->ms[0] += wall_ms() - t0;
    return scan_emit(g, w, nt, nchunk, max_rec, r, err, err_cap);
}

// pageable host bytes -> device, through the two pinned staging buffers that host threads fill in turn; g->st waits for the last copy
static int upload_pageable(lnr_rdgpu *g, u8 *dst, const u8 *src, u64 len, u32 threads, char *err, size_t err_cap) {
    for (Pin &p : g->up) if (!pin_need(p, RD_CHUNK)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    u64 k = 0;
    for (u64 o = 0; o < len; o += RD_CHUNK, k++) {
        const u64 n = len - o < RD_CHUNK ? len - o : RD_CHUNK;
        RD_CK(hipEventSynchronize(g->ev_up[k & 1]), -3);
        par_copy(g->up[k & 1].p, src + o, n, threads);
        RD_CK(hipMemcpyAsync(dst + o, g->up[k & 1].p, n, hipMemcpyHostToDevice, g->s_copy), -3);
        RD_CK(hipEventRecord(g->ev_up[k & 1], g->s_copy), -3);
    }
    if (k) RD_CK(hipStreamWaitEvent(g->st, g->ev_up[(k - 1) & 1], 0), -3);
    return 0;
}

// device text [from, from + n) -> [to, to + n) on g->st, to < from; through g->move where the two overlap
static int move_text(lnr_rdgpu *g, u8 *text, u64 to, u64 from, u64 n, char *err, size_t err_cap) {
    if (!n || to == from) return 0;
    if (to + n <= from) { RD_CK(hipMemcpyAsync(text + to, text + from, n, hipMemcpyDeviceToDevice, g->st), -3); return 0; }
    if (int s = dev_need(g->move, n, err, err_cap)) return s;
    RD_CK(hipMemcpyAsync(g->move.p, text + from, n, hipMemcpyDeviceToDevice, g->st), -3);
    RD_CK(hipMemcpyAsync(text + to, g->move.p, n, hipMemcpyDeviceToDevice, g->st), -3);
    return 0;
}

int lnr_rdgpu_parse_bgzf(lnr_rdgpu *g, const lnr_rdgpu_bgzf *job, lnr_rdgpu_window *w, lnr_rdgpu_result *r, lnr_rdgpu_bgzf_result *br,
                         char *err, size_t err_cap) {
    *br = lnr_rdgpu_bgzf_result{};
    br->first = -1;
    *r = lnr_rdgpu_result{};
    u64 tlen = job->carry + job->new_text;
    if (!tlen || tlen > (1ULL << 30) || w->slot >= g->slots || job->comp_len > (1ULL << 31)) { snprintf(err, err_cap, "internal: window of %llu bytes", (unsigned long long)tlen); return -8; }
    if (job->keep_from + job->carry > g->text.cap) { snprintf(err, err_cap, "internal: carried text outside the buffer"); return -8; }
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    RD_CK(hipSetDevice(g->device), -3);
    int s;
    // ---- the text buffer: whole tiles; the carried text moves to its front (into a new buffer where this one is too small)
    const u64 need = ((tlen + RD_TILE - 1) / RD_TILE) * RD_TILE + 16;
    if (need > g->text.cap) {
        Buf nb;
        if ((s = dev_need(nb, need, err, err_cap))) return s;
        if (job->carry) {
            hipError_t e = hipMemcpyAsync(nb.p, (u8 *)g->text.p + job->keep_from, job->carry, hipMemcpyDeviceToDevice, g->st);
            if (e == hipSuccess) e = hipStreamSynchronize(g->st);
            if (e != hipSuccess) { (void)hipFree(nb.p); snprintf(err, err_cap, "moving the carried text: %s", hipGetErrorString(e)); return -3; }
        }
        if (g->text.p) (void)hipFree(g->text.p);
        g->text = nb;
    } else if ((s = move_text(g, (u8 *)g->text.p, 0, job->keep_from, job->carry, err, err_cap))) return s;
    u8 *d_text = (u8 *)g->text.p;
    // ---- compressed bytes and the block table up, one wave per block
    double t0 = wall_ms();
    const u32 nblk = job->nblk;
    if (nblk) {
        const u64 tb = (u64)nblk * sizeof(lnr_rdgpu_bgzf_blk);
        if ((s = dev_need(g->comp, job->comp_len + 16, err, err_cap)) || (s = dev_need(g->btab, tb, err, err_cap)) || (s = dev_need(g->bstat, 4ULL * nblk, err, err_cap))) return s;
        if (!pin_need(g->h_btab, tb) || !pin_need(g->h_bstat, 4ULL * nblk)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
        memcpy(g->h_btab.p, job->blk, tb);
        RD_CK(hipMemcpyAsync(g->btab.p, g->h_btab.p, tb, hipMemcpyHostToDevice, g->st), -3);
        RD_CK(hipMemsetAsync(g->bstat.p, 0xff, 4ULL * nblk, g->st), -3);
        if ((s = upload_pageable(g, (u8 *)g->comp.p, job->comp, job->comp_len, w->threads, err, err_cap))) return s;
        RD_CK(hipEventRecord(g->ev_i[0], g->st), -3);
        hipLaunchKernelGGL(k_bgzf_inflate, dim3(nblk), dim3(64), 0, g->st, (const u8 *)g->comp.p, (u64)job->comp_len, (const lnr_rdgpu_bgzf_blk *)g->btab.p, nblk,
                           d_text + job->carry, (u64)job->new_text, (u32 *)g->bstat.p);
        RD_CK(hipEventRecord(g->ev_i[1], g->st), -3);
        RD_CK(hipMemcpyAsync(g->h_bstat.p, g->bstat.p, 4ULL * nblk, hipMemcpyDeviceToHost, g->st), -3);
    }
    constexpr u64 HEAD = 65536;                                            // (blanks in front of the first record are used up this many per pass)
    if (!pin_need(g->h_head, HEAD)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    const u64 hl = tlen < HEAD ? tlen : HEAD;
    RD_CK(hipMemcpyAsync(g->h_head.p, d_text, hl, hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    RD_CK(hipGetLastError(), -3);
    g->ms[0] += wall_ms() - t0;
    float f = 0;
    if (nblk) {
        RD_CK(hipEventElapsedTime(&f, g->ev_i[0], g->ev_i[1]), -3); g->ms_inf[0] += f;
        const u32 *stt = (const u32 *)g->h_bstat.p;
        for (u32 k = 0; k < nblk; k++) if (stt[k]) { br->bad_blk = k; br->bad_status = stt[k]; return 0; }
    }
    // ---- a window starts at a record start: white space in front of it (the start of the file) is skipped
    const u8 *head = (const u8 *)g->h_head.p;
    u64 lead = 0;
    while (lead < hl && is_ws(head[lead])) lead++;
    br->lead = lead;
    if (lead == hl) return 0;                                              // nothing but blanks so far: the caller uses them up
    br->first = head[lead];
    if (w->fmt == 0) w->fmt = head[lead] == '>' ? FASTA : head[lead] == '@' ? FASTQ : -1;
    if (w->fmt < 0 || head[lead] != (w->fmt == FASTA ? '>' : '@')) return 0;
    if (lead) {
        if ((s = move_text(g, d_text, 0, lead, tlen - lead, err, err_cap))) return s;
        tlen -= lead;
    }
    w->len = tlen; w->text = nullptr; w->pinned = 1;
    Block &b = g->blk[w->slot];
    const u32 nt = (u32)((tlen + RD_TILE - 1) / RD_TILE);
    const u64 max_rec = w->allowed < tlen / 2 + 1 ? w->allowed : tlen / 2 + 1;
    if ((s = dev_need(g->sums, (u64)nt * sizeof(Sum), err, err_cap)) || (s = dev_need(g->carry, (u64)nt * sizeof(Carry), err, err_cap)) ||
        (s = dev_need(g->hdr, 16 * max_rec + 16, err, err_cap))) return s;
    if (!pin_need(g->h_hdr, 16 * max_rec + 16)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    if (w->base_base + w->free + 16 > b.reads.cap || 8 * (w->rec_base + w->allowed + 1) > b.off.cap) { snprintf(err, err_cap, "internal: block accounting"); return -8; }
    while (g->ev_m.size() < 2) { hipEvent_t e; RD_CK(hipEventCreate(&e), -3); g->ev_m.push_back(e); }
    RD_CK(hipEventRecord(g->ev_m[0], g->st), -3);
    hipLaunchKernelGGL(k_rd_measure, dim3(nt), dim3(64), 0, g->st, (const u8 *)d_text, (u64)tlen, w->fmt, 0u, (Sum *)g->sums.p);
    RD_CK(hipEventRecord(g->ev_m[1], g->st), -3);
    if ((s = scan_emit(g, w, nt, 1, max_rec, r, err, err_cap))) return s;
    br->parsed = 1;
    // ---- the header bytes of the taken records: their places from the spans (host), the bytes by one wave per record
    const u64 n = r->n;
    if (!pin_need(g->h_idoff, 8 * n + 8) || !pin_need(g->h_idlen, 4 * n + 4)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    u64 *ido = (u64 *)g->h_idoff.p, total = 0;
    for (u64 k = 0; k < n; k++) {
        const u64 hb = r->hdr[2 * k], he = r->hdr[2 * k + 1];
        if (hb > he || he > tlen) { snprintf(err, err_cap, "internal: header span of record %llu", (unsigned long long)k); return -8; }
        ido[k] = total; total += he - hb;
    }
    br->id_off = ido; br->id_len = (const uint32_t *)g->h_idlen.p;
    if (!pin_need(g->h_idbytes, total + 1)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    br->ids = (const char *)g->h_idbytes.p;
    if (n) {
        if ((s = dev_need(g->idoff, 8 * n, err, err_cap)) || (s = dev_need(g->idlen, 4 * n, err, err_cap)) || (s = dev_need(g->idbytes, total + 1, err, err_cap))) return s;
        RD_CK(hipMemcpyAsync(g->idoff.p, ido, 8 * n, hipMemcpyHostToDevice, g->st), -3);
        RD_CK(hipEventRecord(g->ev_i[2], g->st), -3);
        hipLaunchKernelGGL(k_rd_gather, dim3((u32)n), dim3(64), 0, g->st, (const u8 *)d_text, (u64)tlen, (const u64 *)g->hdr.p, (const u64 *)g->idoff.p, n,
                           (u8 *)g->idbytes.p, total, (u32 *)g->idlen.p);
        RD_CK(hipEventRecord(g->ev_i[3], g->st), -3);
        RD_CK(hipMemcpyAsync(g->h_idlen.p, g->idlen.p, 4 * n, hipMemcpyDeviceToHost, g->st), -3);
        if (total) RD_CK(hipMemcpyAsync(g->h_idbytes.p, g->idbytes.p, total, hipMemcpyDeviceToHost, g->st), -3);
        RD_CK(hipStreamSynchronize(g->st), -3);
        RD_CK(hipGetLastError(), -3);
        RD_CK(hipEventElapsedTime(&f, g->ev_i[2], g->ev_i[3]), -3); g->ms_inf[1] += f;
        for (u64 k = 0; k < n; k++)
            if (br->id_len[k] > r->hdr[2 * k + 1] - r->hdr[2 * k]) { snprintf(err, err_cap, "internal: gathered header of record %llu", (unsigned long long)k); return -8; }
    }
    return 0;
}

void lnr_rdgpu_inflate_times(const lnr_rdgpu *g, double *ms2) { ms2[0] = g->ms_inf[0]; ms2[1] = g->ms_inf[1]; }

int lnr_rdgpu_append(lnr_rdgpu *g, uint32_t slot, uint64_t base_base, const uint8_t *bases, uint64_t nb, uint64_t rec_base, const uint64_t *off, uint64_t n,
                     char *err, size_t err_cap) {
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    RD_CK(hipSetDevice(g->device), -3);
    Block &b = g->blk[slot];
    if (base_base + nb + 16 > b.reads.cap || 8 * (rec_base + n + 1) > b.off.cap) { snprintf(err, err_cap, "internal: block accounting"); return -8; }
    if (nb) RD_CK(hipMemcpy((u8 *)b.reads.p + base_base, bases, nb, hipMemcpyHostToDevice), -3);
    RD_CK(hipMemcpy((u64 *)b.off.p + rec_base, off, 8 * (n + 1), hipMemcpyHostToDevice), -3);
    return 0;
}

void lnr_rdgpu_times(const lnr_rdgpu *g, double *ms5) { for (int i = 0; i < 5; i++) ms5[i] = g->ms[i]; }
void lnr_rdgpu_times_reset(lnr_rdgpu *g) { for (double &m : g->ms) m = 0; g->ms_inf[0] = g->ms_inf[1] = 0; }

void lnr_rdgpu_close(lnr_rdgpu *g) {
    if (!g) return;
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    free_all(g);
    delete g;
}

}  // extern "C"
