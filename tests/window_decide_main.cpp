// The host decisions of the reader's GPU twin (linear_amd/csrc/lnr_window_hd.h) as a stand-alone program: no HIP, no zlib, built by g++
// with the address and undefined-behaviour sanitizers (tests/test_window_decide_cpu.py).  The expected outcomes are what the five
// hand-written exit ladders of lnr_reader_next_dev did before they became lnr_win::decide -- written down here per site, not computed
// by the function under test.
#include "../linear_amd/csrc/lnr_window_hd.h"

#include <cstdio>

using namespace lnr_win;

static int bad = 0, checks = 0;
static const char *const SITE[] = {"GZIP_TEXT", "BGZF_TEXT", "BGZF_BAM", "STREAM_BAM", "HOST_TEXT"};
static const char *const VERDICT[] = {"NEXT_WINDOW", "GROW_WINDOW", "BLOCK_FULL", "SOURCE_END", "HAND_OVER", "ERR_BLOCK", "ERR_WINDOW", "ERR_SOURCE"};

static void expect(const char *what, const Seen &s, Verdict want) {
    const Verdict got = decide(s);
    checks++;
    if (got != want) { bad++; printf("FAIL %s / %s: %s, expected %s\n", SITE[s.site], what, VERDICT[got], VERDICT[want]); }
}
static void expect_eq(const char *what, uint64_t got, uint64_t want) {
    checks++;
    if (got != want) { bad++; printf("FAIL %s: %llu, expected %llu\n", what, (unsigned long long)got, (unsigned long long)want); }
}

// a window in the middle of a file that gave records: every site goes on to the next window from here
static Seen usual(Site site) {
    Seen s{};
    s.site = site; s.n_block = 5; s.parsed = true; s.taken = 5; s.consumed = 4000; s.len = 5000; s.left = 1000; s.live = true;
    return s;
}
// ... and one that held no whole record
static Seen nothing(Site site) {
    Seen s = usual(site);
    s.n_block = 0; s.taken = 0; s.consumed = 0; s.left = s.len;
    return s;
}

int main() {
    const uint64_t G = 1ULL << 30;
    for (int k = 0; k < 5; k++) {
        const Site site = (Site)k;
        const bool bam = site == BGZF_BAM || site == STREAM_BAM, bgzf = site == BGZF_TEXT || site == BGZF_BAM;
        Seen s = usual(site);
        expect("records taken", s, NEXT_WINDOW);
        // ---- the three rules all sites share
        s = usual(site); s.full = true;
        expect("full", s, BLOCK_FULL);
        s = nothing(site); s.too_big = true; s.full = true;
        expect("too_big, empty block", s, ERR_BLOCK);
        s = usual(site); s.too_big = true; s.full = true; s.taken = 0; s.consumed = 0;
        expect("too_big behind records", s, BLOCK_FULL);
        s = nothing(site); s.handover = true; s.too_big = true; s.full = true;
        expect("hand-over before too_big", s, HAND_OVER);
        s = usual(site); s.handover = true; s.ended = true; s.left = 0;
        expect("hand-over before the end", s, HAND_OVER);
        // ---- "source exhausted": the source has ended and the window left nothing
        s = usual(site); s.ended = true; s.left = 0;
        expect("exhausted", s, SOURCE_END);
        s = usual(site); s.ended = true;
        expect("ended, text left", s, NEXT_WINDOW);
        s = nothing(site); s.ended = true; s.left = 0; s.consumed = s.len;     // (blank lines, records that are not delivered)
        expect("exhausted, nothing ever taken", s, SOURCE_END);
        // ---- "nothing taken": the window is doubled while it can be
        s = nothing(site);
        expect("nothing taken, can grow", s, GROW_WINDOW);
        if (site == GZIP_TEXT) {                         // cannot grow: stuck || gend
            s = nothing(site); s.stuck = true;
            expect("nothing taken, stuck", s, ERR_WINDOW);
            s = nothing(site); s.ended = true;
            expect("nothing taken, ended", s, ERR_WINDOW);
            s = nothing(site); s.len = s.left = G;       // (the rounds stop before: the size alone says nothing here)
            expect("nothing taken, 2^30 bytes", s, GROW_WINDOW);
        } else if (bgzf) {                               // cannot grow: tl + 65536 > 2^30
            s = nothing(site); s.len = s.left = G - 65536;
            expect("nothing taken, one more block fits", s, GROW_WINDOW);
            s = nothing(site); s.len = s.left = G - 65535;
            expect("nothing taken, no block fits", s, ERR_WINDOW);
            s = nothing(site); s.len = s.left = G - 65535; s.live = false;     // ("still BGZF": the next source starts afresh)
            expect("nothing taken, gave way", s, NEXT_WINDOW);
            s = nothing(site); s.live = false;
            expect("nothing taken, gave way, small", s, NEXT_WINDOW);
        } else {                                         // cannot grow: len >= 2^30
            s = nothing(site); s.len = s.left = G - 1;
            expect("nothing taken, below 2^30", s, GROW_WINDOW);
            s = nothing(site); s.len = s.left = G;
            expect("nothing taken, 2^30 bytes", s, ERR_WINDOW);
        }
        // what "nothing" means: text sites ask for a parse that gave no record (BGZF_TEXT, GZIP_TEXT: blanks alone are used up without
        // one), BAM sites for no record taken AND none passed over
        s = nothing(site); s.parsed = false; s.consumed = 0;
        if (site == GZIP_TEXT || site == BGZF_TEXT) expect("no parse ran", s, NEXT_WINDOW);
        s = nothing(site); s.consumed = 300; s.left = s.len - 300;
        expect("no record taken, bytes used up", s, bam ? NEXT_WINDOW : GROW_WINDOW);
    }
    // ---- GZIP_TEXT with bad data behind the text (gz_failed): LNR_ERR_ARG with the gzip message where the parent answered it
    Seen s = usual(GZIP_TEXT); s.failed = true; s.ended = true; s.left = 0;
    expect("failed, exhausted, records in the block", s, SOURCE_END);
    s = nothing(GZIP_TEXT); s.failed = true; s.ended = true; s.left = 0; s.consumed = s.len;
    expect("failed, exhausted, empty block", s, ERR_SOURCE);
    s = nothing(GZIP_TEXT); s.failed = true; s.ended = true;
    expect("failed, nothing taken", s, ERR_SOURCE);
    s = usual(GZIP_TEXT); s.failed = true; s.ended = true; s.handover = true;
    expect("failed, hand-over", s, ERR_SOURCE);
    s = usual(GZIP_TEXT); s.failed = true; s.ended = true; s.full = true;
    expect("failed, full", s, BLOCK_FULL);

    // ---- the window: free = 1000, allowed = 7, no history, default cap
    expect_eq("window FASTA", window_size(1000, 7, true, 0, 0, WINDOW_CAP, 1), 67452);        // 1000 + 20 + 896 + 65536 < 7 * 1152 + 65536 = 73600
    expect_eq("window FASTQ", window_size(1000, 7, false, 0, 0, WINDOW_CAP, 1), 68452);
    expect_eq("window FASTA grow 4", window_size(1000, 7, true, 0, 0, WINDOW_CAP, 4), 269808);
    expect_eq("window clamp", window_size(1000, 7, true, 0, 0, WINDOW_CAP, 1ULL << 20), G);
    expect_eq("window by records", window_size(1ULL << 20, 7, true, 0, 0, WINDOW_CAP, 1), 73600);
    expect_eq("window by history", window_size(1ULL << 20, 7, true, 700, 7, WINDOW_CAP, 1), 7 * (101 + 12) + 65536);
    expect_eq("window cap", window_size(1ULL << 20, 1000, false, 0, 0, 4096, 2), 8192);

    // ---- the chain: blocks of 10 / 20 / 30 bytes of text (one of no text in between never joins the chain)
    std::vector<Block> chain = {{0, 40, 10}, {68, 50, 20}, {118, 60, 30}};
    uint64_t skip = 0;
    chain_advance(chain, skip, 10);
    expect_eq("chain 10: skip", skip, 0); expect_eq("chain 10: blocks", chain.size(), 2); expect_eq("chain 10: first", chain[0].off, 68);
    chain_advance(chain, skip, 25);
    expect_eq("chain 25: skip", skip, 5); expect_eq("chain 25: blocks", chain.size(), 1); expect_eq("chain 25: first", chain[0].off, 118);
    chain_advance(chain, skip, 25);
    expect_eq("chain end: skip", skip, 0); expect_eq("chain end: blocks", chain.size(), 0);

    printf("%s checks %d failed %d\n", bad ? "FAILED" : "ok", checks, bad);
    return bad ? 1 : 0;
}
