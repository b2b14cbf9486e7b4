// lnr_window_hd.h -- the host decisions of the reader's GPU twin (lnr_reader_next_dev in lnr_reader.cpp): how large the next window is, what
// a parsed window means for the loop, how the BGZF chain moves on.  Pure functions over plain values, no HIP and no zlib:
// tests/window_decide_main.cpp runs them under the address and undefined-behaviour sanitizers (tests/test_window_decide_cpu.py).
#pragma once
#include <stdint.h>
#include <vector>

namespace lnr_win {

constexpr uint64_t WINDOW_MAX = 1ULL << 30, WINDOW_CAP = 256ULL << 20;      // bytes of text a window may hold, and holds by default (LNR_READER_GPU_WINDOW)

// Bytes of text to ask the source for: what the free bases can take as text (a FASTA base is one byte of text, anything else at most two),
// but no more than the records still allowed will probably need -- by the bytes per record seen so far (a first window guesses 1 KiB per
// record; a window that runs out is followed by the next one).  `grow` doubles for a window that held no whole record.
inline uint64_t window_size(uint64_t free_bases, uint64_t allowed, bool fasta, uint64_t g_text, uint64_t g_recs, uint64_t cap, uint64_t grow) {
    uint64_t want = free_bases * (fasta ? 1 : 2) + free_bases / 50 + allowed * 128 + 65536;
    const uint64_t per_rec = g_recs ? g_text / g_recs + 1 : 1024;
    const uint64_t by_recs = allowed * (per_rec + per_rec / 8) + 65536;
    if (want > by_recs) want = by_recs;
    if (want > cap) want = cap;
    want *= grow;
    return want > WINDOW_MAX ? WINDOW_MAX : want;
}

// ---- what a parsed window means.  The four sources of text and the two record forms make five sites; what differs between them is named here
enum Site { GZIP_TEXT, BGZF_TEXT, BGZF_BAM, STREAM_BAM, HOST_TEXT };     // HOST_TEXT: the mapped file or an inflate stream, text records
struct Seen {
    Site site;
    bool handover, too_big, full;        // from the parse: the serial parser takes the rest of the file; the next record does not fit the block (too_big: and never will)
    uint64_t n_block;            // records in the block, this window's included
    bool parsed;                 // a parse ran (device text: not over blanks alone)
    uint64_t taken, consumed;    // records the window gave, text bytes it used up
    uint64_t len, left;          // bytes the window held (STREAM_BAM: the header in front of the records included), and those it leaves to the next window
    bool ended;                  // the source has nothing behind this window
    bool live;                   // the source is still the reader's: BGZF gives way to the gzip rounds or to gzread at a member that is not BGZF
    bool stuck;                  // GZIP_TEXT: the device text is full, no round can add to it
    bool failed;                 // GZIP_TEXT: the member's data is bad behind this text; the records in front of it are delivered first
};
enum Verdict {
    NEXT_WINDOW, GROW_WINDOW,    // go on (GROW_WINDOW: with the window doubled)
    BLOCK_FULL, SOURCE_END,      // the block ends here
    HAND_OVER,                   // the serial parser fills the rest of the block
    ERR_BLOCK, ERR_WINDOW,       // LNR_ERR_LIMIT: "a record is longer than the block" / "... than the reader's window"
    ERR_SOURCE                   // LNR_ERR_ARG with the source's own message
};
inline Verdict decide(const Seen &s) {
    if (s.handover) return s.failed ? ERR_SOURCE : HAND_OVER;             // looked at before too_big: that record is the serial parser's to judge
    if (s.too_big && s.n_block == 0) return ERR_BLOCK;
    if (s.full) return BLOCK_FULL;
    if (s.ended && s.left == 0) return s.failed && s.n_block == 0 ? ERR_SOURCE : SOURCE_END;
    bool nothing = s.taken == 0 && s.live;                                // (a source that has just given way starts afresh with the next window)
    bool cannot_grow = s.len >= WINDOW_MAX;                               // text that came through gzread or lies in the mapped file
    switch (s.site) {
    case GZIP_TEXT: nothing = nothing && s.parsed; cannot_grow = s.stuck || s.ended; break;       // blanks alone were used up; the rounds have no more room, or no more data
    case BGZF_TEXT: nothing = nothing && s.parsed; cannot_grow = s.len + 65536 > WINDOW_MAX; break;   // blanks alone were used up; the chain grows by whole blocks of up to 64 KiB
    case BGZF_BAM: nothing = nothing && s.consumed == 0; cannot_grow = s.len + 65536 > WINDOW_MAX; break;   // records that are not delivered are progress too
    case STREAM_BAM: nothing = nothing && s.consumed == 0; break;
    case HOST_TEXT: break;                                                // (the window starts at a record start and a parse always ran)
    }
    if (!nothing) return NEXT_WINDOW;
    if (!cannot_grow) return GROW_WINDOW;
    return s.failed ? ERR_SOURCE : ERR_WINDOW;
}

// ---- the BGZF chain: the blocks whose text lies on the device and is not used up; byte 0 of the device text = byte skip of chain[0]'s text
struct Block { uint64_t off; uint32_t size, isize; };    // file offset, compressed size, text size (never 0: empty blocks do not join the chain)
// the window used up adv bytes of the device text: they leave the chain with the blocks they cover
inline void chain_advance(std::vector<Block> &chain, uint64_t &skip, uint64_t adv) {
    skip += adv;
    uint64_t gone = 0;
    while (gone < chain.size() && skip >= chain[gone].isize) skip -= chain[gone++].isize;
    chain.erase(chain.begin(), chain.begin() + (long)gone);
}

}  // namespace lnr_win
