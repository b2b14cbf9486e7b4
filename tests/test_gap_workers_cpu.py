"""CPU: what the gap stage of the worker pool's reads (tests/gap_pool.py) asks of its worker, by the host account of lnr_gap_hd.h
(GapHostStats, compiled into the test-only host shim), and which team form each size threshold selects -- under the shipped thresholds and
under those of the variant libraries of tests/test_gpu_gap_variants.py.  The thresholds are passed as numbers; nothing here reads the
K_GAP_* macros.  A retuned threshold, or a change of the generator, makes these pins fail: then the inputs have to be tuned again."""
import numpy as np
import pytest

from tests import gap_pool, gap_variant_inputs as vi, shimlib

KEYS = ("dp_n", "dp_cols", "row_max", "sort_max", "join_max", "arena_hw")
# per tandem-expansion read of the pool: largest chain DP (anchors, columns), longest row, longest sort, largest join block, arena high-water mark
PINNED = {
    (50, 1): {2: (2009, 778, 245, 36688, 7140, 1387232), 5: (8291, 747, 324, 271190, 72593, 8785568), 8: (10302, 850, 435, 217473, 71760, 4642224), 11: (10229, 846, 360, 305439, 81200, 8898944), 14: (771, 206, 574, 4917, 320, 288864), 17: (913, 300, 62, 3682, 128, 217184), 20: (10910, 872, 465, 499637, 41109, 9194288), 23: (3198, 627, 161, 6416, 2988, 932672), 26: (11538, 845, 467, 278061, 71176, 8881712), 29: (3368, 731, 119, 115162, 2576, 2581648), 32: (7064, 695, 286, 336913, 93360, 8899904), 35: (1744, 741, 63, 10549, 817, 494048), 38: (10865, 867, 359, 498944, 126378, 9123488), 41: (10734, 865, 388, 238683, 39960, 4652432)},
    (50, 0): {2: (1999, 563, 245, 4477, 7140, 595488), 5: (8291, 747, 324, 13508, 72593, 1290128), 8: (10302, 850, 435, 10711, 71760, 1360656), 11: (10229, 846, 360, 10876, 62491, 1489904), 14: (579, 15, 574, 2398, 59, 136272), 17: (350, 342, 20, 3682, 128, 217184), 20: (10910, 872, 465, 16150, 41109, 1363776), 23: (3198, 627, 161, 4690, 2988, 932672), 26: (11538, 845, 467, 11978, 59122, 1827952), 29: (3368, 731, 119, 11057, 2418, 651408), 32: (7064, 695, 286, 14688, 93360, 1338800), 35: (951, 284, 63, 6949, 666, 205088), 38: (10865, 867, 359, 15550, 72072, 1342688), 41: (10734, 865, 388, 10734, 39960, 1949760)},
}
# the pool reads that select a team form at the SHIPPED thresholds: the column DP from y buckets (cmd 2) / the team join (cmd 4)
FORMS = {
    (50, 1): dict(yb=[8, 11, 20, 26, 38, 41], join=[5, 8, 11, 26, 32, 38], scan=[], row=[]),
    (50, 0): dict(yb=[8, 11, 20, 26, 38, 41], join=[5, 8, 32, 38], scan=[], row=[]),
}


@pytest.fixture(scope="module")
def pool():
    P = gap_pool.make_pool()
    P.sh = shimlib.Shim(P.refs, P.T)
    yield P
    P.sh.close()


def test_pool_shape_cpu(pool):
    assert 38 <= pool.n <= 44 and sum(r.size for r in pool.refs) <= 500_000
    assert len(pool.tandem) == len(gap_pool.ARRAYS) and pool.n - len(pool.tandem) >= 2 * len(pool.tandem)      # most reads are ordinary
    for u, c, cr, div, err, flank in gap_pool.ARRAYS:
        assert 20 <= u <= 170 and 0.02 <= div <= 0.04 and 0.05 <= err <= 0.10 and 2.5 * c <= cr <= 3.5 * c and all(1500 <= f <= 3000 for f in flank)


@pytest.mark.parametrize("mode", gap_pool.MODES, ids=gap_pool.MODE_IDS)
def test_pool_needs_under_the_shipped_thresholds_cpu(pool, mode):
    """Shipped: K_GAP_COL_MIN 1024, K_GAP_COL_MEAN 12, K_GAP_YB_MIN 4096, K_GAP_TEAM_ROW 2048, K_GAP_SORT_TEAM_MIN 4096, K_GAP_JOIN_TEAM_MIN
    65536, K_GAP_SINGLE_MAX 8192.  What the pool reaches at these: chain DPs of 10 000 anchors with 12 per column -- the column DP from y
    buckets (cmd 2; as the host counts it: a duplicate anchor in a column or a y list that does not fit the arena still sends the device
    back to the single-wave form, so the counts are upper bounds of the device's) --, join blocks of 65 536 pairs and more (the team join,
    cmd 4), sorts beyond K_GAP_SINGLE_MAX (a single wave hands the read over) and K_GAP_SORT_TEAM_MIN (the team sort, cmd 3), and at
    -dup 1 arena high-water marks beyond twice the single-wave arena (the last launch under LNR_GAP_ARENA2_MB=1).

    What no read made by this recipe reached, in some 400 reads tried with units of 20 .. 170 and 50 .. 420 copies:
    * the x-window scan form (1024 <= n < 4096 with 12 per column).  The extension's band lets a column at distance dy from the gap's end
      see the read copies within dy / 4 of the diagonal, so the anchors per column grow with the window: the densest DPs measured (12.5 per
      column, units of 20 .. 22) have 850 columns and 10 000 anchors, and every DP under 4096 anchors stayed under 8 per column.  The DPs
      of an inserted stretch (20 columns, 45 anchors each) end below 1000 anchors: their k-mer list is capped (sorts of 2398).
    * the long-row share (cmd 1): a row holds the anchors of 16 columns (dx_depth 80, every 5th reference position), so 2304 predecessors
      need 144 anchors per column where the whole DP has under 12; the longest row measured has 783.
    * at -dup 0 an arena high-water mark beyond twice the single-wave arena: the sorts of 100 000 and more elements that take a read there
      come from the duplication add-on of -dup 1 alone; the most at -dup 0 is 1 949 760 bytes against 2 247 168.
    The scan form and the long-row share are selected under the variants' thresholds (test_variant_inputs_select_every_team_form_cpu)."""
    sh = pool.sh
    need = {i: sh.gap_needs(pool.reads[i], mode[0], mode[1], 1) for i in range(pool.n) if pool.reads[i].size > 200}
    assert {i: tuple(need[i][k] for k in KEYS) for i in pool.tandem} == PINNED[mode]
    assert all(d["arena_hw"] > 0 for i, d in need.items() if i in pool.tandem)                 # every tandem read has gap work
    form = FORMS[mode]
    assert [i for i, d in need.items() if d["n_yb"]] == form["yb"] and len(form["yb"]) >= 5     # cmd 2, y buckets: n >= 4096, 12 * columns <= n
    assert all(need[i]["dp_n"] >= 4096 and 12 * need[i]["dp_cols"] <= need[i]["dp_n"] for i in form["yb"])
    assert [i for i, d in need.items() if d["n_join"]] == form["join"] and len(form["join"]) >= 3   # cmd 4
    assert all(need[i]["join_max"] >= 65536 for i in form["join"])
    assert [i for i, d in need.items() if d["n_scan"]] == form["scan"] == [] and [i for i, d in need.items() if d["n_row"]] == form["row"] == []
    assert max(d["sort_max"] for d in need.values()) >= 8192                                   # K_GAP_SINGLE_MAX: handed over
    assert sum(1 for d in need.values() if d["n_sort"]) >= 9                                  # cmd 3
    arena1 = sh.gap_arena1(max(r.size for r in pool.reads))
    assert arena1 == 1123584
    beyond = [i for i, d in need.items() if d["arena_hw"] > 2 * arena1]
    assert beyond == ([5, 8, 11, 20, 26, 29, 32, 38, 41] if mode[1] else [])
    assert [i for i, d in need.items() if d["arena_hw"] > arena1 and i not in pool.tandem] == []   # the ordinary reads fit a single wave's arena


@pytest.mark.parametrize("variant", sorted(vi.THRESHOLDS))
def test_variant_inputs_select_every_team_form_cpu(pool, variant):
    """reads of what each variant runs (planted-SV set and pool; the goldens only add to these) that select each team form under the
    variant's thresholds"""
    thr = vi.THRESHOLDS[variant]
    tot = dict(n_yb=0, n_scan=0, n_row=0, n_sort=0, n_join=0)
    refs, reads, off = vi.sv_inputs()
    sv = shimlib.Shim(refs, 1)
    sets = [(sv, [reads[int(off[i]):int(off[i + 1])] for i in range(off.size - 1)], 0), (pool.sh, pool.reads, 1)]
    for sh, rl, ext in sets:
        for r in rl:
            if r.size <= 200:
                continue
            for dup in ((1, 0) if ext else (1,)):             # the pool in both modes, the planted-SV set as the variants run it
                d = sh.gap_needs(r, 50, dup, ext, **thr)
                for k in tot:
                    tot[k] += d[k] > 0
    sv.close()
    print(variant, tot)
    assert tot["n_sort"] >= 10 and tot["n_join"] >= 5                                        # cmd 3, cmd 4
    if variant == "columns":
        assert tot["n_yb"] >= 10                                                             # cmd 2, predecessors from y buckets
    elif variant == "scan":
        assert tot["n_scan"] >= 10 and tot["n_yb"] == 0                                      # cmd 2, predecessors from the x-window scan
    else:
        assert tot["n_yb"] == 0 and tot["n_scan"] == 0 and tot["n_row"] >= 2                 # cmd 1
