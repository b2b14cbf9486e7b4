"""GPU (-m gpu), the shipped library: which worker of the gap re-mapper a read ends up with -- a single wave of k_gap_all, a 16-wave team
of k_gap_all (ranked heavy by k_gap_weight, or handed over), a team of the last launch k_gap_team -- does not change its result
(DESIGN.md 5c).  The pool of tests/gap_pool.py against the oracle (pinned to the real program by tests/test_oracle_golden.py) under every
setting of the knobs that decide the worker.  tests/test_gap_workers_cpu.py shows on the host what the pool's reads ask of their worker.
Every value is an integer word: every comparison is exact, and no read is left out of one."""
import numpy as np
import pytest

from tests import gap_pool
from tests.gap_pool import MODES, MODE_IDS, pack, split, differing

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(oracle_lib):
    from tests import shimlib
    P = gap_pool.make_pool()
    P.want, P.plain = gap_pool.oracle_cords(oracle_lib, P)
    P.changed = {m: len(differing(P.want[m], P.plain)) for m in MODES}
    assert all(P.changed[m] >= 10 for m in MODES), P.changed
    sh = shimlib.Shim(P.refs, P.T)
    P.arena1 = sh.gap_arena1(max(r.size for r in P.reads))
    P.hw = {m: [sh.gap_needs(r, m[0], m[1], 1)["arena_hw"] if r.size > 200 else 0 for r in P.reads] for m in MODES}
    sh.close()
    P.heaviest = int(np.argmax(P.hw[(50, 1)]))
    return P


def run(P, mode, idx):
    """the reads idx of the pool as one batch on a fresh context (stream state 1) -> the positions that differ from the oracle, the stats"""
    from linear_amd import build as lb
    lb.build()
    from linear_amd import Filter
    f = Filter(device=0, gap_len=mode[0], dup=mode[1])
    try:
        f.build_index(P.refs, P.T)
        assert f.gap_stream(1) == 1
        reads, off = pack([P.reads[i] for i in idx])
        got = split(*f.filter_batch(reads, off))
        st = f.stats()
        assert f.gap_stream() == 1
    finally:
        f.close()
    return differing(got, [P.want[mode][i] for i in idx]), st


SETTINGS = {"defaults": {}, "heavy_w_1": {"LNR_GAP_HEAVY_W": "1"}, "heavy_w_max": {"LNR_GAP_HEAVY_W": "4294967295"}, "one_team": {"LNR_GAP_TEAMS": "1"},
            "one_team_heavy_w_1": {"LNR_GAP_TEAMS": "1", "LNR_GAP_HEAVY_W": "1"}, "arena2_floor": {"LNR_GAP_ARENA2_MB": "1"}}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_gpu_gap_worker_does_not_change_the_result(pool, monkeypatch, setting, mode):
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    d, st = run(pool, mode, list(range(pool.n)))
    print(f"{setting} {mode}: gap_second_pass {st['gap_second_pass']}, gap_last_launch {st['gap_last_launch']}, reads the oracle changed {pool.changed[mode]}")
    assert not d, f"pool reads that differ from the oracle: {d}"
    if setting in ("defaults", "heavy_w_max", "one_team"):
        assert st["gap_second_pass"] > 0, "no read reached a team of the first stage"
    if SETTINGS[setting].get("LNR_GAP_HEAVY_W") == "1":
        # every read with any weight starts on a team: at least the reads whose cords the gap stage changed
        assert st["gap_second_pass"] >= pool.changed[mode], (st["gap_second_pass"], pool.changed[mode])
    if setting == "arena2_floor":
        # the team arena at its floor 2 x arena1: a read whose arena high-water mark on the host (a lower bound of the device's, which adds the
        # scratch of its parallel sorts and of the column DP) is beyond it must go through k_gap_team.  At -dup 1 nine pool reads are, on the
        # host already (tests/test_gap_workers_cpu.py pins them); at -dup 0 the largest host mark is 1 949 760 of 2 247 168 bytes and the
        # device's additions take reads over it
        beyond = [i for i, h in enumerate(pool.hw[mode]) if h > 2 * pool.arena1]
        assert st["gap_last_launch"] > 0, f"the last launch did no read; beyond a team arena of {2 * pool.arena1} bytes on the host: {beyond}"
        assert st["gap_last_launch"] >= len(beyond)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("count", [1, 2, 9, 17])
def test_gpu_gap_heavy_reads_alone(pool, count, mode):
    """G.nteams = min(nteams, max(1, m / 8)): one team up to 15 reads, two from 16"""
    order = sorted(pool.tandem, key=lambda i: -pool.hw[(50, 1)][i])
    idx = (order + order)[:count]
    d, st = run(pool, mode, idx)
    assert not d, f"batch of the {count} heaviest reads {idx}: positions that differ from the oracle: {d}"
    assert st["gap_second_pass"] > 0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_gap_worker_slots(pool, mode):
    n, h = pool.n, pool.heaviest
    rot = lambda k: [(i + k) % n for i in range(n)]          # noqa: E731
    bad = {}
    for name, idx in {"reversed": list(range(n))[::-1], "heaviest first": rot(h), "heaviest last": rot(h + 1)}.items():
        assert sorted(idx) == list(range(n))
        d, _ = run(pool, mode, idx)
        if d:
            bad[name] = [(p, idx[p]) for p in d[:10]]
    assert not bad, f"(slot, pool read) that differ from the oracle: {bad}"
