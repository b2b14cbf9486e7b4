"""GPU (-m gpu): the team forms of the gap re-mapper -- chain DP by columns, long-row share, team sort, team join -- over everything the
project has expected values for, by libraries built with the forms' size thresholds pulled down (linear_amd/build.py GAP_VARIANTS: the same
device code, selected by small inputs).  tests/test_gap_workers_cpu.py shows on the host that these inputs select each form under each
variant's thresholds.  A library is read when linear_amd.api is imported, so each variant runs in a fresh child process
(tests/gap_variant_child.py), once with every weighted read started on a team (LNR_GAP_HEAVY_W=1) and once with every read started on a
single wave and handed over (4294967295).  Every value is an integer word: every comparison is exact, no read is left out."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gap_pool, gap_variant_inputs as vi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CHILD_TIMEOUT = 300       # the stock gap tests over the same inputs take well under a minute; a team that waits at a barrier for ever ends here


@pytest.fixture(scope="module")
def expected(oracle_lib):
    P = gap_pool.make_pool()
    want, _ = gap_pool.oracle_cords(oracle_lib, P)
    refs, reads, off = vi.sv_inputs()
    o = oracle_lib.Checker("oracle", refs, 1)
    sv = {m: o.map_batch(reads, off, threads=8, gap_len=m[0], dup=m[1])[:3] for m in vi.SV_MODES}
    o.close()
    return P, want, sv


@pytest.mark.parametrize("heavy_w", ["1", "4294967295"])
@pytest.mark.parametrize("variant", sorted(vi.THRESHOLDS))
def test_gpu_gap_variant_equals_goldens_and_oracle(expected, variant, heavy_w, tmp_path):
    from linear_amd import build as lb
    so = lb.gap_variant_path(variant)
    if not os.path.exists(so):
        lb.build(defines=lb.GAP_VARIANTS[variant], out=so, only=("lnr_gap_kernels.hip",))
    out = str(tmp_path / "cords.npz")
    env = dict(os.environ, LNR_LIB=so, LNR_GAP_HEAVY_W=heavy_w)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gap_variant_child.py"), out], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    P, want, sv = expected
    bad = []
    for name in vi.GOLDENS:
        g = np.load(os.path.join(GOLD, f"{name}_g50_T1.npz"))
        for d in (0, 1):
            t = f"golden_{name}_dup{d}"
            if not (np.array_equal(got[t + "_off"], g[f"cord_off_dup{d}"]) and np.array_equal(got[t + "_str"], g[f"cords_str_dup{d}"]) and
                    np.array_equal(got[t + "_end"], g[f"cords_end_dup{d}"]) and int(got[t + "_ext"]) == int(g[f"ext_out_dup{d}"])):
                bad.append(t)
    for m in vi.SV_MODES:
        t = f"sv_g{m[0]}_dup{m[1]}"
        if not all(np.array_equal(got[t + s], w) for s, w in zip(("_off", "_str", "_end"), sv[m])):
            bad.append(t)
    for m in gap_pool.MODES:
        t = f"pool_g{m[0]}_dup{m[1]}"
        d = gap_pool.differing(gap_pool.split(got[t + "_off"], got[t + "_str"], got[t + "_end"]), want[m])
        if d:
            bad.append((t, d[:10]))
        assert int(got[t + "_second"]) > 0, f"{t}: no read reached a team"
    assert not bad, f"variant {variant}, LNR_GAP_HEAVY_W={heavy_w}: differ from the goldens / the oracle: {bad}"
