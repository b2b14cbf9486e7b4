"""What every variant library of the gap re-mapper runs (tests/test_gpu_gap_variants.py, tests/gap_variant_child.py) and what the CPU account
checks against the variants' thresholds (tests/test_gap_workers_cpu.py): the five -g 50 goldens, the planted-SV set at -t 1, the worker pool."""
import numpy as np

GOLDENS = ["ont", "edge", "ccs_sv", "rep", "chim"]
SV_MODES = [(50, 1), (5, 1)]
# the thresholds each variant is built with, as the host account takes them: read off the -D flags of linear_amd/build.py GAP_VARIANTS (one
# table, not two), never off the code under test.  K_GAP_SINGLE_MAX decides the hand-over, not the form: the account does not take it.
MACROS = {"K_GAP_COL_MIN": "col_min", "K_GAP_COL_MEAN": "col_mean", "K_GAP_YB_MIN": "yb_min", "K_GAP_YB_MAX": "yb_max", "K_GAP_TEAM_ROW": "team_row",
          "K_GAP_SORT_TEAM_MIN": "sort_min", "K_GAP_JOIN_TEAM_MIN": "join_min", "K_GAP_SINGLE_MAX": None}


def thresholds(defines):
    kv = [d[2:].split("=") for d in defines]
    assert all(d.startswith("-D") for d in defines) and all(k in MACROS for k, _ in kv), defines
    return {MACROS[k]: int(v) for k, v in kv if MACROS[k]}


def _variants():
    from linear_amd import build as lb
    return {name: thresholds(d) for name, d in lb.GAP_VARIANTS.items()}


THRESHOLDS = _variants()


def golden_inputs(name):
    from tests import cases
    return (cases.CASES[name][0] if name in cases.CASES else cases.CASES_I2[name][0] if name in cases.CASES_I2 else cases.CASES_G50[name][0])()


def sv_inputs():
    from linear_amd import synth
    from tests.test_gap_shim_cpu import sv_reads
    refs = [synth.repeat_ref(300_000, 61), synth.add_n_runs(synth.random_ref(200_000, 62), 63, n_runs=2, max_run=600)]
    rl = sv_reads(refs, 96, 2028)
    off = np.zeros(len(rl) + 1, np.uint64)
    off[1:] = np.cumsum([r.size for r in rl])
    return refs, np.concatenate(rl), off
