#!/usr/bin/env python3
"""Memory-instruction mix of the job and tail kernels, read from the device assembly (needs no GPU):

    hipcc --cuda-device-only -S --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off linear_amd/csrc/lnr_api.hip -o api.s
    python3 tools/measure/isa_table.py api.s [name substring ...]

Per function: instructions, flat / global / ds / scratch loads+stores, lane moves, the forms of s_waitcnt (both counters drained, vmcnt(0)
alone, a vector load left in flight, lgkmcnt alone), VGPRs, SGPRs, LDS bytes, scratch bytes and occupancy from the function's own resource directives."""
import re
import sys

DEFAULT = ("job_group_run", "binning_exact_wave", "binning_wave", "radix_sort_wave", "k_job", "k_tail_a", "k_tail_b")


def main():
    path, want = sys.argv[1], tuple(sys.argv[2:]) or DEFAULT
    rows, cur, c = [], None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".") and not m.group(1).startswith("BB") and not m.group(1).startswith(".L"):
            cur = m.group(1)
            c = dict(name=cur, ins=0, flat_ld=0, flat_st=0, glob_ld=0, glob_st=0, ds=0, scr_ld=0, scr_st=0, lane=0, w_both=0, w_vm0=0, w_vmN=0, w_lgkm=0, waits=0, vgpr="-", sgpr="-", lds="-", scratch="-", occ="-")
            rows.append(c)
            continue
        if c is None:
            continue
        s = line.strip()
        m = re.match(r"^; (NumVgprs|TotalNumSgprs|LDSByteSize|ScratchSize|Occupancy): (\d+)", s)
        if m:
            c[{"NumVgprs": "vgpr", "TotalNumSgprs": "sgpr", "LDSByteSize": "lds", "ScratchSize": "scratch", "Occupancy": "occ"}[m.group(1)]] = m.group(2)
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        op = s.split()[0]
        c["ins"] += 1
        if op.startswith("flat_load"): c["flat_ld"] += 1
        elif op.startswith("flat_store") or op.startswith("flat_atomic"): c["flat_st"] += 1
        elif op.startswith("global_load"): c["glob_ld"] += 1
        elif op.startswith("global_store") or op.startswith("global_atomic"): c["glob_st"] += 1
        elif op.startswith("ds_"): c["ds"] += 1
        elif op.startswith("scratch_load"): c["scr_ld"] += 1
        elif op.startswith("scratch_store"): c["scr_st"] += 1
        elif op in ("v_writelane_b32", "v_readlane_b32"): c["lane"] += 1
        elif op == "s_waitcnt":
            c["waits"] += 1
            vm = re.search(r"vmcnt\((\d+)\)", s)
            lg = re.search(r"lgkmcnt\((\d+)\)", s)
            if vm and int(vm.group(1)) > 0: c["w_vmN"] += 1
            elif vm and lg and int(lg.group(1)) == 0: c["w_both"] += 1
            elif vm: c["w_vm0"] += 1
            elif lg: c["w_lgkm"] += 1
    cols = ("ins", "flat_ld", "flat_st", "glob_ld", "glob_st", "ds", "scr_ld", "scr_st", "lane", "waits", "w_both", "w_vm0", "w_vmN", "w_lgkm", "vgpr", "sgpr", "lds", "scratch", "occ")
    print("| function | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    for r in rows:
        if r["ins"] and any(w in r["name"] for w in want):
            print("| `%s` | " % r["name"] + " | ".join(str(r[k]) for k in cols) + " |")


if __name__ == "__main__":
    main()
