#!/usr/bin/env python3
"""Prints the tables of README.md from the JSON lines beside it: per part of the writer the parent's median, least and largest figure
over its runs, the tree's median, the difference, the parent's max - min, and whether the tree's median exceeds the parent's by no more
than that.  writer_bam_ab / writer_ab: one line per run and tree, the figure of a run is its parts_ms entry.  writer_sort_hold_ab.json:
one run whose legs alternate inside the process, the figures are the repetitions in info_reps (P, T: the parent's library; B, S: the tree's)."""
import json, os, statistics as st
HERE = os.path.dirname(os.path.abspath(__file__))


def parts(d, prefix=""):
    out = {}
    for k, v in d.items():
        if k.endswith("parts_ms"):             # writer_bam_ab: parts_ms; writer_ab: B_parts_ms (host cords in) and C_parts_ms (device cords)
            out.update({prefix + k[:-len("parts_ms")] + kk: vv for kk, vv in v.items()})
        elif isinstance(v, dict):
            out.update(parts(v, prefix + k + "."))
    return out


def row(name, p, t):
    pm, tm, sp = st.median(p), st.median(t), max(p) - min(p)
    print("| `%s` | %.3f | %.3f .. %.3f | %.3f | %+.3f | %.3f | %s |" % (name, pm, min(p), max(p), tm, tm - pm, sp, "within" if tm - pm <= sp else "over"))


for tool in ("writer_bam_ab", "writer_ab"):
    runs = {t: [parts(json.loads(l)) for l in open(os.path.join(HERE, f"{tool}.{t}.jsonl"))] for t in ("parent", "tree")}
    print(tool, len(runs["parent"]), "runs of the parent,", len(runs["tree"]), "of the tree")
    for k in runs["parent"][0]:
        if any(x in k for x in ("measure", "emit", "pack")):
            row(k.split(".", 1)[-1] if tool == "writer_bam_ab" else k, [r[k] for r in runs["parent"]], [r[k] for r in runs["tree"]])
d = json.load(open(os.path.join(HERE, "writer_sort_hold_ab.json")))
print("writer_sort_hold_ab", d["reps"], "repetitions per leg")
for tag in ("plain", "seq"):
    for k in ("keep_ms", "gather_ms"):
        for a, b in (("P", "B"), ("T", "S")):
            row(f"{tag} {k} {a} -> {b}", d[tag][a]["info_reps"][k], d[tag][b]["info_reps"][k])
