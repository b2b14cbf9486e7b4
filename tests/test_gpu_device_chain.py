"""GPU (-m gpu): the front-end's device chain (--gpu-reader) with the calculator submitting ahead through lnr_filter_submit_dev /
lnr_filter_wait_dev.  Every run writes the bytes of the same command with LNR_CLI_DEV_HALVES=0 (one lnr_filter_batch_dev at a time), and its
.sam / .apf are those of the default path without --gpu-reader.  Blocks of 23 reads: the `edge` case is several blocks, so three are in flight."""
import os
import shutil
import subprocess

import pytest

from tests import cases

pytestmark = pytest.mark.gpu

SETS = {
    "reader": ["--gpu-reader"],
    "writer": ["--gpu-reader", "--gpu-writer"],
    "seq": ["--gpu-reader", "--gpu-writer", "--sam-seq"],
    "fence": ["--gpu-reader", "--gpu-writer", "-ot", "4", "--sort"],       # two read files and no -o: a sort round per output file
}
MODES = {"g0": ["-g", "0"], "g50dup1": ["-g", "50", "-dup", "1"]}
_default = {}


@pytest.fixture(scope="module")
def files(case_inputs, tmp_path_factory):
    from linear_amd import build as lb
    lb.build()
    d = tmp_path_factory.mktemp("chain")
    refs, reads, off = case_inputs("edge")
    assert off.size - 1 > 3 * 23, "the case should fill more blocks than the context holds"
    cases.write_fasta_case(d, refs, reads, off)
    for name in ("one.fa", "two.fa"):
        shutil.copy(str(d / "reads.fa"), str(d / name))
    return d, lb.CLI


def run(cli, cwd, args, halves=None):
    """the front-end in `cwd` (made new, the input files linked into it), the same argv whatever `halves` is; returns ({output name: bytes}, stderr)"""
    os.makedirs(cwd)
    for name in ("reads.fa", "one.fa", "two.fa", "ref.fa"):
        os.symlink(os.path.join(os.path.dirname(cwd), name), os.path.join(cwd, name))
    env = dict(os.environ)
    env.pop("LNR_CLI_DEV_HALVES", None)
    if halves is not None:
        env["LNR_CLI_DEV_HALVES"] = str(halves)
    p = subprocess.run(["timeout", "-k", "10", "240", cli, "filter"] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (args, halves, p.stderr.decode()[-1000:])
    return {n: open(os.path.join(cwd, n), "rb").read() for n in sorted(os.listdir(cwd)) if not os.path.islink(os.path.join(cwd, n))}, p.stderr.decode()


def no_pg(sam):
    return [l for l in sam.split(b"\n") if not l.startswith(b"@PG")]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("opts", list(SETS))
def test_gpu_device_chain_submits_ahead_and_writes_the_same_bytes(files, opts, mode):
    d, cli = files
    fence = opts == "fence"
    inputs = ["one.fa", "two.fa", "x", "ref.fa"] if fence else ["reads.fa", "ref.fa", "-o", "out", "-ot", "3"]
    args = inputs + ["-t", "1", "--block-reads", "23"] + SETS[opts] + MODES[mode]
    new, err_new = run(cli, str(d / f"{opts}_{mode}_new"), args, 1)
    old, err_old = run(cli, str(d / f"{opts}_{mode}_old"), args, 0)
    assert sorted(new) == sorted(old) and new, (sorted(new), sorted(old))
    for name in new:
        assert new[name] == old[name] and len(new[name]) > 0, name
    if fence:
        assert sorted(new) == ["one.bam", "one.bam.bai", "two.bam", "two.bam.bai"] and new["one.bam"] == new["two.bam"] and new["one.bam.bai"] == new["two.bam.bai"]
        return
    assert sorted(new) == ["out.apf", "out.sam"]
    key = (mode, opts == "seq")
    if key not in _default:                      # the default path: host reader, host writer, lnr_filter_submit / lnr_filter_wait
        _default[key] = run(cli, str(d / f"default_{mode}_{int(key[1])}"),
                            ["reads.fa", "ref.fa", "-o", "out", "-ot", "3", "-t", "1", "--block-reads", "23"] + (["--sam-seq"] if key[1] else []) + MODES[mode])[0]
    want = _default[key]
    assert no_pg(new["out.sam"]) == no_pg(want["out.sam"]) and new["out.apf"] == want["out.apf"]
    # (not an empty agreement: the .sam holds records behind its header -- the case has 79 reads, several of them without a record)
    assert sum(1 for l in new["out.sam"].split(b"\n") if l and not l.startswith(b"@")) >= 23 and len(new["out.apf"]) > 0
