"""GPU: the SEQ column on the writer's GPU side (lnr_writer_format_seq_gpu / _dev, k_out_measure<SamSeq> / k_out_emit<SamSeq> in
linear_amd/csrc/lnr_output_kernels.hip): byte for byte the host writer's text (lnr_writer_format_seq, itself pinned to the real program's
-ss 1 output in tests/test_output_seq_cpu.py) on the shapes of tests/writer_seq_cases.py; buffer reuse across calls of other sizes and
kinds; the device form behind a Filter result; the front-end's --sam-seq against the real program's text; the error paths."""
import os
import subprocess

import numpy as np
import pytest

from tests import cases, writer_seq_cases as sc
from tests.test_gpu_writer import diff

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def writers():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    made = []

    def make(preset=1):
        w = Writer(sc.GIDS, sc.GLEN)
        w.set_preset(preset)
        w.set_genome(sc.genome())
        w.gpu_open(0)
        made.append(w)
        return w
    yield make
    for w in made:
        w.close()


@pytest.mark.parametrize("preset", [1, 2])
def test_gpu_seq_equals_host_writer(writers, preset):
    w = writers(preset)
    for batch in (sc.synthetic(), sc.one_read(), sc.empty()):
        want = w.format_seq(*batch)
        got = w.format_seq_gpu(*batch)
        assert got == want, diff(want, got)
    assert set(w.gpu_times()) == {"upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"}


def test_gpu_seq_no_stale_bytes_across_calls(writers):
    """Big then small, SEQ then the plain form then SEQ on one writer; the plain form still gives the host writer's text afterwards."""
    w = writers()
    big, small = sc.synthetic(), sc.one_read()
    plain = lambda b: (b[0], b[1], b[2], np.diff(b[4].astype(np.int64)).astype(np.uint64), b[5])
    want_seq = {id(b): w.format_seq(*b) for b in (big, small)}
    want_plain = {(id(b), k): w.format(*plain(b), k) for b in (big, small) for k in ("sam", "apf")}
    for b, kind in ((big, "seq"), (small, "seq"), (small, "sam"), (small, "seq"), (big, "apf"), (small, "seq"), (big, "seq"), (big, "sam"), (small, "apf")):
        if kind == "seq":
            assert w.format_seq_gpu(*b) == want_seq[id(b)], kind
        else:
            assert w.format_gpu(*plain(b), kind) == want_plain[(id(b), kind)], kind
    w.set_genome(sc.genome())                                   # another set_genome: the GPU side takes its copy again
    assert w.format_seq_gpu(*small) == want_seq[id(small)]


def test_gpu_seq_device_form(case_inputs):
    """Filter result in HBM + the batch's device bases -> lnr_writer_format_seq_dev: the text of lnr_writer_format_seq on the downloaded cords."""
    import torch
    from linear_amd import Filter
    from linear_amd.api import Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    flt = Filter(device=0)
    flt.build_index(refs, 3)
    d_reads = torch.from_numpy(np.ascontiguousarray(reads, dtype=np.uint8)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
    w = Writer(gid, [r.size for r in refs])
    w.gpu_open(0)                                               # gpu_open before set_genome: either order
    w.set_genome(refs)
    sam = w.format_seq_dev(dev, d_reads.data_ptr(), d_off.data_ptr(), rid)
    coff, cs, ce = flt.cords_to_host()
    want = w.format_seq(coff, cs, ce, reads, off, rid)
    assert sam == want, diff(want, sam)
    assert len(sam) > 300_000
    w.close(); flt.close()


@pytest.mark.parametrize("name,mode", [("edge", "g0"), ("chim", "g50dup1")])
def test_front_end_sam_seq_equals_the_real_program(case_inputs, tmp_path, name, mode):
    """linear_filter --sam-seq, host writer and --gpu-writer: the bytes `linear filter -ss 1 -t 1` wrote (tests/golden/cli_ss_<case>.npz)."""
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs(name)
    g = np.load(os.path.join(GOLD, f"cli_ss_{name}.npz"))
    assert cases.input_digest(refs, reads, off) == str(g["digest"])
    want = g[f"sam_{mode}"].tobytes()
    rp, gp, _, _ = cases.write_fasta_case(tmp_path, refs, reads, off)
    for tag, extra in (("host", []), ("gpu", ["--gpu-writer"])):
        p = subprocess.run(["timeout", "-k", "10", "240", lb.CLI, "filter", rp, gp, "-t", "1", "-o", str(tmp_path / tag), "--sam-seq"] + cases.CLI_MODES[mode] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        got = open(tmp_path / (tag + ".sam"), "rb").read()
        assert got == want, (tag, diff(want, got))


def test_gpu_seq_errors_and_current_device():
    import torch
    from linear_amd.api import LnrError, Writer
    w = Writer(sc.GIDS, sc.GLEN)
    w.gpu_open(0)
    with pytest.raises(LnrError) as e:                          # before set_genome
        w.format_seq_gpu(*sc.one_read())
    assert e.value.status == -1 and "lnr_writer_set_genome" in str(e.value)
    w.close()
    w = Writer(sc.GIDS, sc.GLEN)
    w.set_genome(sc.genome())
    with pytest.raises(LnrError) as e:                          # before gpu_open
        w.format_seq_gpu(*sc.one_read())
    assert e.value.status == -1 and "lnr_writer_gpu_open" in str(e.value)
    from linear_amd.api import LnrCordsDev
    with pytest.raises(LnrError) as e:                          # (refused before it looks at the cords)
        w.format_seq_dev(LnrCordsDev(), 0, 0, [])
    assert e.value.status == -1 and "lnr_writer_gpu_open" in str(e.value)
    before = torch.cuda.current_device()
    w.gpu_open(0)
    assert w.format_seq_gpu(*sc.one_read()) == w.format_seq(*sc.one_read())
    assert torch.cuda.current_device() == before
    w.close()
