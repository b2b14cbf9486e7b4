"""GPU: PAF from the writer's GPU twin (lnr_writer_format_paf_gpu / lnr_writer_format_paf_dev: k_out_measure<Paf> / k_out_scan /
k_out_emit<Paf> of linear_amd/csrc/lnr_output_kernels.hip) byte for byte the host writer's (lnr_writer_format_paf, pinned on the CPU by
tests/test_output_paf_cpu.py) on the smallest shapes at which the read skeleton can go wrong (tests/paf_cases.py, tests/writer_cases.py);
the device form behind a Filter result; BGZF members of the text; the SAM and APF calls of the same writer untouched; the front-end's
--paf on its three paths."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import cases, paf_cases as pc, writer_cases as wc
from tests.test_gpu_writer import diff, writers  # noqa: F401  (writers: the fixture that opens writers with a GPU side)

pytestmark = pytest.mark.gpu


def inflate_members(data: bytes) -> bytes:
    out = b""
    while data:
        d = zlib.decompressobj(31)
        out += d.decompress(data)
        assert d.eof
        data = d.unused_data
    return out


def test_empty_inputs_give_zero_bytes(writers):
    w = writers()
    assert w.format_paf_gpu(*wc.empty()) == b""                                    # zero reads
    only_dummy = wc.Batch().read([]).read([], dummy=False).arrays()                # a read with only the dummy cord, a read without cords
    assert w.format_paf(*only_dummy) == b"" and w.format_paf_gpu(*only_dummy) == b""


@pytest.mark.parametrize("shape", ["strands_and_clips", "tile_edges", "window_lines", "misaligned", "target_fields"])
@pytest.mark.parametrize("preset", [1, 2])
def test_gpu_paf_equals_host_writer_on_small_shapes(writers, shape, preset):
    w = writers(preset=preset)
    batch = getattr(pc, shape)()
    want = w.format_paf(*batch)
    got = w.format_paf_gpu(*batch)
    assert got == want, diff(want, got)
    assert want.count(b"\n") == pc.sam_records(w.format(*batch, "sam")) > 0
    if shape == "misaligned":
        sizes = [len(l) + 1 for l in want.split(b"\n")[:-1]]
        assert {s % 4 for s in sizes} == {0, 1, 2, 3} and {sum(sizes[:k]) % 4 for k in range(len(sizes))} == {0, 1, 2, 3}
    if shape == "target_fields":
        assert b"\t*\t0\t" in want and b"\tchrA\t4000000000\t" in want


@pytest.mark.parametrize("preset", [1, 2])
def test_gpu_paf_equals_host_writer_on_synthetic_cords(writers, preset):
    """tests/writer_cases.py synthetic(): among others the 70-record read (a second tile of records: rec_carry), reads of 63 .. 130 cords, ids
    beyond nseq, the 10-digit length, the CIGAR splits of preset 1."""
    w = writers(preset=preset)
    for batch in (wc.synthetic(), wc.one_read()):
        want = w.format_paf(*batch)
        got = w.format_paf_gpu(*batch)
        assert got == want, diff(want, got)
    assert want.count(b"\n") == 2
    assert set(w.gpu_times()) == {"upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"}


@pytest.mark.parametrize("name,dup", wc.GAP_SETS)
def test_gpu_paf_equals_host_writer_on_gap_cords(writers, name, dup):
    batch = wc.gap_set(name, dup)
    w = writers()
    want = w.format_paf(*batch)
    got = w.format_paf_gpu(*batch)
    assert got == want, diff(want, got)
    pc.check_valid(got, pc.sam_records(w.format(*batch, "sam")))


def test_gpu_paf_device_form(writers, case_inputs):
    """Filter result in HBM -> lnr_writer_format_paf_dev: the text of lnr_writer_format_paf on the downloaded cords, and the derivation from the
    SAM text of the same call."""
    import torch
    from linear_amd import Filter
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    flt = Filter(device=0)
    flt.build_index(refs, 3)
    d_reads = torch.from_numpy(np.ascontiguousarray(reads, dtype=np.uint8)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = flt.filter_batch_dev(d_reads.data_ptr(), d_off.data_ptr(), n)
    glen = [r.size for r in refs]
    w = writers(gid, glen)
    paf = w.format_paf_dev(dev, d_off.data_ptr(), rid)
    sam = w.format_dev(dev, d_off.data_ptr(), rid, "sam")
    coff, cs, ce = flt.cords_to_host()
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    want = w.format_paf(coff, cs, ce, rl, rid)
    assert paf == want, diff(want, paf)
    assert paf == pc.paf_of_sam(sam, {i.encode(): int(x) for i, x in zip(rid, rl)}, {g.encode(): x for g, x in zip(gid, glen)})
    assert paf.count(b"\n") > 50
    flt.close()


def test_gpu_paf_bgzf_members(writers):
    """With BGZF on, Python's zlib inflates the members to the text; an empty batch gives zero bytes; off again, the text comes back plain."""
    w = writers()
    batch = wc.synthetic()
    want = w.format_paf(*batch)
    w.set_bgzf(True)
    got = w.format_paf_gpu(*batch)
    assert got[:4] == b"\x1f\x8b\x08\x04" and inflate_members(got) == want
    assert w.bgzf_stats()["text_bytes"] == len(want) and w.bgzf_stats()["blocks"] == -(-len(want) // 0xff00)
    assert w.format_paf_gpu(*wc.empty()) == b""
    w.set_bgzf(False)
    assert w.format_paf_gpu(*batch) == want


def test_sam_and_apf_calls_are_untouched_by_a_paf_call(writers):
    """The same writer, the same buffers: SAM and APF before and after a PAF call return the bytes they returned before, and PAF after them
    returns its own."""
    w = writers()
    big, small = wc.synthetic(), wc.one_read()
    before = {(id(b), k): w.format_gpu(*b, k) for b in (big, small) for k in ("sam", "apf")}
    for b in (big, small):
        for k in ("sam", "apf"):
            assert before[(id(b), k)] == w.format(*b, k)
    paf = {id(b): w.format_paf(*b) for b in (big, small)}
    for b, k in ((big, "paf"), (small, "sam"), (big, "apf"), (small, "paf"), (big, "sam"), (big, "paf"), (small, "apf"), (small, "paf")):
        got = w.format_paf_gpu(*b) if k == "paf" else w.format_gpu(*b, k)
        assert got == (paf[id(b)] if k == "paf" else before[(id(b), k)]), k


def test_gpu_paf_needs_gpu_open():
    from linear_amd.api import LnrError, Writer
    w = Writer(wc.GIDS, wc.GLEN)
    with pytest.raises(LnrError) as e:
        w.format_paf_gpu(*wc.one_read())
    assert e.value.status == -1 and "lnr_writer_gpu_open" in str(e.value)
    assert w.format_paf(*wc.one_read()).count(b"\n") == 2                         # the host form needs no device
    w.close()


def test_front_end_paf_on_its_three_paths(case_inputs, tmp_path):
    """linear_filter --paf: the .paf of the host path, of --gpu-writer and of the device chain --gpu-reader --gpu-writer are one and the same, it
    is the derivation from the run's own .sam, and the .sam is that of a run without --paf; with --bgzf the .paf.gz inflates to it."""
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs("edge")
    rp, gp, rid, gid = cases.write_fasta_case(tmp_path, refs, reads, off)
    out = {}
    for tag, extra in (("plain", []), ("host", ["--paf"]), ("gpu", ["--paf", "--gpu-writer"]), ("chain", ["--paf", "--gpu-reader", "--gpu-writer"]),
                       ("bgzf", ["--paf", "--gpu-writer", "--bgzf"])):
        p = subprocess.run(["timeout", "-k", "10", "240", lb.CLI, "filter", rp, gp, "-t", "3", "-g", "50", "-o", str(tmp_path / tag), "--block-reads", "17"] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        out[tag] = sorted(f for f in os.listdir(tmp_path) if f.startswith(tag + "."))
    assert out["plain"] == ["plain.sam"] and out["host"] == ["host.paf", "host.sam"] and out["bgzf"] == ["bgzf.paf.gz", "bgzf.sam.gz"]
    rd = lambda f: open(tmp_path / f, "rb").read()
    paf = rd("host.paf")
    assert rd("gpu.paf") == paf and rd("chain.paf") == paf and len(paf) > 5000
    for tag in ("host", "gpu", "chain"):
        assert rd(tag + ".sam") == rd("plain.sam")
    rl = {i.encode(): int(x) for i, x in zip(rid, np.diff(off.astype(np.int64)))}
    assert paf == pc.paf_of_sam(rd("plain.sam"), rl, {g.encode(): r.size for g, r in zip(gid, refs)})
    gz = rd("bgzf.paf.gz")
    assert gz.endswith(w_eof()) and inflate_members(gz) == paf


def w_eof() -> bytes:
    return bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
