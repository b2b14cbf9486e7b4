"""GPU: the writer's GPU twin (lnr_writer_gpu_open / lnr_writer_format_gpu / lnr_writer_format_dev, kernels in
linear_amd/csrc/lnr_output_kernels.hip): byte for byte the reference's text of the goldens and the host writer's text
(lnr_writer_format, the reference here) on the gap-path cord sets and the synthetic shapes of tests/writer_cases.py; buffer reuse across
calls; the device form behind a Filter result; the front-end's --gpu-writer switch.  Only the last two run the filter itself."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cases, writer_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def writers():
    from linear_amd import build as lb
    lb.build()
    from linear_amd.api import Writer
    made = []

    def make(gids=wc.GIDS, glen=wc.GLEN, preset=1):
        w = Writer(gids, glen)
        w.set_preset(preset)
        w.gpu_open(0)
        made.append(w)
        return w
    yield make
    for w in made:
        w.close()


def diff(want: bytes, got: bytes) -> str:
    for i, (x, y) in enumerate(zip(want.split(b"\n"), got.split(b"\n"))):
        if x != y:
            return f"line {i}: want {x[:160]!r} got {y[:160]!r}"
    return f"{len(want)} vs {len(got)} bytes"


@pytest.mark.parametrize("name,T", [("edge", 3), ("rep", 8), ("scale", 4)])
def test_gpu_writer_equals_reference_text(writers, name, T):
    """The goldens hold the cords and the reference's text for them; what the text does not depend on is not needed: read lengths come
    from the '@' records of the APF (a read without one has no cords and prints nothing), sequence lengths from the @SQ lines."""
    g = np.load(os.path.join(wc.GOLD, f"{name}_T{T}.npz"))
    want_sam, want_apf = g["sam"].tobytes(), g["apf"].tobytes()
    glen = [int(x) for x in re.findall(rb"@SQ\tSN:chr\d+\tLN:(\d+)", want_sam)]
    n = g["cord_off"].size - 1
    rid, gid = cases.text_ids(n, len(glen))
    rl = np.full(n, 1, np.uint64)
    for m in re.finditer(rb"^@ read_(\d+) len extra=\d+ (\d+) ", want_apf, flags=re.M):
        rl[int(m.group(1))] = int(m.group(2))
    w = writers(gid, glen)
    sam = w.format_gpu(g["cord_off"], g["cords_str"], g["cords_end"], rl, rid, "sam")
    apf = w.format_gpu(g["cord_off"], g["cords_str"], g["cords_end"], rl, rid, "apf")
    assert sam == wc.sam_body(want_sam), diff(wc.sam_body(want_sam), sam)
    assert apf == want_apf, diff(want_apf, apf)


@pytest.mark.parametrize("name,dup", wc.GAP_SETS)
def test_gpu_writer_equals_host_writer_on_gap_cords(writers, name, dup):
    coff, cs, ce, rl, rid = wc.gap_set(name, dup)
    w = writers()
    for k in ("sam", "apf"):
        want = w.format(coff, cs, ce, rl, rid, k)
        got = w.format_gpu(coff, cs, ce, rl, rid, k)
        assert got == want, (k, diff(want, got))


@pytest.mark.parametrize("preset", [1, 2])
def test_gpu_writer_equals_host_writer_on_synthetic_cords(writers, preset):
    w = writers(preset=preset)
    for batch in (wc.synthetic(), wc.one_read(), wc.empty()):
        for k in ("sam", "apf"):
            want = w.format(*batch, k)
            got = w.format_gpu(*batch, k)
            assert got == want, (k, diff(want, got))
    assert w.format_gpu(*wc.empty(), "apf") == b""
    t = w.gpu_times()
    assert set(t) == {"upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"}


def test_gpu_writer_no_stale_bytes_across_calls(writers):
    """The writer's buffers are reused: the same batch twice, a large batch then a small one, and SAM after APF give what a fresh call
    gives; the text of a call stays intact until the next one."""
    w = writers()
    big, small = wc.synthetic(), wc.one_read()
    want = {(id(b), k): w.format(*b, k) for b in (big, small) for k in ("sam", "apf")}
    for b, k in ((big, "apf"), (big, "apf"), (small, "apf"), (small, "sam"), (big, "sam"), (small, "apf"), (big, "apf")):
        assert w.format_gpu(*b, k) == want[(id(b), k)], k
    import ctypes
    addr, size = w.format_gpu(*small, "sam", copy=False)
    assert ctypes.string_at(addr, size) == want[(id(small), "sam")]


def test_gpu_writer_needs_gpu_open_and_a_device():
    from linear_amd.api import LnrError, Writer
    w = Writer(wc.GIDS, wc.GLEN)
    with pytest.raises(LnrError) as e:
        w.format_gpu(*wc.one_read(), "sam")
    assert e.value.status == -1 and "lnr_writer_gpu_open" in str(e.value)
    with pytest.raises(LnrError) as e:
        w.gpu_open(4096)
    assert e.value.status == -2
    import torch
    before = torch.cuda.current_device()
    w.gpu_open(0)
    assert w.format_gpu(*wc.one_read(), "sam") == w.format(*wc.one_read(), "sam")
    assert torch.cuda.current_device() == before
    w.close()


def test_gpu_writer_device_form(writers, case_inputs):
    """Filter result in HBM -> lnr_writer_format_dev: the text of lnr_writer_format on the downloaded cords."""
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
    w = writers(gid, [r.size for r in refs])
    sam, apf = w.format_dev(dev, d_off.data_ptr(), rid, "sam"), w.format_dev(dev, d_off.data_ptr(), rid, "apf")
    coff, cs, ce = flt.cords_to_host()
    rl = np.diff(off.astype(np.int64)).astype(np.uint64)
    assert sam == w.format(coff, cs, ce, rl, rid, "sam") and apf == w.format(coff, cs, ce, rl, rid, "apf")
    assert len(sam) > 10_000 and len(apf) > 100_000
    flt.close()


def test_gpu_writer_front_end_switch(case_inputs, tmp_path):
    """linear_filter --gpu-writer: .sam and .apf identical to the same command without the switch."""
    from linear_amd import build as lb
    lb.build()
    refs, reads, off = case_inputs("edge")
    rp, gp, _, _ = cases.write_fasta_case(tmp_path, refs, reads, off)
    out = {}
    for tag, extra in (("host", []), ("gpu", ["--gpu-writer"])):
        p = subprocess.run(["timeout", "-k", "10", "240", lb.CLI, "filter", rp, gp, "-t", "3", "-g", "0", "-o", str(tmp_path / tag), "-ot", "3", "--block-reads", "17"] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        out[tag] = (open(tmp_path / (tag + ".sam"), "rb").read(), open(tmp_path / (tag + ".apf"), "rb").read())
    assert out["gpu"] == out["host"] and len(out["host"][0]) > 10_000 and len(out["host"][1]) > 100_000
