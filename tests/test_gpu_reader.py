"""GPU: the reader's GPU twin (lnr_reader_gpu_open / lnr_reader_next_dev, k_rd_measure / k_rd_scan / k_rd_emit in
linear_amd/csrc/lnr_reader_kernels.hip): the blocks of lnr_reader_next -- the same n per call, offsets, ordinals and ids -- in device
memory; SeqAn's reader through tests/golden/reader.npz; the tile and window edges; buffer reuse and slots; the device-resident chain
reader -> filter -> writer and the front-end's --gpu-reader; the error paths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases, reader_cases, reader_gpu_cases as rg
from tests.test_gpu_writer import diff

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "reader.npz")
_hip = None


def d2h(ptr, nbytes, dtype=np.uint8):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(max(nbytes, 1), np.uint8)
    if nbytes:
        assert _hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out[:nbytes].view(dtype).copy()


def dev_blocks(path, dst_cap, max_reads, slots=2):
    """[(off, bases, ids)] per block of next_dev, ordinals and device offsets copied back"""
    from linear_amd.api import Reader
    r = Reader(path)
    r.gpu_open(0, slots)
    out = []
    while True:
        n, dr, dof, off, ids = r.next_dev(dst_cap, max_reads)
        if n == 0:
            break
        assert np.array_equal(d2h(dof, 8 * (n + 1), np.uint64), off)
        out.append((off, d2h(dr, int(off[n])), ids))
    r.close()
    return out


def same_blocks(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2], (what, k)


@pytest.fixture(scope="module")
def lib():
    from linear_amd import build as lb
    lb.build()
    return lb


@pytest.fixture(scope="module")
def fixture_files(lib, tmp_path_factory):
    return reader_cases.write_cases(str(tmp_path_factory.mktemp("gpu_reader")))


@pytest.fixture(scope="module")
def random_files(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_reader_rnd")
    out = {}
    for fmt in ("fasta", "fastq", "fastq_multiline"):
        out[fmt] = str(d / ("x." + fmt))
        rg.random_file(out[fmt], fmt)
    return out


@pytest.mark.parametrize("dst_cap,max_reads", [(1 << 20, 1000), (12000, 3), (20000, 1), (13000, 1000)])
def test_reference_parity(fixture_files, dst_cap, max_reads):
    paths, seqs = fixture_files
    g = np.load(GOLD)
    for name, path in paths.items():
        blocks = dev_blocks(path, dst_cap, max_reads)
        lens = np.concatenate([np.diff(b[0].astype(np.int64)) for b in blocks])
        off = np.zeros(lens.size + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        assert np.array_equal(off, g[name + ":off"]), name
        assert np.array_equal(np.concatenate([b[1] for b in blocks]), g[name + ":bases"]), name
        assert [i for b in blocks for i in b[2]] == [str(x) for x in g[name + ":ids"]], name
        assert off.size - 1 == len(seqs) and all(b[0].size - 1 <= max_reads and int(b[0][-1]) <= dst_cap for b in blocks)
        if dst_cap < 30000:
            assert len(blocks) > 1


@pytest.mark.parametrize("fmt", ["fasta", "fastq", "fastq_multiline"])
@pytest.mark.parametrize("cap,mr", [(1 << 22, 100000), (5000, 7), (1000, 1), (40000, 64)])
def test_block_identity(random_files, fmt, cap, mr):
    want = rg.serial_blocks(random_files[fmt], cap, mr, serial=False)
    assert sum(b[0].size - 1 for b in want) == 1500
    same_blocks(dev_blocks(random_files[fmt], cap, mr), want, (fmt, cap, mr))


def test_tile_and_window_edges(lib, tmp_path, monkeypatch):
    from linear_amd.api import Reader
    T = Reader.gpu_tile()
    assert T >= 64 and T % 64 == 0
    files = rg.edge_files(str(tmp_path), T)
    want = {name: rg.serial_blocks(p, 1 << 20, 1000) for name, p in files.items()}
    assert all(len(w) == 1 and 1 <= w[0][0].size - 1 <= 5 for w in want.values())
    for name, p in files.items():
        same_blocks(dev_blocks(p, 1 << 20, 1000), want[name], name)
    # a window that cuts the first record (and every later one): it is doubled until a record fits, the blocks stay the same
    for w in (T // 2 + 5, T + 1, 2 * T):
        monkeypatch.setenv("LNR_READER_GPU_WINDOW", str(w))
        for name in ("fa_start_1+0.fa", "fa_long_line.fa", "fa_long_header.fa", "fq_start_2-1.fq", "fq_long_line.fq", "fq_no_final_nl.fq", "fa_header_only.fa", "fq_unequal.fq"):
            same_blocks(dev_blocks(files[name], 1 << 20, 1000), want[name], (name, w))
            same_blocks(dev_blocks(files[name], 1 << 20, 2), rg.serial_blocks(files[name], 1 << 20, 2), (name, w, 2))


def test_buffer_reuse_and_slots(random_files):
    from linear_amd.api import Reader
    path = random_files["fasta"]
    want = []
    from linear_amd.api import Reader as R2
    h = R2(path)
    dst = np.zeros(1 << 20, np.uint8)
    for cap, mr in ((1 << 20, 900), (1 << 20, 1), (1 << 20, 599)):          # large, one read, large
        n, off, ids = h.next(dst[:cap], mr)
        want.append((off, dst[: int(off[n])].copy(), ids))
    h.close()
    r = Reader(path)
    r.gpu_open(0, 2)
    got, ptrs = [], []
    for k, (cap, mr) in enumerate(((1 << 20, 900), (1 << 20, 1), (1 << 20, 599))):
        n, dr, dof, off, ids = r.next_dev(cap, mr)
        got.append((off, d2h(dr, int(off[n])), ids))
        ptrs.append((dr, dof, n, off))
        if k:                                                               # slots = 2: the block of call k - 1 is unchanged after call k
            pdr, pdof, pn, poff = ptrs[k - 1]
            assert np.array_equal(d2h(pdr, int(poff[pn])), want[k - 1][1]) and np.array_equal(d2h(pdof, 8 * (pn + 1), np.uint64), poff)
    same_blocks(got, want, "reuse")
    t = r.gpu_times()
    assert set(t) == {"upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"} and t["measure_ms"] > 0 and t["emit_ms"] > 0
    assert r.next_dev(1 << 20, 10)[0] == 0                                  # end of file
    r.close()


def test_the_chain(lib, case_inputs, tmp_path):
    import torch
    from linear_amd import Filter
    from linear_amd.api import Reader, Writer
    refs, reads, off = case_inputs("edge")
    n = off.size - 1
    rid, gid = cases.text_ids(n, len(refs))
    rp, gp, _, _ = cases.write_fasta_case(tmp_path, refs, reads, off)
    flt = Filter(device=0)
    flt.build_index(refs, 3)
    host = rg.serial_blocks(rp, 1 << 24, 100000, serial=False)
    assert len(host) == 1 and np.array_equal(host[0][1], reads) and np.array_equal(host[0][0], off)
    want = flt.filter_batch(host[0][1], host[0][0])
    before = torch.cuda.current_device()
    r = Reader(rp)
    r.gpu_open(0, 2)
    k, dr, dof, hoff, ids = r.next_dev(1 << 24, 100000)
    assert torch.cuda.current_device() == before and k == n and ids == host[0][2]
    dev = flt.filter_batch_dev(dr, dof, k)
    got = flt.cords_to_host()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    w = Writer(gid, [x.size for x in refs])
    w.gpu_open(0)
    w.set_genome(refs)
    dev = flt.filter_batch_dev(dr, dof, k)
    sam = w.format_seq_dev(dev, dr, dof, ids)
    ref_sam = w.format_seq(*want, reads, off, ids)
    assert sam == ref_sam and len(sam) > 300_000, diff(ref_sam, sam)
    w.close(); r.close(); flt.close()
    # the real front-end
    outs = {}
    for tag, extra in (("plain", []), ("gr", ["--gpu-reader"]), ("seq", ["--sam-seq"]), ("grseq", ["--gpu-reader", "--gpu-writer", "--sam-seq"])):
        p = subprocess.run(["timeout", "-k", "10", "240", lib.CLI, "filter", rp, gp, "-t", "1", "-g", "0", "-ot", "3", "-o", str(tmp_path / tag), "--block-reads", "23"] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        outs[tag] = {e: open(tmp_path / (tag + e), "rb").read() for e in (".sam", ".apf")}
    for a, b in (("plain", "gr"), ("seq", "grseq")):
        for e in (".sam", ".apf"):
            assert outs[a][e] == outs[b][e] and len(outs[a][e]) > 1000, (a, b, e, diff(outs[a][e], outs[b][e]))


def test_errors(lib, tmp_path):
    from linear_amd.api import LnrError, Reader
    p = tmp_path / "x.fa"
    p.write_text(">a\nACGT\n>b\n" + "A" * 500 + "\n")
    r = Reader(str(p))
    with pytest.raises(LnrError) as e:
        r.next_dev(100, 10)
    assert e.value.status == -1 and "lnr_reader_gpu_open" in str(e.value)
    with pytest.raises(LnrError) as e:
        r.gpu_open(0, 0)
    assert e.value.status == -1
    r.gpu_open(0, 1)
    n, dr, dof, off, ids = r.next_dev(100, 10)
    assert n == 1 and ids == ["a"] and d2h(dr, 4).tolist() == [0, 1, 2, 3]
    with pytest.raises(LnrError) as e:
        r.next_dev(100, 10)
    assert e.value.status == -6 and "longer than the block" in str(e.value)
    r.close()
