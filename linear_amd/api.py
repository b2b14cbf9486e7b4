"""Python binding (ctypes) of the C ABI in include/linear_amd.h.

Thin plumbing only: numpy / torch buffers in, the reference's cord words out.  There is no
Python or CPU implementation of the path here; if liblinear_amd.so is missing or no GPU is
usable, construction raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.environ.get("LNR_LIB") or os.path.join(HERE, "liblinear_amd.so")   # LNR_LIB: a variant build (tools/build_variant.sh) for A/B measurements

_u8p, _u64p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


class LnrOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("index_type", C.c_uint32), ("feature_type", C.c_uint32), ("preset", C.c_uint32),
                ("gap_len", C.c_uint32), ("dup", C.c_uint32), ("scratch_budget", C.c_uint64)]


class LnrIndexInfo(C.Structure):
    _fields_ = [("nseq", C.c_uint32), ("layout_threads", C.c_uint32), ("genome_bytes", C.c_uint64), ("dir_len", C.c_uint64),
                ("hs_len", C.c_uint64), ("f2_len", C.c_uint64), ("n_samples", C.c_uint64), ("build_ms", C.c_double)]


class LnrCords(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("n_cords", C.c_uint64), ("cord_off", _u64p), ("cords_str", _u64p), ("cords_end", _u64p)]


class LnrCordsDev(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("n_cords", C.c_uint64), ("d_cord_off", C.c_void_p), ("d_cords_str", C.c_void_p), ("d_cords_end", C.c_void_p)]


class LnrGaps(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("n_gaps", C.c_uint64), ("gap_off", _u64p), ("gaps", _u64p)]


class LnrAnchors(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("n_anchors", C.c_uint64), ("anchor_off", _u64p), ("anchors", _u64p)]


class LnrStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("reads", "bases", "jobs", "samples", "lookups", "bucket_entries", "anchors", "remap_reads", "cords", "seed_bytes")] + \
               [(k, C.c_double) for k in ("prep_ms", "seed_count_ms", "seed_gather_ms", "job_ms", "tail_ms", "total_ms")] + \
               [(k, C.c_uint32) for k in ("seed_count_launches", "seed_gather_launches", "job_launches", "gap_second_pass")] + [("gap_ms", C.c_double), ("gap_last_launch", C.c_uint32)] + \
               [(k, C.c_uint32) for k in ("groups_heavy", "groups_mid", "groups_wave1")]


class LnrInflateCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("blocks", "compressed_bytes", "text_bytes", "gzread_bytes")] + [(k, C.c_double) for k in ("inflate_ms", "gather_ms")]


class LnrInflateStats(C.Structure):
    _fields_ = [("last", LnrInflateCounts), ("total", LnrInflateCounts)]


GZIP_COUNTS = ("rounds", "members", "chunks", "candidates", "true_pieces", "false_candidates", "deflate_blocks", "compressed_bytes", "text_bytes",
               "window_symbols", "gzread_bytes", "grown_rounds")
GZIP_MS = ("find_ms", "measure_ms", "stitch_ms", "emit_ms", "chain_ms", "resolve_ms", "parse_ms", "upload_ms", "download_ms")


class LnrGzipCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in GZIP_COUNTS] + [(k, C.c_double) for k in GZIP_MS]


class LnrGzipStats(C.Structure):
    _fields_ = [("last", LnrGzipCounts), ("total", LnrGzipCounts)]


class LnrBamCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "skipped", "reverse", "tiles", "repaired_tiles")] + [(k, C.c_double) for k in ("find_ms", "stitch_ms", "emit_ms")]


class LnrBamStats(C.Structure):
    _fields_ = [("last", LnrBamCounts), ("total", LnrBamCounts)]


class LnrError(RuntimeError):
    def __init__(self, status: int, msg: str, detail: str = ""):
        super().__init__(f"linear_amd: {msg} (status {status}){': ' + detail if detail else ''}")
        self.status = status


EXPORTS = ["lnr_opts_default", "lnr_create", "lnr_destroy", "lnr_strerror", "lnr_last_error", "lnr_index_build", "lnr_index_info_get",
           "lnr_index_export", "lnr_index_alloc", "lnr_index_blob", "lnr_index_adopt", "lnr_filter_batch", "lnr_filter_batch_dev",
           "lnr_cords_to_host", "lnr_seed_lookup_batch", "lnr_seed_lookup_batch_dev", "lnr_last_stats", "lnr_filter_submit", "lnr_filter_wait",
           "lnr_host_alloc", "lnr_host_free", "lnr_reader_open", "lnr_reader_next", "lnr_reader_ids", "lnr_reader_error", "lnr_reader_close",
           "lnr_writer_create", "lnr_writer_format", "lnr_writer_sam_header", "lnr_writer_destroy", "lnr_last_gaps", "lnr_gap_stream", "lnr_set_gap", "lnr_index_broadcast", "lnr_writer_set_preset", "lnr_writer_set_read_group",
           "lnr_writer_gpu_open", "lnr_writer_format_gpu", "lnr_writer_format_dev", "lnr_writer_gpu_times", "lnr_writer_error",
           "lnr_writer_set_genome", "lnr_writer_format_seq", "lnr_writer_format_seq_gpu", "lnr_writer_format_seq_dev",
           "lnr_writer_set_bgzf", "lnr_writer_bgzf_bytes_gpu", "lnr_writer_bgzf_eof", "lnr_writer_bgzf_stats",
           "lnr_writer_bam_header", "lnr_writer_format_bam", "lnr_writer_format_bam_gpu", "lnr_writer_format_bam_dev",
           "lnr_reader_gpu_open", "lnr_reader_next_dev", "lnr_reader_gpu_times", "lnr_reader_gpu_tile", "lnr_reader_gpu_inflate_stats",
           "lnr_reader_gpu_gzip", "lnr_reader_gpu_gzip_stats", "lnr_gunzip_gpu",
           "lnr_reader_gpu_bam_stats", "lnr_reader_gpu_bam_tile", "lnr_reader_format",
           "lnr_writer_sort_begin", "lnr_writer_sort_finish", "lnr_writer_sort_next", "lnr_writer_sort_bai", "lnr_writer_sort_info_get", "lnr_writer_sort_end",
           "lnr_writer_sort_host", "lnr_writer_bai_host", "lnr_writer_sort_spill", "lnr_writer_sort_hold_info_get",
           "lnr_genome_load_gpu", "lnr_genome_info", "lnr_genome_to_host", "lnr_genome_drop_dev", "lnr_genome_error", "lnr_genome_free", "lnr_writer_set_genome_dev",
           "lnr_writer_format_paf", "lnr_writer_format_paf_gpu", "lnr_writer_format_paf_dev",
           "lnr_filter_submit_dev", "lnr_filter_wait_dev"]


class LnrBgzfStats(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("stored_blocks", C.c_uint64), ("text_bytes", C.c_uint64), ("compressed_bytes", C.c_uint64),
                ("deflate_ms", C.c_double), ("pack_ms", C.c_double)]


class LnrSortInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "record_bytes", "device_bytes", "members")] + \
               [(k, C.c_double) for k in ("index_ms", "sort_ms", "gather_ms", "deflate_ms", "pack_ms", "download_ms")]


class LnrSortHoldInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("stream_bytes", "held_device_bytes", "held_host_bytes", "device_batches", "host_batches")] + \
               [(k, C.c_double) for k in ("keep_ms", "spill_ms")]


def load_library() -> C.CDLL:
    if not os.path.exists(SO):
        raise LnrError(-2, "liblinear_amd.so is not built (run linear_amd.build.build()); there is no fallback path")
    lib = C.CDLL(SO)
    lib.lnr_strerror.restype = C.c_char_p
    lib.lnr_strerror.argtypes = [C.c_int]
    lib.lnr_last_error.restype = C.c_char_p
    lib.lnr_last_error.argtypes = [C.c_void_p]
    lib.lnr_opts_default.argtypes = [C.POINTER(LnrOpts)]
    lib.lnr_create.argtypes = [C.POINTER(LnrOpts), C.POINTER(C.c_void_p)]
    lib.lnr_destroy.argtypes = [C.c_void_p]
    lib.lnr_index_build.argtypes = [C.c_void_p, C.POINTER(_u8p), _u64p, C.c_uint32, C.c_uint32]
    lib.lnr_index_info_get.argtypes = [C.c_void_p, C.POINTER(LnrIndexInfo)]
    lib.lnr_index_export.argtypes = [C.c_void_p, _i32p, _u64p, _i32p, _u64p]
    lib.lnr_index_alloc.argtypes = [C.c_void_p, C.POINTER(LnrIndexInfo), _u64p]
    lib.lnr_index_blob.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_index_adopt.argtypes = [C.c_void_p]
    lib.lnr_filter_batch.argtypes = [C.c_void_p, _u8p, _u64p, C.c_uint32, C.POINTER(LnrCords)]
    lib.lnr_filter_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(LnrCordsDev)]
    lib.lnr_cords_to_host.argtypes = [C.c_void_p, C.POINTER(LnrCords)]
    lib.lnr_seed_lookup_batch.argtypes = [C.c_void_p, _u8p, _u64p, C.c_uint32, C.POINTER(LnrAnchors)]
    lib.lnr_seed_lookup_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.lnr_last_stats.argtypes = [C.c_void_p, C.POINTER(LnrStats)]
    lib.lnr_gap_stream.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.lnr_set_gap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.lnr_filter_submit.argtypes = [C.c_void_p, C.c_void_p, _u64p, C.c_uint32]
    lib.lnr_filter_wait.argtypes = [C.c_void_p, C.POINTER(LnrCords)]
    lib.lnr_filter_submit_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _u64p, C.c_uint32]
    lib.lnr_filter_wait_dev.argtypes = [C.c_void_p, C.POINTER(LnrCordsDev)]
    lib.lnr_host_alloc.restype = C.c_void_p
    lib.lnr_host_alloc.argtypes = [C.c_size_t]
    lib.lnr_host_free.argtypes = [C.c_void_p]
    lib.lnr_reader_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.lnr_reader_next.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.lnr_reader_ids.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(_u64p)]
    lib.lnr_reader_error.restype = C.c_char_p
    lib.lnr_reader_error.argtypes = [C.c_void_p]
    lib.lnr_reader_close.argtypes = [C.c_void_p]
    lib.lnr_reader_gpu_open.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
    lib.lnr_reader_next_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_u64p), C.POINTER(C.c_uint32)]
    lib.lnr_reader_gpu_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.lnr_reader_gpu_inflate_stats.argtypes = [C.c_void_p, C.POINTER(LnrInflateStats)]
    lib.lnr_reader_gpu_gzip.argtypes = [C.c_void_p, C.c_int]
    lib.lnr_reader_gpu_gzip_stats.argtypes = [C.c_void_p, C.POINTER(LnrGzipStats)]
    lib.lnr_gunzip_gpu.argtypes = [C.c_int32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(LnrGzipStats),
                                   C.c_char_p, C.c_size_t]
    lib.lnr_reader_gpu_tile.restype = C.c_uint32
    lib.lnr_reader_gpu_tile.argtypes = []
    lib.lnr_reader_gpu_bam_stats.argtypes = [C.c_void_p, C.POINTER(LnrBamStats)]
    lib.lnr_reader_gpu_bam_tile.restype = C.c_uint32
    lib.lnr_reader_gpu_bam_tile.argtypes = []
    lib.lnr_reader_format.argtypes = [C.c_void_p]
    lib.lnr_writer_create.argtypes = [C.POINTER(C.c_char_p), _u64p, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.lnr_writer_format.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u64p, C.c_char_p, _u64p, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_sam_header.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_destroy.argtypes = [C.c_void_p]
    lib.lnr_last_gaps.argtypes = [C.c_void_p, C.POINTER(LnrGaps)]
    lib.lnr_writer_set_preset.argtypes = [C.c_void_p, C.c_uint32]
    lib.lnr_writer_gpu_open.argtypes = [C.c_void_p, C.c_int32]
    lib.lnr_writer_format_gpu.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u64p, C.c_char_p, _u64p, C.c_int, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_dev.argtypes = [C.c_void_p, C.POINTER(LnrCordsDev), C.c_void_p, C.c_char_p, _u64p, C.c_int, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_gpu_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.lnr_writer_error.restype = C.c_char_p
    lib.lnr_writer_error.argtypes = [C.c_void_p]
    lib.lnr_writer_set_genome.argtypes = [C.c_void_p, C.POINTER(_u8p)]
    lib.lnr_writer_format_seq.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u8p, _u64p, C.c_char_p, _u64p, C.c_uint32, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_seq_gpu.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u8p, _u64p, C.c_char_p, _u64p, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_seq_dev.argtypes = [C.c_void_p, C.POINTER(LnrCordsDev), C.c_void_p, C.c_void_p, C.c_char_p, _u64p, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_set_bgzf.argtypes = [C.c_void_p, C.c_int]
    lib.lnr_writer_bgzf_bytes_gpu.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_bgzf_eof.argtypes = [C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_bgzf_stats.argtypes = [C.c_void_p, C.POINTER(LnrBgzfStats)]
    lib.lnr_writer_bam_header.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_bam.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u8p, _u64p, C.c_char_p, _u64p, C.c_uint32, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_bam_gpu.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u8p, _u64p, C.c_char_p, _u64p, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_bam_dev.argtypes = [C.c_void_p, C.POINTER(LnrCordsDev), C.c_void_p, C.c_void_p, C.c_char_p, _u64p, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_sort_begin.argtypes = [C.c_void_p, C.c_uint64]
    lib.lnr_writer_sort_spill.argtypes = [C.c_void_p, C.c_uint64]
    lib.lnr_writer_sort_hold_info_get.argtypes = [C.c_void_p, C.POINTER(LnrSortHoldInfo)]
    lib.lnr_writer_sort_finish.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(LnrSortInfo)]
    lib.lnr_writer_sort_next.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_sort_bai.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_sort_info_get.argtypes = [C.c_void_p, C.POINTER(LnrSortInfo)]
    lib.lnr_writer_sort_end.argtypes = [C.c_void_p]
    lib.lnr_writer_sort_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]
    lib.lnr_writer_bai_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, _u64p, C.c_uint64, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_genome_load_gpu.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_int32, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
    lib.lnr_genome_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(_u64p), C.POINTER(C.c_void_p), C.POINTER(_u64p), C.POINTER(C.POINTER(C.c_void_p))]
    lib.lnr_genome_to_host.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_void_p))]
    lib.lnr_genome_drop_dev.argtypes = [C.c_void_p]
    lib.lnr_genome_error.restype = C.c_char_p
    lib.lnr_genome_error.argtypes = [C.c_void_p]
    lib.lnr_genome_free.restype = None
    lib.lnr_genome_free.argtypes = [C.c_void_p]
    lib.lnr_writer_set_genome_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.lnr_writer_format_paf.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u64p, C.c_char_p, _u64p, C.c_uint32, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_paf_gpu.argtypes = [C.c_void_p, C.POINTER(LnrCords), _u64p, C.c_char_p, _u64p, C.POINTER(C.c_void_p), _u64p]
    lib.lnr_writer_format_paf_dev.argtypes = [C.c_void_p, C.POINTER(LnrCordsDev), C.c_void_p, C.c_char_p, _u64p, C.POINTER(C.c_void_p), _u64p]
    return lib


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(t)


class Filter:
    """One context = one GPU.  Mirrors the Mapper's compute interface: build the index once, then filter read blocks."""

    def __init__(self, device: int = -1, scratch_budget: int = 0, index_type: int = 1, gap_len: int = 0, dup: int = 0):
        self.lib = load_library()
        o = LnrOpts()
        self.lib.lnr_opts_default(C.byref(o))
        o.device = device
        o.scratch_budget = scratch_budget
        o.index_type = index_type          # the reference's -i: 1 DIndex, 2 HIndex
        o.gap_len = gap_len                # the reference's -g: 0 = apxMap only, > 0 = + gap re-mapper (mapGaps, reformCords)
        o.dup = dup                        # the reference's -dup
        h = C.c_void_p()
        st = self.lib.lnr_create(C.byref(o), C.byref(h))
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode())
        self.h = h
        self._seq_len = None

    def _ck(self, st: int):
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode(), self.lib.lnr_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.lnr_destroy(self.h)
            self.h = None
            for p in getattr(self, "_pinned", []):
                self.lib.lnr_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- index
    def build_index(self, seqs: list[np.ndarray], layout_threads: int = 1) -> "LnrIndexInfo":
        seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        ptrs = (_u8p * len(seqs))(*[_p(s, _u8p) for s in seqs])
        lens = np.array([s.size for s in seqs], dtype=np.uint64)
        self._ck(self.lib.lnr_index_build(self.h, ptrs, _p(lens, _u64p), len(seqs), layout_threads))
        self._seq_len = lens
        return self.index_info()

    def build_index_ptrs(self, ptrs: list[int], lens: list[int], layout_threads: int = 1) -> "LnrIndexInfo":
        """Sequences given as raw addresses (host or device memory, e.g. slices of a torch tensor in HBM)."""
        arr = (_u8p * len(ptrs))(*[C.cast(C.c_void_p(int(p)), _u8p) for p in ptrs])
        lens = np.array(lens, dtype=np.uint64)
        self._ck(self.lib.lnr_index_build(self.h, arr, _p(lens, _u64p), len(ptrs), layout_threads))
        self._seq_len = lens
        return self.index_info()

    def index_info(self) -> "LnrIndexInfo":
        info = LnrIndexInfo()
        self._ck(self.lib.lnr_index_info_get(self.h, C.byref(info)))
        return info

    def index_export(self):
        info = self.index_info()
        dir_ = np.zeros(info.dir_len, np.int32)
        hs = np.zeros(max(info.hs_len, 1), np.uint64)
        f2 = np.zeros((max(info.f2_len, 1), 3), np.int32)
        f2_off = np.zeros(info.nseq + 1, np.uint64)
        self._ck(self.lib.lnr_index_export(self.h, _p(dir_, _i32p), _p(hs, _u64p), _p(f2, _i32p), _p(f2_off, _u64p)))
        return dir_, hs[:info.hs_len], f2[:info.f2_len], f2_off

    def index_blobs(self):
        """(device pointer, bytes) of the four index buffers (genome, dir, hs, f2) for an in-place RCCL broadcast."""
        out = []
        for k in range(4):
            p, b = C.c_void_p(), C.c_uint64()
            self._ck(self.lib.lnr_index_blob(self.h, k, C.byref(p), C.byref(b)))
            out.append((p.value, b.value))
        return out

    def index_alloc(self, info: "LnrIndexInfo", seq_len: np.ndarray):
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint64)
        self._ck(self.lib.lnr_index_alloc(self.h, C.byref(info), _p(seq_len, _u64p)))
        self._seq_len = seq_len

    def index_adopt(self):
        self._ck(self.lib.lnr_index_adopt(self.h))

    # small-vector forms used by linear_amd.dist.broadcast_index
    def index_info_vec(self) -> np.ndarray:
        i = self.index_info()
        return np.array([i.nseq, i.layout_threads, i.genome_bytes, i.dir_len, i.hs_len, i.f2_len, i.n_samples, 0], dtype=np.int64)

    def seq_len(self) -> np.ndarray:
        return np.asarray(self._seq_len, dtype=np.int64)

    def index_alloc_from(self, vec8: np.ndarray, seq_len: np.ndarray):
        info = LnrIndexInfo()
        info.nseq, info.layout_threads, info.genome_bytes, info.dir_len, info.hs_len, info.f2_len, info.n_samples = [int(v) for v in vec8[:7]]
        self.index_alloc(info, np.asarray(seq_len, dtype=np.uint64))

    # --------------------------------------------------------------- batches
    def filter_batch(self, reads: np.ndarray, off: np.ndarray):
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = off.size - 1
        out = LnrCords()
        self._ck(self.lib.lnr_filter_batch(self.h, _p(reads, _u8p), _p(off, _u64p), n, C.byref(out)))
        return self.cords_np(out)

    def host_alloc(self, nbytes: int) -> np.ndarray:
        """uint8 array over pinned host memory from lnr_host_alloc (freed with host_free or at close)."""
        p = self.lib.lnr_host_alloc(nbytes)
        if not p:
            raise LnrError(-4, "pinned host allocation failed")
        a = np.ctypeslib.as_array(C.cast(C.c_void_p(p), _u8p), shape=(nbytes,))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return a

    def filter_submit(self, reads: np.ndarray, off: np.ndarray):
        """Starts the upload of a batch (at most three in flight); reads/off must stay alive and unchanged until the filter_wait that returns it."""
        assert reads.dtype == np.uint8 and reads.flags.c_contiguous and off.dtype == np.uint64 and off.flags.c_contiguous
        self._inflight = getattr(self, "_inflight", [])
        self._ck(self.lib.lnr_filter_submit(self.h, C.c_void_p(reads.ctypes.data), _p(off, _u64p), off.size - 1))
        self._inflight.append((reads, off))

    def filter_wait(self, copy: bool = True):
        """Cords of the oldest submitted batch as numpy copies; copy=False returns the lnr_cords itself, whose host arrays stay valid
        until the second next result of the context (cords_np copies them)."""
        out = LnrCords()
        self._ck(self.lib.lnr_filter_wait(self.h, C.byref(out)))
        if getattr(self, "_inflight", None):
            self._inflight.pop(0)
        return self.cords_np(out) if copy else out

    @staticmethod
    def cords_np(out: "LnrCords"):
        n = out.n_reads
        coff = np.ctypeslib.as_array(out.cord_off, shape=(n + 1,)).copy()
        if out.n_cords:
            cs = np.ctypeslib.as_array(out.cords_str, shape=(out.n_cords,)).copy()
            ce = np.ctypeslib.as_array(out.cords_end, shape=(out.n_cords,)).copy()
        else:
            cs, ce = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        return coff, cs, ce

    def filter_batch_dev(self, d_reads_ptr: int, d_off_ptr: int, n: int) -> "LnrCordsDev":
        out = LnrCordsDev()
        self._ck(self.lib.lnr_filter_batch_dev(self.h, C.c_void_p(d_reads_ptr), C.c_void_p(d_off_ptr), n, C.byref(out)))
        return out

    def filter_submit_dev(self, d_reads_ptr: int, d_off_ptr: int, n: int, h_off=None):
        """Device form of filter_submit (at most three in flight, of either kind): nothing is copied, the device buffers must be complete now
        and stay untouched until the wait that returns the batch.  h_off: the same n + 1 offsets as a host uint64 array (copied during the
        call), which saves the library its read-back of d_off."""
        if h_off is not None:
            h_off = np.ascontiguousarray(h_off, dtype=np.uint64)
            assert h_off.size == n + 1
        self._inflight = getattr(self, "_inflight", [])
        self._ck(self.lib.lnr_filter_submit_dev(self.h, C.c_void_p(d_reads_ptr), C.c_void_p(d_off_ptr), _p(h_off, _u64p) if h_off is not None else None, n))
        self._inflight.append(None)

    def filter_wait_dev(self) -> "LnrCordsDev":
        """The oldest batch in flight (submitted by filter_submit or filter_submit_dev) as device arrays, without a download.  They stay
        valid until the second next filter_wait / filter_wait_dev of this context is called."""
        out = LnrCordsDev()
        self._ck(self.lib.lnr_filter_wait_dev(self.h, C.byref(out)))
        if getattr(self, "_inflight", None):
            self._inflight.pop(0)
        return out

    def last_gaps(self):
        """apx_gaps of the last filter call: (gap_off[n+1], gaps[k, 2])."""
        out = LnrGaps()
        self._ck(self.lib.lnr_last_gaps(self.h, C.byref(out)))
        goff = np.ctypeslib.as_array(out.gap_off, shape=(out.n_reads + 1,)).copy()
        g = np.ctypeslib.as_array(out.gaps, shape=(2 * out.n_gaps,)).copy().reshape(-1, 2) if out.n_gaps else np.zeros((0, 2), np.uint64)
        return goff, g

    def cords_to_host(self):
        out = LnrCords()
        self._ck(self.lib.lnr_cords_to_host(self.h, C.byref(out)))
        return self.cords_np(out)

    def seed_lookup_batch(self, reads: np.ndarray, off: np.ndarray):
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = off.size - 1
        out = LnrAnchors()
        self._ck(self.lib.lnr_seed_lookup_batch(self.h, _p(reads, _u8p), _p(off, _u64p), n, C.byref(out)))
        aoff = np.ctypeslib.as_array(out.anchor_off, shape=(n + 1,)).copy()
        a = np.ctypeslib.as_array(out.anchors, shape=(out.n_anchors,)).copy() if out.n_anchors else np.zeros(0, np.uint64)
        return aoff, a

    def seed_lookup_batch_dev(self, d_reads_ptr: int, d_off_ptr: int, n: int):
        self._ck(self.lib.lnr_seed_lookup_batch_dev(self.h, C.c_void_p(d_reads_ptr), C.c_void_p(d_off_ptr), n))

    def set_gap(self, gap_len: int, dup: int = 0) -> None:
        """-g / -dup of this context from now on (lnr_set_gap); a new read stream starts."""
        self._ck(self.lib.lnr_set_gap(self.h, gap_len, dup))

    def gap_stream(self, set_to: int = -1) -> int:
        """The read stream's state of the gap re-mapper (lnr_gap_stream): -1 query, 0 start a new stream, 1 mark it extended; returns the state."""
        st = C.c_int(0)
        self._ck(self.lib.lnr_gap_stream(self.h, set_to, C.byref(st)))
        return st.value

    def stats(self) -> dict:
        st = LnrStats()
        self._ck(self.lib.lnr_last_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in LnrStats._fields_}


def _gzip_stats(st) -> dict:
    return {w: {k: getattr(getattr(st, w), k) for k, _ in LnrGzipCounts._fields_} for w in ("last", "total")}


def gunzip_gpu(gz: bytes, text_cap: int, device: int = -1):
    """Every member of the plain gzip bytes `gz` inflated on the device (lnr_gunzip_gpu): (text, stats).  text_cap = room for the text.
    LNR_READER_GZ_CHUNK / LNR_READER_GZ_ROUND in the environment set the chunk and round sizes."""
    lib = load_library()
    out = np.zeros(max(int(text_cap), 1), np.uint8)
    n = C.c_uint64()
    st = LnrGzipStats()
    err = C.create_string_buffer(512)
    s = lib.lnr_gunzip_gpu(device, gz, len(gz), out.ctypes.data_as(C.POINTER(C.c_uint8)), int(text_cap), C.byref(n), C.byref(st), err, len(err))
    if s != 0:
        e = LnrError(s, lib.lnr_strerror(s).decode(), err.value.decode())
        e.text = out[: n.value].tobytes()
        e.stats = _gzip_stats(st)
        raise e
    return out[: n.value].tobytes(), _gzip_stats(st)


class Reader:
    """FASTA / FASTQ (plain or gzip) or BAM (found by content) -> blocks in the ABI's layout (host code; no GPU needed)."""

    def __init__(self, path: str):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.lnr_reader_open(os.fsencode(path), C.byref(h))
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode(), path)
        self.h = h

    def next(self, dst: np.ndarray, max_reads: int):
        """Fills dst (uint8, e.g. Filter.host_alloc) -> (n, off[n+1], ids[n]); n == 0 at end of file."""
        off = np.zeros(max_reads + 1, np.uint64)
        n = C.c_uint32()
        st = self.lib.lnr_reader_next(self.h, C.c_void_p(dst.ctypes.data), dst.size, _p(off, _u64p), max_reads, C.byref(n))
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode(), self.lib.lnr_reader_error(self.h).decode())
        return n.value, off[: n.value + 1].copy(), self._ids(n.value)

    def _ids(self, n: int):
        ids_p, ido_p = C.c_char_p(), _u64p()
        self.lib.lnr_reader_ids(self.h, C.byref(ids_p), C.byref(ido_p))
        ido = np.ctypeslib.as_array(ido_p, shape=(n + 1,)) if n else np.zeros(1, np.uint64)
        raw = C.string_at(C.cast(ids_p, C.c_void_p), int(ido[n])) if n else b""
        return [raw[int(ido[k]):int(ido[k + 1]) - 1].decode(errors="replace") for k in range(n)]

    def _ck(self, st: int):
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode(), self.lib.lnr_reader_error(self.h).decode())

    def gpu_open(self, device: int = 0, slots: int = 2) -> None:
        """Gives the reader its GPU side (a stream, staging buffers and `slots` device blocks on `device`); next_dev needs it."""
        self._ck(self.lib.lnr_reader_gpu_open(self.h, device, slots))

    def next_dev(self, dst_cap: int, max_reads: int):
        """The block next() would deliver, parsed on the GPU into a device block of the reader: (n, d_reads_ptr, d_off_ptr, off[n+1], ids[n]);
        n == 0 at end of file.  The device block stays valid until `slots` further calls."""
        dr, dof, off_p, n = C.c_void_p(), C.c_void_p(), _u64p(), C.c_uint32()
        self._ck(self.lib.lnr_reader_next_dev(self.h, dst_cap, max_reads, C.byref(dr), C.byref(dof), C.byref(off_p), C.byref(n)))
        off = np.ctypeslib.as_array(off_p, shape=(n.value + 1,)).copy()
        return n.value, dr.value, dof.value, off, self._ids(n.value)

    def gpu_times(self) -> dict:
        """Milliseconds of the last next_dev: stage + upload and download (wall), measure / scan / emit (HIP events)."""
        ms = (C.c_double * 5)()
        self._ck(self.lib.lnr_reader_gpu_times(self.h, ms))
        return dict(zip(("upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"), ms))

    def gpu_inflate_stats(self) -> dict:
        """BGZF input: {"last": counts of the last next_dev, "total": of all calls}; each {blocks, compressed_bytes, text_bytes, gzread_bytes,
        inflate_ms, gather_ms} -- blocks inflated on the device, bytes uploaded for them, text produced there, text that came through gzread."""
        st = LnrInflateStats()
        self._ck(self.lib.lnr_reader_gpu_inflate_stats(self.h, C.byref(st)))
        return {w: {k: getattr(getattr(st, w), k) for k, _ in LnrInflateCounts._fields_} for w in ("last", "total")}

    def gpu_gzip(self, on: bool = True) -> None:
        """Plain gzip files (not BGZF) are inflated on the device, in parallel from DEFLATE block starts.  After gpu_open, before the first read."""
        self._ck(self.lib.lnr_reader_gpu_gzip(self.h, 1 if on else 0))

    def gpu_gzip_stats(self) -> dict:
        """Plain gzip input: {"last": counts of the last next_dev, "total": of all calls} (the fields of lnr_gzip_counts)."""
        st = LnrGzipStats()
        self._ck(self.lib.lnr_reader_gpu_gzip_stats(self.h, C.byref(st)))
        return _gzip_stats(st)

    @staticmethod
    def gpu_tile() -> int:
        return int(load_library().lnr_reader_gpu_tile())

    def format(self) -> int:
        """3 BAM (looked up in the file's first bytes), else what the reads so far have shown: 1 FASTA, 2 FASTQ, 0 undecided."""
        return int(self.lib.lnr_reader_format(self.h))

    def gpu_bam_stats(self) -> dict:
        """BAM input: {"last": counts of the last next_dev, "total": of all calls}; each {records, skipped, reverse, tiles, repaired_tiles,
        find_ms, stitch_ms, emit_ms} -- records delivered, secondary / supplementary records passed over, reverse-complemented ones, tiles
        k_bam_find guessed in, tiles whose guess did not stand, and the kernels' milliseconds (HIP events)."""
        st = LnrBamStats()
        self._ck(self.lib.lnr_reader_gpu_bam_stats(self.h, C.byref(st)))
        return {w: {k: getattr(getattr(st, w), k) for k, _ in LnrBamCounts._fields_} for w in ("last", "total")}

    @staticmethod
    def gpu_bam_tile() -> int:
        """Bytes of records per tile of k_bam_find (0 when the library has no device half)."""
        return int(load_library().lnr_reader_gpu_bam_tile())

    def close(self):
        if getattr(self, "h", None):
            self.lib.lnr_reader_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LNR_GENOME_GPU_GZIP = 1


class _GenomeView(np.ndarray):
    """A view of a Genome's host copy that keeps the Genome (and so the memory) alive: arrays derived from it hold it as their base."""
    _owner = None


class Genome:
    """The reference genome loaded on the GPU (lnr_genome_load_gpu): files -> device-resident sequences, parsed (and, for BGZF, inflated)
    on the device.  lens / ids (whole header lines) live on the host; device_ptrs() is what Filter.build_index_ptrs and
    Writer.set_genome_dev take."""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h
        n, lens, ids, ido = C.c_uint32(), _u64p(), C.c_void_p(), _u64p()
        self._ck(lib.lnr_genome_info(h, C.byref(n), C.byref(lens), C.byref(ids), C.byref(ido), None))
        self.nseq = n.value
        self.lens = [int(lens[i]) for i in range(self.nseq)]
        raw = C.string_at(ids, int(ido[self.nseq])) if self.nseq else b""
        self.ids = [raw[int(ido[k]):int(ido[k + 1]) - 1].decode(errors="replace") for k in range(self.nseq)]

    @classmethod
    def load_gpu(cls, paths, device: int = 0, gpu_gzip: bool = False, block_bases: int = 0) -> "Genome":
        """paths: one file name or a list, read in order.  gpu_gzip: plain gzip files are inflated on the device too (BGZF always is).
        block_bases: bases per delivered block (0 = 2^30); the sequences do not depend on it."""
        lib = load_library()
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        h = C.c_void_p()
        st = lib.lnr_genome_load_gpu(arr, len(paths), device, LNR_GENOME_GPU_GZIP if gpu_gzip else 0, block_bases, C.byref(h))
        if st != 0:
            raise LnrError(st, lib.lnr_strerror(st).decode(), lib.lnr_genome_error(None).decode(errors="replace"))
        return cls(lib, h)

    def _ck(self, st: int):
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode(), self.lib.lnr_genome_error(self.h).decode(errors="replace"))

    def device_ptrs(self):
        """Device addresses of the sequences (ints, never 0), or None after drop_dev()."""
        d = C.POINTER(C.c_void_p)()
        self._ck(self.lib.lnr_genome_info(self.h, None, None, None, None, C.byref(d)))
        return [int(d[i] or 0) for i in range(self.nseq)] if d else None

    def to_host(self) -> list:
        """One download (kept by the object): a list of uint8 arrays of Dna5 ordinals, views of the object's host copy.  The arrays hold a
        reference to the Genome, so the memory lives while one of them (or an array sliced from it) does; close() frees it at once: do
        not touch the arrays after an explicit close()."""
        if not self.h:
            raise LnrError(-1, "invalid argument", "the Genome is closed")
        p = C.POINTER(C.c_void_p)()
        self._ck(self.lib.lnr_genome_to_host(self.h, C.byref(p)))
        out = []
        for i in range(self.nseq):
            n = self.lens[i]
            a = (np.ctypeslib.as_array(C.cast(p[i], _u8p), shape=(n,)) if n else np.zeros(0, np.uint8)).view(_GenomeView)
            a._owner = self
            out.append(a)
        return out

    def build_index(self, flt: "Filter", layout_threads: int = 1) -> "LnrIndexInfo":
        """lnr_index_build on `flt` (a Filter on the same device) from the device pointers."""
        ptrs = self.device_ptrs()
        if ptrs is None:
            raise LnrError(-1, "invalid argument", "Genome.build_index: the device copy has been dropped (drop_dev)")
        return flt.build_index_ptrs(ptrs, self.lens, layout_threads)

    def drop_dev(self) -> None:
        self._ck(self.lib.lnr_genome_drop_dev(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.lnr_genome_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Writer:
    """Cords of a batch -> SAM records / APF text: format() on host threads (no GPU needed), format_gpu() / format_dev() on the GPU; PAF lines
    likewise: format_paf() / format_paf_gpu() / format_paf_dev()."""

    def __init__(self, genome_ids: list[str], genome_len: list[int]):
        self.lib = load_library()
        arr = (C.c_char_p * len(genome_ids))(*[g.encode() for g in genome_ids])
        lens = np.array(genome_len, dtype=np.uint64)
        h = C.c_void_p()
        st = self.lib.lnr_writer_create(arr, _p(lens, _u64p), len(genome_ids), C.byref(h))
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode())
        self.h = h

    def format(self, cord_off: np.ndarray, cords_str: np.ndarray, cords_end: np.ndarray, read_len: np.ndarray, read_ids: list[str], what: str, threads: int = 4) -> bytes:
        cord_off = np.ascontiguousarray(cord_off, dtype=np.uint64)
        cs = np.ascontiguousarray(cords_str, dtype=np.uint64)
        ce = np.ascontiguousarray(cords_end, dtype=np.uint64)
        rl = np.ascontiguousarray(read_len, dtype=np.uint64)
        c = LnrCords()
        c.n_reads, c.n_cords = cord_off.size - 1, cs.size
        c.cord_off, c.cords_str, c.cords_end = _p(cord_off, _u64p), _p(cs, _u64p), _p(ce, _u64p)
        blob = b"".join(i.encode() + b"\0" for i in read_ids)
        ido = np.zeros(len(read_ids) + 1, np.uint64)
        ido[1:] = np.cumsum([len(i.encode()) + 1 for i in read_ids])
        text, size = C.c_void_p(), C.c_uint64()
        st = self.lib.lnr_writer_format(self.h, C.byref(c), _p(rl, _u64p), blob, _p(ido, _u64p), {"sam": 1, "apf": 2}[what], threads, C.byref(text), C.byref(size))
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode())
        return C.string_at(text, size.value)

    def set_preset(self, preset: int) -> None:
        st = self.lib.lnr_writer_set_preset(self.h, preset)
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode())

    def _check(self, st: int) -> None:
        if st != 0:
            raise LnrError(st, self.lib.lnr_strerror(st).decode(), self.lib.lnr_writer_error(self.h).decode())

    @staticmethod
    def _ids(read_ids: list[str]):
        blob = b"".join(i.encode() + b"\0" for i in read_ids)
        ido = np.zeros(len(read_ids) + 1, np.uint64)
        ido[1:] = np.cumsum([len(i.encode()) + 1 for i in read_ids])
        return blob, ido

    def gpu_open(self, device: int = 0) -> None:
        """Gives the writer its GPU side (a stream and buffers on `device`); format_gpu / format_dev need it."""
        self._check(self.lib.lnr_writer_gpu_open(self.h, device))

    def format_gpu(self, cord_off: np.ndarray, cords_str: np.ndarray, cords_end: np.ndarray, read_len: np.ndarray, read_ids: list[str], what: str, copy: bool = True):
        """The bytes of format(), formatted on the GPU.  copy=False: (address, size) of the writer's pinned text instead of a bytes object."""
        cord_off = np.ascontiguousarray(cord_off, dtype=np.uint64)
        cs = np.ascontiguousarray(cords_str, dtype=np.uint64)
        ce = np.ascontiguousarray(cords_end, dtype=np.uint64)
        rl = np.ascontiguousarray(read_len, dtype=np.uint64)
        c = LnrCords()
        c.n_reads, c.n_cords = cord_off.size - 1, cs.size
        c.cord_off, c.cords_str, c.cords_end = _p(cord_off, _u64p), _p(cs, _u64p), _p(ce, _u64p)
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_gpu(self.h, C.byref(c), _p(rl, _u64p), blob, _p(ido, _u64p), {"sam": 1, "apf": 2}[what], C.byref(text), C.byref(size)))
        return C.string_at(text, size.value) if copy else (text.value, size.value)

    def format_dev(self, cords_dev: "LnrCordsDev", d_off_ptr: int, read_ids: list[str], what: str, copy: bool = True):
        """Device form: the result of Filter.filter_batch_dev and the batch's device read offsets (n + 1)."""
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_dev(self.h, C.byref(cords_dev), d_off_ptr, blob, _p(ido, _u64p), {"sam": 1, "apf": 2}[what], C.byref(text), C.byref(size)))
        return C.string_at(text, size.value) if copy else (text.value, size.value)

    # ---- PAF: one line per SAM record (twelve columns and cg:Z:, include/linear_amd.h)
    def format_paf(self, cord_off: np.ndarray, cords_str: np.ndarray, cords_end: np.ndarray, read_len: np.ndarray, read_ids: list[str], threads: int = 4) -> bytes:
        """The PAF lines of the batch on host threads (no GPU needed)."""
        c, _r, rl, _keep = self._seq_args(cord_off, cords_str, cords_end, np.zeros(1, np.uint8), read_len)
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_paf(self.h, C.byref(c), _p(rl, _u64p), blob, _p(ido, _u64p), threads, C.byref(text), C.byref(size)))
        return C.string_at(text, size.value)

    def format_paf_gpu(self, cord_off: np.ndarray, cords_str: np.ndarray, cords_end: np.ndarray, read_len: np.ndarray, read_ids: list[str], copy: bool = True):
        """The bytes of format_paf(), formatted on the GPU; with set_bgzf(True) BGZF members of them."""
        c, _r, rl, _keep = self._seq_args(cord_off, cords_str, cords_end, np.zeros(1, np.uint8), read_len)
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_paf_gpu(self.h, C.byref(c), _p(rl, _u64p), blob, _p(ido, _u64p), C.byref(text), C.byref(size)))
        return C.string_at(text, size.value) if copy else (text.value, size.value)

    def format_paf_dev(self, cords_dev: "LnrCordsDev", d_off_ptr: int, read_ids: list[str], copy: bool = True):
        """Device form: the result of Filter.filter_batch_dev and the batch's device read offsets (n + 1)."""
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_paf_dev(self.h, C.byref(cords_dev), d_off_ptr, blob, _p(ido, _u64p), C.byref(text), C.byref(size)))
        return C.string_at(text, size.value) if copy else (text.value, size.value)

    def set_genome(self, seqs) -> None:
        """The genome's bases (one uint8 array of Dna5 ordinals per sequence, lengths as given to the constructor) for the SEQ column of
        format_seq*; None = off.  The arrays are kept alive by the writer."""
        if seqs is None:
            self._genome = None
            self._check(self.lib.lnr_writer_set_genome(self.h, None))
            return
        keep = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        keep = [s if s.size else np.zeros(1, np.uint8) for s in keep]
        arr = (_u8p * max(len(keep), 1))(*[_p(s, _u8p) for s in keep])
        self._genome = (keep, arr)
        self._check(self.lib.lnr_writer_set_genome(self.h, arr))

    def set_genome_dev(self, device_ptrs) -> None:
        """The GPU side's genome copied from device memory (Genome.device_ptrs()); after gpu_open.  None = off."""
        if device_ptrs is None:
            self._check(self.lib.lnr_writer_set_genome_dev(self.h, None))
            return
        arr = (C.c_void_p * max(len(device_ptrs), 1))(*[int(p) for p in device_ptrs])
        self._check(self.lib.lnr_writer_set_genome_dev(self.h, arr))

    @staticmethod
    def _seq_args(cord_off, cords_str, cords_end, reads, read_off):
        cord_off = np.ascontiguousarray(cord_off, dtype=np.uint64)
        cs = np.ascontiguousarray(cords_str, dtype=np.uint64)
        ce = np.ascontiguousarray(cords_end, dtype=np.uint64)
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        if reads.size == 0:
            reads = np.zeros(1, np.uint8)
        off = np.ascontiguousarray(read_off, dtype=np.uint64)
        c = LnrCords()
        c.n_reads, c.n_cords = cord_off.size - 1, cs.size
        c.cord_off, c.cords_str, c.cords_end = _p(cord_off, _u64p), _p(cs, _u64p), _p(ce, _u64p)
        return c, reads, off, (cord_off, cs, ce)

    def format_seq(self, cord_off: np.ndarray, cords_str: np.ndarray, cords_end: np.ndarray, reads: np.ndarray, read_off: np.ndarray, read_ids: list[str], threads: int = 4) -> bytes:
        """SAM records with the SEQ column (the reference's -ss 1) on host threads; reads / read_off[n + 1] as filter_batch takes them."""
        c, reads, off, _keep = self._seq_args(cord_off, cords_str, cords_end, reads, read_off)
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_seq(self.h, C.byref(c), _p(reads, _u8p), _p(off, _u64p), blob, _p(ido, _u64p), threads, C.byref(text), C.byref(size)))
        return C.string_at(text, size.value)

    def format_seq_gpu(self, cord_off: np.ndarray, cords_str: np.ndarray, cords_end: np.ndarray, reads: np.ndarray, read_off: np.ndarray, read_ids: list[str], copy: bool = True):
        """The bytes of format_seq(), formatted on the GPU."""
        c, reads, off, _keep = self._seq_args(cord_off, cords_str, cords_end, reads, read_off)
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_seq_gpu(self.h, C.byref(c), _p(reads, _u8p), _p(off, _u64p), blob, _p(ido, _u64p), C.byref(text), C.byref(size)))
        return C.string_at(text, size.value) if copy else (text.value, size.value)

    def format_seq_dev(self, cords_dev: "LnrCordsDev", d_reads_ptr: int, d_off_ptr: int, read_ids: list[str], copy: bool = True):
        """Device form of format_seq_gpu: the result of Filter.filter_batch_dev with the batch's device bases and read offsets (n + 1)."""
        blob, ido = self._ids(read_ids)
        text, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_seq_dev(self.h, C.byref(cords_dev), d_reads_ptr, d_off_ptr, blob, _p(ido, _u64p), C.byref(text), C.byref(size)))
        return C.string_at(text, size.value) if copy else (text.value, size.value)

    def gpu_times(self) -> dict:
        """Milliseconds of the last GPU format call: upload and download (wall), measure / scan / emit (HIP events)."""
        ms = (C.c_double * 5)()
        self._check(self.lib.lnr_writer_gpu_times(self.h, ms))
        return dict(zip(("upload_ms", "measure_ms", "scan_ms", "emit_ms", "download_ms"), ms))

    def set_bgzf(self, on: bool) -> None:
        """on: format_gpu / format_dev / format_seq_gpu / format_seq_dev return BGZF members (compressed on the GPU, no EOF marker) that
        inflate to the text they return with it off.  Needs gpu_open."""
        self._check(self.lib.lnr_writer_set_bgzf(self.h, 1 if on else 0))

    def bgzf_bytes_gpu(self, data: bytes, copy: bool = True):
        """Any bytes (the SAM header) as BGZF members, compressed on the writer's GPU."""
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_bgzf_bytes_gpu(self.h, data, len(data), C.byref(out), C.byref(size)))
        return C.string_at(out, size.value) if copy else (out.value, size.value)

    def bgzf_eof(self) -> bytes:
        """The 28-byte empty member that ends a BGZF file."""
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_bgzf_eof(C.byref(out), C.byref(size)))
        return C.string_at(out, size.value)

    def bgzf_stats(self) -> dict:
        """The last GPU call: blocks, stored_blocks, text_bytes, compressed_bytes, deflate_ms and pack_ms (HIP events)."""
        s = LnrBgzfStats()
        self._check(self.lib.lnr_writer_bgzf_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in LnrBgzfStats._fields_}

    # ---- BAM: the records of the SAM lines in binary (the reference's -ot 4 / 8)
    def bam_header(self, command_line: str, pbsv: bool = False) -> bytes:
        """"BAM\\1", l_text, the text of sam_header (pbsv: the -ot 8 form of the @RG line), the reference list of the writer's sequences."""
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_bam_header(self.h, command_line.encode(), 1 if pbsv else 0, C.byref(out), C.byref(size)))
        return C.string_at(out, size.value)

    def _bam_args(self, cord_off, cords_str, cords_end, read_len, reads, read_off):
        """no SEQ: read_len[n], reads None; SEQ: reads + read_off[n + 1] (set_genome needed)"""
        if reads is None:
            c, _r, arr, keep = self._seq_args(cord_off, cords_str, cords_end, np.zeros(1, np.uint8), read_len)
            return c, None, arr, keep
        c, r, arr, keep = self._seq_args(cord_off, cords_str, cords_end, reads, read_off)
        return c, _p(r, _u8p), arr, (keep, r)

    def format_bam(self, cord_off, cords_str, cords_end, read_len, read_ids: list[str], reads=None, read_off=None, threads: int = 4) -> bytes:
        """The BAM records of the batch on host threads.  reads / read_off given: with SEQ (as format_seq), read_len is ignored."""
        c, rp, arr, _keep = self._bam_args(cord_off, cords_str, cords_end, read_len, reads, read_off)
        blob, ido = self._ids(read_ids)
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_bam(self.h, C.byref(c), rp, _p(arr, _u64p), blob, _p(ido, _u64p), threads, C.byref(out), C.byref(size)))
        return C.string_at(out, size.value)

    def format_bam_gpu(self, cord_off, cords_str, cords_end, read_len, read_ids: list[str], reads=None, read_off=None, copy: bool = True):
        """The bytes of format_bam(), encoded on the GPU; with set_bgzf(True) BGZF members of them."""
        c, rp, arr, _keep = self._bam_args(cord_off, cords_str, cords_end, read_len, reads, read_off)
        blob, ido = self._ids(read_ids)
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_bam_gpu(self.h, C.byref(c), rp, _p(arr, _u64p), blob, _p(ido, _u64p), C.byref(out), C.byref(size)))
        return C.string_at(out, size.value) if copy else (out.value, size.value)

    def format_bam_dev(self, cords_dev: "LnrCordsDev", d_off_ptr: int, read_ids: list[str], d_reads_ptr: int | None = None, copy: bool = True):
        """Device form: the result of Filter.filter_batch_dev, the batch's device read offsets (n + 1) and, for SEQ, its device bases."""
        blob, ido = self._ids(read_ids)
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_format_bam_dev(self.h, C.byref(cords_dev), d_reads_ptr, d_off_ptr, blob, _p(ido, _u64p), C.byref(out), C.byref(size)))
        return C.string_at(out, size.value) if copy else (out.value, size.value)

    # ---- coordinate-sorted BAM with a BAI index: a sort mode of the GPU writer (include/linear_amd.h)
    def sort_begin(self, max_device_bytes: int = 0) -> None:
        """From here on format_bam_gpu / format_bam_dev keep their records on the device and return b""; bam_header carries @HD SO:coordinate."""
        self._check(self.lib.lnr_writer_sort_begin(self.h, max_device_bytes))

    def sort_spill(self, max_host_bytes: int) -> None:
        """While collecting: batches that do not fit on the device go to pinned host memory, max_host_bytes of it at most (0: off again)."""
        self._check(self.lib.lnr_writer_sort_spill(self.h, max_host_bytes))

    def sort_hold_info(self) -> dict:
        """What the round holds so far and where (lnr_sort_hold_info); any time between sort_begin and sort_end."""
        info = LnrSortHoldInfo()
        self._check(self.lib.lnr_writer_sort_hold_info_get(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in LnrSortHoldInfo._fields_}

    def sort_finish(self, piece_members: int = 0) -> dict:
        """Sorts the kept records on the device; the pieces then come from sort_pieces().  Returns sort_info()."""
        info = LnrSortInfo()
        self._check(self.lib.lnr_writer_sort_finish(self.h, piece_members, C.byref(info)))
        return {k: getattr(info, k) for k, _ in LnrSortInfo._fields_}

    def sort_pieces(self):
        """Iterator over the BGZF members of the sorted stream, a piece of at most piece_members members at a time."""
        while True:
            out, size = C.c_void_p(), C.c_uint64()
            self._check(self.lib.lnr_writer_sort_next(self.h, C.byref(out), C.byref(size)))
            if size.value == 0:
                return
            yield C.string_at(out, size.value)

    def sort_bai(self, first_offset: int) -> bytes:
        """The .bai of header members (first_offset bytes) + pieces + EOF; valid once sort_pieces() is exhausted."""
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_sort_bai(self.h, first_offset, C.byref(out), C.byref(size)))
        return C.string_at(out, size.value)

    def sort_info(self) -> dict:
        info = LnrSortInfo()
        self._check(self.lib.lnr_writer_sort_info_get(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in LnrSortInfo._fields_}

    def sort_end(self) -> None:
        self._check(self.lib.lnr_writer_sort_end(self.h))

    def sort_host(self, records: bytes) -> bytes:
        """The record stream in the coordinate order, on the host (no device needed)."""
        out = C.c_void_p()
        self._check(self.lib.lnr_writer_sort_host(self.h, records, len(records), C.byref(out)))
        return C.string_at(out, len(records))

    def bai_host(self, sorted_records: bytes, first_offset: int, member_off) -> bytes:
        """The .bai of a sorted record stream whose members (0xff00 bytes of it each) lie at first_offset + member_off[k]; member_off has one more entry than members."""
        mo = np.ascontiguousarray(member_off, dtype=np.uint64)
        out, size = C.c_void_p(), C.c_uint64()
        self._check(self.lib.lnr_writer_bai_host(self.h, sorted_records, len(sorted_records), first_offset, _p(mo, _u64p), mo.size - 1, C.byref(out), C.byref(size)))
        return C.string_at(out, size.value)

    def sam_header(self, command_line: str) -> bytes:
        text, size = C.c_void_p(), C.c_uint64()
        self.lib.lnr_writer_sam_header(self.h, command_line.encode(), C.byref(text), C.byref(size))
        return C.string_at(text, size.value)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lnr_writer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
