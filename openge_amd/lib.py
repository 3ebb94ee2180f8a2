"""ctypes binding of libopenge_hip.so (the C ABI declared in include/openge_hip.h).

Python is test/bench plumbing here: the product is the C ABI and the C++ `openge` CLI.  Device
buffers can be torch tensors (``tensor.data_ptr()``) so torch owns HBM allocation and RCCL, and
the library only runs kernels on the context's stream.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["OGE_LIB"]) if os.environ.get("OGE_LIB") else PKG / "libopenge_hip.so"  # OGE_LIB: an A/B build

MAX_REF = 64
DEFLATE_SEARCH = ("fast", "near", "span", "near+span")  # OGE_DEFL_* values 0..3 (include/openge_hip.h)


class SynthParams(C.Structure):
    """Mirror of oge_synth_params (openge_amd/csrc/synth.h)."""

    _fields_ = [
        ("seed", C.c_uint64), ("n_pairs", C.c_uint64), ("n_ref", C.c_uint32), ("read_len", C.c_uint32),
        ("ins_min", C.c_uint32), ("ins_max", C.c_uint32), ("dup_ppm", C.c_uint32), ("inter_ppm", C.c_uint32),
        ("munmap_ppm", C.c_uint32), ("clip_ppm", C.c_uint32), ("n_rg", C.c_uint32), ("qual_min", C.c_uint32),
        ("qual_max", C.c_uint32), ("shuffle", C.c_uint32),
        ("ref_len", C.c_uint64 * MAX_REF), ("ref_cum", C.c_uint64 * (MAX_REF + 1)),
    ]


class MarkdupOpts(C.Structure):
    """Mirror of oge_markdup_opts (include/openge_hip.h)."""

    _fields_ = [
        ("n_ref", C.c_int32), ("rg_ids", C.c_void_p), ("rg_ids_bytes", C.c_uint64), ("rg_lib", C.c_void_p),
        ("n_rg", C.c_int32), ("unknown_lib", C.c_int16), ("debug_sort_groups", C.c_int16),
        ("compat_nonverbose_index", C.c_int32), ("remove_duplicates", C.c_int32), ("debug_hash_bits", C.c_int32),
        ("split_chains", C.c_int32),
    ]


class FilterOpts(C.Structure):
    """oge_filter_opts (include/openge_hip.h): Filter's settings (algorithms/filter.h:34-47)."""

    _fields_ = [(k, C.c_int32) for k in ("has_region", "ref_id", "left_pos", "right_pos", "mapq_min", "min_len",
                                         "max_len", "trim_total")] + [("count_limit", C.c_uint64)]


class Region(C.Structure):
    """oge_region: one region of a region list, the ref_id / left_pos / right_pos of oge_filter_opts."""

    _fields_ = [(k, C.c_int32) for k in ("ref_id", "left_pos", "right_pos")]


class BamStats(C.Structure):
    """Mirror of oge_bam_stats (include/openge_hip.h)."""

    COUNTERS = ("reads", "mapped", "forward", "reverse", "failed_qc", "duplicates", "paired", "proper_pair", "read1", "read2",
                "both_mapped", "singletons")
    _fields_ = ([(k, C.c_uint64) for k in COUNTERS] + [("sorted", C.c_int32), ("pad0", C.c_int32)] +
                [(k, C.c_uint64) for k in ("n_insert", "insert_sum", "insert_mid_lo", "insert_mid_hi", "n_lengths")])


STATS_INSERTS, STATS_LENGTHS = 1, 2


class CompareRegion(C.Structure):
    """Mirror of oge_compare_region: start positions left..right on contigs left_ref..right_ref, all inclusive."""
    _fields_ = [(k, C.c_int32) for k in ("left_ref", "left_pos", "right_ref", "right_pos")]


class CompareResult(C.Structure):
    """Mirror of oge_compare_result (include/openge_hip.h)."""
    FIELDS = ("n_ref", "n_other", "common", "additions", "deletions", "diff_entries", "hard_runs")
    _fields_ = [(k, C.c_uint64) for k in FIELDS]


COMPARE_DIFF = 1
COMPARE_ALL = (0, 0, 2**31 - 1, 2**31 - 1)  # the region of `openge compare` without -r


def decode_compare_diff(image: bytes) -> list[tuple]:
    """The diff image of oge_compare(_dev) -> [(side, refID, pos, surplus, (op word, ...))], in image order."""
    import struct
    out, p = [], 0
    while p < len(image):
        refid, pos, surplus, side, nops = struct.unpack_from("<iiQII", image, p)
        out.append((side, refid, pos, surplus, struct.unpack_from(f"<{nops}I", image, p + 24)))
        p += 24 + 4 * nops
    return out


class TargetsOpts(C.Structure):
    """Mirror of oge_targets_opts (include/openge_hip.h)."""
    _fields_ = [("max_interval", C.c_int32), ("gap", C.c_int32), ("want", C.c_uint32)]


class TargetsResult(C.Structure):
    """Mirror of oge_targets_result."""
    FIELDS = ("reads_used", "events", "intervals", "dropped_long", "targets", "text_bytes")
    _fields_ = [(k, C.c_uint64) for k in FIELDS]


TARGETS_TEXT = 1


class CalmdOpts(C.Structure):
    """Mirror of oge_calmd_opts (include/openge_hip.h)."""
    _fields_ = [("threads", C.c_int32), ("flags", C.c_uint32)]


class CalmdResult(C.Structure):
    """Mirror of oge_calmd_result."""
    FIELDS = ("records", "skipped", "no_reference", "nm_changed", "md_changed", "bytes_out")
    _fields_ = [(k, C.c_uint64) for k in FIELDS]


def _ref_table(refs) -> tuple[np.ndarray, bytes]:
    """[(name, length)] -> (lengths i32, the names NUL-terminated one after the other)"""
    return np.array([ln for _, ln in refs], np.int32), b"".join(nm.encode() + b"\0" for nm, _ in refs)


TEXT_SAM, TEXT_FASTQ = 0, 1


class TextOpts(C.Structure):
    """oge_text_opts: the text mode, the FASTQ trim window and the contig names of the header."""
    _fields_ = [("mode", C.c_int32), ("trim_begin", C.c_int32), ("trim_end", C.c_int32), ("n_ref", C.c_int32),
                ("ref_names", C.c_char_p), ("ref_name_off", C.c_void_p)]


def text_opts(names: list[str], mode: int = TEXT_SAM, trim: tuple[int, int] = (0, 0)) -> tuple[TextOpts, tuple]:
    """(oge_text_opts, the buffers it points into: keep them alive while it is in use)"""
    enc = [nm.encode() for nm in names]
    off = np.zeros(len(enc) + 1, np.uint32)
    off[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64) if enc else []
    blob = b"".join(enc)
    o = TextOpts(mode, trim[0], trim[1], len(enc), blob, _ptr(off))
    return o, (blob, off)


class MergesortOpts(C.Structure):
    """Mirror of oge_mergesort_opts (include/openge_hip.h)."""

    _fields_ = [(k, C.c_int32) for k in ("level", "mark_duplicates", "remove_duplicates", "compat_nonverbose_index",
                                         "split_chains", "build_index")] + [("program_line", C.c_char_p)]


def mergesort_opts(**over) -> MergesortOpts:
    o = MergesortOpts()
    lib().oge_mergesort_opts_init(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


class RealignSynthParams(C.Structure):
    """Mirror of oge_realign_synth_params (include/openge_hip.h)."""

    _fields_ = [("seed", C.c_uint64)] + [(k, C.c_uint32) for k in (
        "n_ref", "n_intervals", "spacing", "read_len", "frags_per_interval", "qual_min", "qual_max", "ins_min", "ins_max",
        "err_ppm", "noindel_ppm", "gapped_ppm", "alt_indel_ppm", "dup_ppm", "mapq0_ppm", "clip_ppm", "lower_ppm", "n_ppm",
        "md_ppm", "uq_ppm")]


class RealignOpts(C.Structure):
    """Mirror of oge_realign_opts (include/openge_hip.h)."""

    _fields_ = [("lod_threshold", C.c_double), ("mismatch_threshold", C.c_double)] + [(k, C.c_int32) for k in (
        "max_records_in_memory", "max_isize_for_movement", "max_pos_move_allowed", "max_reads",
        "no_original_alignment_tags", "threads")]


class RealignScanBatch(C.Structure):
    """Mirror of oge_realign_scan_batch (include/openge_hip.h)."""

    _fields_ = [("cons", C.c_void_p), ("cons_bytes", C.c_uint64), ("cons_off", C.c_void_p), ("n_cons", C.c_uint32),
                ("n_reads", C.c_uint32), ("bases", C.c_void_p), ("quals", C.c_void_p), ("read_bytes", C.c_uint64),
                ("read_off", C.c_void_p), ("pairs", C.c_void_p), ("n_pairs", C.c_uint64)]


def realign_synth_params(**over) -> RealignSynthParams:
    """C5-shaped realignment data set parameters (defaults: 50k intervals on 24 contigs)."""
    p = RealignSynthParams()
    lib().oge_realign_synth_defaults(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def synth_realign(p: RealignSynthParams, directory, level: int = 6, threads: int = 8) -> tuple[str, str, str]:
    """Write ref.fa (+ .fai), targets.intervals and reads.bam into `directory`; returns their paths."""
    d = Path(directory)
    fa, iv, bam = str(d / "ref.fa"), str(d / "targets.intervals"), str(d / "reads.bam")
    check(lib().oge_synth_realign(C.byref(p), fa.encode(), iv.encode(), bam.encode(), level, threads))
    return fa, iv, bam


def realign_opts(**over) -> RealignOpts:
    o = RealignOpts()
    lib().oge_realign_opts_init(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


# GRCh38 primary-assembly lengths chr1..22, X, Y (Mbp, rounded) -- relative contig sizes of C2.
GRCH38_MB = [248.96, 242.19, 198.30, 190.21, 181.54, 170.81, 159.35, 145.14, 138.39, 133.80, 135.09, 133.28,
             114.36, 107.04, 101.99, 90.34, 83.26, 80.37, 58.62, 64.44, 46.71, 50.82, 156.04, 57.23]


def synth_params(n_pairs: int, *, preset: str = "c1", seed: int = 1234, **over) -> SynthParams:
    """Synthetic read-set parameters.

    preset "c1": SURVEY §8d C1 -- one 5 Mbp contig, 150 bp pairs, 10% duplicate pairs, 1 RG.
    preset "c2": SURVEY §8d C2 -- 24 contigs with GRCh38 relative lengths scaled to 1.5 Gbp, 8% dup
                 pairs, 1% inter-contig, 0.5% mate-unmapped, 2 read groups / libraries.
    preset "mix": small multi-contig set exercising clipping, inter-contig and unmapped mates.
    """
    p = SynthParams()
    p.seed, p.n_pairs, p.read_len = seed, n_pairs, 150
    p.ins_min, p.ins_max, p.qual_min, p.qual_max, p.shuffle = 250, 450, 2, 40, 1
    if preset == "c1":
        p.n_ref, p.n_rg = 1, 1
        p.ref_len[0] = 5_000_000
        p.dup_ppm, p.inter_ppm, p.munmap_ppm, p.clip_ppm = 100_000, 0, 0, 0
    elif preset == "c2":
        p.n_ref, p.n_rg = 24, 2
        tot = sum(GRCH38_MB)
        for i, mb in enumerate(GRCH38_MB):
            p.ref_len[i] = int(1.5e9 * mb / tot)
        p.dup_ppm, p.inter_ppm, p.munmap_ppm, p.clip_ppm = 80_000, 10_000, 5_000, 50_000
    elif preset == "mix":
        p.n_ref, p.n_rg = 5, 3
        for i in range(5):
            p.ref_len[i] = 20_000 + 7_000 * i
        p.dup_ppm, p.inter_ppm, p.munmap_ppm, p.clip_ppm = 150_000, 40_000, 20_000, 200_000
    else:
        raise ValueError(preset)
    for k, v in over.items():
        if k == "ref_len":
            for i, x in enumerate(v):
                p.ref_len[i] = x
        else:
            setattr(p, k, v)
    return p


class OgeError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load libopenge_hip.so (fails loudly if it has not been built: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise OgeError(f"{LIB_PATH} is missing: run `python -m openge_amd.build` (no CPU fallback exists)")
    # torch wheels bundle their own libamdhip64.so.7.  Load torch first so the dynamic loader
    # resolves our NEEDED libamdhip64.so.7 to that same, already-loaded runtime: two HIP runtimes
    # in one process make the second one see no GPUs.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(str(LIB_PATH))
    vp, u64, i32, u32 = C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32
    sig = {
        "oge_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "oge_ctx_set_stream": (C.c_int, [vp, vp]),
        "oge_ctx_stream": (vp, [vp]),
        "oge_ctx_sync": (C.c_int, [vp]),
        "oge_ctx_destroy": (None, [vp]),
        "oge_last_error": (C.c_char_p, [vp]),
        "oge_ctx_timing": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_double)]),
        "oge_ctx_counter": (C.c_int, [vp, C.c_char_p, C.POINTER(u64)]),
        "oge_mergesort_reserve": (C.c_int, [vp, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]),
        "oge_version": (C.c_char_p, []),
        "oge_sort_coord": (C.c_int, [vp, vp, u64, vp, u64, i32, vp]),
        "oge_sort_coord_dev": (C.c_int, [vp, vp, vp, u64, i32, vp]),
        "oge_gather_records_dev": (C.c_int, [vp, vp, vp, vp, u64, vp, vp]),
        "oge_radix_sort_pairs_dev": (C.c_int, [vp, vp, vp, vp, vp, u64, u64, C.POINTER(C.c_int)]),
        "oge_exclusive_scan_dev": (C.c_int, [vp, vp, vp, u64, C.c_int]),
        "oge_markdup": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, C.POINTER(u64)]),
        "oge_markdup_dev": (C.c_int, [vp, vp, vp, u64, vp, vp, C.c_int, C.POINTER(u64)]),
        "oge_sort_markdup_dev": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64)]),
        "oge_synth_finalize": (C.c_int, [vp]),
        "oge_synth_params_size": (u64, []),
        "oge_synth_offsets_host": (C.c_int, [vp, vp, C.c_int]),
        "oge_synth_records_host": (C.c_int, [vp, vp, vp, C.c_int]),
        "oge_synth_header_text": (C.c_int, [vp, vp, u64, C.POINTER(u64)]),
        "oge_synth_offsets_dev": (C.c_int, [vp, vp, vp]),
        "oge_synth_records_dev": (C.c_int, [vp, vp, vp, vp]),
        "oge_bam_read": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(vp)]),
        "oge_bam_free": (None, [vp]),
        "oge_bam_count": (u64, [vp]),
        "oge_bam_records": (vp, [vp, C.POINTER(u64)]),
        "oge_bam_offsets": (vp, [vp]),
        "oge_bam_n_ref": (i32, [vp]),
        "oge_bam_header_text": (C.c_int, [vp, vp, u64, C.POINTER(u64)]),
        "oge_bam_markdup_opts": (C.c_int, [vp, vp, C.POINTER(vp), C.POINTER(vp)]),
        "oge_bam_write": (C.c_int, [C.c_char_p, C.c_char_p, u64, C.c_int, vp, vp, u64, vp, vp, C.c_int, C.c_int]),
        "oge_realign_scan": (C.c_int, [vp, vp, vp, vp]),
        "oge_sort_markdup_chunked": (C.c_int, [vp, vp, vp, u64, i32, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64),
                                               C.POINTER(u64)]),
        "oge_mem_info": (C.c_int, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "oge_device_count": (C.c_int, []),
        "oge_comm_unique_id_bytes": (u64, []),
        "oge_comm_unique_id": (C.c_int, [vp, u64]),
        "oge_comm_init_rank": (C.c_int, [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]),
        "oge_comm_init_rank_mode": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_char_p, C.POINTER(vp)]),
        "oge_comm_stats_json": (C.c_int64, [vp, C.c_char_p, u64]),
        "oge_comm_init": (C.c_int, [vp, C.c_int, vp]),
        "oge_comm_destroy": (None, [vp]),
        "oge_comm_rank": (C.c_int, [vp]),
        "oge_comm_size": (C.c_int, [vp]),
        "oge_comm_transport": (C.c_char_p, [vp]),
        "oge_mergesort_bgzf_host": (C.c_int, [vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "oge_mergesort_bgzf_dist": (C.c_int, [vp, vp, u64, vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64),
                                              C.POINTER(u64)]),
        "oge_sort_markdup_dist": (C.c_int, [vp, vp, vp, u64, i32, C.c_int, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64),
                                            C.POINTER(u64)]),
        "oge_mergesort_bgzf_shard": (C.c_int, [vp, vp, u64, u64, vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64),
                                               C.POINTER(u64)]),
        "oge_bgzf_decode_shard": (C.c_int, [vp, vp, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), vp, u64,
                                            C.POINTER(u64)]),
        "oge_synth_offsets_range_dev": (C.c_int, [vp, vp, u64, u64, vp]),
        "oge_synth_records_range_dev": (C.c_int, [vp, vp, u64, u64, vp, vp]),
        "oge_dev_alloc": (C.c_int, [vp, u64, C.POINTER(vp)]),
        "oge_dev_free": (C.c_int, [vp, vp]),
        "oge_memcpy": (C.c_int, [vp, vp, vp, u64, C.c_int]),
        "oge_host_alloc": (C.c_int, [vp, u64, C.POINTER(vp)]),
        "oge_ctx_set_pool": (C.c_int, [vp, C.c_int]),
        "oge_ctx_set_deflate_search": (C.c_int, [vp, C.c_int]),
        "oge_ctx_deflate_search": (C.c_int, [vp]),
        "oge_host_free": (C.c_int, [vp, vp]),
        "oge_realign_opts_init": (None, [vp]),
        "oge_localrealign": (C.c_int, [vp, C.c_char_p, u64, vp, vp, u64, C.c_char_p, C.c_char_p, vp, C.POINTER(vp)]),
        "oge_localrealign_multi": (C.c_int, [vp, C.c_int, C.c_char_p, u64, vp, vp, u64, C.c_char_p, C.c_char_p, vp,
                                             C.POINTER(vp)]),
        "oge_realign_result_count": (u64, [vp]),
        "oge_realign_result_records": (vp, [vp, C.POINTER(u64)]),
        "oge_realign_result_offsets": (vp, [vp]),
        "oge_realign_result_stats": (C.c_char_p, [vp]),
        "oge_realign_result_free": (None, [vp]),
        "oge_realign_synth_defaults": (None, [vp]),
        "oge_synth_realign": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]),
        "oge_bgzf_bound": (u64, [u64]),
        "oge_defl_emit_cap": (u32, []),
        "oge_bgzf_deflate_dev": (C.c_int, [vp, vp, u64, C.c_int, vp, u64, C.POINTER(u64)]),
        "oge_bgzf_deflate": (C.c_int, [vp, vp, u64, C.c_int, vp, u64, C.POINTER(u64)]),
        "oge_fix_bins_dev": (C.c_int, [vp, vp, vp, u64]),
        "oge_bgzf_index": (C.c_int, [vp, u64, vp, vp, vp, vp, u64, C.POINTER(u64)]),
        "oge_bgzf_inflate_dev": (C.c_int, [vp, vp, u64, vp, vp, vp, vp, u64, vp]),
        "oge_bgzf_inflate": (C.c_int, [vp, vp, u64, vp, u64, C.POINTER(u64)]),
        "oge_infl_plan": (u64, [u64, u64, u64, u64, C.c_int, vp, u64]),
        "oge_bam_record_offsets_dev": (C.c_int, [vp, vp, u64, u64, i32, vp, u64, C.POINTER(u64)]),
        "oge_drop_flagged_dev": (C.c_int, [vp, vp, vp, u64, C.c_uint16, vp, vp, C.POINTER(u64)]),
        "oge_filter_opts_init": (None, [vp]),
        "oge_parse_region": (C.c_int, [C.c_char_p, C.c_char_p, i32, vp, vp]),
        "oge_filter_records_dev": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, C.POINTER(u64)]),
        "oge_bai_open": (C.c_int, [vp, vp, u64, i32, C.POINTER(vp)]),
        "oge_bai_close": (None, [vp]),
        "oge_bai_query_dev": (C.c_int, [vp, vp, vp, u64, i32, C.POINTER(vp), C.POINTER(u64)]),
        "oge_bai_query": (C.c_int, [vp, vp, vp, u64, i32, vp, u64, C.POINTER(u64)]),
        "oge_bam_decode_ranges_dev": (C.c_int, [vp, vp, u64, vp, vp, u64, vp, u64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64),
                                                C.POINTER(u64)]),
        "oge_filter_regions_dev": (C.c_int, [vp, vp, vp, u64, vp, vp, u64, vp, vp, C.POINTER(u64)]),
        "oge_sort_name_dev": (C.c_int, [vp, vp, vp, u64, vp]),
        "oge_sort_name": (C.c_int, [vp, vp, u64, vp, u64, vp]),
        "oge_bgzf_index_dev": (C.c_int, [vp, vp, u64, vp, vp, vp, vp, u64, C.POINTER(u64)]),
        "oge_bai_build_dev": (C.c_int, [vp, vp, vp, u64, i32, u64, vp, vp, u64, C.POINTER(vp), C.POINTER(u64)]),
        "oge_bai_build": (C.c_int, [vp, vp, u64, vp, u64, i32, u64, vp, vp, u64, vp, u64, C.POINTER(u64)]),
        "oge_bam_index_dev": (C.c_int, [vp, vp, u64, C.POINTER(vp), C.POINTER(u64)]),
        "oge_ctx_last_bai": (C.c_int, [vp, C.POINTER(vp), C.POINTER(u64)]),
        "oge_stats_dev": (C.c_int, [vp, vp, vp, u64, u32, vp, C.POINTER(vp), C.POINTER(vp)]),
        "oge_stats": (C.c_int, [vp, vp, u64, vp, u64, u32, vp, vp, vp, u64]),
        "oge_compare_dev": (C.c_int, [vp, vp, vp, u64, vp, vp, u64, i32, vp, u32, C.c_int, vp, C.POINTER(vp), C.POINTER(u64)]),
        "oge_compare": (C.c_int, [vp, vp, u64, vp, u64, vp, u64, vp, u64, i32, vp, u32, C.c_int, vp, vp, u64, C.POINTER(u64)]),
        "oge_coverage_layout": (C.c_int, [i32, vp, i32, vp]),
        "oge_coverage_dev": (C.c_int, [vp, vp, vp, u64, i32, vp, i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(i32)]),
        "oge_coverage": (C.c_int, [vp, vp, u64, vp, u64, i32, vp, i32, vp, u64, C.POINTER(u64), C.POINTER(i32)]),
        "oge_targets_opts_init": (None, [vp]),
        "oge_targets_dev": (C.c_int, [vp, vp, vp, u64, i32, vp, C.c_char_p, u64, vp, vp, C.POINTER(vp), C.POINTER(vp)]),
        "oge_targets": (C.c_int, [vp, vp, u64, vp, u64, i32, vp, C.c_char_p, u64, vp, vp, vp, u64, vp, u64]),
        "oge_bam_targets_dev": (C.c_int, [vp, vp, u64, vp, vp, C.POINTER(vp), C.POINTER(vp)]),
        "oge_calmd_opts_init": (None, [vp]),
        "oge_calmd_dev": (C.c_int, [vp, vp, vp, u64, i32, C.c_char_p, u64, C.c_char_p, vp, vp, C.POINTER(vp), C.POINTER(vp)]),
        "oge_calmd": (C.c_int, [vp, vp, u64, vp, u64, i32, C.c_char_p, u64, C.c_char_p, vp, vp, vp, u64, vp]),
        "oge_bam_calmd_dev": (C.c_int, [vp, vp, u64, C.c_char_p, vp, vp, C.POINTER(vp), C.POINTER(vp)]),
        "oge_dup_metrics_dev": (C.c_int, [vp, vp, vp, u64, vp, i32, vp]),
        "oge_dup_metrics": (C.c_int, [vp, vp, u64, vp, u64, vp, i32, vp]),
        "oge_bam_dup_metrics_dev": (C.c_int, [vp, vp, u64, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), C.POINTER(u64), C.POINTER(i32)]),
        "oge_estimate_library_size": (C.c_int, [u64, u64, C.POINTER(u64)]),
        "oge_dup_metrics_text": (C.c_int, [vp, vp, i32, C.c_char_p, vp, u64, C.POINTER(u64)]),
        "oge_dup_sets_dev": (C.c_int, [vp, vp, vp, u64, vp, C.c_int64, i32, vp, vp]),
        "oge_dup_sets": (C.c_int, [vp, vp, u64, vp, u64, vp, C.c_int64, i32, vp, vp]),
        "oge_bam_dup_sets_dev": (C.c_int, [vp, vp, u64, C.c_int64, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]),
        "oge_dup_sets_text": (C.c_int, [vp, vp, vp, i32, vp, C.c_char_p, vp, u64, C.POINTER(u64)]),
        "oge_bam_stats_dev": (C.c_int, [vp, vp, u64, u32, vp, C.POINTER(vp), C.POINTER(vp)]),
        "oge_bam_coverage_dev": (C.c_int, [vp, vp, u64, i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)]),
        "oge_bam_count_dev": (C.c_int, [vp, vp, u64, C.POINTER(u64)]),
        "oge_ctx_last_refs": (C.c_int, [vp, C.POINTER(i32), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp)]),
        "oge_text_size_dev": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)]),
        "oge_text_emit_dev": (C.c_int, [vp, vp, vp, vp, u64, u64, vp, vp, u64]),
        "oge_text_host_line": (C.c_int, [vp, u64, vp, vp, u64, C.POINTER(u64)]),
        "oge_text_format": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, u64, C.POINTER(u64)]),
        "oge_sam_header": (C.c_int, [vp, u64, C.POINTER(u64), C.POINTER(u64)]),
        "oge_sam_lines_dev": (C.c_int, [vp, vp, u64, u64, vp, u64, C.POINTER(u64)]),
        "oge_sam_size_dev": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)]),
        "oge_sam_emit_dev": (C.c_int, [vp, vp, vp, vp, u64, u64, vp, vp, u64]),
        "oge_sam_host_record": (C.c_int, [vp, u64, vp, vp, u64, C.POINTER(u64)]),
        "oge_sam_parse": (C.c_int, [vp, vp, u64, C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp)]),
        "oge_mergesort_opts_init": (None, [vp]),
        "oge_mergesort_bgzf_dev": (C.c_int, [vp, vp, u64, vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64),
                                             C.POINTER(u64)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name, None)
        if f is None:
            continue
        f.restype, f.argtypes = res, args
    _lib = L
    return L


def filter_opts(**over) -> FilterOpts:
    """Filter::Filter() defaults (algorithms/filter.cpp:185-194) with overrides."""
    o = FilterOpts()
    lib().oge_filter_opts_init(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


def parse_region(region: str, refs: list[tuple[str, int]], opts: FilterOpts | None = None) -> FilterOpts:
    """Filter::ParseRegionString through the C ABI; raises OgeError with the reference's message."""
    o = opts if opts is not None else filter_opts()
    names = b"".join(nm.encode() + b"\0" for nm, _ in refs)
    lens = np.array([ln for _, ln in refs] or [0], dtype=np.int64)
    check(lib().oge_parse_region(region.encode(), names, len(refs), _ptr(lens), C.byref(o)))
    return o


def infl_plan(nblk: int, lanes: int, budget: int, max_per_lane: int = 0, balanced: bool = False) -> list[int]:
    """oge_infl_plan: the sizes of the phase-1 launches the inflate cuts nblk blocks into (host arithmetic, no
    device); max_per_lane 0 is the build's value."""
    n = int(lib().oge_infl_plan(nblk, lanes, budget, max_per_lane, int(balanced), None, 0))
    sizes = np.zeros(max(n, 1), dtype=np.uint64)
    lib().oge_infl_plan(nblk, lanes, budget, max_per_lane, int(balanced), _ptr(sizes), n)
    return [int(x) for x in sizes[:n]]


def estimate_library_size(pairs: int, unique_pairs: int) -> int | None:
    """oge_estimate_library_size (host only): Picard's estimate, None when there is none."""
    size = C.c_uint64()
    return None if lib().oge_estimate_library_size(pairs, unique_pairs, C.byref(size)) else size.value


def dup_metrics_text(rows, command_line: str, cap: int | None = None) -> bytes:
    """oge_dup_metrics_text (host only): rows = [(library name, the six counters of oge_dup_metrics)] -> the
    metrics file.  cap: the buffer of the second call (default: the size the first call reports, + 1 for the NUL);
    a smaller one gets the text cut to cap - 1 bytes."""
    names = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm, _ in rows]
    arr = (C.c_char_p * max(len(rows), 1))(*names)
    m = np.array([list(c6) for _, c6 in rows] or [[0] * 6], dtype=np.uint64)
    need = C.c_uint64()
    check(lib().oge_dup_metrics_text(arr, _ptr(m), len(rows), command_line.encode(), None, 0, C.byref(need)))
    cap = need.value + 1 if cap is None else cap
    buf = C.create_string_buffer(max(cap, 1))
    check(lib().oge_dup_metrics_text(arr, _ptr(m), len(rows), command_line.encode(), buf, cap, C.byref(need)))
    return buf.raw[:min(max(cap, 1) - 1, need.value)]


DUP_SETS_BINS = 1024  # OGE_DUP_SETS_BINS


def dup_sets_text(rows, hist, command_line: str) -> bytes:
    """oge_dup_sets_text (host only): rows = [(library name, the six counters of oge_dup_metrics, the four of
    oge_dup_sets_lib)], hist = the three histogram columns (3, DUP_SETS_BINS) -> the metrics file with the optical
    column and the set-size histogram."""
    names = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm, _, _ in rows]
    arr = (C.c_char_p * max(len(rows), 1))(*names)
    m = np.array([list(c6) for _, c6, _ in rows] or [[0] * 6], dtype=np.uint64)
    s4 = np.array([list(c4) for _, _, c4 in rows] or [[0] * 4], dtype=np.uint64)
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(3 * DUP_SETS_BINS)
    need = C.c_uint64()
    check(lib().oge_dup_sets_text(arr, _ptr(m), _ptr(s4), len(rows), _ptr(h), command_line.encode(), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value + 1)
    check(lib().oge_dup_sets_text(arr, _ptr(m), _ptr(s4), len(rows), _ptr(h), command_line.encode(), buf, need.value + 1, C.byref(need)))
    return buf.raw[:need.value]


def exported_symbols() -> list[str]:
    """Symbols include/openge_hip.h declares (parsed from the header)."""
    import re

    text = (PKG.parent / "include" / "openge_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(oge_[a-z0-9_]+)\s*\(", text)))


def check(rc: int, ctx=None) -> None:
    if rc != 0:
        msg = lib().oge_last_error(ctx)
        raise OgeError(f"openge_hip error {rc}: {msg.decode() if msg else ''}")


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


# ------------------------------------------------------------------------- synthetic data (host)
def synth_host(p: SynthParams, threads: int = 0) -> tuple[np.ndarray, np.ndarray, str]:
    """Generate the records on the host: (recs u8, offs u64[n+1], header text)."""
    L = lib()
    check(L.oge_synth_finalize(C.byref(p)))
    n = 2 * p.n_pairs
    offs = np.empty(n + 1, dtype=np.uint64)
    check(L.oge_synth_offsets_host(C.byref(p), _ptr(offs), threads))
    recs = np.empty(int(offs[-1]) + 16, dtype=np.uint8)
    recs[-16:] = 0
    check(L.oge_synth_records_host(C.byref(p), _ptr(offs), _ptr(recs), threads))
    ln = C.c_uint64()
    check(L.oge_synth_header_text(C.byref(p), None, 0, C.byref(ln)))
    buf = C.create_string_buffer(ln.value + 1)
    check(L.oge_synth_header_text(C.byref(p), buf, ln.value + 1, None))
    return recs, offs, buf.value.decode()


# ------------------------------------------------------------------------- BAM files
class Bam:
    """A BAM file decoded into one record arena (records in file order)."""

    def __init__(self, path: str | os.PathLike, threads: int = 8):
        L = lib()
        h = C.c_void_p()
        check(L.oge_bam_read(str(path).encode(), threads, C.byref(h)))
        self._h = h
        n = L.oge_bam_count(h)
        nb = C.c_uint64()
        rp = L.oge_bam_records(h, C.byref(nb))
        self.n = int(n)
        self.recs = np.ctypeslib.as_array((C.c_uint8 * nb.value).from_address(rp)) if nb.value else np.zeros(0, np.uint8)
        op = L.oge_bam_offsets(h)
        self.offs = np.ctypeslib.as_array((C.c_uint64 * self.n).from_address(op)) if self.n else np.zeros(0, np.uint64)
        self.n_ref = int(L.oge_bam_n_ref(h))
        ln = C.c_uint64()
        check(L.oge_bam_header_text(h, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(ln.value + 1)
        check(L.oge_bam_header_text(h, buf, ln.value + 1, None))
        self.header_text = buf.value.decode()

    def markdup_opts(self) -> tuple[MarkdupOpts, tuple]:
        o = MarkdupOpts()
        ids, libs = C.c_void_p(), C.c_void_p()
        check(lib().oge_bam_markdup_opts(self._h, C.byref(o), C.byref(ids), C.byref(libs)))
        return o, (ids, libs)

    def __del__(self):
        try:
            lib().oge_bam_free(self._h)
        except Exception:
            pass


def markdup_opts_from_header(header_text: str, n_ref: int, compat_nonverbose: bool = False,
                             split_chains: int = 0) -> tuple[MarkdupOpts, tuple]:
    """RG -> library table as MarkDuplicates::getLibraryName resolves it (mark_duplicates.cpp:301-318)."""
    ids, libs, names = [], [], {}
    for line in header_text.splitlines():
        if not line.startswith("@RG\t"):
            continue
        f = dict(x.split(":", 1) for x in line.split("\t")[1:] if len(x) >= 3)
        lb = f.get("LB", "") or "Unknown Library"
        names.setdefault(lb, len(names) + 1)
        ids.append(f.get("ID", ""))
        libs.append(names[lb])
    unknown = names.get("Unknown Library", len(names) + 1)
    idbuf = b"".join(i.encode() + b"\0" for i in ids)
    ida = np.frombuffer(idbuf + b"\0", dtype=np.uint8).copy()
    liba = np.array(libs + [0], dtype=np.int16)
    o = MarkdupOpts()
    o.n_ref, o.rg_ids, o.rg_ids_bytes = n_ref, _ptr(ida), len(idbuf)
    o.rg_lib, o.n_rg, o.unknown_lib = _ptr(liba), len(ids), unknown
    o.compat_nonverbose_index = 1 if compat_nonverbose else 0
    o.split_chains = split_chains
    return o, (ida, liba)


def write_bam(path, header_text: str, recs: np.ndarray, offs: np.ndarray, n: int, order=None, flags=None,
              sort_order: int = -1, level: int = 6, threads: int = 8) -> None:
    L = lib()
    hb = header_text.encode()
    check(L.oge_bam_write(str(path).encode(), hb, len(hb), sort_order, _ptr(recs), _ptr(offs), n,
                          _ptr(order) if order is not None else None, _ptr(flags) if flags is not None else None,
                          level, threads))


# ------------------------------------------------------------------------- device context
class _RealignResult:
    """Owns an oge_realign_result; the record/offset arrays returned by Context.localrealign are
    zero-copy views that keep it alive."""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        if self.h:
            lib().oge_realign_result_free(self.h)
            self.h = None


class Context:
    """A HIP device context (one per process/GPU)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        L = lib()
        h = C.c_void_p()
        check(L.oge_ctx_create(device, C.byref(h)))
        self.h = h
        if stream:
            check(L.oge_ctx_set_stream(h, C.c_void_p(stream)), h)

    def close(self):
        if self.h:
            lib().oge_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return lib().oge_ctx_stream(self.h) or 0

    def sync(self):
        check(lib().oge_ctx_sync(self.h), self.h)

    def counter(self, name: str) -> int | None:
        """A work count of the last pipeline call (oge_ctx_counter), None when it recorded none."""
        v = C.c_uint64()
        return v.value if lib().oge_ctx_counter(self.h, name.encode(), C.byref(v)) == 0 else None

    def timing(self, stage: str) -> float:
        ms = C.c_double()
        check(lib().oge_ctx_timing(self.h, stage.encode(), C.byref(ms)), self.h)
        return ms.value

    # host-buffer entry points
    def sort_coord(self, recs: np.ndarray, offs: np.ndarray, n: int, n_ref: int) -> np.ndarray:
        perm = np.empty(max(n, 1), dtype=np.uint32)
        check(lib().oge_sort_coord(self.h, _ptr(recs), recs.nbytes, _ptr(offs), n, n_ref, _ptr(perm)), self.h)
        return perm[:n]

    def markdup(self, recs: np.ndarray, offs: np.ndarray, n: int, opts: MarkdupOpts) -> tuple[np.ndarray, int]:
        dup = np.empty(max(n, 1), dtype=np.uint8)
        nd = C.c_uint64()
        check(lib().oge_markdup(self.h, _ptr(recs), recs.nbytes, _ptr(offs), n, C.byref(opts), _ptr(dup),
                                C.byref(nd)), self.h)
        return dup[:n], nd.value

    # device entry points (pointers are ints, e.g. torch tensor .data_ptr())
    def sort_coord_dev(self, d_recs: int, d_off: int, n: int, n_ref: int, d_perm: int) -> None:
        check(lib().oge_sort_coord_dev(self.h, d_recs, d_off, n, n_ref, d_perm), self.h)

    def gather_records_dev(self, d_recs, d_off, d_perm, n, d_out, d_out_off) -> None:
        check(lib().oge_gather_records_dev(self.h, d_recs, d_off, d_perm, n, d_out, d_out_off), self.h)

    def radix_sort_pairs_dev(self, d_keys, d_vals, d_ktmp, d_vtmp, n, bit_mask) -> bool:
        """Stable radix sort of device (u64 key, u32 value) pairs on the bits of bit_mask; returns True
        when the result sits in the tmp buffers."""
        t = C.c_int()
        check(lib().oge_radix_sort_pairs_dev(self.h, d_keys, d_vals, d_ktmp, d_vtmp, n, bit_mask, C.byref(t)), self.h)
        return bool(t.value)

    def exclusive_scan_dev(self, d_in, d_out, n: int, elem_bytes: int) -> None:
        """oge_exclusive_scan_dev: exclusive prefix sum of n u32 (elem_bytes 4) or u64 (8) device elements."""
        check(lib().oge_exclusive_scan_dev(self.h, d_in, d_out, n, elem_bytes), self.h)

    def set_deflate_search(self, search: str | int) -> None:
        """The GPU deflate's match search for this context: "fast" (0, the default), "near" (1), "span" (2)
        or "near+span" (3) -- see oge_ctx_set_deflate_search."""
        if isinstance(search, str):
            if search not in DEFLATE_SEARCH:
                raise OgeError(f"deflate search {search!r}: one of {', '.join(DEFLATE_SEARCH)}")
            search = DEFLATE_SEARCH.index(search)
        check(lib().oge_ctx_set_deflate_search(self.h, int(search)), self.h)

    @property
    def deflate_search(self) -> int:
        return lib().oge_ctx_deflate_search(self.h)

    @contextlib.contextmanager
    def _search(self, search: str | int | None):
        """search for the duration of one call (None: the context's own)."""
        if search is None:
            yield
            return
        old = self.deflate_search
        self.set_deflate_search(search)
        try:
            yield
        finally:
            self.set_deflate_search(old)

    def bgzf_deflate(self, data: bytes | np.ndarray, level: int = 6, search: str | int | None = None) -> bytes:
        """BGZF-compress host bytes on the device (no EOF marker)."""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
        cap = int(lib().oge_bgzf_bound(len(a)))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        got = C.c_uint64()
        with self._search(search):
            check(lib().oge_bgzf_deflate(self.h, _ptr(a), len(a), level, _ptr(out), cap, C.byref(got)), self.h)
        return out[:got.value].tobytes()

    def bgzf_deflate_dev(self, d_src, n: int, level: int, d_dst, dst_cap: int, search: str | int | None = None) -> int:
        got = C.c_uint64()
        with self._search(search):
            check(lib().oge_bgzf_deflate_dev(self.h, d_src, n, level, d_dst, dst_cap, C.byref(got)), self.h)
        return got.value

    def bgzf_inflate(self, z: bytes, out_cap: int | None = None) -> bytes:
        """Decompress a BGZF stream on the device (host buffers in and out)."""
        a = np.frombuffer(z, dtype=np.uint8)
        nb = C.c_uint64()
        lib().oge_bgzf_index(_ptr(a), len(a), None, None, None, None, 0, C.byref(nb))
        uo = np.zeros(nb.value + 1, dtype=np.uint64)
        if nb.value:
            check(lib().oge_bgzf_index(_ptr(a), len(a), None, None, _ptr(uo), None, nb.value, C.byref(nb)))
        cap = int(uo[-1]) if out_cap is None else out_cap
        out = np.empty(max(cap, 1), dtype=np.uint8)
        got = C.c_uint64()
        check(lib().oge_bgzf_inflate(self.h, _ptr(a), len(a), _ptr(out), cap, C.byref(got)), self.h)
        return out[:got.value].tobytes()

    def bgzf_index_dev(self, d_z, zbytes: int, d_d0=None, d_d1=None, d_uoff=None, d_crc=None, cap: int = 0) -> int:
        nb = C.c_uint64()
        check(lib().oge_bgzf_index_dev(self.h, d_z, zbytes, d_d0, d_d1, d_uoff, d_crc, cap, C.byref(nb)), self.h)
        return nb.value

    def mergesort_bgzf_dev(self, d_z, zbytes: int, opts: "MergesortOpts") -> tuple[int, int, int, int]:
        """The whole mergesort [-M] chain on a BAM file resident in HBM -> (d_out, out_bytes, n_reads,
        n_dup); d_out (device pointer) is valid until the next call on this context."""
        d = C.c_void_p()
        ob, nr, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().oge_mergesort_bgzf_dev(self.h, d_z, zbytes, C.byref(opts), C.byref(d), C.byref(ob), C.byref(nr),
                                           C.byref(nd)), self.h)
        return d.value or 0, ob.value, nr.value, nd.value

    def _fetch(self, d: int, nbytes: int) -> bytes:
        out = np.empty(max(nbytes, 1), dtype=np.uint8)
        check(lib().oge_memcpy(self.h, _ptr(out), d, nbytes, 2), self.h)
        return out[:nbytes].tobytes()

    def bai_build_dev(self, d_recs, d_off, n: int, n_ref: int, stream_base: int, d_uoff, d_cstart, nblk: int) -> bytes:
        """oge_bai_build_dev: the .bai image of coordinate-sorted device records (d_off: n offsets; block table
        d_uoff / d_cstart: nblk + 1 entries each), copied to the host."""
        d, nb = C.c_void_p(), C.c_uint64()
        check(lib().oge_bai_build_dev(self.h, d_recs, d_off, n, n_ref, stream_base, d_uoff, d_cstart, nblk, C.byref(d),
                                      C.byref(nb)), self.h)
        return self._fetch(d.value, nb.value)

    def bai_build(self, recs: np.ndarray, offs: np.ndarray, n: int, n_ref: int, stream_base: int, uoff: np.ndarray,
                  cstart: np.ndarray) -> bytes:
        """oge_bai_build: the same from host buffers."""
        uoff = np.ascontiguousarray(uoff, dtype=np.uint64)
        cstart = np.ascontiguousarray(cstart, dtype=np.uint64)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nb = C.c_uint64()
        args = (self.h, _ptr(recs), recs.nbytes, _ptr(offs), n, n_ref, stream_base, _ptr(uoff), _ptr(cstart), len(uoff) - 1)
        rc = lib().oge_bai_build(*args, None, 0, C.byref(nb))
        if rc != -3 or not nb.value:  # OGE_ERR_LIMIT with the size: the sizing call
            check(rc, self.h)
        out = np.empty(nb.value, dtype=np.uint8)
        check(lib().oge_bai_build(*args, _ptr(out), out.nbytes, C.byref(nb)), self.h)
        return out[:nb.value].tobytes()

    def bam_index(self, bam_bytes: bytes) -> bytes:
        """The .bai image of a whole BAM file (oge_bam_index_dev on a copy of the file in HBM)."""
        a = np.frombuffer(bam_bytes, dtype=np.uint8)
        dz = C.c_void_p()
        check(lib().oge_dev_alloc(self.h, len(a) + 64, C.byref(dz)), self.h)
        try:
            check(lib().oge_memcpy(self.h, dz, _ptr(a), len(a), 1), self.h)
            d, nb = C.c_void_p(), C.c_uint64()
            check(lib().oge_bam_index_dev(self.h, dz, len(a), C.byref(d), C.byref(nb)), self.h)
            return self._fetch(d.value, nb.value)
        finally:
            lib().oge_dev_free(self.h, dz)

    def last_bai(self) -> bytes:
        """The index the context's last call built (oge_ctx_last_bai); OgeError when there is none."""
        d, nb = C.c_void_p(), C.c_uint64()
        check(lib().oge_ctx_last_bai(self.h, C.byref(d), C.byref(nb)), self.h)
        return self._fetch(d.value, nb.value)

    # ---- stats / count / coverage (csrc/qc.hip)
    def _stats_dict(self, st: BamStats, d_len, d_cnt, lengths: bool) -> dict:
        out = {k: getattr(st, k) for k in BamStats.COUNTERS}
        out["sorted"] = bool(st.sorted)
        for k in ("n_insert", "insert_sum", "insert_mid_lo", "insert_mid_hi"):
            out[k] = getattr(st, k)
        if lengths:
            m = st.n_lengths
            out["lengths"] = (np.frombuffer(self._fetch(d_len.value or 0, 4 * m), np.uint32).copy(),
                              np.frombuffer(self._fetch(d_cnt.value or 0, 8 * m), np.uint64).copy())
        return out

    @staticmethod
    def _want(inserts: bool, lengths: bool) -> int:
        return (STATS_INSERTS if inserts else 0) | (STATS_LENGTHS if lengths else 0)

    def stats_dev(self, d_recs, d_off, n: int, inserts: bool = False, lengths: bool = False) -> dict:
        """oge_stats_dev on device records (d_off: n offsets) -> the counters, `sorted`, the insert figures and,
        with lengths, `lengths` = (l_seq values ascending, their counts)."""
        st, dl, dc = BamStats(), C.c_void_p(), C.c_void_p()
        check(lib().oge_stats_dev(self.h, d_recs, d_off, n, self._want(inserts, lengths), C.byref(st), C.byref(dl), C.byref(dc)), self.h)
        return self._stats_dict(st, dl, dc, lengths)

    def stats(self, recs: np.ndarray, offs: np.ndarray, n: int, inserts: bool = False, lengths: bool = False) -> dict:
        """oge_stats: the same from host buffers."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        st = BamStats()
        args = (self.h, _ptr(recs), recs.nbytes, _ptr(offs), n, self._want(inserts, lengths), C.byref(st))
        rc = lib().oge_stats(*args, None, None, 0)
        if not (rc == -3 and lengths and st.n_lengths):  # OGE_ERR_LIMIT with the size: the sizing call
            check(rc, self.h)
        ln, ct = np.empty(max(st.n_lengths, 1), np.uint32), np.empty(max(st.n_lengths, 1), np.uint64)
        if rc:
            check(lib().oge_stats(*args, _ptr(ln), _ptr(ct), len(ln)), self.h)
        out = self._stats_dict(st, C.c_void_p(), C.c_void_p(), False)
        if lengths:
            out["lengths"] = (ln[:st.n_lengths], ct[:st.n_lengths])
        return out

    # ---- compare (csrc/compare.hip)
    def compare_dev(self, d_recs_a, d_off_a, n_a: int, d_recs_b, d_off_b, n_b: int, n_ref: int, region=COMPARE_ALL,
                    diff: bool = False, hash_bits: int = -1) -> dict:
        """oge_compare_dev on two device record sets (set a is the reference set) -> the counts of
        oge_compare_result and, with diff, `diff` = the decoded image (decode_compare_diff)."""
        rg, res, dd, nb = CompareRegion(*region), CompareResult(), C.c_void_p(), C.c_uint64()
        check(lib().oge_compare_dev(self.h, d_recs_a, d_off_a, n_a, d_recs_b, d_off_b, n_b, n_ref, C.byref(rg),
                                    COMPARE_DIFF if diff else 0, hash_bits, C.byref(res), C.byref(dd), C.byref(nb)), self.h)
        out = {k: getattr(res, k) for k in CompareResult.FIELDS}
        if diff:
            out["diff"] = decode_compare_diff(self._fetch(dd.value or 0, nb.value))
        return out

    def compare(self, recs_a: np.ndarray, offs_a: np.ndarray, n_a: int, recs_b: np.ndarray, offs_b: np.ndarray, n_b: int, n_ref: int,
                region=COMPARE_ALL, diff: bool = False, hash_bits: int = -1) -> dict:
        """oge_compare: the same from host buffers (a sizing call, then the call that copies the image)."""
        offs_a, offs_b = np.ascontiguousarray(offs_a, dtype=np.uint64), np.ascontiguousarray(offs_b, dtype=np.uint64)
        rg, res, nb = CompareRegion(*region), CompareResult(), C.c_uint64()
        args = (self.h, _ptr(recs_a), recs_a.nbytes, _ptr(offs_a), n_a, _ptr(recs_b), recs_b.nbytes, _ptr(offs_b),
                n_b, n_ref, C.byref(rg), COMPARE_DIFF if diff else 0, hash_bits, C.byref(res))
        rc = lib().oge_compare(*args, None, 0, C.byref(nb))
        if not (rc == -3 and diff and nb.value):  # OGE_ERR_LIMIT with the size: the sizing call
            check(rc, self.h)
        buf = np.empty(max(nb.value, 1), np.uint8)
        if rc:
            check(lib().oge_compare(*args, _ptr(buf), len(buf), C.byref(nb)), self.h)
        out = {k: getattr(res, k) for k in CompareResult.FIELDS}
        if diff:
            out["diff"] = decode_compare_diff(buf[:nb.value].tobytes())
        return out

    # ---- realignment targets (csrc/targets.hip)
    @staticmethod
    def _targets_opts(max_interval: int, gap: int) -> TargetsOpts:
        o = TargetsOpts()
        lib().oge_targets_opts_init(C.byref(o))
        o.max_interval, o.gap, o.want = max_interval, gap, TARGETS_TEXT
        return o

    def _targets_out(self, res: TargetsResult, dt, dx) -> tuple[dict, np.ndarray, bytes]:
        raw = np.frombuffer(self._fetch(dt.value or 0, 16 * res.targets), np.int32).reshape(res.targets, 4).astype(np.int64)
        raw[:, 3] &= 0xFFFFFFFF  # n_events is unsigned
        return {k: getattr(res, k) for k in TargetsResult.FIELDS}, raw, self._fetch(dx.value or 0, res.text_bytes)

    def targets_dev(self, d_recs, d_off, n: int, refs, max_interval: int = 500, gap: int = 0) -> tuple[dict, np.ndarray, bytes]:
        """oge_targets_dev on device records; refs = [(name, length)] -> (the counters of oge_targets_result, the
        intervals as int64 (targets, 4): refID, start, stop, n_events, the text "contig:start-stop\\n" per interval)."""
        lens, names = _ref_table(refs)
        o, res, dt, dx = self._targets_opts(max_interval, gap), TargetsResult(), C.c_void_p(), C.c_void_p()
        check(lib().oge_targets_dev(self.h, d_recs, d_off, n, len(lens), _ptr(lens) if len(lens) else None, names, len(names),
                                    C.byref(o), C.byref(res), C.byref(dt), C.byref(dx)), self.h)
        return self._targets_out(res, dt, dx)

    def targets(self, recs: np.ndarray, offs: np.ndarray, n: int, refs, max_interval: int = 500, gap: int = 0) -> tuple[dict, np.ndarray, bytes]:
        """oge_targets: the same from host buffers (a sizing call, then the call that copies the outputs)."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens, names = _ref_table(refs)
        o, res = self._targets_opts(max_interval, gap), TargetsResult()
        args = (self.h, _ptr(recs), max(recs.nbytes - 16, 0), _ptr(offs), n, len(lens), _ptr(lens) if len(lens) else None, names,
                len(names), C.byref(o), C.byref(res))
        rc = lib().oge_targets(*args, None, 0, None, 0)
        if not (rc == -3 and res.targets):  # OGE_ERR_LIMIT with the sizes: the sizing call
            check(rc, self.h)
        arr, text = np.zeros((max(res.targets, 1), 4), np.int32), np.zeros(max(res.text_bytes, 1), np.uint8)
        if rc:
            check(lib().oge_targets(*args, _ptr(arr), res.targets, _ptr(text), res.text_bytes), self.h)
        out = arr[:res.targets].astype(np.int64)
        out[:, 3] &= 0xFFFFFFFF
        return {k: getattr(res, k) for k in TargetsResult.FIELDS}, out, text[:res.text_bytes].tobytes()

    def bam_targets(self, data: bytes, max_interval: int = 500, gap: int = 0) -> tuple[dict, np.ndarray, bytes]:
        """`openge targets` of a whole BAM file (oge_bam_targets_dev on a copy of the file in HBM)."""
        def run(dz, nbytes):
            o, res, dt, dx = self._targets_opts(max_interval, gap), TargetsResult(), C.c_void_p(), C.c_void_p()
            check(lib().oge_bam_targets_dev(self.h, dz, nbytes, C.byref(o), C.byref(res), C.byref(dt), C.byref(dx)), self.h)
            return self._targets_out(res, dt, dx)
        return self._with_file(data, run)

    # ---- NM / MD tags (csrc/calmd.hip)
    @staticmethod
    def _calmd_opts(threads: int) -> CalmdOpts:
        o = CalmdOpts()
        lib().oge_calmd_opts_init(C.byref(o))
        o.threads = threads
        return o

    def _calmd_out(self, res: CalmdResult, n: int, dr, do) -> tuple[dict, np.ndarray, np.ndarray]:
        recs = np.frombuffer(self._fetch(dr.value or 0, res.bytes_out), np.uint8)
        offs = np.frombuffer(self._fetch(do.value or 0, 8 * (n + 1)), np.uint64)
        return {k: getattr(res, k) for k in CalmdResult.FIELDS}, recs, offs

    def calmd_dev(self, d_recs, d_off, n: int, refs, fasta: str, threads: int = 0) -> tuple[dict, np.ndarray, np.ndarray]:
        """oge_calmd_dev on device records; refs = [(name, length)], fasta = the reference's path -> (the counters of
        oge_calmd_result, the new records as uint8, their n + 1 offsets as uint64)."""
        _, names = _ref_table(refs)
        o, res, dr, do = self._calmd_opts(threads), CalmdResult(), C.c_void_p(), C.c_void_p()
        check(lib().oge_calmd_dev(self.h, d_recs, d_off, n, len(refs), names, len(names), fasta.encode(), C.byref(o), C.byref(res),
                                  C.byref(dr), C.byref(do)), self.h)
        return self._calmd_out(res, n, dr, do)

    def calmd(self, recs: np.ndarray, offs: np.ndarray, n: int, refs, fasta: str, threads: int = 0) -> tuple[dict, np.ndarray, np.ndarray]:
        """oge_calmd: the same from host buffers (a sizing call, then the call that copies the records)."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        _, names = _ref_table(refs)
        o, res = self._calmd_opts(threads), CalmdResult()
        out_off = np.zeros(n + 1, np.uint64)
        args = (self.h, _ptr(recs), max(recs.nbytes - 16, 0), _ptr(offs), n, len(refs), names, len(names), fasta.encode(), C.byref(o),
                C.byref(res))
        rc = lib().oge_calmd(*args, None, 0, _ptr(out_off))
        if not (rc == -3 and res.bytes_out):  # OGE_ERR_LIMIT with the size: the sizing call
            check(rc, self.h)
        out = np.zeros(max(res.bytes_out, 1), np.uint8)
        if rc:
            check(lib().oge_calmd(*args, _ptr(out), res.bytes_out, _ptr(out_off)), self.h)
        return {k: getattr(res, k) for k in CalmdResult.FIELDS}, out[:res.bytes_out], out_off

    def bam_calmd(self, data: bytes, fasta: str, threads: int = 0) -> tuple[dict, np.ndarray, np.ndarray]:
        """`openge calmd` of a whole BAM file (oge_bam_calmd_dev on a copy of the file in HBM)."""
        def run(dz, nbytes):
            o, res, dr, do = self._calmd_opts(threads), CalmdResult(), C.c_void_p(), C.c_void_p()
            check(lib().oge_bam_calmd_dev(self.h, dz, nbytes, fasta.encode(), C.byref(o), C.byref(res), C.byref(dr), C.byref(do)), self.h)
            return self._calmd_out(res, res.records, dr, do)
        return self._with_file(data, run)

    # ---- duplication metrics (csrc/dupmetrics.hip)
    def dup_metrics_dev(self, d_recs, d_off, n: int, opts: MarkdupOpts, n_lib: int) -> np.ndarray:
        """oge_dup_metrics_dev on device records -> uint64 (n_lib, 6): the fields of oge_dup_metrics by library id."""
        out = np.full((max(n_lib, 1), 6), 0xDEADBEEF, np.uint64)  # the call sets it
        check(lib().oge_dup_metrics_dev(self.h, d_recs, d_off, n, C.byref(opts), n_lib, _ptr(out)), self.h)
        return out[:n_lib]

    def dup_metrics(self, recs: np.ndarray, offs: np.ndarray, n: int, opts: MarkdupOpts, n_lib: int) -> np.ndarray:
        """oge_dup_metrics: the same from host buffers (recs with 16 bytes of slack behind the last record)."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        out = np.full((max(n_lib, 1), 6), 0xDEADBEEF, np.uint64)
        check(lib().oge_dup_metrics(self.h, _ptr(recs), max(recs.nbytes - 16, 0), _ptr(offs), n, C.byref(opts), n_lib, _ptr(out)), self.h)
        return out[:n_lib]

    def bam_dup_metrics(self, data: bytes) -> tuple[np.ndarray, list[str], int]:
        """`openge dupmetrics` of a whole BAM file (oge_bam_dup_metrics_dev on a copy of the file in HBM) -> (the
        counters (n_lib, 6), the library names by id, "" where no @RG names the id, unknown_lib)."""
        def run(dz, nbytes):
            po, n, pn, nb, unk = C.c_void_p(), C.c_int32(), C.c_void_p(), C.c_uint64(), C.c_int32()
            check(lib().oge_bam_dup_metrics_dev(self.h, dz, nbytes, C.byref(po), C.byref(n), C.byref(pn), C.byref(nb), C.byref(unk)), self.h)
            out = np.frombuffer(C.string_at(po.value, 48 * n.value), np.uint64).reshape(n.value, 6).copy()
            names = C.string_at(pn.value, nb.value).split(b"\0")[:n.value]
            return out, [x.decode() for x in names], unk.value
        return self._with_file(data, run)

    # ---- duplicate sets: optical duplicates and set-size histograms (csrc/dupsets.hip)
    def dup_sets_dev(self, d_recs, d_off, n: int, opts: MarkdupOpts, distance: int, n_lib: int) -> tuple[np.ndarray, np.ndarray]:
        """oge_dup_sets_dev on device records -> (uint64 (n_lib, 4): pairs, sets, located, optical by library id,
        uint64 (3, DUP_SETS_BINS): all_sets, optical_sets, non_optical_sets)."""
        out = np.full((max(n_lib, 1), 4), 0xDEADBEEF, np.uint64)  # the call sets both
        hist = np.full((3, DUP_SETS_BINS), 0xDEADBEEF, np.uint64)
        check(lib().oge_dup_sets_dev(self.h, d_recs, d_off, n, C.byref(opts), distance, n_lib, _ptr(out), _ptr(hist)), self.h)
        return out[:n_lib], hist

    def dup_sets(self, recs: np.ndarray, offs: np.ndarray, n: int, opts: MarkdupOpts, distance: int, n_lib: int) -> tuple[np.ndarray, np.ndarray]:
        """oge_dup_sets: the same from host buffers (recs with 16 bytes of slack behind the last record)."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        out = np.full((max(n_lib, 1), 4), 0xDEADBEEF, np.uint64)
        hist = np.full((3, DUP_SETS_BINS), 0xDEADBEEF, np.uint64)
        check(lib().oge_dup_sets(self.h, _ptr(recs), max(recs.nbytes - 16, 0), _ptr(offs), n, C.byref(opts), distance, n_lib, _ptr(out), _ptr(hist)), self.h)
        return out[:n_lib], hist

    def bam_dup_sets(self, data: bytes, distance: int) -> tuple[np.ndarray, np.ndarray]:
        """oge_bam_dup_sets_dev on a copy of a whole BAM file in HBM: the libraries numbered from its own header."""
        def run(dz, nbytes):
            po, ph, n = C.c_void_p(), C.c_void_p(), C.c_int32()
            check(lib().oge_bam_dup_sets_dev(self.h, dz, nbytes, distance, C.byref(po), C.byref(ph), C.byref(n)), self.h)
            out = np.frombuffer(C.string_at(po.value, 32 * n.value), np.uint64).reshape(n.value, 4).copy()
            hist = np.frombuffer(C.string_at(ph.value, 24 * DUP_SETS_BINS), np.uint64).reshape(3, DUP_SETS_BINS).copy()
            return out, hist
        return self._with_file(data, run)

    # ---- SAM / FASTQ text (csrc/sam.hip)
    def text_size_dev(self, d_recs, d_off, n: int, opts: TextOpts, d_text_off, d_host_mark) -> tuple[int, int]:
        """oge_text_size_dev: fills d_text_off (n + 1 u64) and d_host_mark (n u8) -> (device text bytes, host lines)."""
        total, n_host = C.c_uint64(), C.c_uint64()
        check(lib().oge_text_size_dev(self.h, d_recs, d_off, n, C.byref(opts), d_text_off, d_host_mark, C.byref(total), C.byref(n_host)), self.h)
        return total.value, n_host.value

    def text_emit_dev(self, d_recs, d_off, d_text_off, first: int, count: int, opts: TextOpts, d_out, cap: int) -> None:
        """oge_text_emit_dev: the text of records [first, first + count) at d_out."""
        check(lib().oge_text_emit_dev(self.h, d_recs, d_off, d_text_off, first, count, C.byref(opts), d_out, cap), self.h)

    def text_format(self, recs: np.ndarray, offs: np.ndarray, n: int, opts: TextOpts) -> bytes:
        """oge_text_format: the whole text of host records, the host-formatted lines spliced in."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nb = C.c_uint64()
        args = (self.h, _ptr(recs), max(recs.nbytes - 16, 0), _ptr(offs), n, C.byref(opts))
        rc = lib().oge_text_format(*args, None, 0, C.byref(nb))
        if not (rc == -3 and nb.value):  # OGE_ERR_LIMIT with the size: the sizing call
            check(rc, self.h)
            return b""
        out = np.empty(nb.value, np.uint8)
        check(lib().oge_text_format(*args, _ptr(out), out.nbytes, C.byref(nb)), self.h)
        return out[:nb.value].tobytes()

    @staticmethod
    def text_host_line(rec: bytes, opts: TextOpts) -> bytes:
        """oge_text_host_line: one record's text formatted on the host."""
        nb = C.c_uint64()
        buf = C.create_string_buffer(16 + 12 * len(rec) + 256 * 2)
        check(lib().oge_text_host_line(rec, len(rec), C.byref(opts), buf, len(buf), C.byref(nb)))
        return buf.raw[:nb.value]

    # ---- SAM input (csrc/sam_parse.hip)
    @staticmethod
    def sam_header(text: bytes) -> tuple[int, int]:
        """oge_sam_header: (the bytes, the lines) of the leading '@' lines."""
        hl, nl = C.c_uint64(), C.c_uint64()
        check(lib().oge_sam_header(text, len(text), C.byref(hl), C.byref(nl)))
        return hl.value, nl.value

    def sam_lines_dev(self, d_text, nbytes: int, body_off: int, d_line_off=None, cap: int = 0) -> int:
        """oge_sam_lines_dev: the line count; with d_line_off (cap entries) also the line table."""
        n = C.c_uint64()
        check(lib().oge_sam_lines_dev(self.h, d_text, nbytes, body_off, d_line_off, cap, C.byref(n)), self.h)
        return n.value

    def sam_size_dev(self, d_text, d_line_off, n: int, opts: TextOpts, d_rec_off, d_host_mark, d_warn) -> tuple[int, int]:
        """oge_sam_size_dev: fills d_rec_off (n + 1 u64), d_host_mark and d_warn (n u8) -> (record bytes, host lines)."""
        total, n_host = C.c_uint64(), C.c_uint64()
        check(lib().oge_sam_size_dev(self.h, d_text, d_line_off, n, C.byref(opts), d_rec_off, d_host_mark, d_warn, C.byref(total),
                                     C.byref(n_host)), self.h)
        return total.value, n_host.value

    def sam_emit_dev(self, d_text, d_line_off, d_rec_off, first: int, count: int, opts: TextOpts, d_recs, cap: int) -> None:
        """oge_sam_emit_dev: the records of lines [first, first + count) at d_recs."""
        check(lib().oge_sam_emit_dev(self.h, d_text, d_line_off, d_rec_off, first, count, C.byref(opts), d_recs, cap), self.h)

    @staticmethod
    def sam_host_record(line: bytes, opts: TextOpts) -> bytes:
        """oge_sam_host_record: one line's record built on the host."""
        nb = C.c_uint64()
        buf = C.create_string_buffer(64 + 4 * len(line))
        check(lib().oge_sam_host_record(line, len(line), C.byref(opts), buf, len(buf), C.byref(nb)))
        return buf.raw[:nb.value]

    def sam_parse(self, text: bytes) -> tuple[int, np.ndarray, np.ndarray, np.ndarray]:
        """oge_sam_parse: (header bytes, records u8 with 16 bytes of slack, offsets u64[n + 1], warning bytes u8[n])."""
        hl, nb, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        recs, offs, warn = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().oge_sam_parse(self.h, text, len(text), C.byref(hl), C.byref(recs), C.byref(nb), C.byref(offs), C.byref(n), C.byref(warn)),
              self.h)

        def copy(p, count, ty):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ty)), (count,)).copy() if count else np.zeros(0, ty)
        return hl.value, copy(recs, nb.value + 16, C.c_uint8), copy(offs, n.value + 1, C.c_uint64), copy(warn, n.value, C.c_uint8)

    @staticmethod
    def coverage_layout(ref_len, binsize: int) -> np.ndarray:
        """oge_coverage_layout: base[r] = the bins in front of contig r (n_ref + 1 entries)."""
        lens = np.ascontiguousarray(ref_len, dtype=np.int32)
        base = np.zeros(len(lens) + 1, np.uint64)
        check(lib().oge_coverage_layout(len(lens), _ptr(lens) if len(lens) else None, binsize, _ptr(base)))
        return base

    def coverage_dev(self, d_recs, d_off, n: int, ref_len, binsize: int = 100, fetch: bool = True):
        """oge_coverage_dev on device records -> (bins u32 in header order, skipped reads, overflow); with
        fetch=False the bins stay on the device: (device pointer, number of bins, skipped reads, overflow)."""
        lens = np.ascontiguousarray(ref_len, dtype=np.int32)
        d, sk, ov = C.c_void_p(), C.c_uint64(), C.c_int32()
        check(lib().oge_coverage_dev(self.h, d_recs, d_off, n, len(lens), _ptr(lens) if len(lens) else None, binsize, C.byref(d),
                                     C.byref(sk), C.byref(ov)), self.h)
        nb = int(self.coverage_layout(lens, binsize)[-1])
        if not fetch:
            return d.value or 0, nb, sk.value, bool(ov.value)
        return np.frombuffer(self._fetch(d.value or 0, 4 * nb), np.uint32).copy(), sk.value, bool(ov.value)

    def coverage(self, recs: np.ndarray, offs: np.ndarray, n: int, ref_len, binsize: int = 100) -> tuple[np.ndarray, int, bool]:
        """oge_coverage: the same from host buffers."""
        lens = np.ascontiguousarray(ref_len, dtype=np.int32)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nb = int(self.coverage_layout(lens, binsize)[-1])
        bins, sk, ov = np.zeros(max(nb, 1), np.uint32), C.c_uint64(), C.c_int32()
        check(lib().oge_coverage(self.h, _ptr(recs), recs.nbytes, _ptr(offs), n, len(lens), _ptr(lens) if len(lens) else None, binsize,
                                 _ptr(bins), nb, C.byref(sk), C.byref(ov)), self.h)
        return bins[:nb], sk.value, bool(ov.value)

    def _with_file(self, data: bytes, fn):
        a = np.frombuffer(data, dtype=np.uint8)
        dz = C.c_void_p()
        check(lib().oge_dev_alloc(self.h, len(a) + 64, C.byref(dz)), self.h)
        try:
            check(lib().oge_memcpy(self.h, dz, _ptr(a), len(a), 1), self.h)
            return fn(dz, len(a))
        finally:
            lib().oge_dev_free(self.h, dz)

    def last_refs(self) -> tuple[list[str], np.ndarray]:
        """oge_ctx_last_refs: names and lengths of the file the last whole-file stats / coverage / count call read."""
        n, p, nb, pl = C.c_int32(), C.c_void_p(), C.c_uint64(), C.c_void_p()
        check(lib().oge_ctx_last_refs(self.h, C.byref(n), C.byref(p), C.byref(nb), C.byref(pl)), self.h)
        names = C.string_at(p.value, nb.value).split(b"\0")[:n.value] if nb.value else []
        lens = np.frombuffer(C.string_at(pl.value, 4 * n.value), np.int32).copy() if n.value else np.zeros(0, np.int32)
        return [x.decode() for x in names], lens

    def bam_stats(self, data: bytes, inserts: bool = False, lengths: bool = False) -> dict:
        """`openge stats` of a whole BAM file (oge_bam_stats_dev on a copy of the file in HBM)."""
        def run(dz, nbytes):
            st, dl, dc = BamStats(), C.c_void_p(), C.c_void_p()
            check(lib().oge_bam_stats_dev(self.h, dz, nbytes, self._want(inserts, lengths), C.byref(st), C.byref(dl), C.byref(dc)),
                  self.h)
            return self._stats_dict(st, dl, dc, lengths)
        return self._with_file(data, run)

    def bam_coverage(self, data: bytes, binsize: int = 100):
        """`openge coverage` of a whole BAM file -> (names, lens, base, bins, n_skipped, overflow); bins in header
        order, contig r at bins[base[r]:base[r + 1]]."""
        def run(dz, nbytes):
            d, nb, sk, ov = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_int32()
            check(lib().oge_bam_coverage_dev(self.h, dz, nbytes, binsize, C.byref(d), C.byref(nb), C.byref(sk), C.byref(ov)), self.h)
            bins = np.frombuffer(self._fetch(d.value or 0, 4 * nb.value), np.uint32).copy()
            names, lens = self.last_refs()
            return names, lens, self.coverage_layout(lens, binsize), bins, sk.value, bool(ov.value)
        return self._with_file(data, run)

    def bam_count(self, data: bytes) -> int:
        """`openge count`: the number of records of a whole BAM file (oge_bam_count_dev)."""
        def run(dz, nbytes):
            n = C.c_uint64()
            check(lib().oge_bam_count_dev(self.h, dz, nbytes, C.byref(n)), self.h)
            return n.value
        return self._with_file(data, run)

    def mem_info(self) -> tuple[int, int]:
        f, t = C.c_uint64(), C.c_uint64()
        check(lib().oge_mem_info(self.h, C.byref(f), C.byref(t)), self.h)
        return f.value, t.value

    def mergesort_reserve(self, total: int) -> tuple[int, int, int]:
        """Allocate the chain's two record arenas for streams of up to `total` decompressed bytes ->
        (x, y, cap): device pointers the caller may stage data in between chain calls."""
        x, y, cap = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib().oge_mergesort_reserve(self.h, total, C.byref(x), C.byref(y), C.byref(cap)), self.h)
        return x.value, y.value, cap.value

    def mergesort_bgzf_host(self, h_z: int, zbytes: int, opts: "MergesortOpts", h_out: int, out_cap: int) -> tuple[int, int, int]:
        """The chain on a BAM file in host memory (page-locked for full speed), PCIe overlapped with the
        codec -> (out_bytes written to h_out, n_reads, n_dup)."""
        ob, nr, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().oge_mergesort_bgzf_host(self.h, h_z, zbytes, C.byref(opts), h_out, out_cap, C.byref(ob), C.byref(nr),
                                            C.byref(nd)), self.h)
        return ob.value, nr.value, nd.value

    def record_offsets_dev(self, d_stream, rec_base: int, end: int, n_ref: int, d_off=None, cap: int = 0) -> int:
        n = C.c_uint64()
        check(lib().oge_bam_record_offsets_dev(self.h, d_stream, rec_base, end, n_ref, d_off, cap, C.byref(n)), self.h)
        return n.value

    def fix_bins_dev(self, d_recs, d_off, n: int) -> None:
        check(lib().oge_fix_bins_dev(self.h, d_recs, d_off, n), self.h)

    def drop_flagged_dev(self, d_recs, d_off, n: int, flag_mask: int, d_out, d_out_off) -> int:
        m = C.c_uint64()
        check(lib().oge_drop_flagged_dev(self.h, d_recs, d_off, n, flag_mask, d_out, d_out_off, C.byref(m)), self.h)
        return m.value

    def filter_records_dev(self, d_recs, d_off, n: int, opts: "FilterOpts", d_out, d_out_off) -> int:
        m = C.c_uint64()
        check(lib().oge_filter_records_dev(self.h, d_recs, d_off, n, C.byref(opts), d_out, d_out_off, C.byref(m)),
              self.h)
        return m.value

    def bai_open(self, bai: bytes, n_ref_expected: int = -1) -> int:
        """oge_bai_open -> the handle (release it with bai_close)."""
        h = C.c_void_p()
        check(lib().oge_bai_open(self.h, bai, len(bai), n_ref_expected, C.byref(h)), self.h)
        return h.value

    def bai_close(self, handle: int) -> None:
        lib().oge_bai_close(handle)

    def bai_query(self, handle: int, regions, widen: int = 0, cap: int | None = None) -> list[tuple[int, int]]:
        """oge_bai_query: the merged (beg, end) virtual-offset ranges of (ref_id, left_pos, right_pos) triples."""
        arr = (Region * max(len(regions), 1))(*[Region(*r) for r in regions])
        n = C.c_uint64()
        if cap is None:  # sized by the device form's count
            d = C.c_void_p()
            check(lib().oge_bai_query_dev(self.h, handle, arr, len(regions), widen, C.byref(d), C.byref(n)), self.h)
            cap = n.value
        out = np.zeros(2 * max(cap, 1), dtype=np.uint64)
        check(lib().oge_bai_query(self.h, handle, arr, len(regions), widen, _ptr(out), cap, C.byref(n)), self.h)
        return [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(n.value)]

    def bai_query_dev(self, handle: int, regions, widen: int = 0) -> tuple[int, int]:
        """oge_bai_query_dev -> (device pointer of the pairs or 0, n_ranges)."""
        arr = (Region * max(len(regions), 1))(*[Region(*r) for r in regions])
        d, n = C.c_void_p(), C.c_uint64()
        check(lib().oge_bai_query_dev(self.h, handle, arr, len(regions), widen, C.byref(d), C.byref(n)), self.h)
        return d.value or 0, n.value

    def bam_decode_ranges_dev(self, d_z: int, zbytes: int, span_z, span_file, d_ranges: int, n_ranges: int, n_ref: int) -> tuple[bytes, list[int]]:
        """oge_bam_decode_ranges_dev -> (the packed records, their n + 1 offsets), copied to the host."""
        sz, sf = np.asarray(span_z, dtype=np.uint64), np.asarray(span_file, dtype=np.uint64)
        dr, do, n, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(lib().oge_bam_decode_ranges_dev(self.h, d_z, zbytes, _ptr(sz), _ptr(sf), len(sf), d_ranges, n_ranges, n_ref, C.byref(dr),
                                              C.byref(do), C.byref(n), C.byref(nb)), self.h)
        try:
            if not n.value:
                return b"", [0]
            offs = np.frombuffer(self._fetch(do.value, 8 * (n.value + 1)), dtype=np.uint64)
            return self._fetch(dr.value, nb.value), [int(x) for x in offs]
        finally:  # the arena and the offsets are the caller's
            for p in (dr.value, do.value):
                if p:
                    lib().oge_dev_free(self.h, p)

    def filter_regions_dev(self, d_recs, d_off, n: int, opts: "FilterOpts", regions, d_out, d_out_off) -> int:
        """oge_filter_regions_dev; regions: (ref_id, left_pos, right_pos) triples (a host list)."""
        arr = (Region * max(len(regions), 1))(*[Region(*r) for r in regions])
        m = C.c_uint64()
        check(lib().oge_filter_regions_dev(self.h, d_recs, d_off, n, C.byref(opts), arr if regions else None, len(regions),
                                           d_out, d_out_off, C.byref(m)), self.h)
        return m.value

    def sort_name(self, recs: np.ndarray, offs: np.ndarray, n: int) -> np.ndarray:
        perm = np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().oge_sort_name(self.h, _ptr(recs), recs.nbytes, _ptr(offs), n, _ptr(perm)), self.h)
        return perm[:n]

    def sort_name_dev(self, d_recs, d_off, n: int, d_perm) -> None:
        check(lib().oge_sort_name_dev(self.h, d_recs, d_off, n, d_perm), self.h)

    def markdup_dev(self, d_recs, d_off, n, opts: MarkdupOpts, d_dup, apply: bool = True) -> int:
        nd = C.c_uint64()
        check(lib().oge_markdup_dev(self.h, d_recs, d_off, n, C.byref(opts), d_dup, 1 if apply else 0, C.byref(nd)),
              self.h)
        return nd.value

    def sort_markdup_dev(self, d_recs, d_off, n, opts: MarkdupOpts, d_perm, d_out, d_out_off) -> int:
        nd = C.c_uint64()
        check(lib().oge_sort_markdup_dev(self.h, d_recs, d_off, n, C.byref(opts), d_perm, d_out, d_out_off,
                                         C.byref(nd)), self.h)
        return nd.value

    def realign_scan(self, cons: np.ndarray, cons_off: np.ndarray, bases: np.ndarray, quals: np.ndarray,
                     read_off: np.ndarray, pairs: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """findBestOffset for every (consensus, read) pair -> (best_index, best_score)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 4)
        n = len(pairs)
        b = RealignScanBatch(_ptr(cons), cons.nbytes, _ptr(cons_off), len(cons_off) - 1, len(read_off) - 1, _ptr(bases),
                             _ptr(quals), bases.nbytes, _ptr(read_off), _ptr(pairs), n)
        bi, bs = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
        check(lib().oge_realign_scan(self.h, C.byref(b), _ptr(bi), _ptr(bs)), self.h)
        return bi[:n], bs[:n]

    def localrealign(self, header_text: str, recs: np.ndarray, offs: np.ndarray, n: int, fasta: str, intervals: str,
                     opts: RealignOpts | None = None, more: "list[Context] | None" = None) -> tuple[np.ndarray, np.ndarray, dict]:
        """LocalRealignment over coordinate-sorted records -> (out recs, out offsets[n+1], stats).
        The arrays are read-only-by-convention views of the library's result buffer (no copy).  more: further
        contexts -- the device work is then spread over [self] + more by interval ranges
        (oge_localrealign_multi)."""
        import json
        L = lib()
        hb = header_text.encode()
        res = C.c_void_p()
        if more:
            hs = (C.c_void_p * (1 + len(more)))(self.h.value, *[c.h.value for c in more])
            check(L.oge_localrealign_multi(hs, len(hs), hb, len(hb), _ptr(recs), _ptr(offs), n, fasta.encode(),
                                           intervals.encode(), C.byref(opts) if opts is not None else None, C.byref(res)),
                  self.h)
        else:
            check(L.oge_localrealign(self.h, hb, len(hb), _ptr(recs), _ptr(offs), n, fasta.encode(), intervals.encode(),
                                     C.byref(opts) if opts is not None else None, C.byref(res)), self.h)
        holder = _RealignResult(res)  # frees the result when the last view goes away
        cnt = int(L.oge_realign_result_count(res))
        nb = C.c_uint64()
        rp = L.oge_realign_result_records(res, C.byref(nb))
        stats = json.loads(L.oge_realign_result_stats(res).decode())
        if nb.value:
            ra = (C.c_uint8 * nb.value).from_address(rp)
            ra._holder = holder
            out = np.ctypeslib.as_array(ra)
        else:
            out = np.zeros(0, np.uint8)
        oa = (C.c_uint64 * (cnt + 1)).from_address(L.oge_realign_result_offsets(res))
        oa._holder = holder
        oo = np.ctypeslib.as_array(oa)
        return out, oo, stats

    def synth_range_dev(self, p: SynthParams, slot0: int, nslots: int, d_offs: int, d_out: int | None) -> None:
        """Slots [slot0, slot0 + nslots) of the data set (one rank's input shard)."""
        L = lib()
        check(L.oge_synth_finalize(C.byref(p)))
        if d_offs and not d_out:
            check(L.oge_synth_offsets_range_dev(self.h, C.byref(p), slot0, nslots, d_offs), self.h)
        if d_out:
            check(L.oge_synth_records_range_dev(self.h, C.byref(p), slot0, nslots, d_offs, d_out), self.h)

    def synth_dev(self, p: SynthParams, d_offs: int, d_out: int | None) -> None:
        L = lib()
        check(L.oge_synth_finalize(C.byref(p)))
        if d_offs:
            check(L.oge_synth_offsets_dev(self.h, C.byref(p), d_offs), self.h)
        if d_out:
            check(L.oge_synth_records_dev(self.h, C.byref(p), d_offs, d_out), self.h)


# ------------------------------------------------------------------------- multi-GPU (oge_comm)
class Comm:
    """One rank of a multi-GPU communicator (oge_comm_*): RCCL over xGMI, or the in-process
    transport when several contexts share a GPU.  Every method is collective."""

    def __init__(self, h: C.c_void_p, ctx: "Context"):
        self.h, self.ctx = h, ctx

    @property
    def rank(self) -> int:
        return lib().oge_comm_rank(self.h)

    @property
    def size(self) -> int:
        return lib().oge_comm_size(self.h)

    @property
    def transport(self) -> str:
        return lib().oge_comm_transport(self.h).decode()

    def sort_markdup_dist(self, d_recs: int, d_off: int, n: int, n_ref: int, opts: "MarkdupOpts | None", sort: bool = True):
        """This rank's shard -> its slice of the sorted (and, with opts, duplicate-marked) output, or
        with sort=False its shard marked in place order (dedup): (d_out pointer, d_out_off pointer,
        records in the slice, duplicates over all ranks).  The pointers are owned by the rank's
        context (valid until its next call)."""
        d, do = C.c_void_p(), C.c_void_p()
        no, nd = C.c_uint64(), C.c_uint64()
        check(lib().oge_sort_markdup_dist(self.h, d_recs, d_off, n, n_ref, 1 if sort else 0,
                                          C.byref(opts) if opts is not None else None,
                                          C.byref(d), C.byref(do), C.byref(no), C.byref(nd)), self.ctx.h)
        return d.value or 0, do.value or 0, no.value, nd.value

    def mergesort_bgzf_dist(self, d_z: int, zbytes: int, opts: "MergesortOpts"):
        """Rank's input BAM file in HBM -> (its slice of the output file: device pointer, bytes; records
        written by all ranks; duplicates flagged by all ranks)."""
        d = C.c_void_p()
        ob, nr, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().oge_mergesort_bgzf_dist(self.h, d_z, zbytes, C.byref(opts), C.byref(d), C.byref(ob), C.byref(nr),
                                            C.byref(nd)), self.ctx.h)
        return d.value or 0, ob.value, nr.value, nd.value

    def mergesort_bgzf_shard(self, d_z: int, zbytes: int, own_bytes: int, opts: "MergesortOpts"):
        """ONE input file over the ranks: this rank holds the file's bytes from a_g on (a_g = the earlier
        ranks' own_bytes summed) and decodes the blocks that start in its own_bytes -> (its slice of the
        output file: device pointer, bytes; records written by all ranks; duplicates flagged by all)."""
        d = C.c_void_p()
        ob, nr, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().oge_mergesort_bgzf_shard(self.h, d_z, zbytes, own_bytes, C.byref(opts), C.byref(d), C.byref(ob),
                                             C.byref(nr), C.byref(nd)), self.ctx.h)
        return d.value or 0, ob.value, nr.value, nd.value

    def decode_shard(self, d_z: int, zbytes: int, own_bytes: int, hdr_cap: int = 1 << 22):
        """oge_bgzf_decode_shard: this rank's records of one sharded BGZF file -> (d_recs pointer, d_off
        pointer (n + 1 offsets), n, raw BAM header bytes)."""
        dr, do = C.c_void_p(), C.c_void_p()
        n, hl = C.c_uint64(), C.c_uint64()
        hb = C.create_string_buffer(hdr_cap)
        check(lib().oge_bgzf_decode_shard(self.h, d_z, zbytes, own_bytes, C.byref(dr), C.byref(do), C.byref(n), hb, hdr_cap,
                                          C.byref(hl)), self.ctx.h)
        return dr.value or 0, do.value or 0, n.value, hb.raw[:hl.value]

    def exchange_stats(self) -> list:
        """This rank's per-exchange record of its last sort_markdup_dist / mergesort_bgzf_dist call:
        [{tag, calls, bytes_sent, bytes_recv, bytes_self, ms}] (bytes to / from other ranks, kept here;
        host wall time of the collectives, waiting for peers included)."""
        import json
        n = lib().oge_comm_stats_json(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().oge_comm_stats_json(self.h, buf, n + 1)
        return json.loads(buf.value.decode())

    def close(self):
        if self.h:
            lib().oge_comm_destroy(self.h)
            self.h = None


BGZF_MAX_BLOCK = 65536  # BSIZE - 1 is a u16 (SAM spec 4.1): no block is longer


def shard_ranges(file_bytes: int, world: int) -> list[tuple[int, int, int]]:
    """Byte ranges of ONE BGZF file for `world` ranks (oge_bgzf_decode_shard / Comm.mergesort_bgzf_shard):
    (a_g, own_g, end_g) -- rank g decodes the blocks that start in [a_g, a_g + own_g) and holds the file's
    bytes [a_g, end_g) (its last block may run up to 64 KiB past its range; the last rank's ends at the
    end of the file)."""
    out = []
    for g in range(world):
        a, b = file_bytes * g // world, file_bytes * (g + 1) // world
        out.append((a, b - a, min(file_bytes, b + BGZF_MAX_BLOCK)))
    return out


def comm_init(ctxs: list["Context"]) -> list[Comm]:
    """One process, one rank per context (call each rank's methods from its own thread)."""
    n = len(ctxs)
    arr = (C.c_void_p * n)(*[c.h for c in ctxs])
    out = (C.c_void_p * n)()
    check(lib().oge_comm_init(arr, n, out))
    return [Comm(C.c_void_p(out[i]), ctxs[i]) for i in range(n)]


def comm_unique_id() -> bytes:
    nb = lib().oge_comm_unique_id_bytes()
    buf = C.create_string_buffer(nb)
    check(lib().oge_comm_unique_id(buf, nb))
    return buf.raw


def comm_init_rank(ctx: "Context", nranks: int, rank: int, uid: bytes, mode: str | None = None) -> Comm:
    """One process per GPU (RCCL): uid from comm_unique_id() on one rank, shared by the caller.  mode:
    "auto" | "rccl" | "host" (None = OGE_COMM)."""
    h = C.c_void_p()
    if mode is None:
        check(lib().oge_comm_init_rank(ctx.h, nranks, rank, uid, C.byref(h)), ctx.h)
    else:
        check(lib().oge_comm_init_rank_mode(ctx.h, nranks, rank, uid, mode.encode(), C.byref(h)), ctx.h)
    return Comm(h, ctx)


RANGE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)


def sort_markdup_chunked(ctx: "Context", recs: np.ndarray, offs: np.ndarray, n: int, n_ref: int,
                         opts: "MarkdupOpts | None", chunk_bytes: int = 0):
    """Out-of-core mergesort [-M] of host records (oge_sort_markdup_chunked).  `recs` is used as the
    spill space (it holds the sorted runs afterwards).  Returns (output record stream bytes,
    duplicates, runs, ranges)."""
    parts = []

    def on_range(user, d_recs, d_off, m):
        try:
            oo = np.empty(m + 1, np.uint64)
            check(lib().oge_memcpy(ctx.h, oo.ctypes.data, d_off, 8 * (m + 1), 2), ctx.h)
            b = np.empty(int(oo[m] - oo[0]), np.uint8)
            if b.size:
                check(lib().oge_memcpy(ctx.h, b.ctypes.data, d_recs + int(oo[0]), b.size, 2), ctx.h)
            parts.append(b.tobytes())
            return 0
        except Exception:  # noqa: BLE001
            return -1

    cb = RANGE_CB(on_range)
    nd, nr, ng = C.c_uint64(), C.c_uint64(), C.c_uint64()
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    check(lib().oge_sort_markdup_chunked(ctx.h, recs.ctypes.data, offs.ctypes.data, n, n_ref,
                                         C.byref(opts) if opts is not None else None, chunk_bytes, cb, None,
                                         C.byref(nd), C.byref(nr), C.byref(ng)), ctx.h)
    return b"".join(parts), nd.value, nr.value, ng.value
