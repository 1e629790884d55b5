"""ctypes binding of libkmx.so (include/kmx.h).  No fallback of any kind."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KMX_LIB") or os.path.join(_HERE, "libkmx.so")      # (KMX_LIB: a tuning build, scripts/dev/build_variant.sh)
if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(libkmx has no CPU fallback)")
_lib = C.CDLL(LIB_PATH)

MODE_COUNT, MODE_PA, MODE_BF, MODE_BFC, MODE_BFT = 0, 1, 2, 3, 4
STATS_ROWS = 6


class KmxList(C.Structure):
    _fields_ = [("recs", C.c_void_p), ("n", C.c_uint64)]


class KmxMergeTask(C.Structure):
    _fields_ = [("n_lists", C.c_uint32), ("key_words", C.c_uint32), ("lists", C.POINTER(KmxList)),
                ("soft_min", C.POINTER(C.c_uint32)), ("rec_min", C.c_uint32), ("share_min", C.c_uint32),
                ("mode", C.c_uint32), ("bitw", C.c_uint32), ("lower", C.c_uint64), ("upper", C.c_uint64),
                ("rows_hint", C.c_uint64), ("list_on_device", C.c_void_p)]


class KmxFilterTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("want", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("key", KmxList), ("marks", C.c_void_p),
                ("key_on_device", C.c_uint32)]


FILTER_M, FILTER_V, FILTER_K = 1, 2, 4


class KmxBlock(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_uint64), ("n_cols", C.c_uint32), ("count_bytes", C.c_uint32)]


class KmxCombineTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_blocks", C.c_uint32), ("flags", C.c_uint32),
                ("blocks", C.POINTER(KmxBlock)), ("block_on_device", C.c_void_p)]


COMBINE_DROP_LAST, COMBINE_MAX_BLOCKS = 1, 64


class KmxQueryTask(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_seqs", C.c_uint64), ("kmer_size", C.c_uint32),
                ("minim_size", C.c_uint32), ("repart", C.c_void_p), ("nb_parts", C.c_uint32), ("n_cols", C.c_uint32),
                ("window", C.c_uint64), ("rows", C.POINTER(C.c_void_p)), ("hits", C.c_void_p)]


class KmxZqueryTask(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_seqs", C.c_uint64), ("kmer_size", C.c_uint32),
                ("minim_size", C.c_uint32), ("repart", C.c_void_p), ("nb_parts", C.c_uint32), ("n_cols", C.c_uint32),
                ("window", C.c_uint64), ("rows", C.POINTER(C.c_void_p)), ("z", C.c_uint32), ("last", C.c_uint32),
                ("bits", C.c_void_p), ("hits", C.c_void_p)]


class KmxKqueryTask(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_seqs", C.c_uint64), ("kmer_size", C.c_uint32),
                ("minim_size", C.c_uint32), ("repart", C.c_void_p), ("nb_parts", C.c_uint32), ("n_cols", C.c_uint32),
                ("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_rows", C.POINTER(C.c_uint64)),
                ("rows", C.POINTER(C.c_void_p)), ("hits", C.c_void_p), ("sums", C.c_void_p), ("want_sums", C.c_uint32)]


class KmxCqueryTask(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_seqs", C.c_uint64), ("kmer_size", C.c_uint32),
                ("minim_size", C.c_uint32), ("repart", C.c_void_p), ("nb_parts", C.c_uint32), ("n_cols", C.c_uint32),
                ("window", C.c_uint64), ("rows", C.POINTER(C.c_void_p)), ("bitw", C.c_uint32), ("min_class", C.c_uint32),
                ("hits", C.c_void_p), ("sums", C.c_void_p)]


class KmxDistTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("want_mins", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("inter", C.c_void_p), ("mins", C.c_void_p)]


class KmxColsumsTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("reserved", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("sums", C.c_void_p)]


class KmxDiffTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("min_rec", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("group", C.c_void_p), ("total_ctrl", C.c_uint64),
                ("total_case", C.c_uint64), ("threshold", C.c_double)]


# kmx_diff_rec: 40 bytes
DIFF_REC = np.dtype([("sum_ctrl", "<u8"), ("sum_case", "<u8"), ("stat", "<f8"), ("rec_ctrl", "<u4"), ("rec_case", "<u4"),
                     ("row", "<u4"), ("over", "<u4")])
assert DIFF_REC.itemsize == 40


class KmxAssocTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("n_use", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("vecs", C.c_void_p),
                ("n_vec", C.c_uint32), ("frac_bits", C.c_uint32), ("min_abund", C.c_uint32), ("flags", C.c_uint32),
                ("gain", C.c_double), ("vmin", C.c_double), ("threshold", C.c_double), ("min_rec", C.c_uint32), ("max_rec", C.c_uint32)]


assert C.sizeof(KmxAssocTask) == 96
# kmx_assoc_rec: 32 bytes
ASSOC_REC = np.dtype([("stat", "<f8"), ("beta", "<f8"), ("s0", "<i8"), ("rec", "<u4"), ("row", "<u4")])
assert ASSOC_REC.itemsize == 32


class KmxSelectTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("n_out", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("min_abund", C.c_uint32),
                ("min_rec", C.c_uint32), ("max_rec", C.c_uint32), ("out_mode", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


# kmx_select_rec: 8 bytes
SELECT_REC = np.dtype([("row", "<u4"), ("rec", "<u4")])
assert SELECT_REC.itemsize == 8 and C.sizeof(KmxSelectTask) == 64
SELECT_ZERO_BELOW = 1


class KmxPanTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("n_use", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("min_abund", C.c_uint32),
                ("flags", C.c_uint32), ("spectrum", C.c_void_p), ("shared", C.c_void_p)]


assert C.sizeof(KmxPanTask) == 64
PAN_SHARED = 1


class KmxSpectraTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("n_use", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("pairs", C.c_void_p),
                ("n_pairs", C.c_uint32), ("cap1", C.c_uint32), ("cap2", C.c_uint32), ("flags", C.c_uint32),
                ("hist", C.c_void_p), ("joint", C.c_void_p)]


assert C.sizeof(KmxSpectraTask) == 80
SPECTRA_HIST, SPECTRA_JOINT = 1, 2


class KmxColorsTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("n_use", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("min_abund", C.c_uint32),
                ("flags", C.c_uint32)]


assert C.sizeof(KmxColorsTask) == 48


class KmxUnitigsTask(C.Structure):
    _fields_ = [("keys", C.c_void_p), ("n", C.c_uint64), ("kmer_size", C.c_uint32), ("key_words", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(KmxUnitigsTask) == 32


class KmxGroupsumTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("n_use", C.c_uint32), ("rows", C.c_void_p),
                ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("groups", C.c_void_p), ("min_abund", C.c_uint32), ("flags", C.c_uint32),
                ("g0", C.c_uint32), ("n_groups", C.c_uint32), ("present", C.c_void_p), ("sums", C.c_void_p), ("size", C.c_void_p)]


assert C.sizeof(KmxGroupsumTask) == 88
GROUPSUM_SUMS = 1


class KmxKsetTask(C.Structure):
    _fields_ = [("keys", C.c_void_p), ("n", C.c_uint64), ("kmer_size", C.c_uint32), ("key_words", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class KmxMatchTask(C.Structure):
    _fields_ = [("set", C.c_void_p), ("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_seqs", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("occ", C.c_void_p), ("reserved2", C.c_uint64)]


assert C.sizeof(KmxKsetTask) == 32 and C.sizeof(KmxMatchTask) == 56
MATCH_IDS, MATCH_OCC = 1, 2
MATCH_REC = np.dtype([("n_kmers", "<u4"), ("hits", "<u4"), ("fwd", "<u4"), ("covered", "<u4"), ("first", "<u4"), ("last", "<u4")])
assert MATCH_REC.itemsize == 24
MATCH_NONE = 0xFFFFFFFF


class KmxGramTask(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("mode", C.c_uint32), ("n_cols", C.c_uint32), ("n_use", C.c_uint32),
                ("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("weights", C.c_void_p),
                ("min_abund", C.c_uint32), ("flags", C.c_uint32), ("table", C.c_void_p)]


assert C.sizeof(KmxGramTask) == 64
E_INTERNAL = -6

_vp = C.c_void_p
_lib.kmx_version.restype = C.c_int
_lib.kmx_create.argtypes = [C.c_int, C.POINTER(_vp)]
_lib.kmx_destroy.argtypes = [_vp]
_lib.kmx_last_error.restype = C.c_char_p
_lib.kmx_last_error.argtypes = [_vp]
_lib.kmx_stream.restype = _vp
_lib.kmx_stream.argtypes = [_vp]
_lib.kmx_set_profiling.argtypes = [_vp, C.c_int]
_lib.kmx_set_file_order.argtypes = [_vp, C.c_int]
KMX_VERSION = 2
if _lib.kmx_version() != KMX_VERSION:
    raise ImportError(f"{LIB_PATH} is version {_lib.kmx_version()}, this binding is for version {KMX_VERSION} (kmx_merge_task layout)")
_lib.kmx_result_kernel.restype = C.c_char_p
_lib.kmx_result_kernel.argtypes = [_vp]
_lib.kmx_result_kernel_ms.restype = C.c_double
_lib.kmx_result_kernel_ms.argtypes = [_vp]
_lib.kmx_result_kernel_parts_ms.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.kmx_result_transpose_ms.restype = C.c_double
_lib.kmx_result_transpose_ms.argtypes = [_vp]
_lib.kmx_result_body_dev.restype = _vp
_lib.kmx_result_body_dev.argtypes = [_vp, C.c_uint32]
_lib.kmx_merge_dev.argtypes = [_vp, C.POINTER(KmxMergeTask), C.c_uint32, C.POINTER(_vp)]
_lib.kmx_result_wait.argtypes = [_vp]
for _f in ("kmx_result_rows", "kmx_result_sparse_rows", "kmx_result_row_bytes", "kmx_result_body_bytes", "kmx_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp, C.c_uint32]
_lib.kmx_result_copy_body.argtypes = [_vp, C.c_uint32, _vp, C.c_uint64]
_lib.kmx_result_copy_stats.argtypes = [_vp, C.c_uint32, _vp]
_lib.kmx_result_copy_body_dev.argtypes = [_vp, C.c_uint32, _vp, C.c_uint64]
_lib.kmx_result_prepare_body.argtypes = [_vp, C.c_uint32]
_lib.kmx_result_arena.argtypes = [_vp, C.c_uint32, C.POINTER(_vp), C.POINTER(C.c_uint64)]
_lib.kmx_result_copy_order.argtypes = [_vp, C.c_uint32, _vp]
_lib.kmx_result_free.argtypes = [_vp]
_lib.kmx_merge.argtypes = [_vp, C.POINTER(KmxMergeTask), C.POINTER(_vp), C.POINTER(C.c_uint64),
                           C.POINTER(C.c_uint64), _vp]
_lib.kmx_free.argtypes = [_vp]
_lib.kmx_count_kmer.argtypes = [_vp, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_vp), C.POINTER(_vp),
                                C.POINTER(C.c_uint64)]
_lib.kmx_count_hash.argtypes = [_vp, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_uint64)]
_lib.kmx_count_batch.argtypes = [_vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.c_int,
                                 C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(_vp), C.POINTER(_vp),
                                 C.POINTER(C.c_uint64)]
_lib.kmx_transpose_bits.argtypes = [_vp, _vp, C.c_uint64, C.c_uint64, _vp]
_lib.kmx_superk_partition.argtypes = [_vp, C.c_char_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint32,
                                      C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

class KmxSuperkStats(C.Structure):
    _fields_ = [("part_counters", _vp), ("minim_superks", _vp), ("minim_kmers", _vp), ("minim_kxmers", _vp),
                ("nb_superk", C.c_uint64)]


PINFO_STRIDE = 2 + 5 * 256
_lib.kmx_superk_partition_stats.argtypes = [_vp, C.c_char_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint32,
                                            C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(KmxSuperkStats)]

_lib.kmx_merge_host.argtypes = [_vp, C.POINTER(KmxMergeTask), C.c_uint32, C.POINTER(_vp)]
_lib.kmx_alloc_pinned.restype = _vp
_lib.kmx_reads_upload.argtypes = [_vp, _vp, C.c_uint64, C.POINTER(_vp)]
_lib.kmx_reads_release.argtypes = [_vp, _vp]
_lib.kmx_reads_release.restype = None
_lib.kmx_alloc_pinned.argtypes = [C.c_size_t]
_lib.kmx_free_pinned.argtypes = [_vp]

_lib.kmx_count_reads.argtypes = [_vp, C.c_char_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32,
                                 C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                 C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(KmxSuperkStats)]

_lib.kmx_superk_sample.argtypes = [_vp, C.c_char_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(KmxSuperkStats),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]


class KmxSuperkRaw(C.Structure):
    _fields_ = [("part_radix", _vp), ("minim_superks", _vp), ("minim_kmers", _vp), ("nb_superk", C.c_uint64),
                ("minim_sparse", _vp), ("minim_sparse_cap", C.c_uint64), ("minim_sparse_n", C.c_uint64)]


_lib.kmx_device_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
_lib.kmx_store_create.argtypes = [C.c_int, C.c_uint64, C.POINTER(_vp)]
_lib.kmx_store_destroy.argtypes = [_vp]
_lib.kmx_store_used.restype = C.c_uint64
_lib.kmx_store_used.argtypes = [_vp]
_lib.kmx_store_limit.restype = C.c_uint64
_lib.kmx_store_limit.argtypes = [_vp]
_lib.kmx_copy_to_host.argtypes = [_vp, _vp, _vp, C.c_uint64]
_lib.kmx_count_reads_dev_multi.argtypes = [_vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32,
                                            _vp, C.c_uint32, _vp, _vp, _vp, _vp]
_lib.kmx_count_reads_dev_multi.restype = C.c_int
_lib.kmx_count_reads_dev.argtypes = [_vp, C.c_char_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32,
                                     C.POINTER(_vp), C.c_uint32, C.POINTER(KmxList), C.POINTER(C.c_uint64),
                                     C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(KmxSuperkStats),
                                     C.POINTER(KmxSuperkRaw)]
_lib.kmx_hist_reset.argtypes = [_vp]
_lib.kmx_hist_off.argtypes = [_vp]
_lib.kmx_hist_read.argtypes = [_vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp]
_lib.kmx_peer_access.argtypes = [C.c_int, C.c_int]
EXPORTS = ["kmx_copy_to_host_async", "kmx_copy_wait", "kmx_reads_upload", "kmx_reads_release", "kmx_peer_access", "kmx_set_file_order", "kmx_count_reads_dev_multi", "kmx_version", "kmx_result_prepare_body", "kmx_result_arena", "kmx_result_copy_order", "kmx_result_sparse_rows", "kmx_device_memory", "kmx_superk_sample", "kmx_store_create", "kmx_store_destroy", "kmx_store_used", "kmx_store_limit", "kmx_copy_to_host", "kmx_count_reads_dev", "kmx_hist_reset", "kmx_hist_read", "kmx_hist_off", "kmx_device_count", "kmx_count_reads", "kmx_result_copy_body_dev", "kmx_merge_host", "kmx_alloc_pinned", "kmx_free_pinned", "kmx_superk_partition_stats", "kmx_result_transpose_ms", "kmx_result_body_dev", "kmx_set_profiling", "kmx_result_kernel_ms", "kmx_result_kernel", "kmx_create", "kmx_destroy", "kmx_last_error", "kmx_stream", "kmx_merge_dev",
           "kmx_result_wait", "kmx_result_rows", "kmx_result_row_bytes", "kmx_result_body_bytes",
           "kmx_result_algo_bytes", "kmx_result_copy_body", "kmx_result_copy_stats", "kmx_result_free",
           "kmx_merge", "kmx_count_kmer", "kmx_count_hash", "kmx_count_batch", "kmx_transpose_bits", "kmx_superk_partition",
           "kmx_free"]

_lib.kmx_filter_dev.argtypes = [_vp, C.POINTER(KmxFilterTask), C.POINTER(_vp)]
_lib.kmx_filter_host.argtypes = [_vp, C.POINTER(KmxFilterTask), C.POINTER(_vp)]
_lib.kmx_filter_result_wait.argtypes = [_vp]
for _f in ("kmx_filter_result_rows", "kmx_filter_result_row_bytes", "kmx_filter_result_body_bytes", "kmx_filter_result_vector_len",
           "kmx_filter_result_absent", "kmx_filter_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_filter_result_body_dev", "kmx_filter_result_vector_dev", "kmx_filter_result_absent_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_filter_result_copy_body", "kmx_filter_result_copy_vector", "kmx_filter_result_copy_absent"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_filter_result_kernel_ms.restype = C.c_double
_lib.kmx_filter_result_kernel_ms.argtypes = [_vp]
_lib.kmx_filter_result_free.argtypes = [_vp]
_lib.kmx_filter_marks_alloc.restype = _vp
_lib.kmx_filter_marks_alloc.argtypes = [_vp, C.c_uint64]
_lib.kmx_filter_marks_free.argtypes = [_vp, _vp]


_lib.kmx_combine_dev.argtypes = [_vp, C.POINTER(KmxCombineTask), C.POINTER(_vp)]
_lib.kmx_combine_host.argtypes = [_vp, C.POINTER(KmxCombineTask), C.POINTER(_vp)]
_lib.kmx_combine_result_wait.argtypes = [_vp]
for _f in ("kmx_combine_result_rows", "kmx_combine_result_row_bytes", "kmx_combine_result_body_bytes", "kmx_combine_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_combine_result_body_dev.restype = _vp
_lib.kmx_combine_result_body_dev.argtypes = [_vp]
_lib.kmx_combine_result_copy_body.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_combine_result_kernel_ms.restype = C.c_double
_lib.kmx_combine_result_kernel_ms.argtypes = [_vp]
_lib.kmx_combine_result_free.argtypes = [_vp]

_lib.kmx_query_dev.argtypes = [_vp, C.POINTER(KmxQueryTask), C.POINTER(_vp)]
_lib.kmx_query_host.argtypes = [_vp, C.POINTER(KmxQueryTask), C.POINTER(_vp)]
_lib.kmx_query_result_wait.argtypes = [_vp]
for _f in ("kmx_query_result_n_seqs", "kmx_query_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_query_result_copy_kmers", "kmx_query_result_copy_hits"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_query_result_hits_dev.restype = _vp
_lib.kmx_query_result_hits_dev.argtypes = [_vp]
_lib.kmx_query_result_kernel_ms.restype = C.c_double
_lib.kmx_query_result_kernel_ms.argtypes = [_vp]
_lib.kmx_query_result_free.argtypes = [_vp]

_lib.kmx_kquery_dev.argtypes = [_vp, C.POINTER(KmxKqueryTask), C.POINTER(_vp)]
_lib.kmx_kquery_host.argtypes = [_vp, C.POINTER(KmxKqueryTask), C.POINTER(_vp)]
_lib.kmx_kquery_result_wait.argtypes = [_vp]
for _f in ("kmx_kquery_result_n_seqs", "kmx_kquery_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_kquery_result_copy_kmers", "kmx_kquery_result_copy_hits", "kmx_kquery_result_copy_sums"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
for _f in ("kmx_kquery_result_hits_dev", "kmx_kquery_result_sums_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_kquery_result_kernel_ms.restype = C.c_double
_lib.kmx_kquery_result_kernel_ms.argtypes = [_vp]
_lib.kmx_kquery_result_free.argtypes = [_vp]
KQUERY_EXPORTS = ["kmx_kquery_dev", "kmx_kquery_host", "kmx_kquery_result_wait", "kmx_kquery_result_n_seqs", "kmx_kquery_result_copy_kmers",
                  "kmx_kquery_result_copy_hits", "kmx_kquery_result_copy_sums", "kmx_kquery_result_hits_dev", "kmx_kquery_result_sums_dev",
                  "kmx_kquery_result_kernel_ms", "kmx_kquery_result_algo_bytes", "kmx_kquery_result_free"]

_lib.kmx_cquery_dev.argtypes = [_vp, C.POINTER(KmxCqueryTask), C.POINTER(_vp)]
_lib.kmx_cquery_host.argtypes = [_vp, C.POINTER(KmxCqueryTask), C.POINTER(_vp)]
_lib.kmx_cquery_result_wait.argtypes = [_vp]
for _f in ("kmx_cquery_result_n_seqs", "kmx_cquery_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_cquery_result_copy_kmers", "kmx_cquery_result_copy_hits", "kmx_cquery_result_copy_sums"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
for _f in ("kmx_cquery_result_hits_dev", "kmx_cquery_result_sums_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_cquery_result_kernel_ms.restype = C.c_double
_lib.kmx_cquery_result_kernel_ms.argtypes = [_vp]
_lib.kmx_cquery_result_free.argtypes = [_vp]
CQUERY_EXPORTS = ["kmx_cquery_dev", "kmx_cquery_host", "kmx_cquery_result_wait", "kmx_cquery_result_n_seqs", "kmx_cquery_result_copy_kmers",
                  "kmx_cquery_result_copy_hits", "kmx_cquery_result_copy_sums", "kmx_cquery_result_hits_dev", "kmx_cquery_result_sums_dev",
                  "kmx_cquery_result_kernel_ms", "kmx_cquery_result_algo_bytes", "kmx_cquery_result_free"]

_lib.kmx_zquery_bits_bytes.restype = C.c_uint64
_lib.kmx_zquery_bits_bytes.argtypes = [C.c_uint64, C.c_uint32]
_lib.kmx_zquery_dev.argtypes = [_vp, C.POINTER(KmxZqueryTask), C.POINTER(_vp)]
_lib.kmx_zquery_host.argtypes = [_vp, C.POINTER(KmxZqueryTask), C.POINTER(_vp)]
_lib.kmx_zquery_result_wait.argtypes = [_vp]
for _f in ("kmx_zquery_result_n_seqs", "kmx_zquery_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_zquery_result_copy_kmers", "kmx_zquery_result_copy_hits"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
for _f in ("kmx_zquery_result_hits_dev", "kmx_zquery_result_bits_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_zquery_result_kernel_ms.restype = C.c_double
_lib.kmx_zquery_result_kernel_ms.argtypes = [_vp]
_lib.kmx_zquery_result_free.argtypes = [_vp]
ZQUERY_EXPORTS = ["kmx_zquery_bits_bytes", "kmx_zquery_dev", "kmx_zquery_host", "kmx_zquery_result_wait", "kmx_zquery_result_n_seqs",
                  "kmx_zquery_result_copy_kmers", "kmx_zquery_result_copy_hits", "kmx_zquery_result_hits_dev", "kmx_zquery_result_bits_dev",
                  "kmx_zquery_result_kernel_ms", "kmx_zquery_result_algo_bytes", "kmx_zquery_result_free"]

_lib.kmx_dist_dev.argtypes = [_vp, C.POINTER(KmxDistTask), C.POINTER(_vp)]
_lib.kmx_dist_host.argtypes = [_vp, C.POINTER(KmxDistTask), C.POINTER(_vp)]
_lib.kmx_dist_result_wait.argtypes = [_vp]
_lib.kmx_dist_result_algo_bytes.restype = C.c_uint64
_lib.kmx_dist_result_algo_bytes.argtypes = [_vp]
for _f in ("kmx_dist_result_copy_inter", "kmx_dist_result_copy_mins"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
for _f in ("kmx_dist_result_inter_dev", "kmx_dist_result_mins_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_dist_result_kernel_ms.restype = C.c_double
_lib.kmx_dist_result_kernel_ms.argtypes = [_vp]
_lib.kmx_dist_result_kernel_parts_ms.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.kmx_dist_result_free.argtypes = [_vp]
DIST_EXPORTS = ["kmx_dist_dev", "kmx_dist_host", "kmx_dist_result_wait", "kmx_dist_result_inter_dev", "kmx_dist_result_mins_dev",
                "kmx_dist_result_copy_inter", "kmx_dist_result_copy_mins", "kmx_dist_result_kernel_ms", "kmx_dist_result_kernel_parts_ms",
                "kmx_dist_result_algo_bytes", "kmx_dist_result_free"]
_lib.kmx_colsums_dev.argtypes = [_vp, C.POINTER(KmxColsumsTask), C.POINTER(_vp)]
_lib.kmx_colsums_host.argtypes = [_vp, C.POINTER(KmxColsumsTask), C.POINTER(_vp)]
_lib.kmx_colsums_result_wait.argtypes = [_vp]
_lib.kmx_colsums_result_sums_dev.restype = _vp
_lib.kmx_colsums_result_sums_dev.argtypes = [_vp]
_lib.kmx_colsums_result_copy_sums.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_colsums_result_kernel_ms.restype = C.c_double
_lib.kmx_colsums_result_kernel_ms.argtypes = [_vp]
_lib.kmx_colsums_result_algo_bytes.restype = C.c_uint64
_lib.kmx_colsums_result_algo_bytes.argtypes = [_vp]
_lib.kmx_colsums_result_free.argtypes = [_vp]
_lib.kmx_diff_dev.argtypes = [_vp, C.POINTER(KmxDiffTask), C.POINTER(_vp)]
_lib.kmx_diff_host.argtypes = [_vp, C.POINTER(KmxDiffTask), C.POINTER(_vp)]
_lib.kmx_diff_result_wait.argtypes = [_vp]
for _f in ("kmx_diff_result_rows", "kmx_diff_result_row_bytes", "kmx_diff_result_body_bytes", "kmx_diff_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_diff_result_body_dev", "kmx_diff_result_recs_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_diff_result_copy_body.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_diff_result_copy_recs.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_diff_result_kernel_ms.restype = C.c_double
_lib.kmx_diff_result_kernel_ms.argtypes = [_vp]
_lib.kmx_diff_result_free.argtypes = [_vp]
DIFF_EXPORTS = ["kmx_colsums_dev", "kmx_colsums_host", "kmx_colsums_result_wait", "kmx_colsums_result_sums_dev", "kmx_colsums_result_copy_sums",
                "kmx_colsums_result_kernel_ms", "kmx_colsums_result_algo_bytes", "kmx_colsums_result_free",
                "kmx_diff_dev", "kmx_diff_host", "kmx_diff_result_wait", "kmx_diff_result_rows", "kmx_diff_result_row_bytes",
                "kmx_diff_result_body_bytes", "kmx_diff_result_body_dev", "kmx_diff_result_copy_body", "kmx_diff_result_recs_dev",
                "kmx_diff_result_copy_recs", "kmx_diff_result_kernel_ms", "kmx_diff_result_algo_bytes", "kmx_diff_result_free"]

_lib.kmx_assoc_dev.argtypes = [_vp, C.POINTER(KmxAssocTask), C.POINTER(_vp)]
_lib.kmx_assoc_host.argtypes = [_vp, C.POINTER(KmxAssocTask), C.POINTER(_vp)]
_lib.kmx_assoc_result_wait.argtypes = [_vp]
for _f in ("kmx_assoc_result_rows", "kmx_assoc_result_row_bytes", "kmx_assoc_result_body_bytes", "kmx_assoc_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_assoc_result_body_dev", "kmx_assoc_result_recs_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_assoc_result_copy_body.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_assoc_result_copy_recs.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_assoc_result_kernel_ms.restype = C.c_double
_lib.kmx_assoc_result_kernel_ms.argtypes = [_vp]
_lib.kmx_assoc_result_free.argtypes = [_vp]
ASSOC_EXPORTS = ["kmx_assoc_dev", "kmx_assoc_host", "kmx_assoc_result_wait", "kmx_assoc_result_rows", "kmx_assoc_result_row_bytes",
                 "kmx_assoc_result_body_bytes", "kmx_assoc_result_body_dev", "kmx_assoc_result_copy_body", "kmx_assoc_result_recs_dev",
                 "kmx_assoc_result_copy_recs", "kmx_assoc_result_kernel_ms", "kmx_assoc_result_algo_bytes", "kmx_assoc_result_free"]

_lib.kmx_select_dev.argtypes = [_vp, C.POINTER(KmxSelectTask), C.POINTER(_vp)]
_lib.kmx_select_host.argtypes = [_vp, C.POINTER(KmxSelectTask), C.POINTER(_vp)]
_lib.kmx_select_result_wait.argtypes = [_vp]
for _f in ("kmx_select_result_rows", "kmx_select_result_row_bytes", "kmx_select_result_body_bytes", "kmx_select_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
for _f in ("kmx_select_result_body_dev", "kmx_select_result_recs_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_select_result_copy_body.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_select_result_copy_recs.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_select_result_kernel_ms.restype = C.c_double
_lib.kmx_select_result_kernel_ms.argtypes = [_vp]
_lib.kmx_select_result_free.argtypes = [_vp]
SELECT_EXPORTS = ["kmx_select_dev", "kmx_select_host", "kmx_select_result_wait", "kmx_select_result_rows", "kmx_select_result_row_bytes",
                  "kmx_select_result_body_bytes", "kmx_select_result_body_dev", "kmx_select_result_copy_body", "kmx_select_result_recs_dev",
                  "kmx_select_result_copy_recs", "kmx_select_result_kernel_ms", "kmx_select_result_algo_bytes", "kmx_select_result_free"]
_lib.kmx_pan_dev.argtypes = [_vp, C.POINTER(KmxPanTask), C.POINTER(_vp)]
_lib.kmx_pan_host.argtypes = [_vp, C.POINTER(KmxPanTask), C.POINTER(_vp)]
_lib.kmx_pan_result_wait.argtypes = [_vp]
_lib.kmx_pan_result_algo_bytes.restype = C.c_uint64
_lib.kmx_pan_result_algo_bytes.argtypes = [_vp]
for _f in ("kmx_pan_result_copy_spectrum", "kmx_pan_result_copy_shared"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
for _f in ("kmx_pan_result_spectrum_dev", "kmx_pan_result_shared_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_pan_result_kernel_ms.restype = C.c_double
_lib.kmx_pan_result_kernel_ms.argtypes = [_vp]
_lib.kmx_pan_result_kernel_parts_ms.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.kmx_pan_result_free.argtypes = [_vp]
_lib.kmx_colors_dev.argtypes = [_vp, C.POINTER(KmxColorsTask), C.POINTER(_vp)]
_lib.kmx_colors_host.argtypes = [_vp, C.POINTER(KmxColorsTask), C.POINTER(_vp)]
_lib.kmx_colors_result_wait.argtypes = [_vp]
for _f in ("kmx_colors_result_n_classes", "kmx_colors_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_colors_result_ids_dev.restype = _vp
_lib.kmx_colors_result_ids_dev.argtypes = [_vp]
for _f in ("kmx_colors_result_copy_ids", "kmx_colors_result_copy_first", "kmx_colors_result_copy_sizes", "kmx_colors_result_copy_patterns"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_colors_result_kernel_ms.restype = C.c_double
_lib.kmx_colors_result_kernel_ms.argtypes = [_vp]
_lib.kmx_colors_result_kernel_parts_ms.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.kmx_colors_result_free.argtypes = [_vp]
COLORS_EXPORTS = ["kmx_colors_dev", "kmx_colors_host", "kmx_colors_result_wait", "kmx_colors_result_n_classes", "kmx_colors_result_ids_dev",
                  "kmx_colors_result_copy_ids", "kmx_colors_result_copy_first", "kmx_colors_result_copy_sizes", "kmx_colors_result_copy_patterns",
                  "kmx_colors_result_kernel_ms", "kmx_colors_result_kernel_parts_ms", "kmx_colors_result_algo_bytes", "kmx_colors_result_free"]
_lib.kmx_unitigs_dev.argtypes = [_vp, C.POINTER(KmxUnitigsTask), C.POINTER(_vp)]
_lib.kmx_unitigs_host.argtypes = [_vp, C.POINTER(KmxUnitigsTask), C.POINTER(_vp)]
_lib.kmx_unitigs_result_wait.argtypes = [_vp]
for _f in ("kmx_unitigs_result_n_unitigs", "kmx_unitigs_result_seq_bytes", "kmx_unitigs_result_algo_bytes"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_unitigs_result_unitig_dev.restype = _vp
_lib.kmx_unitigs_result_unitig_dev.argtypes = [_vp]
UNITIGS_COPIES = ["unitig", "pos", "ori", "start", "len", "circ", "seq_off", "seqs"]
for _f in UNITIGS_COPIES:
    getattr(_lib, "kmx_unitigs_result_copy_" + _f).argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_unitigs_result_kernel_ms.restype = C.c_double
_lib.kmx_unitigs_result_kernel_ms.argtypes = [_vp]
_lib.kmx_unitigs_result_kernel_parts_ms.argtypes = [_vp] + [C.POINTER(C.c_double)] * 4
_lib.kmx_unitigs_result_free.argtypes = [_vp]
UNITIGS_EXPORTS = (["kmx_unitigs_dev", "kmx_unitigs_host", "kmx_unitigs_result_wait", "kmx_unitigs_result_n_unitigs", "kmx_unitigs_result_unitig_dev",
                    "kmx_unitigs_result_seq_bytes", "kmx_unitigs_result_kernel_ms", "kmx_unitigs_result_kernel_parts_ms", "kmx_unitigs_result_algo_bytes",
                    "kmx_unitigs_result_free"] + ["kmx_unitigs_result_copy_" + _f for _f in UNITIGS_COPIES])
_lib.kmx_groupsum_dev.argtypes = [_vp, C.POINTER(KmxGroupsumTask), C.POINTER(_vp)]
_lib.kmx_groupsum_host.argtypes = [_vp, C.POINTER(KmxGroupsumTask), C.POINTER(_vp)]
_lib.kmx_groupsum_result_wait.argtypes = [_vp]
_lib.kmx_groupsum_result_algo_bytes.restype = C.c_uint64
_lib.kmx_groupsum_result_algo_bytes.argtypes = [_vp]
for _f in ("present", "sums", "size"):
    getattr(_lib, f"kmx_groupsum_result_{_f}_dev").restype = _vp
    getattr(_lib, f"kmx_groupsum_result_{_f}_dev").argtypes = [_vp]
    getattr(_lib, f"kmx_groupsum_result_copy_{_f}").argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_groupsum_result_kernel_ms.restype = C.c_double
_lib.kmx_groupsum_result_kernel_ms.argtypes = [_vp]
_lib.kmx_groupsum_result_free.argtypes = [_vp]
GROUPSUM_EXPORTS = ["kmx_groupsum_dev", "kmx_groupsum_host", "kmx_groupsum_result_wait", "kmx_groupsum_result_present_dev", "kmx_groupsum_result_sums_dev",
                    "kmx_groupsum_result_size_dev", "kmx_groupsum_result_copy_present", "kmx_groupsum_result_copy_sums", "kmx_groupsum_result_copy_size",
                    "kmx_groupsum_result_kernel_ms", "kmx_groupsum_result_algo_bytes", "kmx_groupsum_result_free"]
_lib.kmx_kset_dev.argtypes = [_vp, C.POINTER(KmxKsetTask), C.POINTER(_vp)]
_lib.kmx_kset_host.argtypes = [_vp, C.POINTER(KmxKsetTask), C.POINTER(_vp)]
_lib.kmx_kset_wait.argtypes = [_vp]
for _f in ("kmx_kset_n", "kmx_kset_n_distinct"):
    getattr(_lib, _f).restype = C.c_uint64
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_kset_kmer_size.restype = C.c_uint32
_lib.kmx_kset_kmer_size.argtypes = [_vp]
_lib.kmx_kset_copy_ids.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_kset_kernel_ms.restype = C.c_double
_lib.kmx_kset_kernel_ms.argtypes = [_vp]
_lib.kmx_kset_free.argtypes = [_vp]
KSET_EXPORTS = ["kmx_kset_dev", "kmx_kset_host", "kmx_kset_wait", "kmx_kset_n", "kmx_kset_n_distinct", "kmx_kset_kmer_size", "kmx_kset_copy_ids",
                "kmx_kset_kernel_ms", "kmx_kset_free"]
_lib.kmx_match_dev.argtypes = [_vp, C.POINTER(KmxMatchTask), C.POINTER(_vp)]
_lib.kmx_match_host.argtypes = [_vp, C.POINTER(KmxMatchTask), C.POINTER(_vp)]
_lib.kmx_match_result_wait.argtypes = [_vp]
for _f in ("n_seqs", "n_bases", "total_kmers", "total_hits", "algo_bytes"):
    getattr(_lib, "kmx_match_result_" + _f).restype = C.c_uint64
    getattr(_lib, "kmx_match_result_" + _f).argtypes = [_vp]
MATCH_COPIES = ["recs", "ids", "occ"]
for _f in MATCH_COPIES:
    getattr(_lib, "kmx_match_result_copy_" + _f).argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_match_result_occ_dev.restype = _vp
_lib.kmx_match_result_occ_dev.argtypes = [_vp]
_lib.kmx_match_result_kernel_ms.restype = C.c_double
_lib.kmx_match_result_kernel_ms.argtypes = [_vp]
_lib.kmx_match_result_kernel_parts_ms.argtypes = [_vp] + [C.POINTER(C.c_double)] * 2
_lib.kmx_match_result_free.argtypes = [_vp]
MATCH_EXPORTS = (["kmx_match_dev", "kmx_match_host", "kmx_match_result_wait", "kmx_match_result_n_seqs", "kmx_match_result_n_bases",
                  "kmx_match_result_occ_dev", "kmx_match_result_total_kmers", "kmx_match_result_total_hits", "kmx_match_result_kernel_ms",
                  "kmx_match_result_kernel_parts_ms", "kmx_match_result_algo_bytes", "kmx_match_result_free"] +
                 ["kmx_match_result_copy_" + _f for _f in MATCH_COPIES])
_lib.kmx_gram_dev.argtypes = [_vp, C.POINTER(KmxGramTask), C.POINTER(_vp)]
_lib.kmx_gram_host.argtypes = [_vp, C.POINTER(KmxGramTask), C.POINTER(_vp)]
_lib.kmx_gram_result_wait.argtypes = [_vp]
_lib.kmx_gram_result_algo_bytes.restype = C.c_uint64
_lib.kmx_gram_result_algo_bytes.argtypes = [_vp]
_lib.kmx_gram_result_copy_table.argtypes = [_vp, _vp, C.c_uint64]
_lib.kmx_gram_result_table_dev.restype = _vp
_lib.kmx_gram_result_table_dev.argtypes = [_vp]
_lib.kmx_gram_result_kernel_ms.restype = C.c_double
_lib.kmx_gram_result_kernel_ms.argtypes = [_vp]
_lib.kmx_gram_result_kernel_parts_ms.argtypes = [_vp] + [C.POINTER(C.c_double)] * 4
_lib.kmx_gram_result_free.argtypes = [_vp]
GRAM_EXPORTS = ["kmx_gram_dev", "kmx_gram_host", "kmx_gram_result_wait", "kmx_gram_result_table_dev", "kmx_gram_result_copy_table",
                "kmx_gram_result_kernel_ms", "kmx_gram_result_kernel_parts_ms", "kmx_gram_result_algo_bytes", "kmx_gram_result_free"]
_lib.kmx_spectra_dev.argtypes = [_vp, C.POINTER(KmxSpectraTask), C.POINTER(_vp)]
_lib.kmx_spectra_host.argtypes = [_vp, C.POINTER(KmxSpectraTask), C.POINTER(_vp)]
_lib.kmx_spectra_result_wait.argtypes = [_vp]
_lib.kmx_spectra_result_algo_bytes.restype = C.c_uint64
_lib.kmx_spectra_result_algo_bytes.argtypes = [_vp]
for _f in ("kmx_spectra_result_copy_hist", "kmx_spectra_result_copy_joint"):
    getattr(_lib, _f).argtypes = [_vp, _vp, C.c_uint64]
for _f in ("kmx_spectra_result_hist_dev", "kmx_spectra_result_joint_dev"):
    getattr(_lib, _f).restype = _vp
    getattr(_lib, _f).argtypes = [_vp]
_lib.kmx_spectra_result_kernel_ms.restype = C.c_double
_lib.kmx_spectra_result_kernel_ms.argtypes = [_vp]
_lib.kmx_spectra_result_kernel_parts_ms.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.kmx_spectra_result_free.argtypes = [_vp]
SPECTRA_EXPORTS = ["kmx_spectra_dev", "kmx_spectra_host", "kmx_spectra_result_wait", "kmx_spectra_result_hist_dev", "kmx_spectra_result_joint_dev",
                   "kmx_spectra_result_copy_hist", "kmx_spectra_result_copy_joint", "kmx_spectra_result_kernel_ms", "kmx_spectra_result_kernel_parts_ms",
                   "kmx_spectra_result_algo_bytes", "kmx_spectra_result_free"]
PAN_EXPORTS = ["kmx_pan_dev", "kmx_pan_host", "kmx_pan_result_wait", "kmx_pan_result_spectrum_dev", "kmx_pan_result_shared_dev",
               "kmx_pan_result_copy_spectrum", "kmx_pan_result_copy_shared", "kmx_pan_result_kernel_ms", "kmx_pan_result_kernel_parts_ms",
               "kmx_pan_result_algo_bytes", "kmx_pan_result_free"]


def zquery_bits_bytes(n_bases, n_cols):
    """bytes of the bits table a series of zquery calls shares: n_bases rows of 4 * ceil(ceil(n_cols / 8) / 4) bytes"""
    return _lib.kmx_zquery_bits_bytes(n_bases, n_cols)


def filter_want(want):
    """'m,v' / 'kmv' / a KMX_FILTER_* mask -> the mask"""
    if isinstance(want, int):
        return want
    bits = {"m": FILTER_M, "v": FILTER_V, "k": FILTER_K}
    return sum({bits[c] for c in want.replace(",", "")})


def key_words_of(k):
    """64-bit words of a k-mer key: ceil(k / 32) (kmer.hpp:215 m_n_data; io/kmer_file.hpp:84 kmer_slots) -- 3 for 65 ... 96, 4 for 97 ... 127"""
    return (k + 31) // 32


class KmxError(RuntimeError):
    pass


def pack_records(keys, counts, key_words=1):
    """(keys uint64[n] or [n, kw], counts uint32[n]) -> packed record bytes (key words + u32 count)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, key_words)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n = len(counts)
    rec = np.zeros((n, key_words * 2 + 1), dtype=np.uint32)
    rec[:, :key_words * 2] = keys.view(np.uint32).reshape(n, key_words * 2)
    rec[:, key_words * 2] = counts
    return rec


class Context:
    """One engine context = one GPU + one HIP stream (a merge task pool thread in the reference)."""

    def __init__(self, device=0):
        h = _vp()
        rc = _lib.kmx_create(device, C.byref(h))
        if rc != 0:
            raise KmxError(f"kmx_create failed ({rc}): {_lib.kmx_last_error(None).decode()}")
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            _lib.kmx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise KmxError(f"{what} failed ({rc}): {_lib.kmx_last_error(self._h).decode()}")

    def set_profiling(self, on=True):
        self._check(_lib.kmx_set_profiling(self._h, 1 if on else 0), "kmx_set_profiling")

    def set_file_order(self, on=True):
        """COUNT / PA rows at their final place out of the column-blocked kernels (default), or where the kernels leave them"""
        self._check(_lib.kmx_set_file_order(self._h, 1 if on else 0), "kmx_set_file_order")

    @property
    def stream(self):
        return _lib.kmx_stream(self._h)

    @staticmethod
    def _task(lists_ptr_n, key_words, soft_min, rec_min, share_min, mode, lower, upper, bitw, rows_hint, keep):
        n = len(lists_ptr_n)
        arr = (KmxList * n)()
        for i, (p, cnt) in enumerate(lists_ptr_n):
            arr[i].recs = p
            arr[i].n = cnt
        sm = (C.c_uint32 * n)(*[int(x) for x in soft_min])
        keep.extend([arr, sm])
        t = KmxMergeTask()
        t.n_lists, t.key_words, t.lists, t.soft_min = n, key_words, arr, sm
        t.rec_min, t.share_min, t.mode, t.bitw = rec_min, share_min, mode, bitw
        t.lower, t.upper, t.rows_hint = lower, upper, rows_hint
        return t

    def merge(self, lists, key_words, soft_min, rec_min, share_min, mode, lower=0, upper=0, bitw=2, rows_hint=0):
        """Host-buffer merge of one partition (kmx_merge).  lists: [(keys, counts)] numpy arrays.
        -> (body bytes, rows, stats uint64[6, N])"""
        keep, recs = [], []
        for k, c in lists:
            r = pack_records(k, c, key_words)
            recs.append(r)
        t = self._task([(r.ctypes.data if len(r) else None, len(r)) for r in recs], key_words, soft_min, rec_min,
                       share_min, mode, lower, upper, bitw, rows_hint, keep)
        body, nb, rows = _vp(), C.c_uint64(), C.c_uint64()
        stats = np.zeros((STATS_ROWS, len(lists)), dtype=np.uint64)
        self._check(_lib.kmx_merge(self._h, C.byref(t), C.byref(body), C.byref(nb), C.byref(rows), stats.ctypes.data),
                    "kmx_merge")
        data = (C.string_at(body.value, nb.value) if nb.value < (1 << 31) else bytes((C.c_ubyte * nb.value).from_address(body.value))) if nb.value else b""      # (string_at takes an int)
        _lib.kmx_free(body)
        return data, rows.value, stats

    def _take(self, kp, cp, n, width):
        keys = np.ctypeslib.as_array((C.c_uint64 * (n * width)).from_address(kp.value)).copy().reshape(n, width) if n \
            else np.zeros((0, width), np.uint64)
        cnts = np.ctypeslib.as_array((C.c_uint32 * n).from_address(cp.value)).copy() if n else np.zeros(0, np.uint32)
        _lib.kmx_free(kp)
        _lib.kmx_free(cp)
        return keys, cnts

    def count_kmer(self, superk: bytes, k, hard_min):
        """kmx_count_kmer: super-k-mer record stream -> (canonical k-mers uint64[n, ceil(k/32)], counts)"""
        kp, cp, n = _vp(), _vp(), C.c_uint64()
        self._check(_lib.kmx_count_kmer(self._h, superk, len(superk), k, hard_min, C.byref(kp), C.byref(cp),
                                        C.byref(n)), "kmx_count_kmer")
        return self._take(kp, cp, n.value, key_words_of(k))

    def count_hash(self, superk: bytes, k, window, partition, hard_min):
        kp, cp, n = _vp(), _vp(), C.c_uint64()
        self._check(_lib.kmx_count_hash(self._h, superk, len(superk), k, window, partition, hard_min, C.byref(kp),
                                        C.byref(cp), C.byref(n)), "kmx_count_hash")
        keys, cnts = self._take(kp, cp, n.value, 1)
        return keys.reshape(-1), cnts

    def count_batch(self, streams, k, hard_min, window=0, partitions=None):
        """kmx_count_batch: the partition streams of one sample -> [(keys, counts)] per stream.
        window != 0 selects window hashes (partitions[p] = window index of stream p)."""
        n = len(streams)
        sp = (C.c_char_p * n)(*[s if s else None for s in streams])
        ln = (C.c_uint64 * n)(*[len(s) for s in streams])
        pid = (C.c_uint64 * n)(*(partitions if partitions is not None else range(n)))
        kp, cp, no = (_vp * n)(), (_vp * n)(), (C.c_uint64 * n)()
        self._check(_lib.kmx_count_batch(self._h, n, sp, ln, k, 1 if window else 0, window, pid, hard_min, kp, cp, no),
                    "kmx_count_batch")
        width = 1 if window else key_words_of(k)
        out = []
        for p in range(n):
            keys, cnts = self._take(_vp(kp[p]), _vp(cp[p]), no[p], width)
            out.append((keys.reshape(-1) if window else keys, cnts))
        return out

    def transpose_bits(self, mat, nrows, ncols):
        mat = np.ascontiguousarray(mat, dtype=np.uint8)
        out = np.zeros(ncols * (nrows // 8), dtype=np.uint8)
        self._check(_lib.kmx_transpose_bits(self._h, mat.ctypes.data, nrows, ncols, out.ctypes.data),
                    "kmx_transpose_bits")
        return out

    @staticmethod
    def pack_reads(reads):
        """list of reads (str/bytes) -> (concatenated bases, uint64 offsets[n + 1]) as kmx_superk_partition takes them"""
        bs = [r if isinstance(r, bytes) else r.encode() for r in reads]
        offs = np.zeros(len(bs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        return b"".join(bs), offs

    def superk_partition(self, reads, k, m, repart, nb_parts):
        """kmx_superk_partition: list of reads (str/bytes), or pack_reads() output -> [(record stream bytes, n_kmers)]
        per partition"""
        blob, offs = reads if isinstance(reads, tuple) else self.pack_reads(reads)
        rep = np.ascontiguousarray(repart, dtype=np.uint16)
        ob = (_vp * nb_parts)()
        ol = (C.c_uint64 * nb_parts)()
        okm = (C.c_uint64 * nb_parts)()
        self._check(_lib.kmx_superk_partition(self._h, blob, offs.ctypes.data, len(offs) - 1, k, m, rep.ctypes.data, nb_parts,
                                              ob, ol, okm), "kmx_superk_partition")
        out = []
        for p in range(nb_parts):
            out.append((C.string_at(ob[p], ol[p]) if ol[p] else b"", int(okm[p])))
            _lib.kmx_free(ob[p])
        return out

    def superk_partition_stats(self, reads, k, m, repart, nb_parts, streams=True):
        """kmx_superk_partition_stats -> ([(record stream, n_kmers)] or None, pinfo[nb_parts, 2 + 5*256], minim_superks,
        minim_kmers, minim_kxmers); streams=False: the statistics-only pass"""
        blob, offs = reads if isinstance(reads, tuple) else self.pack_reads(reads)
        rep = np.ascontiguousarray(repart, dtype=np.uint16)
        pin = np.zeros(nb_parts * PINFO_STRIDE, dtype=np.uint64)
        ms, mk, mx = (np.zeros(4 ** m, dtype=np.uint64) for _ in range(3))
        st = KmxSuperkStats(pin.ctypes.data, ms.ctypes.data, mk.ctypes.data, mx.ctypes.data, 0)
        ob = (_vp * nb_parts)()
        ol = (C.c_uint64 * nb_parts)()
        okm = (C.c_uint64 * nb_parts)()
        self._check(_lib.kmx_superk_partition_stats(self._h, blob, offs.ctypes.data, len(offs) - 1, k, m, rep.ctypes.data,
                                                    nb_parts, ob if streams else None, ol, okm, C.byref(st)),
                    "kmx_superk_partition_stats")
        out = None
        if streams:
            out = []
            for p in range(nb_parts):
                out.append((C.string_at(ob[p], ol[p]) if ol[p] else b"", int(okm[p])))
                _lib.kmx_free(ob[p])
        assert st.nb_superk == int(ms.sum())
        return out, pin.reshape(nb_parts, -1), ms, mk, mx

    def count_reads(self, reads, k, m, repart, nb_parts, hard_min, window=0, streams=False):
        """kmx_count_reads: reads -> [(keys, counts)] per partition without the super-k-mer streams leaving HBM
        -> (counts per partition, k-mers per partition, [(stream, ...)] or None, info numbers uint64[nb_parts, 2])"""
        blob, offs = reads if isinstance(reads, tuple) else self.pack_reads(reads)
        rep = np.ascontiguousarray(repart, dtype=np.uint16)
        kp, cp, no, nk = (_vp * nb_parts)(), (_vp * nb_parts)(), (C.c_uint64 * nb_parts)(), (C.c_uint64 * nb_parts)()
        ob, ol = (_vp * nb_parts)(), (C.c_uint64 * nb_parts)()
        info = (C.c_uint64 * (2 * nb_parts))()
        self._check(_lib.kmx_count_reads(self._h, blob, offs.ctypes.data, len(offs) - 1, k, m, rep.ctypes.data, nb_parts,
                                         1 if window else 0, window, hard_min, kp, cp, no, nk, ob if streams else None,
                                         ol if streams else None, info, None), "kmx_count_reads")
        width = 1 if window else key_words_of(k)
        out = []
        for p in range(nb_parts):
            keys, cnts = self._take(_vp(kp[p]), _vp(cp[p]), no[p], width)
            out.append((keys.reshape(-1) if window else keys, cnts))
        st = None
        if streams:
            st = []
            for p in range(nb_parts):
                st.append(C.string_at(ob[p], ol[p]) if ol[p] else b"")
                _lib.kmx_free(ob[p])
        return out, [int(x) for x in nk], st, np.array(list(info), dtype=np.uint64).reshape(nb_parts, 2)

    def upload_reads(self, blob, offs=None):
        """kmx_reads_upload: the bases of a batch sent to the device ahead of the count call (from page-locked memory, on the context's
        upload stream) -> a handle for count_reads_dev(resident=...) and release_reads.  What `kmx pipeline` does with the NEXT
        sample while this one is counted.  offs: the reads' offsets are put behind the bases in the same page-locked block, as
        `kmx pipeline` does, and count_reads_dev(resident=handle) hands the call THAT array (a DMA, no staging copy inside the call)."""
        n = len(blob)
        at = (n + 63) & ~63
        nb = 0 if offs is None else 8 * len(offs)
        pin = _lib.kmx_alloc_pinned(max(at + nb, 1))
        C.memmove(pin, blob, n)
        po = None
        if offs is not None:
            po = np.frombuffer((C.c_char * nb).from_address(pin + at), dtype=np.uint64)
            po[:] = np.ascontiguousarray(offs, dtype=np.uint64)
        dev = _vp()
        self._check(_lib.kmx_reads_upload(self._h, pin, n, C.byref(dev)), "kmx_reads_upload")
        return (dev, pin, po)

    def release_reads(self, handle):
        _lib.kmx_reads_release(self._h, handle[0])
        _lib.kmx_free_pinned(handle[1])

    def count_reads_dev(self, reads, k, m, repart, nb_parts, hard_min, stores, window=0, raw=False, sparse=False, ahead=False, resident=None):
        """kmx_count_reads_dev: as count_reads, the results left on the device as packed records in `stores` (partition p ->
        stores[p % len(stores)]) -> ([(device pointer, records)] per partition, k-mers per partition, raw tables or None).
        resident: a handle of upload_reads for the same bases (the call is given the device pointer; the handle stays the caller's)"""
        blob, offs = reads if isinstance(reads, tuple) else self.pack_reads(reads)
        rep = np.ascontiguousarray(repart, dtype=np.uint16)
        sp = (_vp * len(stores))(*[s._h for s in stores])
        lists, nk = (KmxList * nb_parts)(), (C.c_uint64 * nb_parts)()
        rw, tabs = None, None
        spt = None
        if raw:
            tabs = (np.zeros(nb_parts * 1280, np.uint32), np.zeros(4 ** m, np.uint32), np.zeros(4 ** m, np.uint32))
            rw = KmxSuperkRaw(tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, 0, None, 0, 0)
            if sparse:      # the per-minimizer records as {minimizer, super-k-mers, k-mers} triples: turned back into the tables here
                spt = np.zeros((4 ** m, 3), np.uint32)
                rw = KmxSuperkRaw(tabs[0].ctypes.data, None, None, 0, spt.ctypes.data, 4 ** m, 0)
        dev = None
        if resident is not None:
            ahead = False
            blob_arg = C.cast(resident[0], C.c_char_p)
            if len(resident) > 2 and resident[2] is not None:
                offs = resident[2]
        elif ahead:      # kmx_reads_upload: the bases sent to the device ahead of the call (from page-locked memory), the call given the device pointer
            n = len(blob)
            pin = _lib.kmx_alloc_pinned(max(n, 1))
            C.memmove(pin, blob, n)
            dev = _vp()
            self._check(_lib.kmx_reads_upload(self._h, pin, n, C.byref(dev)), "kmx_reads_upload")
            blob_arg = C.cast(dev, C.c_char_p)
        elif resident is None:
            blob_arg = blob
        try:
            self._check(_lib.kmx_count_reads_dev(self._h, blob_arg, offs.ctypes.data, len(offs) - 1, k, m, rep.ctypes.data, nb_parts,
                                                 1 if window else 0, window, hard_min, sp, len(stores), lists, nk, None, None, None, None,
                                                 C.byref(rw) if raw else None), "kmx_count_reads_dev")
        finally:
            if ahead:
                _lib.kmx_reads_release(self._h, dev)
                _lib.kmx_free_pinned(pin)
        if spt is not None:
            t = spt[:int(rw.minim_sparse_n)]
            assert len(np.unique(t[:, 0])) == len(t)
            tabs[1][t[:, 0]] = t[:, 1]; tabs[2][t[:, 0]] = t[:, 2]
        return [(lists[p].recs, int(lists[p].n)) for p in range(nb_parts)], [int(x) for x in nk], (tabs + (int(rw.nb_superk),)) if raw else None

    def count_reads_dev_multi(self, samples, k, m, repart, nb_parts, hard_min, stores, window=0, raw=False):
        """kmx_count_reads_dev_multi: several samples (lists of reads) in ONE call -> per sample what count_reads_dev returns
        (raw: the sparse form, turned back into tables here)"""
        S = len(samples)
        packed = [self.pack_reads(r) for r in samples]
        rep = np.ascontiguousarray(repart, dtype=np.uint16)
        bp = (C.c_char_p * S)(*[b for b, _ in packed])
        op = (_vp * S)(*[o.ctypes.data for _, o in packed])
        ns = (C.c_uint64 * S)(*[len(o) - 1 for _, o in packed])
        sp = (_vp * len(stores))(*[s._h for s in stores])
        lists, nk = (KmxList * (S * nb_parts))(), (C.c_uint64 * (S * nb_parts))()
        info = np.zeros((S * nb_parts, 2), np.uint64)
        rws, tabs, spts = None, [], []
        if raw:
            rws = (KmxSuperkRaw * S)()
            for i in range(S):
                t = (np.zeros(nb_parts * 1280, np.uint32), np.zeros(4 ** m, np.uint32), np.zeros(4 ** m, np.uint32))
                q = np.zeros((4 ** m, 3), np.uint32)
                tabs.append(t); spts.append(q)
                rws[i] = KmxSuperkRaw(t[0].ctypes.data, None, None, 0, q.ctypes.data, 4 ** m, 0)
        self._check(_lib.kmx_count_reads_dev_multi(self._h, S, bp, op, ns, k, m, rep.ctypes.data, nb_parts, 1 if window else 0, window, hard_min,
                                                   sp, len(stores), lists, nk, info.ctypes.data, rws), "kmx_count_reads_dev_multi")
        out = []
        for i in range(S):
            r = None
            if raw:
                t = spts[i][:int(rws[i].minim_sparse_n)]
                assert len(np.unique(t[:, 0])) == len(t)
                tabs[i][1][t[:, 0]] = t[:, 1]; tabs[i][2][t[:, 0]] = t[:, 2]
                r = tabs[i] + (int(rws[i].nb_superk),)
            out.append(([(lists[i * nb_parts + p].recs, int(lists[i * nb_parts + p].n)) for p in range(nb_parts)],
                        [int(nk[i * nb_parts + p]) for p in range(nb_parts)], info[i * nb_parts:(i + 1) * nb_parts], r))
        return out

    def read_list(self, dev_ptr, n, key_words=1):
        """a device-resident count list -> (keys uint64[n, key_words], counts uint32[n])"""
        w = key_words * 2 + 1
        rec = np.zeros((n, w), np.uint32)
        if n:
            self._check(_lib.kmx_copy_to_host(self._h, rec.ctypes.data, dev_ptr, n * w * 4), "kmx_copy_to_host")
        keys = np.ascontiguousarray(rec[:, :key_words * 2]).view(np.uint64).reshape(n, key_words)
        return keys, rec[:, key_words * 2].copy()

    def hist_reset(self):
        """kmx_hist_reset: zero the abundance histogram; the count calls that follow add their distinct keys to it"""
        self._check(_lib.kmx_hist_reset(self._h), "kmx_hist_reset")

    def hist_off(self):
        self._check(_lib.kmx_hist_off(self._h), "kmx_hist_off")

    def hist_read(self, lower=1, upper=255):
        """kmx_hist_read -> dict(unique, total (bins lower..upper), oob [lower unique, upper unique, lower total, upper total], sums [unique, total])"""
        n = upper - lower + 1
        h = dict(unique=np.zeros(n, np.uint64), total=np.zeros(n, np.uint64), oob=np.zeros(4, np.uint64), sums=np.zeros(2, np.uint64))
        self._check(_lib.kmx_hist_read(self._h, lower, upper, h["unique"].ctypes.data, h["total"].ctypes.data, h["oob"].ctypes.data, h["sums"].ctypes.data), "kmx_hist_read")
        return h

    def superk_sample(self, reads, k, m, budget):
        """kmx_superk_sample -> (reads used, their super-k-mers, kx-mers per minimizer)"""
        blob, offs = reads if isinstance(reads, tuple) else self.pack_reads(reads)
        mx = np.zeros(4 ** m, dtype=np.uint64)
        st = KmxSuperkStats(None, None, None, mx.ctypes.data, 0)
        used, nsk = C.c_uint64(), C.c_uint64()
        self._check(_lib.kmx_superk_sample(self._h, blob, offs.ctypes.data, len(offs) - 1, k, m, budget, C.byref(st),
                                           C.byref(used), C.byref(nsk)), "kmx_superk_sample")
        return used.value, nsk.value, mx

    def prepare(self, tasks):
        """Builds the kmx_merge_task array once (so a timed loop does no Python marshalling).
        tasks: list of dicts with keys lists=[(device_ptr, n)], key_words, soft_min, rec_min, share_min,
        mode, [lower, upper, bitw, rows_hint]."""
        keep = []
        arr = (KmxMergeTask * len(tasks))()
        for i, d in enumerate(tasks):
            arr[i] = self._task(d["lists"], d["key_words"], d["soft_min"], d["rec_min"], d["share_min"], d["mode"],
                                d.get("lower", 0), d.get("upper", 0), d.get("bitw", 2), d.get("rows_hint", 0), keep)
        return (arr, len(tasks), [len(d["lists"]) for d in tasks], keep)

    def merge_host(self, tasks):
        """kmx_merge_host: like merge_dev with HOST record pointers (uploaded by libkmx on its upload stream)"""
        prep = tasks if isinstance(tasks, tuple) else self.prepare(tasks)
        res = _vp()
        self._check(_lib.kmx_merge_host(self._h, prep[0], prep[1], C.byref(res)), "kmx_merge_host")
        return MergeResult(self, res, prep[2])

    def merge_dev(self, tasks):
        """Device-resident batch merge (kmx_merge_dev) of a task list or a prepare()d batch.
        -> MergeResult (asynchronous; call .wait())."""
        prep = tasks if isinstance(tasks, tuple) else self.prepare(tasks)
        res = _vp()
        self._check(_lib.kmx_merge_dev(self._h, prep[0], prep[1], C.byref(res)), "kmx_merge_dev")
        return MergeResult(self, res, prep[2])

    def filter(self, rows_body, n_cols, key_words, mode, key_list, want="mv", marks=None):
        """kmx_filter_host: whole rows of a .count / .pa matrix body (bytes or uint8 array) against one sample's count list
        (keys uint64[n, key_words], counts uint32[n]).  marks: None (the rows are the whole partition) or a uint8 array of len(keys),
        zero before the first run of rows, updated in place.  -> FilterOutput"""
        rows = np.frombuffer(rows_body, dtype=np.uint8) if isinstance(rows_body, (bytes, bytearray, memoryview)) else np.ascontiguousarray(rows_body, dtype=np.uint8).reshape(-1)
        rec = pack_records(key_list[0], key_list[1], key_words)
        irb = key_words * 8 + (4 * n_cols if mode == MODE_COUNT else (n_cols + 7) // 8)
        if len(rows) % irb:
            raise ValueError(f"{len(rows)} bytes are not whole rows of {irb} bytes")
        if marks is not None and (marks.dtype != np.uint8 or len(marks) != len(rec) or not marks.flags.c_contiguous):
            raise ValueError("marks: a contiguous uint8 array with one entry per key record")
        t = KmxFilterTask(key_words, mode, n_cols, filter_want(want), rows.ctypes.data if len(rows) else None, len(rows) // irb,
                          KmxList(rec.ctypes.data if len(rec) else None, len(rec)), marks.ctypes.data if marks is not None and len(marks) else None, 0)
        if marks is not None and not len(marks):      # (an empty key list has no marks to carry)
            t.marks = None
        res = _vp()
        self._check(_lib.kmx_filter_host(self._h, C.byref(t), C.byref(res)), "kmx_filter_host")
        r = FilterResult(self, res, key_words)
        try:
            return r.output()
        finally:
            r.free()

    def filter_dev(self, rows_dev, n_rows, n_cols, key_words, mode, key_dev, want="mv", marks_dev=None, keep=False):
        """kmx_filter_dev: rows_dev a device pointer to n_rows whole rows (MergeResult.body_dev), key_dev = (device pointer, records)
        (a list of count_reads_dev), marks_dev None or a device pointer to one byte per key record.
        -> FilterOutput (numpy copies), or with keep the FilterResult itself (results left in HBM; .free() it)"""
        t = KmxFilterTask(key_words, mode, n_cols, filter_want(want), rows_dev, n_rows, KmxList(key_dev[0], key_dev[1]), marks_dev, 0)
        res = _vp()
        self._check(_lib.kmx_filter_dev(self._h, C.byref(t), C.byref(res)), "kmx_filter_dev")
        r = FilterResult(self, res, key_words)
        if keep:
            return r
        try:
            return r.output()
        finally:
            r.free()

    def _seq_inputs(self, reads, repart, matrices, fit):
        """the ctypes pieces of a sequence-query call.  reads: a list of sequences (str / bytes) or pack_reads() output; matrices[p]: bytes,
        a uint8 array or None; fit(p, a) is the family's rule for the flat uint8 body a of partition p: it raises ValueError, or returns
        the array to send.  -> (bases, offsets, n_seqs, repart, rows, keepalive): pointers into arrays that keepalive holds"""
        blob, offs = reads if isinstance(reads, tuple) else self.pack_reads(reads)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        rep = np.ascontiguousarray(repart, dtype=np.uint16)
        bb = np.frombuffer(blob, dtype=np.uint8) if len(blob) else np.zeros(1, np.uint8)
        keepalive, rows = [bb, offs, rep], (C.c_void_p * len(matrices))()
        for p, mt in enumerate(matrices):
            if mt is None:
                continue
            a = np.frombuffer(mt, dtype=np.uint8) if isinstance(mt, (bytes, bytearray, memoryview)) else np.ascontiguousarray(mt, dtype=np.uint8).reshape(-1)
            a = fit(p, a)
            keepalive.append(a)
            rows[p] = a.ctypes.data
        return bb.ctypes.data, offs.ctypes.data, len(offs) - 1, rep.ctypes.data, rows, keepalive

    @staticmethod
    def _window_rows(window, nb, checked=True):
        """_seq_inputs' rule for a Bloom matrix: a body is window rows of nb bytes"""
        def fit(p, a):
            if checked and len(a) != window * nb:
                raise ValueError(f"partition {p}: {len(a)} bytes are not {window} rows of {nb} bytes")
            return a
        return fit

    def query(self, reads, k, m, repart, window, n_cols, matrices, hits_dev=None, keep=False):
        """kmx_query_host: reads a list of sequences (str / bytes) or pack_reads() output; matrices[p] the body of partition p's
        .cmbf (bytes or a uint8 array of window * ceil(n_cols / 8) bytes) or None (the partition is not part of the call);
        hits_dev None or a device pointer to a uint32 table [queries, n_cols] the call adds to.
        -> QueryOutput (numpy copies), or with keep the QueryResult itself (the table left in HBM; .free() it)"""
        bases, offs, n_seqs, rep, rows, keepalive = self._seq_inputs(reads, repart, matrices, self._window_rows(window, (n_cols + 7) // 8))
        t = KmxQueryTask(bases, offs, n_seqs, k, m, rep, len(matrices), n_cols, window, rows, hits_dev)
        res = _vp()
        self._check(_lib.kmx_query_host(self._h, C.byref(t), C.byref(res)), "kmx_query_host")
        r = QueryResult(self, res, n_cols)
        r.wait()      # (the host buffers above may go once the call has run)
        return self._finish(r, keep)

    def query_dev(self, bases_dev, offsets_dev, n_seqs, k, m, repart_dev, window, n_cols, rows_dev, hits_dev=None, keep=False):
        """kmx_query_dev: device pointers (a torch tensor's data_ptr()) to the bases, the uint64 offsets [n_seqs + 1] and the uint16
        repartition table; rows_dev[p] a device pointer to partition p's matrix body or None.  -> as query"""
        rows = (C.c_void_p * len(rows_dev))(*rows_dev)
        t = KmxQueryTask(bases_dev, offsets_dev, n_seqs, k, m, repart_dev, len(rows_dev), n_cols, window, rows, hits_dev)
        res = _vp()
        self._check(_lib.kmx_query_dev(self._h, C.byref(t), C.byref(res)), "kmx_query_dev")
        return self._finish(QueryResult(self, res, n_cols), keep)

    @staticmethod
    def _zquery_result(r, last, keep, owns_bits):
        if keep:
            return r
        if not last and owns_bits:
            r.free()
            raise ValueError("a call that opens a series (bits_dev=None, last=False) owns the series' table: keep=True")
        try:
            return r.output() if last else None
        finally:
            r.free()

    def zquery(self, reads, k, m, repart, window, n_cols, matrices, z, bits_dev=None, hits_dev=None, last=True, keep=False):
        """kmx_zquery_host: as query, for (k + z)-mers (the findere trick): a position counts for a sample when the rows of its z + 1
        overlapping k-mers all have the sample's bit.  A series of calls over the same reads, each with other partitions in
        `matrices`, shares one device table: the first call has bits_dev=None and keep=True (its result owns the table: .bits_dev()),
        the later ones pass that pointer, the one with last=True produces the result.  hits_dev None or a device pointer to a uint32
        table [queries, n_cols] the last call adds to.
        -> QueryOutput (numpy copies) when last, else None; with keep the ZqueryResult itself (.free() it)"""
        bases, offs, n_seqs, rep, rows, keepalive = self._seq_inputs(reads, repart, matrices, self._window_rows(window, (n_cols + 7) // 8))
        t = KmxZqueryTask(bases, offs, n_seqs, k, m, rep, len(matrices), n_cols, window, rows, z, 1 if last else 0, bits_dev, hits_dev)
        res = _vp()
        self._check(_lib.kmx_zquery_host(self._h, C.byref(t), C.byref(res)), "kmx_zquery_host")
        r = ZqueryResult(self, res, n_cols)
        r.wait()      # (the host buffers above may go once the call has run)
        return self._zquery_result(r, last, keep, bits_dev is None)

    def zquery_dev(self, bases_dev, offsets_dev, n_seqs, k, m, repart_dev, window, n_cols, rows_dev, z, bits_dev=None, hits_dev=None, last=True, keep=False):
        """kmx_zquery_dev: device pointers (a torch tensor's data_ptr()) to the bases, the uint64 offsets [n_seqs + 1] and the uint16
        repartition table; rows_dev[p] a device pointer to partition p's matrix body or None.  -> as zquery"""
        rows = (C.c_void_p * len(rows_dev))(*rows_dev)
        t = KmxZqueryTask(bases_dev, offsets_dev, n_seqs, k, m, repart_dev, len(rows_dev), n_cols, window, rows, z, 1 if last else 0, bits_dev, hits_dev)
        res = _vp()
        self._check(_lib.kmx_zquery_dev(self._h, C.byref(t), C.byref(res)), "kmx_zquery_dev")
        return self._zquery_result(ZqueryResult(self, res, n_cols), last, keep, bits_dev is None)

    @staticmethod
    def _kquery_sums(sums):
        return (1, None) if sums is True else (0, None) if sums is False or sums is None else (1, sums)

    def kquery(self, reads, k, m, repart, n_cols, key_words, mode, matrices, n_rows=None, hits_dev=None, sums=False, keep=False):
        """kmx_kquery_host: reads a list of sequences (str / bytes) or pack_reads() output; matrices[p] the body of partition p's
        .count / .pa (bytes or a uint8 array of whole rows: key words, then n_cols u32 counts or ceil(n_cols / 8) bytes) or None (the
        partition is not part of the call); n_rows None (from the bodies' sizes) or the rows per partition; hits_dev None or a device
        pointer to a uint32 table [queries, n_cols] the call adds to; sums False, True (the result owns the uint64 table) or a device
        pointer to a uint64 table the call adds to.
        -> KqueryOutput (numpy copies), or with keep the KqueryResult itself (the tables left in HBM; .free() it)"""
        stride = key_words * 8 + (4 * n_cols if mode == MODE_COUNT else (n_cols + 7) // 8)
        nr = (C.c_uint64 * len(matrices))()

        def fit(p, a):
            if n_rows is None and len(a) % stride:
                raise ValueError(f"partition {p}: {len(a)} bytes are not whole rows of {stride} bytes")
            nr[p] = len(a) // stride if n_rows is None else n_rows[p]
            return a if len(a) else np.zeros(1, np.uint8)      # (a partition of no rows is still part of the call)

        bases, offs, n_seqs, rep, rows, keepalive = self._seq_inputs(reads, repart, matrices, fit)
        want, sums_dev = self._kquery_sums(sums)
        t = KmxKqueryTask(bases, offs, n_seqs, k, m, rep, len(matrices), n_cols, key_words, mode, nr, rows, hits_dev, sums_dev, want)
        res = _vp()
        self._check(_lib.kmx_kquery_host(self._h, C.byref(t), C.byref(res)), "kmx_kquery_host")
        r = KqueryResult(self, res, n_cols, bool(want))
        r.wait()      # (the host buffers above may go once the call has run)
        return self._finish(r, keep)

    def kquery_dev(self, bases_dev, offsets_dev, n_seqs, k, m, repart_dev, n_cols, key_words, mode, rows_dev, n_rows, hits_dev=None, sums=False, keep=False):
        """kmx_kquery_dev: device pointers (a torch tensor's data_ptr()) to the bases, the uint64 offsets [n_seqs + 1] and the uint16
        repartition table; rows_dev[p] a device pointer to partition p's matrix body or None, n_rows[p] its rows.  -> as kquery"""
        rows = (C.c_void_p * len(rows_dev))(*rows_dev)
        nr = (C.c_uint64 * len(rows_dev))(*[int(x) for x in n_rows])
        want, sums_dev = self._kquery_sums(sums)
        t = KmxKqueryTask(bases_dev, offsets_dev, n_seqs, k, m, repart_dev, len(rows_dev), n_cols, key_words, mode, nr, rows, hits_dev, sums_dev, want)
        res = _vp()
        self._check(_lib.kmx_kquery_dev(self._h, C.byref(t), C.byref(res)), "kmx_kquery_dev")
        return self._finish(KqueryResult(self, res, n_cols, bool(want)), keep)

    def cquery(self, reads, k, m, repart, window, n_cols, matrices, bitw, min_class=1, hits_dev=None, sums_dev=None, keep=False):
        """kmx_cquery_host: reads a list of sequences (str / bytes) or pack_reads() output; matrices[p] the body of partition p's
        counting .cmbf (bytes or a uint8 array of window * ceil(n_cols * bitw / 8) bytes) or None (the partition is not part of the
        call); a hit is a class of at least min_class; hits_dev / sums_dev both None or device pointers to a uint32 and a uint64 table
        [queries, n_cols] the call adds to.
        -> CqueryOutput (numpy copies), or with keep the CqueryResult itself (the tables left in HBM; .free() it)"""
        fit = self._window_rows(window, (n_cols * bitw + 7) // 8, 1 <= bitw <= 8)      # (a bitw the library refuses is the library's to refuse)
        bases, offs, n_seqs, rep, rows, keepalive = self._seq_inputs(reads, repart, matrices, fit)
        t = KmxCqueryTask(bases, offs, n_seqs, k, m, rep, len(matrices), n_cols, window, rows, bitw, min_class, hits_dev, sums_dev)
        res = _vp()
        self._check(_lib.kmx_cquery_host(self._h, C.byref(t), C.byref(res)), "kmx_cquery_host")
        r = CqueryResult(self, res, n_cols)
        r.wait()      # (the host buffers above may go once the call has run)
        return self._finish(r, keep)

    def cquery_dev(self, bases_dev, offsets_dev, n_seqs, k, m, repart_dev, window, n_cols, rows_dev, bitw, min_class=1, hits_dev=None, sums_dev=None, keep=False):
        """kmx_cquery_dev: device pointers (a torch tensor's data_ptr()) to the bases, the uint64 offsets [n_seqs + 1] and the uint16
        repartition table; rows_dev[p] a device pointer to partition p's matrix body or None.  -> as cquery"""
        rows = (C.c_void_p * len(rows_dev))(*rows_dev)
        t = KmxCqueryTask(bases_dev, offsets_dev, n_seqs, k, m, repart_dev, len(rows_dev), n_cols, window, rows, bitw, min_class, hits_dev, sums_dev)
        res = _vp()
        self._check(_lib.kmx_cquery_dev(self._h, C.byref(t), C.byref(res)), "kmx_cquery_dev")
        return self._finish(CqueryResult(self, res, n_cols), keep)

    @staticmethod
    def _dist_mins(mins):
        return (1, None) if mins is True else (0, None) if mins is False or mins is None else (1, mins)

    def dist(self, body, n_rows, n_cols, key_words, mode, mins=False, inter_dev=None, mins_dev=None, keep=False):
        """kmx_dist_host: body the bytes (or a uint8 array) of n_rows whole rows of one partition's matrix (None: from the body's size):
        key words, then n_cols u32 counts (MODE_COUNT) or ceil(n_cols / 8) bytes (MODE_PA; MODE_BF with key_words 0).  mins: the
        min-count table is computed too (MODE_COUNT).  inter_dev / mins_dev: None (the result owns a zeroed table) or a device pointer
        to a uint64 table [n_cols, n_cols] the call adds to (mins_dev implies mins).
        -> DistOutput (numpy copies), or with keep the DistResult itself (the tables left in HBM; .free() it)"""
        a = np.frombuffer(body, dtype=np.uint8) if isinstance(body, (bytes, bytearray, memoryview)) else np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
        stride = key_words * 8 + (4 * n_cols if mode == MODE_COUNT else (n_cols + 7) // 8)
        if n_rows is None:
            if stride == 0 or len(a) % stride:
                raise ValueError(f"{len(a)} bytes are not whole rows of {stride} bytes")
            n_rows = len(a) // stride
        elif len(a) < n_rows * stride:
            raise ValueError(f"{len(a)} bytes are fewer than {n_rows} rows of {stride} bytes")
        want, md = self._dist_mins(mins_dev if mins_dev is not None else mins)
        t = KmxDistTask(key_words, mode, n_cols, want, a.ctypes.data if len(a) else None, n_rows, inter_dev, md)
        res = _vp()
        self._check(_lib.kmx_dist_host(self._h, C.byref(t), C.byref(res)), "kmx_dist_host")
        r = DistResult(self, res, n_cols, bool(want))
        r.wait()      # (the host buffer above may go once the call has run)
        if keep:
            return r
        try:
            return r.output()
        finally:
            r.free()

    def dist_dev(self, rows_dev, n_rows, n_cols, key_words, mode, mins=False, inter_dev=None, mins_dev=None, keep=False):
        """kmx_dist_dev: rows_dev a device pointer to n_rows rows (a torch tensor's data_ptr(), MergeResult.body_dev(), ...).  -> as dist"""
        want, md = self._dist_mins(mins_dev if mins_dev is not None else mins)
        t = KmxDistTask(key_words, mode, n_cols, want, rows_dev, n_rows, inter_dev, md)
        res = _vp()
        self._check(_lib.kmx_dist_dev(self._h, C.byref(t), C.byref(res)), "kmx_dist_dev")
        r = DistResult(self, res, n_cols, bool(want))
        if keep:
            return r
        try:
            return r.output()
        finally:
            r.free()

    @staticmethod
    def _whole_rows(body, n_rows, n_cols, key_words, mode):
        a = np.frombuffer(body, dtype=np.uint8) if isinstance(body, (bytes, bytearray, memoryview)) else np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
        stride = key_words * 8 + (4 * n_cols if mode == MODE_COUNT else (n_cols + 7) // 8)
        if n_rows is None:
            if stride == 0 or len(a) % stride:
                raise ValueError(f"{len(a)} bytes are not whole rows of {stride} bytes")
            n_rows = len(a) // stride
        elif len(a) < n_rows * stride:
            raise ValueError(f"{len(a)} bytes are fewer than {n_rows} rows of {stride} bytes")
        return a, n_rows

    def _finish(self, r, keep):
        if keep:
            return r
        try:
            return r.output()
        finally:
            r.free()

    def colsums(self, body, n_rows, n_cols, key_words, mode, sums_dev=None, keep=False):
        """kmx_colsums_host: body the bytes (or a uint8 array) of n_rows whole rows of one partition's matrix (None: from the body's
        size).  sums_dev: None (the result owns a zeroed table) or a device pointer to n_cols uint64 the call adds to.
        -> uint64[n_cols] (a numpy copy of the table as it stands), or with keep the ColsumsResult (.free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t = KmxColsumsTask(key_words, mode, n_cols, 0, a.ctypes.data if len(a) else None, n_rows, sums_dev)
        res = _vp()
        self._check(_lib.kmx_colsums_host(self._h, C.byref(t), C.byref(res)), "kmx_colsums_host")
        r = ColsumsResult(self, res, n_cols)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def colsums_dev(self, rows_dev, n_rows, n_cols, key_words, mode, sums_dev=None, keep=False):
        """kmx_colsums_dev: rows_dev a device pointer to n_rows rows.  -> as colsums"""
        t = KmxColsumsTask(key_words, mode, n_cols, 0, rows_dev, n_rows, sums_dev)
        res = _vp()
        self._check(_lib.kmx_colsums_dev(self._h, C.byref(t), C.byref(res)), "kmx_colsums_dev")
        return self._finish(ColsumsResult(self, res, n_cols), keep)

    @staticmethod
    def _diff_task(rows, n_rows, n_cols, key_words, mode, group, total_ctrl, total_case, threshold, min_rec):
        g = np.ascontiguousarray(group, dtype=np.uint8).reshape(-1)
        if len(g) != n_cols:
            raise ValueError(f"{len(g)} groups for {n_cols} columns")
        return KmxDiffTask(key_words, mode, n_cols, min_rec, rows, n_rows, g.ctypes.data, total_ctrl, total_case, threshold), g

    def diff(self, body, n_rows, n_cols, key_words, mode, group, total_ctrl, total_case, threshold, min_rec=0, keep=False):
        """kmx_diff_host: body as for colsums; group: n_cols values 0 (control), 1 (case), 2 (ignored); total_ctrl / total_case: the
        groups' totals over the whole run (sums of colsums); a row is kept when at least min_rec of its control and case columns are
        non-zero and its statistic is at least threshold.
        -> DiffOutput (numpy copies), or with keep the DiffResult itself (the kept rows and records left in HBM; .free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t, g = self._diff_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, group, total_ctrl, total_case, threshold, min_rec)
        res = _vp()
        self._check(_lib.kmx_diff_host(self._h, C.byref(t), C.byref(res)), "kmx_diff_host")
        r = DiffResult(self, res)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def diff_dev(self, rows_dev, n_rows, n_cols, key_words, mode, group, total_ctrl, total_case, threshold, min_rec=0, keep=False):
        """kmx_diff_dev: rows_dev a device pointer to n_rows rows (group stays a host array).  -> as diff"""
        t, g = self._diff_task(rows_dev, n_rows, n_cols, key_words, mode, group, total_ctrl, total_case, threshold, min_rec)
        res = _vp()
        self._check(_lib.kmx_diff_dev(self._h, C.byref(t), C.byref(res)), "kmx_diff_dev")
        return self._finish(DiffResult(self, res), keep)

    @staticmethod
    def _assoc_task(rows, n_rows, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, threshold, cols, min_abund, min_rec, max_rec):
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        n_use = n_cols if c is None else len(c)
        v = None
        n_vec = 0
        if vecs is not None:
            v = np.ascontiguousarray(vecs, dtype=np.int32)
            if v.ndim != 2 or v.shape[0] != n_use:
                raise ValueError(f"vecs of shape {v.shape} for {n_use} listed columns: expected (M, V)")
            n_vec = v.shape[1]
        t = KmxAssocTask(key_words, mode, n_cols, n_use, rows, n_rows, c.ctypes.data if c is not None and len(c) else None,
                         v.ctypes.data if v is not None and v.size else None, n_vec, frac_bits, min_abund, 0, gain, vmin, threshold, min_rec, max_rec)
        return t, (c, v)

    def assoc(self, body, n_rows, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, threshold, cols=None, min_abund=1, min_rec=0,
              max_rec=2**32 - 1, keep=False):
        """kmx_assoc_host: body as for diff; vecs: int32[M, V], row m the values of the V vectors for the m-th listed sample (vector 0
        the residual phenotype, 1 ... V - 1 an orthonormal basis of the covariates), in fixed point with frac_bits fraction bits; a row
        is kept when its recurrence over the listed columns lies in [min_rec, max_rec] and its statistic is at least threshold.
        -> AssocOutput (numpy copies), or with keep the AssocResult itself (the kept rows and records left in HBM; .free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t, hold = self._assoc_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, threshold, cols,
                                   min_abund, min_rec, max_rec)
        res = _vp()
        self._check(_lib.kmx_assoc_host(self._h, C.byref(t), C.byref(res)), "kmx_assoc_host")
        r = AssocResult(self, res)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def assoc_dev(self, rows_dev, n_rows, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, threshold, cols=None, min_abund=1, min_rec=0,
                  max_rec=2**32 - 1, keep=False):
        """kmx_assoc_dev: rows_dev a device pointer to n_rows rows (vecs and cols stay host arrays).  -> as assoc"""
        t, hold = self._assoc_task(rows_dev, n_rows, n_cols, key_words, mode, vecs, frac_bits, gain, vmin, threshold, cols, min_abund, min_rec, max_rec)
        res = _vp()
        self._check(_lib.kmx_assoc_dev(self._h, C.byref(t), C.byref(res)), "kmx_assoc_dev")
        return self._finish(AssocResult(self, res), keep)

    @staticmethod
    def _select_task(rows, n_rows, n_cols, key_words, mode, cols, out_mode, min_abund, min_rec, max_rec, zero_below):
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        n_out = n_cols if c is None else len(c)
        t = KmxSelectTask(key_words, mode, n_cols, n_out, rows, n_rows, c.ctypes.data if c is not None and len(c) else None, min_abund, min_rec,
                          0xFFFFFFFF if max_rec is None else max_rec, mode if out_mode is None else out_mode,
                          SELECT_ZERO_BELOW if zero_below else 0, 0)
        return t, c

    def select(self, body, n_rows, n_cols, key_words, mode, cols=None, out_mode=None, min_abund=1, min_rec=0, max_rec=None,
               zero_below=False, keep=False):
        """kmx_select_host: body as for colsums; cols: the input columns of the result in its order (None: all, as they stand); out_mode:
        MODE_COUNT or MODE_PA (None: the input's); a sample holds a row from min_abund upwards; a row is kept when min_rec <= the number
        of selected samples that hold it <= max_rec (None: no upper bound); zero_below: counts below min_abund leave as 0.
        -> SelectOutput (numpy copies), or with keep the SelectResult itself (the kept rows and records left in HBM; .free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t, c = self._select_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, cols, out_mode, min_abund, min_rec, max_rec, zero_below)
        res = _vp()
        self._check(_lib.kmx_select_host(self._h, C.byref(t), C.byref(res)), "kmx_select_host")
        r = SelectResult(self, res)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def select_dev(self, rows_dev, n_rows, n_cols, key_words, mode, cols=None, out_mode=None, min_abund=1, min_rec=0, max_rec=None,
                   zero_below=False, keep=False):
        """kmx_select_dev: rows_dev a device pointer to n_rows rows (cols stays a host array).  -> as select"""
        t, c = self._select_task(rows_dev, n_rows, n_cols, key_words, mode, cols, out_mode, min_abund, min_rec, max_rec, zero_below)
        res = _vp()
        self._check(_lib.kmx_select_dev(self._h, C.byref(t), C.byref(res)), "kmx_select_dev")
        return self._finish(SelectResult(self, res), keep)

    @staticmethod
    def _pan_task(rows, n_rows, n_cols, key_words, mode, cols, min_abund, shared, spectrum_dev, shared_dev):
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        n_use = n_cols if c is None else len(c)
        want = bool(shared) or shared_dev is not None
        t = KmxPanTask(key_words, mode, n_cols, n_use, rows, n_rows, c.ctypes.data if c is not None and len(c) else None, min_abund,
                       PAN_SHARED if want else 0, spectrum_dev, shared_dev)
        return t, c, n_use, want      # (c is kept alive by the caller until the call has copied it)

    def pan(self, body, n_rows, n_cols, key_words, mode, cols=None, min_abund=1, shared=False, spectrum_dev=None, shared_dev=None, keep=False):
        """kmx_pan_host: body as for select; cols: the input columns of the list in the order they are added (None: all, as they stand);
        shared: the per-sample table by recurrence is computed too; spectrum_dev / shared_dev: None (the result owns a zeroed table) or a
        device pointer to a uint64 table [3, M + 1] / [M + 1, n_cols] the call adds to (shared_dev implies shared).
        -> PanOutput (numpy copies), or with keep the PanResult itself (the tables left in HBM; .free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t, c, n_use, want = self._pan_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, cols, min_abund, shared, spectrum_dev, shared_dev)
        res = _vp()
        self._check(_lib.kmx_pan_host(self._h, C.byref(t), C.byref(res)), "kmx_pan_host")
        r = PanResult(self, res, n_cols, n_use, want)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def pan_dev(self, rows_dev, n_rows, n_cols, key_words, mode, cols=None, min_abund=1, shared=False, spectrum_dev=None, shared_dev=None, keep=False):
        """kmx_pan_dev: rows_dev a device pointer to n_rows rows (cols stays a host array).  -> as pan"""
        t, c, n_use, want = self._pan_task(rows_dev, n_rows, n_cols, key_words, mode, cols, min_abund, shared, spectrum_dev, shared_dev)
        res = _vp()
        self._check(_lib.kmx_pan_dev(self._h, C.byref(t), C.byref(res)), "kmx_pan_dev")
        return self._finish(PanResult(self, res, n_cols, n_use, want), keep)

    @staticmethod
    def _spectra_task(rows, n_rows, n_cols, key_words, mode, cols, cap, pairs, joint_cap, hist_dev, joint_dev, hist):
        want_h = bool(hist) or hist_dev is not None
        want_j = pairs is not None or joint_dev is not None
        c = None if cols is None or not want_h else np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        n_use = 0 if not want_h else n_cols if c is None else len(c)
        p = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1)
        n_pairs = 0 if p is None else len(p) // 2
        t = KmxSpectraTask(key_words, mode, n_cols, n_use, rows, n_rows, c.ctypes.data if c is not None and len(c) else None,
                           p.ctypes.data if p is not None and len(p) else None, n_pairs, cap if want_h else 0, joint_cap if want_j else 0,
                           (SPECTRA_HIST if want_h else 0) | (SPECTRA_JOINT if want_j else 0), hist_dev, joint_dev)
        shape = (n_use, cap, n_pairs, joint_cap, want_h, want_j)
        return t, (c, p), shape      # (the arrays are kept alive by the caller until the call has copied them)

    def spectra(self, body, n_rows, n_cols, key_words, mode, cols=None, cap=255, pairs=None, joint_cap=63, hist_dev=None, joint_dev=None,
                keep=False, hist=True):
        """kmx_spectra_host: body as for pan.  The abundance spectra (unless hist is False) of the input columns cols (None: all, as they
        stand), counts of cap and more in the last bin; the joint spectra of pairs, a sequence of (x, y) input columns, counts capped at
        joint_cap (None: no joint spectra).  hist_dev / joint_dev: None (the result owns a zeroed table) or a device pointer to a
        uint64 table [M, cap + 2] / [P, joint_cap + 1, joint_cap + 1] the call adds to.
        -> SpectraOutput (numpy copies), or with keep the SpectraResult itself (the tables left in HBM; .free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t, hold, shape = self._spectra_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, cols, cap, pairs, joint_cap, hist_dev, joint_dev, hist)
        res = _vp()
        self._check(_lib.kmx_spectra_host(self._h, C.byref(t), C.byref(res)), "kmx_spectra_host")
        r = SpectraResult(self, res, *shape)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def spectra_dev(self, rows_dev, n_rows, n_cols, key_words, mode, cols=None, cap=255, pairs=None, joint_cap=63, hist_dev=None, joint_dev=None,
                    keep=False, hist=True):
        """kmx_spectra_dev: rows_dev a device pointer to n_rows rows (cols and pairs stay host arrays).  -> as spectra"""
        t, hold, shape = self._spectra_task(rows_dev, n_rows, n_cols, key_words, mode, cols, cap, pairs, joint_cap, hist_dev, joint_dev, hist)
        res = _vp()
        self._check(_lib.kmx_spectra_dev(self._h, C.byref(t), C.byref(res)), "kmx_spectra_dev")
        return self._finish(SpectraResult(self, res, *shape), keep)

    @staticmethod
    def _colors_task(rows, n_rows, n_cols, key_words, mode, cols, min_abund):
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        n_use = n_cols if c is None else len(c)
        t = KmxColorsTask(key_words, mode, n_cols, n_use, rows, n_rows, c.ctypes.data if c is not None and len(c) else None, min_abund, 0)
        return t, c, n_use      # (c is kept alive by the caller until the call has copied it)

    def colors(self, body, n_rows, n_cols, key_words, mode, cols=None, min_abund=1, keep=False):
        """kmx_colors_host: body as for pan; cols: the input columns of the list in the caller's order (None: all, as they stand); a
        sample holds a row from min_abund upwards.
        -> ColorsOutput (numpy copies), or with keep the ColorsResult itself (ids and the class table left in HBM; .free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t, c, n_use = self._colors_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, cols, min_abund)
        res = _vp()
        self._check(_lib.kmx_colors_host(self._h, C.byref(t), C.byref(res)), "kmx_colors_host")
        r = ColorsResult(self, res, n_rows, n_use)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def colors_dev(self, rows_dev, n_rows, n_cols, key_words, mode, cols=None, min_abund=1, keep=False):
        """kmx_colors_dev: rows_dev a device pointer to n_rows rows (cols stays a host array).  -> as colors"""
        t, c, n_use = self._colors_task(rows_dev, n_rows, n_cols, key_words, mode, cols, min_abund)
        res = _vp()
        self._check(_lib.kmx_colors_dev(self._h, C.byref(t), C.byref(res)), "kmx_colors_dev")
        return self._finish(ColorsResult(self, res, n_rows, n_use), keep)

    def unitigs(self, keys, kmer_size, keep=False):
        """kmx_unitigs_host: keys uint64[n, ceil(kmer_size / 32)] (low word first), n distinct canonical k-mers in any order.
        -> UnitigsOutput (numpy copies), or with keep the UnitigsResult itself (the arrays left in HBM; .free() it)"""
        kw = key_words_of(kmer_size)
        a = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, kw)
        t = KmxUnitigsTask(a.ctypes.data if len(a) else None, len(a), kmer_size, kw, 0, 0)
        res = _vp()
        self._check(_lib.kmx_unitigs_host(self._h, C.byref(t), C.byref(res)), "kmx_unitigs_host")
        r = UnitigsResult(self, res, len(a), kmer_size)
        try:
            r.wait()      # (the host buffer above may go once the call has run)
        except KmxError:      # a data error found on the device: nothing of the result is of use
            r.free()
            raise
        return self._finish(r, keep)

    def unitigs_dev(self, keys_dev, n, kmer_size, keep=False):
        """kmx_unitigs_dev: keys_dev a device pointer to n keys.  -> as unitigs"""
        t = KmxUnitigsTask(keys_dev, n, kmer_size, key_words_of(kmer_size), 0, 0)
        res = _vp()
        self._check(_lib.kmx_unitigs_dev(self._h, C.byref(t), C.byref(res)), "kmx_unitigs_dev")
        return self._finish(UnitigsResult(self, res, n, kmer_size), keep)

    def kset(self, keys_words, k):
        """kmx_kset_host: keys_words uint64[n, ceil(k / 32)] (low word first), canonical k-mers in any order, duplicates allowed.
        -> Kset (the set stays in HBM for match(); .free() it)"""
        kw = key_words_of(k)
        a = np.ascontiguousarray(keys_words, dtype=np.uint64).reshape(-1, kw)
        t = KmxKsetTask(a.ctypes.data if len(a) else None, len(a), k, kw, 0, 0)
        h = _vp()
        self._check(_lib.kmx_kset_host(self._h, C.byref(t), C.byref(h)), "kmx_kset_host")
        s = Kset(self, h)
        try:
            s.wait()      # (the host buffer above may go once the build has run)
        except KmxError:      # a data error found on the device: the set is of no use
            s.free()
            raise
        return s

    def kset_dev(self, keys_dev, n, k):
        """kmx_kset_dev: keys_dev a device pointer to n keys.  -> Kset (a data error shows at .wait() and at every use)"""
        t = KmxKsetTask(keys_dev, n, k, key_words_of(k), 0, 0)
        h = _vp()
        self._check(_lib.kmx_kset_dev(self._h, C.byref(t), C.byref(h)), "kmx_kset_dev")
        return Kset(self, h)

    def match(self, kset, reads, ids=False, occ=False, occ_dev=None, keep=False):
        """kmx_match_host: reads a list of sequences (str / bytes) or pack_reads() output, against a Kset.  ids: the id per base of the
        call; occ: the occurrences per key -- occ_dev None (the result owns a zeroed table) or a device pointer to n uint64 the call
        adds to.  -> MatchOutput (numpy copies), or with keep the MatchResult itself (the tables left in HBM; .free() it)"""
        blob, offs = reads if isinstance(reads, tuple) else self.pack_reads(reads)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        bb = np.frombuffer(blob, dtype=np.uint8) if len(blob) else np.zeros(1, np.uint8)
        flags = (MATCH_IDS if ids else 0) | (MATCH_OCC if occ or occ_dev is not None else 0)
        t = KmxMatchTask(kset._h, bb.ctypes.data, offs.ctypes.data, len(offs) - 1, flags, 0, occ_dev, 0)
        res = _vp()
        self._check(_lib.kmx_match_host(self._h, C.byref(t), C.byref(res)), "kmx_match_host")
        r = MatchResult(self, res, kset.n, flags)
        r.wait()      # (the host buffers above may go once the call has run)
        return self._finish(r, keep)

    def match_dev(self, kset, bases_dev, offsets_dev, n_seqs, ids=False, occ=False, occ_dev=None, keep=False):
        """kmx_match_dev: device pointers to the bases and the uint64 offsets [n_seqs + 1].  -> as match"""
        flags = (MATCH_IDS if ids else 0) | (MATCH_OCC if occ or occ_dev is not None else 0)
        t = KmxMatchTask(kset._h, bases_dev, offsets_dev, n_seqs, flags, 0, occ_dev, 0)
        res = _vp()
        self._check(_lib.kmx_match_dev(self._h, C.byref(t), C.byref(res)), "kmx_match_dev")
        return self._finish(MatchResult(self, res, kset.n, flags), keep)

    @staticmethod
    def _groupsum_task(rows, n_rows, n_cols, key_words, mode, groups, g0, n_groups, cols, min_abund, sums, present_dev, sums_dev, size_dev):
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        n_use = n_cols if c is None else len(c)
        want = bool(sums) or sums_dev is not None
        t = KmxGroupsumTask(key_words, mode, n_cols, n_use, rows, n_rows, c.ctypes.data if c is not None and len(c) else None, groups, min_abund,
                            GROUPSUM_SUMS if want else 0, g0, n_groups, present_dev, sums_dev, size_dev)
        return t, c, n_use, want      # (c is kept alive by the caller until the call has copied it)

    def groupsum(self, body, n_rows, n_cols, key_words, mode, groups, g0, n_groups, cols=None, min_abund=1, sums=False, present_dev=None,
                 sums_dev=None, size_dev=None, keep=False):
        """kmx_groupsum_host: body as for pan; groups uint32[n_rows]: a label per row; the window [g0, g0 + n_groups); sums: the counts'
        sums are wanted too (COUNT); present_dev / sums_dev / size_dev: None (the result owns a zeroed table) or a device pointer to a
        uint32 [G, M] / uint64 [G, M] / uint32 [G] table the call adds to.
        -> GroupsumOutput (numpy copies), or with keep the GroupsumResult itself (.free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        if len(g) != n_rows:
            raise ValueError(f"{len(g)} labels for {n_rows} rows")
        t, c, n_use, want = self._groupsum_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, g.ctypes.data if len(g) else None,
                                                g0, n_groups, cols, min_abund, sums, present_dev, sums_dev, size_dev)
        res = _vp()
        self._check(_lib.kmx_groupsum_host(self._h, C.byref(t), C.byref(res)), "kmx_groupsum_host")
        r = GroupsumResult(self, res, n_groups, n_use, want)
        r.wait()      # (the host buffers above may go once the call has run)
        return self._finish(r, keep)

    def groupsum_dev(self, rows_dev, n_rows, n_cols, key_words, mode, groups_dev, g0, n_groups, cols=None, min_abund=1, sums=False,
                     present_dev=None, sums_dev=None, size_dev=None, keep=False):
        """kmx_groupsum_dev: rows_dev and groups_dev device pointers (cols stays a host array).  -> as groupsum"""
        t, c, n_use, want = self._groupsum_task(rows_dev, n_rows, n_cols, key_words, mode, groups_dev, g0, n_groups, cols, min_abund, sums,
                                                present_dev, sums_dev, size_dev)
        res = _vp()
        self._check(_lib.kmx_groupsum_dev(self._h, C.byref(t), C.byref(res)), "kmx_groupsum_dev")
        return self._finish(GroupsumResult(self, res, n_groups, n_use, want), keep)

    @staticmethod
    def _gram_task(rows, n_rows, n_cols, key_words, mode, weights, cols, min_abund, table_dev):
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        n_use = n_cols if c is None else len(c)
        w = np.ascontiguousarray(weights, dtype=np.uint32).reshape(-1)
        if len(w) != n_use + 1:
            raise ValueError(f"{len(w)} class weights for {n_use} listed columns: M + 1 are needed")
        t = KmxGramTask(key_words, mode, n_cols, n_use, rows, n_rows, c.ctypes.data if c is not None and len(c) else None, w.ctypes.data,
                        min_abund, 0, table_dev)
        return t, (c, w)      # (the arrays are kept alive by the caller until the call has copied them)

    def gram(self, body, n_rows, n_cols, key_words, mode, weights, cols=None, min_abund=1, table_dev=None, keep=False):
        """kmx_gram_host: body as for pan; weights: M + 1 uint32, the weight of a row by the number of listed samples that hold it; cols:
        the listed input columns (None: all); table_dev: None (the result owns a zeroed table) or a device pointer to a uint64 table
        [n_cols, n_cols] the call adds to.
        -> GramOutput (numpy copies), or with keep the GramResult itself (the table left in HBM; .free() it)"""
        a, n_rows = self._whole_rows(body, n_rows, n_cols, key_words, mode)
        t, alive = self._gram_task(a.ctypes.data if len(a) else None, n_rows, n_cols, key_words, mode, weights, cols, min_abund, table_dev)
        res = _vp()
        self._check(_lib.kmx_gram_host(self._h, C.byref(t), C.byref(res)), "kmx_gram_host")
        r = GramResult(self, res, n_cols)
        r.wait()      # (the host buffer above may go once the call has run)
        return self._finish(r, keep)

    def gram_dev(self, rows_dev, n_rows, n_cols, key_words, mode, weights, cols=None, min_abund=1, table_dev=None, keep=False):
        """kmx_gram_dev: rows_dev a device pointer to n_rows rows (weights and cols stay host arrays).  -> as gram"""
        t, alive = self._gram_task(rows_dev, n_rows, n_cols, key_words, mode, weights, cols, min_abund, table_dev)
        res = _vp()
        self._check(_lib.kmx_gram_dev(self._h, C.byref(t), C.byref(res)), "kmx_gram_dev")
        return self._finish(GramResult(self, res, n_cols), keep)

    @staticmethod
    def _block_row_bytes(key_words, mode, n_cols, count_bytes):
        return key_words * 8 + (n_cols * count_bytes if mode == MODE_COUNT else (n_cols + 7) // 8)

    def combine(self, blocks, key_words, mode, drop_last=False):
        """kmx_combine_host: blocks = [(body, n_cols[, count_bytes])] in column order, body the bytes (or a uint8 array) of whole rows:
        key words, then n_cols counts of count_bytes (1, 2 or 4; 4 when left out) bytes or ceil(n_cols / 8) presence/absence bytes.
        -> CombineOutput (rows, row_bytes, body, kernel_ms, algo_bytes)"""
        keep, arr = [], (KmxBlock * max(len(blocks), 1))()
        for i, b in enumerate(blocks):
            body, n_cols, cb = b[0], b[1], (b[2] if len(b) > 2 else 4)
            a = np.frombuffer(body, dtype=np.uint8) if isinstance(body, (bytes, bytearray, memoryview)) else np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
            irb = self._block_row_bytes(key_words, mode, n_cols, cb)
            if len(a) % irb:
                raise ValueError(f"block {i}: {len(a)} bytes are not whole rows of {irb} bytes")
            keep.append(a)
            arr[i] = KmxBlock(a.ctypes.data if len(a) else None, len(a) // irb, n_cols, cb)
        t = KmxCombineTask(key_words, mode, len(blocks), COMBINE_DROP_LAST if drop_last else 0, arr, None)
        res = _vp()
        self._check(_lib.kmx_combine_host(self._h, C.byref(t), C.byref(res)), "kmx_combine_host")
        r = CombineResult(self, res)
        try:
            return r.output()
        finally:
            r.free()

    def combine_dev(self, blocks, key_words, mode, drop_last=False, keep=False):
        """kmx_combine_dev: blocks = [(device pointer, n_rows, n_cols[, count_bytes])] in column order -- a torch tensor's data_ptr(),
        MergeResult.body_dev(), FilterResult.body_dev(), CombineResult.body_dev().
        -> CombineOutput (numpy copy of the body), or with keep the CombineResult itself (the body left in HBM; .free() it)"""
        arr = (KmxBlock * max(len(blocks), 1))()
        for i, b in enumerate(blocks):
            arr[i] = KmxBlock(b[0], b[1], b[2], b[3] if len(b) > 3 else 4)
        t = KmxCombineTask(key_words, mode, len(blocks), COMBINE_DROP_LAST if drop_last else 0, arr, None)
        res = _vp()
        self._check(_lib.kmx_combine_dev(self._h, C.byref(t), C.byref(res)), "kmx_combine_dev")
        r = CombineResult(self, res)
        if keep:
            return r
        try:
            return r.output()
        finally:
            r.free()


class CombineOutput:
    """body: the bytes of `rows` rows of `row_bytes`; kernel_ms < 0 without set_profiling; algo_bytes: every input row read once plus
    every output row written once"""

    def __init__(self, body, rows, row_bytes, kernel_ms, algo_bytes):
        self.body, self.rows, self.row_bytes, self.kernel_ms, self.algo_bytes = body, rows, row_bytes, kernel_ms, algo_bytes


class QueryOutput:
    """n_kmers uint32[queries]: positions with a valid k-mer; hits uint32[queries, n_cols]: those whose row has the sample's bit set
    (the table the call added to, when one was given); kernel_ms < 0 without set_profiling"""

    def __init__(self, n_kmers, hits, kernel_ms, algo_bytes):
        self.n_kmers, self.hits, self.kernel_ms, self.algo_bytes = n_kmers, hits, kernel_ms, algo_bytes


class _Result:
    """what the result wrappers of the matrix tools and of the sequence queries share: the calls kmx_<_prefix>_result_<name> of libkmx"""
    _prefix = None

    def __init__(self, ctx, h):
        self._ctx, self._h = ctx, h

    def _call(self, name, *args, check=False):
        full = f"kmx_{self._prefix}_result_{name}"
        rc = getattr(_lib, full)(self._h, *args)
        if check:
            self._ctx._check(rc, full)
        return rc

    def wait(self):
        self._call("wait", check=True)

    def kernel_ms(self):
        return self._call("kernel_ms")

    def _kernel_parts_ms(self, n):
        p = [C.c_double(-1) for _ in range(n)]
        self._call("kernel_parts_ms", *[C.byref(x) for x in p], check=True)
        return tuple(x.value for x in p)

    def algo_bytes(self):
        return self._call("algo_bytes")

    def _copy(self, name, array):
        """the result's table `name` into array (kmx_..._result_copy_<name>) -> array"""
        self._call("copy_" + name, array.ctypes.data, array.size, check=True)
        return array

    def free(self):
        if self._h:
            self._call("free")
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _RowsResult(_Result):
    """a result of kept rows and one record a kept row (diff, assoc, select): _rec the records' dtype, _output the *Output class"""
    _rec = _output = None

    def rows(self):
        return self._call("rows")

    def row_bytes(self):
        return self._call("row_bytes")

    def body_bytes(self):
        return self._call("body_bytes")

    def body_dev(self):
        return self._call("body_dev")

    def recs_dev(self):
        return self._call("recs_dev")

    def output(self):
        self.wait()
        body = self._copy("body", np.zeros(self.body_bytes(), np.uint8))
        recs = self._copy("recs", np.zeros(self.rows(), self._rec))
        return self._output(body.tobytes(), recs, self.kernel_ms(), self.algo_bytes())


class DistOutput:
    """inter uint64[n_cols, n_cols]: rows that hold both samples (the table the call added to, when one was given); mins
    uint64[n_cols, n_cols] (None unless asked for): the sums of the smaller count; kernel_ms < 0 without set_profiling"""

    def __init__(self, inter, mins, kernel_ms, algo_bytes):
        self.inter, self.mins, self.kernel_ms, self.algo_bytes = inter, mins, kernel_ms, algo_bytes

class DistResult(_Result):
    _prefix = "dist"

    def __init__(self, ctx, h, n_cols, has_mins):
        super().__init__(ctx, h)
        self._n, self._mins = n_cols, has_mins

    def inter_dev(self):
        return self._call("inter_dev")

    def mins_dev(self):
        return self._call("mins_dev")

    def kernel_parts_ms(self):
        """(clearing + k_dist_slab, k_dist_pairs, k_dist_mins) in ms; -1 where unavailable"""
        return self._kernel_parts_ms(3)

    def output(self):
        self.wait()
        inter = self._copy("inter", np.zeros((self._n, self._n), np.uint64))
        mins = self._copy("mins", np.zeros((self._n, self._n), np.uint64)) if self._mins else None
        return DistOutput(inter, mins, self.kernel_ms(), self.algo_bytes())


class ColsumsResult(_Result):
    _prefix = "colsums"

    def __init__(self, ctx, h, n_cols):
        super().__init__(ctx, h)
        self._n = n_cols

    def sums_dev(self):
        return self._call("sums_dev")

    def output(self):
        self.wait()
        return self._copy("sums", np.zeros(self._n, np.uint64))


class DiffOutput:
    """body: the kept rows, whole and in the input's order (bytes); recs: one DIFF_REC (kmx_diff_rec, 40 bytes) per kept row in the
    same order, a numpy structured array; kernel_ms < 0 without set_profiling"""

    def __init__(self, body, recs, kernel_ms, algo_bytes):
        self.body, self.recs, self.kernel_ms, self.algo_bytes = body, recs, kernel_ms, algo_bytes

class DiffResult(_RowsResult):
    _prefix, _rec, _output = "diff", DIFF_REC, DiffOutput


class AssocOutput:
    """body: the kept rows, whole and in the input's order (bytes); recs: one ASSOC_REC (kmx_assoc_rec, 32 bytes) per kept row in the
    same order, a numpy structured array; kernel_ms < 0 without set_profiling"""

    def __init__(self, body, recs, kernel_ms, algo_bytes):
        self.body, self.recs, self.kernel_ms, self.algo_bytes = body, recs, kernel_ms, algo_bytes

class AssocResult(_RowsResult):
    _prefix, _rec, _output = "assoc", ASSOC_REC, AssocOutput


class PanOutput:
    """spectrum uint64[3, M + 1]: rows by recurrence, by first ordinal, by first missing ordinal (the table the call added to, when one
    was given); shared uint64[M + 1, n_cols] (None unless asked for): rows of recurrence r that input column c holds; kernel_ms < 0
    without set_profiling"""

    def __init__(self, spectrum, shared, kernel_ms, algo_bytes):
        self.spectrum, self.shared, self.kernel_ms, self.algo_bytes = spectrum, shared, kernel_ms, algo_bytes

class PanResult(_Result):
    _prefix = "pan"

    def __init__(self, ctx, h, n_cols, n_use, has_shared):
        super().__init__(ctx, h)
        self._n, self._m, self._shared = n_cols, n_use, has_shared

    def spectrum_dev(self):
        return self._call("spectrum_dev")

    def shared_dev(self):
        return self._call("shared_dev")

    def kernel_parts_ms(self):
        """(clearing + k_pan_score + k_pan_fold, k_pan_order, k_pan_shared) in ms; -1 where unavailable"""
        return self._kernel_parts_ms(3)

    def output(self):
        self.wait()
        spectrum = self._copy("spectrum", np.zeros((3, self._m + 1), np.uint64))
        shared = self._copy("shared", np.zeros((self._m + 1, self._n), np.uint64)) if self._shared else None
        return PanOutput(spectrum, shared, self.kernel_ms(), self.algo_bytes())


class SpectraOutput:
    """hist uint64[M, cap + 2] (None unless asked for): per listed sample the rows by count, counts of cap and more in bin cap, the
    volume of that bin last; joint uint64[P, joint_cap + 1, joint_cap + 1] (None unless asked for): per pair the rows by the two capped
    counts -- the tables the call added to, when they were given; kernel_ms < 0 without set_profiling"""

    def __init__(self, hist, joint, kernel_ms, algo_bytes):
        self.hist, self.joint, self.kernel_ms, self.algo_bytes = hist, joint, kernel_ms, algo_bytes

class SpectraResult(_Result):
    _prefix = "spectra"

    def __init__(self, ctx, h, n_use, cap, n_pairs, joint_cap, has_hist, has_joint):
        super().__init__(ctx, h)
        self._m, self._c1, self._p, self._c2, self._hist, self._joint = n_use, cap, n_pairs, joint_cap, has_hist, has_joint

    def hist_dev(self):
        return self._call("hist_dev")

    def joint_dev(self):
        return self._call("joint_dev")

    def kernel_parts_ms(self):
        """(clearing + the HIST kernel, the JOINT kernel) in ms; -1 where unavailable"""
        return self._kernel_parts_ms(2)

    def output(self):
        self.wait()
        hist = self._copy("hist", np.zeros((self._m, self._c1 + 2), np.uint64)) if self._hist else None
        joint = self._copy("joint", np.zeros((self._p, self._c2 + 1, self._c2 + 1), np.uint64)) if self._joint else None
        return SpectraOutput(hist, joint, self.kernel_ms(), self.algo_bytes())


class GramOutput:
    """table uint64[n_cols, n_cols]: the class weights summed over the rows that hold both samples (the table the call added to, when
    one was given); kernel_ms < 0 without set_profiling"""

    def __init__(self, table, kernel_ms, algo_bytes):
        self.table, self.kernel_ms, self.algo_bytes = table, kernel_ms, algo_bytes

class GramResult(_Result):
    _prefix = "gram"

    def __init__(self, ctx, h, n_cols):
        super().__init__(ctx, h)
        self._n = n_cols

    def table_dev(self):
        return self._call("table_dev")

    def kernel_parts_ms(self):
        """(clearing + k_gram_score + k_gram_fold, k_gram_order, k_gram_slab, k_gram_pairs) in ms; -1 where unavailable"""
        return self._kernel_parts_ms(4)

    def output(self):
        self.wait()
        return GramOutput(self._copy("table", np.zeros((self._n, self._n), np.uint64)), self.kernel_ms(), self.algo_bytes())


class ColorsOutput:
    """n_classes C; ids uint32[n_rows]: the class of every row; first uint32[C]: a class's first row; sizes uint32[C]: its rows;
    patterns uint64[C, W]: ordinal j of the list = bit j & 63 of word j >> 6; kernel_ms < 0 without set_profiling"""

    def __init__(self, n_classes, ids, first, sizes, patterns, kernel_ms, algo_bytes):
        self.n_classes, self.ids, self.first, self.sizes, self.patterns = n_classes, ids, first, sizes, patterns
        self.kernel_ms, self.algo_bytes = kernel_ms, algo_bytes

class ColorsResult(_Result):
    _prefix = "colors"

    def __init__(self, ctx, h, n_rows, n_use):
        super().__init__(ctx, h)
        self._rows, self._w = n_rows, (n_use + 63) // 64

    def n_classes(self):
        return self._call("n_classes")

    def ids_dev(self):
        return self._call("ids_dev")

    def kernel_parts_ms(self):
        """(k_col_pack, clearing + k_col_claim, the numbering kernels) in ms; -1 where unavailable"""
        return self._kernel_parts_ms(3)

    def output(self):
        self.wait()
        n = self.n_classes()
        ids = self._copy("ids", np.zeros(self._rows, np.uint32))
        first, sizes = self._copy("first", np.zeros(n, np.uint32)), self._copy("sizes", np.zeros(n, np.uint32))
        patterns = self._copy("patterns", np.zeros((n, self._w), np.uint64))
        return ColorsOutput(n, ids, first, sizes, patterns, self.kernel_ms(), self.algo_bytes())


class UnitigsOutput:
    """n_unitigs U; unitig / pos uint32[n], ori uint8[n]: every k-mer's unitig, position and strand; start / len uint32[U], circ uint8[U];
    seq_off uint64[U + 1]; seqs: the U sequences (bytes each); kernel_ms < 0 without set_profiling"""

    def __init__(self, n_unitigs, unitig, pos, ori, start, length, circ, seq_off, seqs, kernel_ms, algo_bytes):
        self.n_unitigs, self.unitig, self.pos, self.ori, self.start, self.len, self.circ = n_unitigs, unitig, pos, ori, start, length, circ
        self.seq_off, self.seqs, self.kernel_ms, self.algo_bytes = seq_off, seqs, kernel_ms, algo_bytes

class UnitigsResult(_Result):
    _prefix = "unitigs"

    def __init__(self, ctx, h, n, kmer_size):
        super().__init__(ctx, h)
        self._n, self._k = n, kmer_size

    def n_unitigs(self):
        return self._call("n_unitigs")

    def unitig_dev(self):
        return self._call("unitig_dev")

    def seq_bytes(self):
        return self._call("seq_bytes")

    def kernel_parts_ms(self):
        """(clearing + k_ug_table, k_ug_cand + k_ug_link, the rounds of k_ug_jump, the finish) in ms; -1 where unavailable"""
        return self._kernel_parts_ms(4)

    def output(self):
        self.wait()
        n, U = self._n, self.n_unitigs()
        unitig, pos, ori = self._copy("unitig", np.zeros(n, np.uint32)), self._copy("pos", np.zeros(n, np.uint32)), self._copy("ori", np.zeros(n, np.uint8))
        start, length, circ = self._copy("start", np.zeros(U, np.uint32)), self._copy("len", np.zeros(U, np.uint32)), self._copy("circ", np.zeros(U, np.uint8))
        seq_off = self._copy("seq_off", np.zeros(U + 1, np.uint64))
        flat = self._copy("seqs", np.zeros(self.seq_bytes(), np.uint8)).tobytes()
        seqs = [flat[int(seq_off[u]):int(seq_off[u + 1])] for u in range(U)]
        return UnitigsOutput(U, unitig, pos, ori, start, length, circ, seq_off, seqs, self.kernel_ms(), self.algo_bytes())


class Kset:
    """a set of k-mers resident on the device (kmx_kset_*): n keys as given, n_distinct ids; ids() uint32[n]: for every input index the
    least index of its key; kernel_ms < 0 without set_profiling"""

    def __init__(self, ctx, h):
        self._ctx, self._h = ctx, h
        self._n = None

    def wait(self):
        self._ctx._check(_lib.kmx_kset_wait(self._h), "kmx_kset_wait")

    @property
    def n(self):
        if self._n is None:
            self.wait()
            self._n = _lib.kmx_kset_n(self._h)
        return self._n

    @property
    def n_distinct(self):
        self.wait()
        return _lib.kmx_kset_n_distinct(self._h)

    @property
    def kmer_size(self):
        self.wait()
        return _lib.kmx_kset_kmer_size(self._h)

    @property
    def kernel_ms(self):
        return _lib.kmx_kset_kernel_ms(self._h)

    def ids(self):
        a = np.zeros(self.n, np.uint32)
        self._ctx._check(_lib.kmx_kset_copy_ids(self._h, a.ctypes.data, a.size), "kmx_kset_copy_ids")
        return a

    def free(self):
        if self._h:
            _lib.kmx_kset_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MatchOutput:
    """recs: a structured array (MATCH_REC: n_kmers, hits, fwd, covered, first, last), one record a read; ids uint32[n_bases] or None; occ
    uint64[n] (the table as it stands) or None; total_kmers, total_hits; kernel_ms < 0 without set_profiling"""

    def __init__(self, recs, ids, occ, total_kmers, total_hits, kernel_ms, algo_bytes):
        self.recs, self.ids, self.occ, self.total_kmers, self.total_hits = recs, ids, occ, total_kmers, total_hits
        self.kernel_ms, self.algo_bytes = kernel_ms, algo_bytes


class MatchResult(_Result):
    _prefix = "match"

    def __init__(self, ctx, h, n_keys, flags):
        super().__init__(ctx, h)
        self._n, self._flags = n_keys, flags

    def occ_dev(self):
        return self._call("occ_dev")

    def kernel_parts_ms(self):
        """(the clears + k_mt_probe, k_mt_cover + k_mt_last) in ms; -1 where unavailable"""
        return self._kernel_parts_ms(2)

    def output(self):
        self.wait()
        recs = self._copy("recs", np.zeros(self._call("n_seqs"), MATCH_REC))
        ids = self._copy("ids", np.zeros(self._call("n_bases"), np.uint32)) if self._flags & MATCH_IDS else None
        occ = self._copy("occ", np.zeros(self._n, np.uint64)) if self._flags & MATCH_OCC else None
        return MatchOutput(recs, ids, occ, self._call("total_kmers"), self._call("total_hits"), self.kernel_ms(), self.algo_bytes())


class GroupsumOutput:
    """size uint32[G]: the rows of every group of the window; present uint32[G, M]: those that hold the listed sample; sums uint64[G, M]
    (None unless asked for): the sums of their counts -- the tables the call added to, when they were given; kernel_ms < 0 without set_profiling"""

    def __init__(self, size, present, sums, kernel_ms, algo_bytes):
        self.size, self.present, self.sums, self.kernel_ms, self.algo_bytes = size, present, sums, kernel_ms, algo_bytes

class GroupsumResult(_Result):
    _prefix = "groupsum"

    def __init__(self, ctx, h, n_groups, n_use, has_sums):
        super().__init__(ctx, h)
        self._g, self._m, self._sums = n_groups, n_use, has_sums

    def present_dev(self):
        return self._call("present_dev")

    def sums_dev(self):
        return self._call("sums_dev")

    def size_dev(self):
        return self._call("size_dev")

    def output(self):
        self.wait()
        size = self._copy("size", np.zeros(self._g, np.uint32))
        present = self._copy("present", np.zeros((self._g, self._m), np.uint32))
        sums = self._copy("sums", np.zeros((self._g, self._m), np.uint64)) if self._sums else None
        return GroupsumOutput(size, present, sums, self.kernel_ms(), self.algo_bytes())


class SelectOutput:
    """body: the kept rows at their new size, in the input's order (bytes); recs: one SELECT_REC (kmx_select_rec, 8 bytes) per kept row
    in the same order, a numpy structured array; kernel_ms < 0 without set_profiling"""

    def __init__(self, body, recs, kernel_ms, algo_bytes):
        self.body, self.recs, self.kernel_ms, self.algo_bytes = body, recs, kernel_ms, algo_bytes

class SelectResult(_RowsResult):
    _prefix, _rec, _output = "select", SELECT_REC, SelectOutput


class KqueryOutput:
    """n_kmers uint32[queries]: positions with a valid k-mer; hits uint32[queries, n_cols]: those whose k-mer is a row's key with a
    non-zero count / a set bit in the column; sums uint64[queries, n_cols] (None unless asked for): those rows' counts added up;
    kernel_ms < 0 without set_profiling"""

    def __init__(self, n_kmers, hits, sums, kernel_ms, algo_bytes):
        self.n_kmers, self.hits, self.sums, self.kernel_ms, self.algo_bytes = n_kmers, hits, sums, kernel_ms, algo_bytes


class _SeqResult(_Result):
    """what the results of the four sequence-query families add: the queries, their hits, their tables as numpy copies"""

    def __init__(self, ctx, h, n_cols):
        super().__init__(ctx, h)
        self._n = n_cols

    def n_seqs(self):
        return self._call("n_seqs")

    def hits_dev(self):
        return self._call("hits_dev")

    def _tables(self, sums=False):
        """-> n_kmers uint32[queries], hits uint32[queries, n_cols], sums uint64[queries, n_cols] or None: numpy copies"""
        self.wait()
        q = self.n_seqs()
        return (self._copy("kmers", np.zeros(q, np.uint32)), self._copy("hits", np.zeros((q, self._n), np.uint32)),
                self._copy("sums", np.zeros((q, self._n), np.uint64)) if sums else None)


class KqueryResult(_SeqResult):
    _prefix = "kquery"

    def __init__(self, ctx, h, n_cols, has_sums):
        super().__init__(ctx, h, n_cols)
        self._sums = has_sums

    def sums_dev(self):
        return self._call("sums_dev")

    def output(self):
        nk, hits, sums = self._tables(self._sums)
        return KqueryOutput(nk, hits, sums, self.kernel_ms(), self.algo_bytes())


class CqueryOutput:
    """n_kmers uint32[queries]: positions with a valid k-mer; hits uint32[queries, n_cols]: those whose abundance class in the column is
    at least min_class; sums uint64[queries, n_cols]: the least counts of the classes (floor_of) added up; kernel_ms < 0 without
    set_profiling"""

    def __init__(self, n_kmers, hits, sums, kernel_ms, algo_bytes):
        self.n_kmers, self.hits, self.sums, self.kernel_ms, self.algo_bytes = n_kmers, hits, sums, kernel_ms, algo_bytes


class CqueryResult(_SeqResult):
    _prefix = "cquery"

    def sums_dev(self):
        return self._call("sums_dev")

    def output(self):
        nk, hits, sums = self._tables(True)
        return CqueryOutput(nk, hits, sums, self.kernel_ms(), self.algo_bytes())


class ZqueryResult(_SeqResult):
    """a call of a zquery series: bits_dev() the series' table; hits_dev() and output() on the last call only"""
    _prefix = "zquery"

    def bits_dev(self):
        return self._call("bits_dev")

    def output(self):
        """-> QueryOutput: n_kmers the K-positions of every query, hits those whose z + 1 rows all have the sample's bit"""
        nk, hits, _ = self._tables()
        return QueryOutput(nk, hits, self.kernel_ms(), self.algo_bytes())


class QueryResult(_SeqResult):
    _prefix = "query"

    def output(self):
        nk, hits, _ = self._tables()
        return QueryOutput(nk, hits, self.kernel_ms(), self.algo_bytes())


class FilterOutput:
    """body: bytes of M (rows kept rows of row_bytes); vector: uint32 per input row (V); absent_keys uint64[n, key_words] and
    absent_counts uint32[n] (K); what was not asked for is empty"""

    def __init__(self, body, rows, row_bytes, vector, absent_keys, absent_counts):
        self.body, self.rows, self.row_bytes, self.vector = body, rows, row_bytes, vector
        self.absent_keys, self.absent_counts = absent_keys, absent_counts


class FilterResult(_Result):
    _prefix = "filter"

    def __init__(self, ctx, h, key_words):
        super().__init__(ctx, h)
        self._kw = key_words

    def rows(self):
        return self._call("rows")

    def row_bytes(self):
        return self._call("row_bytes")

    def body_dev(self):
        return self._call("body_dev")

    def output(self):
        self.wait()
        body = self._copy("body", np.zeros(self._call("body_bytes"), np.uint8))
        vec = self._copy("vector", np.zeros(self._call("vector_len"), np.uint32))
        n, w = self._call("absent"), self._kw * 2 + 1
        rec = self._copy("absent", np.zeros(n * w * 4, np.uint8)).view(np.uint32).reshape(n, w)
        keys = np.ascontiguousarray(rec[:, :self._kw * 2]).view(np.uint64).reshape(n, self._kw)
        return FilterOutput(body.tobytes(), self.rows(), self.row_bytes(), vec, keys, rec[:, self._kw * 2].copy())


class CombineResult(_Result):
    _prefix = "combine"

    def rows(self):
        return self._call("rows")

    def row_bytes(self):
        return self._call("row_bytes")

    def body_dev(self):
        return self._call("body_dev")

    def body(self):
        self.wait()
        return self._copy("body", np.zeros(self._call("body_bytes"), np.uint8)).tobytes()

    def output(self):
        return CombineOutput(self.body(), self.rows(), self.row_bytes(), self.kernel_ms(), self.algo_bytes())


class MergeResult:
    def __init__(self, ctx, h, n_lists):
        self._ctx, self._h, self._n = ctx, h, n_lists

    def wait(self):
        self._ctx._check(_lib.kmx_result_wait(self._h), "kmx_result_wait")

    def kernel_ms(self):
        return _lib.kmx_result_kernel_ms(self._h)

    def kernel_parts_ms(self):
        """(k_merge_cols ms, k_cols_sparse ms) of a result of the column-blocked pair; (-1, -1) otherwise"""
        a, b = C.c_double(-1.0), C.c_double(-1.0)
        self._ctx._check(_lib.kmx_result_kernel_parts_ms(self._h, C.byref(a), C.byref(b)), "kmx_result_kernel_parts_ms")
        return a.value, b.value

    def kernel(self):
        return _lib.kmx_result_kernel(self._h).decode()

    def transpose_ms(self):
        return _lib.kmx_result_transpose_ms(self._h)

    def body_dev(self, t=0):
        """device address of a BF / BFC / BFT body (None for COUNT / PA)"""
        return _lib.kmx_result_body_dev(self._h, t)

    def rows(self, t=0):
        return _lib.kmx_result_rows(self._h, t)

    def sparse_rows(self, t=0):
        return _lib.kmx_result_sparse_rows(self._h, t)

    def row_bytes(self, t=0):
        return _lib.kmx_result_row_bytes(self._h, t)

    def body_bytes(self, t=0):
        return _lib.kmx_result_body_bytes(self._h, t)

    def algo_bytes(self, t=0):
        return _lib.kmx_result_algo_bytes(self._h, t)

    def body(self, t=0):
        nb = self.body_bytes(t)
        buf = np.zeros(max(nb, 1), dtype=np.uint8)
        self._ctx._check(_lib.kmx_result_copy_body(self._h, t, buf.ctypes.data, nb), "kmx_result_copy_body")
        return buf[:nb].tobytes()

    def body_from_arena(self, t=0):
        """the body put together on the HOST from the arena and the order of its rows (kmx_result_arena + kmx_result_copy_order):
        what the pipeline's file writer does with pwrite"""
        rows, rb = self.rows(t), self.row_bytes(t)
        if rows == 0:
            return b""
        dev, nar = _vp(), C.c_uint64()
        self._ctx._check(_lib.kmx_result_arena(self._h, t, C.byref(dev), C.byref(nar)), "kmx_result_arena")
        arena = np.zeros((nar.value, rb), np.uint8)
        self._ctx._check(_lib.kmx_copy_to_host(self._ctx._h, arena.ctypes.data, dev, nar.value * rb), "kmx_copy_to_host")
        order = np.zeros(rows, np.uint32)
        self._ctx._check(_lib.kmx_result_copy_order(self._h, t, order.ctypes.data), "kmx_result_copy_order")
        return arena[order].tobytes()

    def body_to_device(self, t, dev_ptr, nbytes):
        """BF / BFC / BFT body -> device memory of the caller (a torch tensor's data_ptr())"""
        self._ctx._check(_lib.kmx_result_copy_body_dev(self._h, t, dev_ptr, nbytes), "kmx_result_copy_body_dev")

    def stats(self, t=0):
        st = np.zeros((STATS_ROWS, self._n[t]), dtype=np.uint64)
        self._ctx._check(_lib.kmx_result_copy_stats(self._h, t, st.ctypes.data), "kmx_result_copy_stats")
        return st

    def free(self):
        if self._h:
            _lib.kmx_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Store:
    """kmx_store: count lists resident in HBM between the count and the merge stage"""

    def __init__(self, device=0, limit_bytes=0):
        h = _vp()
        rc = _lib.kmx_store_create(device, limit_bytes, C.byref(h))
        if rc != 0:
            raise KmxError(f"kmx_store_create failed ({rc}): {_lib.kmx_last_error(None).decode()}")
        self._h = h

    def used(self):
        return _lib.kmx_store_used(self._h)

    def limit(self):
        return _lib.kmx_store_limit(self._h)

    def close(self):
        if self._h:
            _lib.kmx_store_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
