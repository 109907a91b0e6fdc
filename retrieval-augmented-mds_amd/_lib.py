"""ctypes binding of the C ABI declared in include/mips_hip.h (libmips_hip.so, hipcc, gfx950).

There is NO CPU fallback: if the library cannot be built or loaded, or no GPU is visible when a
device call is made, the product raises.  (The CPU oracle under oracle/ is test infrastructure and
is never imported from here.)
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libmips_hip.so")
HEADER = os.path.join(_ROOT, "include", "mips_hip.h")
HEADER_SHARDED = os.path.join(_ROOT, "include", "mips_hip_sharded.h")  # helpers of the shard exchange (no index handle)
HEADER_UPDATE = os.path.join(_ROOT, "include", "mips_hip_update.h")  # calls that change the rows an index holds
HEADER_ROWS = os.path.join(_ROOT, "include", "mips_hip_rows.h")  # stored rows, labels and scores by row id
HEADER_HOOK = os.path.join(_ROOT, "include", "mips_hip_hook.h")  # the one-launch hook search under a group filter
HEADER_SQ8 = os.path.join(_ROOT, "include", "mips_hip_sq8.h")  # the trained 8-bit scalar quantiser of an SQ8 index
HEADER_IVF = os.path.join(_ROOT, "include", "mips_hip_ivf.h")  # the IVF index: k-means lists over a flat index, nprobe
HEADER_IVF_RANGE = os.path.join(_ROOT, "include", "mips_hip_ivf_range.h")  # range search over the probed lists of an IVF index
HEADER_WRITE = os.path.join(_ROOT, "include", "mips_hip_write.h")  # stored rows overwritten in place by id (flat and IVF index)
HEADER_IVF_SHARDED = os.path.join(_ROOT, "include", "mips_hip_ivf_sharded.h")  # the IVF search cut at its merge, for row shards
HEADER_PQ = os.path.join(_ROOT, "include", "mips_hip_pq.h")  # the product-quantised index: M one-byte codes per row, ADC search
HEADER_IVFPQ = os.path.join(_ROOT, "include", "mips_hip_ivfpq.h")  # the IVF index over PQ codes: lists, residual codes, ADC list scan
HEADER_REFINE = os.path.join(_ROOT, "include", "mips_hip_refine.h")  # candidate search on PQ codes (k <= 1024) and exact re-ranking
ABI_VERSION = 1

# constants of include/mips_hip.h
DTYPE_F32, DTYPE_BF16, DTYPE_FP8_E4M3, DTYPE_FP8_E4M3_DOCS, DTYPE_SQ8 = 0, 1, 2, 3, 4
METRIC_IP, METRIC_L2 = 0, 1
Q_DEVICE, OUT_DEVICE, OUT_PACKED, FORCE_IP, SEL_DEVICE, GRP_DEVICE = 1, 2, 4, 8, 16, 32
IDS_DEVICE, ROWS_ZERO_MISSING = 64, 128  # include/mips_hip_rows.h
RADII_DEVICE = 256  # include/mips_hip_ivf_range.h
GRP_EXCLUDE, GRP_ONLY = 0, 1  # MIPS_GRP_*: the mode of a grouped search
LABEL_NONE = -(1 << 31)  # MIPS_LABEL_NONE = INT32_MIN: a query that is not group-filtered
SYNTH_LATTICE, SYNTH_GAUSS, SYNTH_LATTICE_FP8 = 0, 1, 2
SEED_DOCS, SEED_QUERIES = 0xD0C5, 0x0E21  # fixed seeds of the synthetic workloads
MAX_K = 29
MAX_K_WIDE = 1024  # MIPS_MAX_K_WIDE: largest k of mips_search_wide
IDX_POISON = -2  # MIPS_IDX_POISON: what a search whose scan kernel timed out returns in every slot

_lock = threading.Lock()
_lib = None


def _sources():
    out = [HEADER, HEADER_SHARDED, HEADER_UPDATE, HEADER_ROWS, HEADER_HOOK, HEADER_SQ8, HEADER_IVF, HEADER_IVF_RANGE, HEADER_WRITE,
           HEADER_IVF_SHARDED, HEADER_PQ, HEADER_IVFPQ, HEADER_REFINE]
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp", ".h")):
            out.append(os.path.join(CSRC, f))
    return out


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(s) > t for s in _sources())


# -amdgpu-mfma-vgpr-form: MFMA results in architectural VGPRs even in kernels that pin values in AGPRs.  The
# query-stationary kernels fill the AGPR half of the register file with stationary B fragments (inline-asm "a"
# constraints); without the option LLVM then selects the AGPR-destination MFMA forms for the whole kernel, the
# accumulators compete with the fragments for AGPRs (the retired 64-queries-per-wave kernel spilled fragments, reloaded
# behind a vmcnt(0) that drains the LDS-DMA ring; with it: 254 VGPRs + 256 AGPRs, no scratch).  The shipped kernels were
# measured and tuned with the option; none changes its spill count.
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]

def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 csrc/mips_hip.hip -> lib/libmips_hip.so (in-tree)."""
    if not force and not _stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libmips_hip.so (no CPU fallback exists)")
    os.makedirs(LIB_DIR, exist_ok=True)
    import fcntl

    # one builder at a time (the ranks of a multi-GPU job import the package together)
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not _stale():  # another process built it while we waited
                return LIB_PATH
            tmp = LIB_PATH + f".tmp{os.getpid()}"
            cmd = [hipcc, *HIPCC_FLAGS, "-o", tmp, os.path.join(CSRC, "mips_hip.hip")]
            if verbose:
                print(" ".join(cmd), flush=True)
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:
                raise RuntimeError(f"hipcc failed ({proc.returncode}):\n{proc.stderr[-4000:]}")
            os.replace(tmp, LIB_PATH)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


def _bind(lib):
    c = ctypes
    vp, i64, i32, u64 = c.c_void_p, c.c_int64, c.c_int, c.c_uint64
    sig = {
        "mips_abi_version": (i32, []),
        "mips_last_error": (c.c_char_p, []),
        "mips_index_create": (i32, [c.POINTER(vp), i32, i64, i32, i32]),
        "mips_index_destroy": (i32, [vp]),
        "mips_index_reserve": (i32, [vp, i64]),
        "mips_index_add": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_index_reset": (i32, [vp]),
        "mips_index_ntotal": (i64, [vp]),
        "mips_index_dim": (i64, [vp]),
        "mips_index_metric": (i32, [vp]),
        "mips_index_phi": (i32, [vp, c.POINTER(c.c_double), vp]),
        "mips_index_set_phi": (i32, [vp, c.c_double]),
        "mips_index_read_rows": (i32, [vp, i64, i64, vp, vp]),
        "mips_index_add_synthetic": (i32, [vp, i64, i64, u64, i32, vp]),
        "mips_synth_fill": (i32, [vp, i64, i64, i64, u64, i32, i32, i32, vp]),
        "mips_search": (i32, [vp, vp, i32, i64, i32, vp, vp, i64, i32, vp]),
        "mips_search_wide": (i32, [vp, vp, i32, i64, i32, vp, vp, i64, i32, vp]),
        "mips_range_search": (i32, [vp, vp, i32, i64, vp, vp, vp, vp, i64, i64, i32, vp]),
        "mips_search_wide_sel": (i32, [vp, vp, i32, i64, i32, vp, vp, i64, i32, vp, i64, i64, vp]),
        "mips_range_search_sel": (i32, [vp, vp, i32, i64, vp, vp, vp, vp, i64, i64, i32, vp, i64, i64, vp]),
        "mips_index_set_labels": (i32, [vp, vp, i64, i64, i32, vp]),
        "mips_index_read_labels": (i32, [vp, i64, i64, vp, vp]),
        "mips_search_wide_grp": (i32, [vp, vp, i32, i64, i32, vp, vp, i64, i32, vp, i64, i64, vp, i32, vp]),
        "mips_range_search_grp": (i32, [vp, vp, i32, i64, vp, vp, vp, vp, i64, i64, i32, vp, i64, i64, vp, i32, vp]),
        "mips_search_split": (i32, [vp, vp, i32, i64, i32, vp, vp, i64, i32, vp, vp]),
        "mips_search_fused": (i32, [vp, vp, i32, i64, i32, i32, vp, vp, vp, i64, vp]),
        "mips_merge_topk": (i32, [vp, vp, i64, i32, i32, i32, vp, vp, i32, vp]),
        "mips_merge_topk_packed": (i32, [vp, i64, i32, i32, i32, vp, vp, i32, vp]),
        "mips_merge_topk_sorted_packed": (i32, [vp, i64, i32, i32, i32, vp, vp, i32, vp]),
        "mips_filter_ignore": (i32, [vp, vp, vp, i64, i32, i32, vp, vp, i32, vp]),
        "mips_cosine_rescore": (i32, [vp, vp, i32, i64, i32, i64, vp, i32, vp]),
        "mips_cosine_rescore_bias": (i32, [vp, vp, i32, i64, i32, i64, vp, i64, vp, i32, vp]),
        "mips_cosine_rescore_backward": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, vp, vp, i32, vp]),
        "mips_l2_normalize": (i32, [vp, i64, i64, i32, vp]),
        "mips_rows_max_sumsq": (i32, [vp, i64, i64, c.POINTER(c.c_double), i32, vp]),
        "mips_rows_max_sumsq_device": (i32, [vp, i64, i64, vp, i32, vp]),
        "mips_index_set_param": (i32, [vp, c.c_char_p, i64]),
        "mips_scan_timing": (i32, [vp, c.POINTER(c.c_float), c.POINTER(c.c_int), i32]),
        "mips_index_check_error": (i32, [vp, i32, vp]),
        "mips_index_last_kernel": (c.c_char_p, [vp]),
        "mips_index_margin_stats": (i32, [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64), i32, vp]),
    }
    sig_sharded = {  # include/mips_hip_sharded.h
        "mips_range_merge_records": (i32, [vp, i32, i64, i64, vp, vp, vp, i64, vp, i32, vp]),
    }
    sig_update = {  # include/mips_hip_update.h
        "mips_index_remove": (i32, [vp, vp, i64, i64, i32, c.POINTER(i64), vp]),
    }
    sig_rows = {  # include/mips_hip_rows.h
        "mips_index_reconstruct": (i32, [vp, vp, i64, i64, vp, i32, i64, i32, vp]),
        "mips_index_gather_labels": (i32, [vp, vp, i64, i64, vp, i32, vp]),
        "mips_score_subset": (i32, [vp, vp, i32, i64, vp, i32, vp, i64, i32, vp]),
    }
    sig_hook = {  # include/mips_hip_hook.h
        "mips_search_fused_grp": (i32, [vp, vp, i32, i64, i32, i32, vp, vp, vp, i64, vp, i32, i32, vp]),
    }
    sig_sq8 = {  # include/mips_hip_sq8.h
        "mips_index_sq8_train": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_index_sq8_set_params": (i32, [vp, vp, vp]),
        "mips_index_sq8_get_params": (i32, [vp, vp, vp]),
        "mips_index_sq8_is_trained": (i32, [vp]),
    }
    sig_ivf = {  # include/mips_hip_ivf.h
        "mips_ivf_create": (i32, [c.POINTER(vp), i32, i64, i32, i32, i64]),
        "mips_ivf_destroy": (i32, [vp]),
        "mips_ivf_flat": (vp, [vp]),
        "mips_ivf_train": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_ivf_is_trained": (i32, [vp]),
        "mips_ivf_set_centroids": (i32, [vp, vp]),
        "mips_ivf_get_centroids": (i32, [vp, vp]),
        "mips_ivf_add": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_ivf_probe": (i32, [vp, vp, i32, i64, i64, vp, i32, vp]),
        "mips_ivf_remove": (i32, [vp, vp, i64, i64, i32, c.POINTER(i64), vp]),
        "mips_ivf_reset": (i32, [vp]),
        "mips_ivf_list_sizes": (i32, [vp, vp, vp]),
        "mips_ivf_read_assign": (i32, [vp, i64, i64, vp, vp]),
        "mips_ivf_set_assign": (i32, [vp, vp, i64, vp]),
        "mips_ivf_set_param": (i32, [vp, c.c_char_p, i64]),
        "mips_ivf_nlist": (i64, [vp]),
        "mips_ivf_search": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp]),
        "mips_ivf_search_sel": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp, i64, i64, vp]),
        "mips_ivf_search_grp": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp, i64, i64, vp, i32, vp]),
        "mips_ivf_search_wide": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp]),
        "mips_ivf_search_wide_grp": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp, i64, i64, vp, i32, vp]),
    }
    sig_ivf_range = {  # include/mips_hip_ivf_range.h
        "mips_ivf_range_search": (i32, [vp, vp, i32, i64, vp, i64, vp, vp, vp, i64, i64, i32, vp]),
        "mips_ivf_range_search_grp": (i32, [vp, vp, i32, i64, vp, i64, vp, vp, vp, i64, i64, i32, vp, i64, i64, vp, i32, vp]),
    }
    sig_write = {  # include/mips_hip_write.h
        "mips_index_update": (i32, [vp, vp, i64, i64, vp, i32, i32, vp, vp]),
        "mips_ivf_update": (i32, [vp, vp, i64, i64, vp, i32, i32, vp, vp]),
    }
    sig_ivf_sharded = {  # include/mips_hip_ivf_sharded.h
        "mips_ivf_search_part": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp, i64, i64, vp, i32, vp]),
        "mips_ivf_merge_parts": (i32, [vp, i32, i64, i32, vp, vp, vp, i32, vp]),
    }
    sig_pq = {  # include/mips_hip_pq.h
        "mips_pq_create": (i32, [c.POINTER(vp), i32, i64, i64, i32, i32]),
        "mips_pq_destroy": (i32, [vp]),
        "mips_pq_train": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_pq_is_trained": (i32, [vp]),
        "mips_pq_set_codebook": (i32, [vp, vp]),
        "mips_pq_get_codebook": (i32, [vp, vp]),
        "mips_pq_add": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_pq_add_codes": (i32, [vp, vp, i64, i32, vp]),
        "mips_pq_read_codes": (i32, [vp, i64, i64, vp, vp]),
        "mips_pq_search": (i32, [vp, vp, i32, i64, i32, vp, vp, i64, i32, vp]),
        "mips_pq_reconstruct": (i32, [vp, vp, i64, i64, vp, i32, i64, i32, vp]),
        "mips_pq_score_subset": (i32, [vp, vp, i32, i64, vp, i32, vp, i64, i32, vp]),
        "mips_pq_reset": (i32, [vp]),
        "mips_pq_set_param": (i32, [vp, c.c_char_p, i64]),
        "mips_pq_ntotal": (i64, [vp]),
        "mips_pq_m": (i64, [vp]),
    }
    sig_ivfpq = {  # include/mips_hip_ivfpq.h
        "mips_ivfpq_create": (i32, [c.POINTER(vp), i32, i64, i64, i64, i32, i32, i32]),
        "mips_ivfpq_destroy": (i32, [vp]),
        "mips_ivfpq_train": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_ivfpq_is_trained": (i32, [vp]),
        "mips_ivfpq_set_centroids": (i32, [vp, vp]),
        "mips_ivfpq_get_centroids": (i32, [vp, vp]),
        "mips_ivfpq_set_codebook": (i32, [vp, vp]),
        "mips_ivfpq_get_codebook": (i32, [vp, vp]),
        "mips_ivfpq_add": (i32, [vp, vp, i64, i32, i32, vp]),
        "mips_ivfpq_add_codes": (i32, [vp, vp, vp, i64, i32, vp]),
        "mips_ivfpq_read_codes": (i32, [vp, i64, i64, vp, vp]),
        "mips_ivfpq_read_assign": (i32, [vp, i64, i64, vp, vp]),
        "mips_ivfpq_list_sizes": (i32, [vp, vp, vp]),
        "mips_ivfpq_probe": (i32, [vp, vp, i32, i64, i64, vp, vp, i32, vp]),
        "mips_ivfpq_search": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp]),
        "mips_ivfpq_reconstruct": (i32, [vp, vp, i64, i64, vp, i32, i64, i32, vp]),
        "mips_ivfpq_score_subset": (i32, [vp, vp, i32, i64, vp, i32, vp, i64, i32, vp]),
        "mips_ivfpq_reset": (i32, [vp]),
        "mips_ivfpq_set_param": (i32, [vp, c.c_char_p, i64]),
        "mips_ivfpq_ntotal": (i64, [vp]),
        "mips_ivfpq_nlist": (i64, [vp]),
        "mips_ivfpq_m": (i64, [vp]),
    }
    sig_refine = {  # include/mips_hip_refine.h
        "mips_pq_search_candidates": (i32, [vp, vp, i32, i64, i32, vp, vp, i64, i32, vp]),
        "mips_ivfpq_search_candidates": (i32, [vp, vp, i32, i64, i32, i64, vp, vp, i64, i32, vp]),
        "mips_index_rerank": (i32, [vp, vp, i32, i64, vp, i32, i32, vp, vp, i64, i32, vp]),
    }
    for name, (res, args) in {**sig, **sig_sharded, **sig_update, **sig_rows, **sig_hook, **sig_sq8, **sig_ivf, **sig_ivf_range, **sig_write,
                              **sig_ivf_sharded, **sig_pq, **sig_ivfpq, **sig_refine}.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return sig


EXPORTS = (
    "mips_abi_version", "mips_last_error", "mips_index_create", "mips_index_destroy",
    "mips_index_reserve", "mips_index_add", "mips_index_reset", "mips_index_ntotal",
    "mips_index_dim", "mips_index_metric", "mips_index_phi", "mips_index_set_phi", "mips_index_read_rows",
    "mips_index_add_synthetic", "mips_synth_fill", "mips_search", "mips_merge_topk",
    "mips_merge_topk_packed", "mips_filter_ignore", "mips_cosine_rescore", "mips_cosine_rescore_bias", "mips_l2_normalize", "mips_rows_max_sumsq", "mips_index_set_param", "mips_scan_timing",
    "mips_index_check_error", "mips_index_last_kernel", "mips_cosine_rescore_backward", "mips_index_margin_stats", "mips_search_fused", "mips_search_split",
    "mips_rows_max_sumsq_device", "mips_search_wide", "mips_merge_topk_sorted_packed", "mips_range_search",
    "mips_search_wide_sel", "mips_range_search_sel",
    "mips_index_set_labels", "mips_index_read_labels", "mips_search_wide_grp", "mips_range_search_grp",
)

EXPORTS_SHARDED = ("mips_range_merge_records",)  # what include/mips_hip_sharded.h declares; the same library exports it
EXPORTS_UPDATE = ("mips_index_remove",)  # what include/mips_hip_update.h declares; the same library exports it
EXPORTS_ROWS = ("mips_index_reconstruct", "mips_index_gather_labels", "mips_score_subset")  # include/mips_hip_rows.h, likewise
EXPORTS_HOOK = ("mips_search_fused_grp",)  # include/mips_hip_hook.h, likewise
EXPORTS_SQ8 = ("mips_index_sq8_train", "mips_index_sq8_set_params", "mips_index_sq8_get_params", "mips_index_sq8_is_trained")  # mips_hip_sq8.h
EXPORTS_IVF = ("mips_ivf_create", "mips_ivf_destroy", "mips_ivf_flat", "mips_ivf_train", "mips_ivf_is_trained", "mips_ivf_set_centroids",
               "mips_ivf_get_centroids", "mips_ivf_add", "mips_ivf_probe", "mips_ivf_remove", "mips_ivf_reset",
               "mips_ivf_list_sizes", "mips_ivf_read_assign", "mips_ivf_set_assign", "mips_ivf_set_param", "mips_ivf_nlist",
               "mips_ivf_search", "mips_ivf_search_sel", "mips_ivf_search_grp", "mips_ivf_search_wide", "mips_ivf_search_wide_grp")  # mips_hip_ivf.h
EXPORTS_IVF_RANGE = ("mips_ivf_range_search", "mips_ivf_range_search_grp")  # include/mips_hip_ivf_range.h, likewise
EXPORTS_WRITE = ("mips_index_update", "mips_ivf_update")  # include/mips_hip_write.h, likewise
EXPORTS_IVF_SHARDED = ("mips_ivf_search_part", "mips_ivf_merge_parts")  # include/mips_hip_ivf_sharded.h, likewise
EXPORTS_PQ = ("mips_pq_create", "mips_pq_destroy", "mips_pq_train", "mips_pq_is_trained", "mips_pq_set_codebook", "mips_pq_get_codebook",
              "mips_pq_add", "mips_pq_add_codes", "mips_pq_read_codes", "mips_pq_search", "mips_pq_reconstruct", "mips_pq_score_subset",
              "mips_pq_reset", "mips_pq_set_param", "mips_pq_ntotal", "mips_pq_m")  # include/mips_hip_pq.h, likewise
EXPORTS_IVFPQ = ("mips_ivfpq_create", "mips_ivfpq_destroy", "mips_ivfpq_train", "mips_ivfpq_is_trained", "mips_ivfpq_set_centroids",
                 "mips_ivfpq_get_centroids", "mips_ivfpq_set_codebook", "mips_ivfpq_get_codebook", "mips_ivfpq_add", "mips_ivfpq_add_codes",
                 "mips_ivfpq_read_codes", "mips_ivfpq_read_assign", "mips_ivfpq_list_sizes", "mips_ivfpq_probe", "mips_ivfpq_search",
                 "mips_ivfpq_reconstruct", "mips_ivfpq_score_subset", "mips_ivfpq_reset", "mips_ivfpq_set_param", "mips_ivfpq_ntotal",
                 "mips_ivfpq_nlist", "mips_ivfpq_m")  # include/mips_hip_ivfpq.h, likewise
EXPORTS_REFINE = ("mips_pq_search_candidates", "mips_ivfpq_search_candidates", "mips_index_rerank")  # include/mips_hip_refine.h, likewise


def range_record_words(nq: int, stride: int) -> int:
    """MIPS_RANGE_RECORD_WORDS of include/mips_hip_sharded.h: int64 words of a shard's range-search record."""
    return int(nq) + 1 + int(stride) + (int(stride) + 1) // 2


def load():
    """Load (building first if needed) libmips_hip.so.  torch is imported first on purpose: its
    bundled libamdhip64 has the same SONAME as /opt/rocm's, so the dynamic loader binds our
    library to the HIP runtime torch already brought in -- one runtime per process, and torch
    device pointers are valid in our calls."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (must precede dlopen, see docstring)

        lib = ctypes.CDLL(build(), mode=ctypes.RTLD_GLOBAL)
        _bind(lib)
        ver = lib.mips_abi_version()
        if ver != ABI_VERSION:
            raise RuntimeError(f"libmips_hip.so ABI {ver} != expected {ABI_VERSION}; rebuild")
        _lib = lib
        return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mips_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what or 'libmips_hip'} failed (code {rc}): {msg}")


def require_gpu(device: int | None = None) -> int:
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(
            "retrieval-augmented-mds_amd: no AMD GPU visible; this backend has no CPU path "
            "(the reference's CPU FAISS search is what it replaces)")
    return torch.cuda.current_device() if device is None else int(device)
