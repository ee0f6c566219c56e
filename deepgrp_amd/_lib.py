"""ctypes binding of libdeepgrp_hip.so (the C ABI declared in include/deepgrp_hip.h)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdeepgrp_hip.so")

i64, i32, vp, cint = C.c_int64, C.c_int32, C.c_void_p, C.c_int


class DgrpError(RuntimeError):
    """A libdeepgrp_hip call failed (message from dgrp_last_error())."""


class Segment(C.Structure):
    """struct dgrp_segment"""
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("label", C.c_int32), ("contig", C.c_int32)]


class TrainJob(C.Structure):
    """struct dgrp_train_job: the argument list of dgrp_train_step"""
    _fields_ = [("T", cint), ("u", cint), ("C", cint), ("attention", cint), ("d_params", vp), ("d_idx", vp), ("d_truth", vp),
                ("n", i64), ("d_starts", vp), ("B", i64), ("d_masks", vp), ("d_loss", vp), ("d_grads", vp), ("d_work", vp),
                ("work_bytes", i64)]


class InflateStreamStats(C.Structure):
    """struct dgrp_inflate_stream_stats"""
    _fields_ = [(k, C.c_int64) for k in ("spans", "candidates", "repaired", "rounds", "longest_span", "false_starts", "chunks", "reserved")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


TRAIN_MAX_JOBS = 8                 # DGRP_TRAIN_MAX_JOBS

_SIGNATURES = {
    "dgrp_abi_version": (cint, []),
    "dgrp_last_error": (C.c_char_p, []),
    "dgrp_device_info": (cint, [C.c_char_p, C.c_size_t, C.POINTER(cint), C.POINTER(i64)]),
    "dgrp_strip_n": (cint, [vp, i64, C.POINTER(i64), C.POINTER(i64)]),
    "dgrp_encode": (cint, [vp, i64, vp, vp]),
    "dgrp_onehot": (cint, [vp, i64, vp, vp]),
    "dgrp_fasta_workspace_bytes": (i64, [i64]),
    "dgrp_fasta_encode": (cint, [vp, i64, vp, C.POINTER(i64), vp, i64, vp]),
    "dgrp_fasta_batch_workspace_bytes": (i64, [i64, i64]),
    "dgrp_fasta_encode_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_fasta_chunks_workspace_bytes": (i64, [i64]),
    "dgrp_fasta_chunks": (cint, [vp, i64, i64, vp, vp, C.POINTER(i64), vp, i64, vp]),
    "dgrp_fasta_mask_workspace_bytes": (i64, [i64, i64, i64]),
    "dgrp_fasta_mask_batch": (cint, [vp, i64, vp, vp, vp, vp, cint, C.c_uint64, vp, vp, i64, vp]),
    "dgrp_fasta_extract_workspace_bytes": (i64, [i64, i64, i64]),
    "dgrp_fasta_extract_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, i64, cint, C.c_uint64, vp, i64, C.POINTER(i64), vp, C.POINTER(i64),
                                        vp, i64, vp]),
    "dgrp_repeat_summary_workspace_bytes": (i64, [i64, i64, i64]),
    "dgrp_repeat_summary_batch": (cint, [vp, i64, vp, vp, vp, vp, cint, i64, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_twobit_workspace_bytes": (i64, [i64]),
    "dgrp_twobit_encode_batch": (cint, [vp, i64, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, vp]),
    "dgrp_twobit_text_batch": (cint, [vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, i64, vp]),
    "dgrp_twobit_pack_workspace_bytes": (i64, [i64, i64]),
    "dgrp_twobit_pack_batch": (cint, [vp, i64, vp, vp, vp, i64, i64, vp, vp, vp, i64, vp]),
    "dgrp_format_rows_bound": (i64, [i64, i64]),
    "dgrp_format_rows": (cint, [vp, vp, i64, cint, vp, i64, vp, i64, C.POINTER(i64)]),
    "dgrp_track_workspace_bytes": (i64, [i64, i64]),
    "dgrp_track_text": (cint, [vp, i64, cint, cint, cint, i64, i64, C.c_char_p, i64, vp, i64, C.POINTER(i64), vp, i64, vp]),
    "dgrp_track_batch_workspace_bytes": (i64, [i64, vp, vp, i64, cint, i64]),
    "dgrp_track_text_batch": (cint, [vp, cint, i64, vp, vp, vp, C.c_char_p, vp, vp, cint, cint, i64, vp, i64, vp, vp, i64, vp]),
    "dgrp_track_index_workspace_bytes": (i64, [i64, vp, vp, i64, cint, i64]),
    "dgrp_track_index_batch": (cint, [vp, cint, i64, vp, vp, vp, C.c_char_p, vp, vp, cint, cint, i64, vp, i64, vp, vp, i64, vp, i64, vp]),
    "dgrp_track_csi_workspace_bytes": (i64, [i64, vp, vp, i64, cint, i64, cint]),
    "dgrp_track_csi_batch": (cint, [vp, cint, i64, vp, vp, vp, C.c_char_p, vp, vp, cint, cint, i64, cint, vp, i64, vp, vp, i64, vp, i64, vp]),
    "dgrp_track_sections_workspace_bytes": (i64, [i64, vp, vp, i64, cint]),
    "dgrp_track_sections_batch": (cint, [vp, cint, i64, vp, vp, vp, vp, cint, cint, i64, i64, vp, i64, vp, vp, i64, vp, vp, i64, vp]),
    "dgrp_track_zoom_workspace_bytes": (i64, [i64, vp, vp, i64, cint]),
    "dgrp_track_zoom_batch": (cint, [vp, cint, i64, vp, vp, vp, vp, cint, cint, i64, i64, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp]),
    "dgrp_zlib_bound": (i64, [i64, i64]),
    "dgrp_zlib_workspace_bytes": (i64, [i64, cint]),
    "dgrp_zlib_compress_batch": (cint, [vp, i64, vp, i64, i64, cint, vp, i64, vp, C.POINTER(i64), vp, i64, vp]),
    "dgrp_zlib_compress_host": (cint, [vp, i64, vp, i64, i64, cint, vp, i64, vp, C.POINTER(i64)]),
    "dgrp_window_count":(i64, [i64, i64, i64]),
    "dgrp_windows_onehot": (cint, [vp, i64, i64, i64, i64, i64, cint, vp, vp]),
    "dgrp_model_create": (cint, [C.POINTER(vp), cint, cint, cint, cint, vp, vp, vp, vp, vp, vp]),
    "dgrp_model_create_lstm": (cint, [C.POINTER(vp), cint, cint, cint, vp, vp, vp, vp, vp]),
    "dgrp_model_destroy": (cint, [vp]),
    "dgrp_model_dims": (cint, [vp, C.POINTER(cint), C.POINTER(cint), C.POINTER(cint), C.POINTER(cint)]),
    "dgrp_model_flags": (cint, [vp]),
    "dgrp_model_set_precision": (cint, [vp, cint]),
    "dgrp_model_view": (cint, [vp, cint, C.POINTER(vp)]),
    "dgrp_model_plan": (cint, [vp, cint, i64, C.POINTER(cint), C.POINTER(i64), C.POINTER(cint), C.POINTER(cint)]),
    "dgrp_forward_workspace_bytes": (i64, [vp, i64]),
    "dgrp_forward_window_chunk": (i64, [vp]),
    "dgrp_forward_windows": (cint, [vp, vp, i64, i64, i64, i64, vp, vp, i64, vp]),
    "dgrp_forward_merge": (cint, [vp, vp, i64, i64, i64, i64, i64, vp, vp, i64, vp]),
    "dgrp_forward_merge_record": (cint, [vp, vp, i64, i64, i64, vp, vp, i64, vp]),
    "dgrp_forward_merge_record_workspace_bytes": (i64, [vp, i64, i64]),
    "dgrp_forward_reference_workspace_bytes": (i64, [vp, i64]),
    "dgrp_forward_windows_reference": (cint, [vp, vp, i64, i64, i64, i64, vp, vp, i64, vp]),
    "dgrp_get_max": (cint, [vp, i64, vp, i64, i64, i64, i64, vp]),
    "dgrp_scores": (cint, [vp, i64, cint, vp, vp, vp]),
    "dgrp_softmax_labels": (cint, [vp, i64, cint, vp, vp, vp, i64, vp]),
    "dgrp_mss_workspace_bytes": (i64, [i64]),
    "dgrp_mss_labels": (cint, [vp, vp, i64, cint, cint, cint, vp, vp, vp, i64, vp]),
    "dgrp_mss_segments_host": (cint, [vp, i64, vp, i64, C.POINTER(i64)]),
    "dgrp_mss_batch_workspace_bytes": (i64, [i64, i64]),
    "dgrp_mss_labels_batch": (cint, [vp, vp, i64, i64, vp, cint, cint, cint, vp, vp, i64, vp]),
    "dgrp_segments_workspace_bytes": (i64, [i64]),
    "dgrp_segments": (cint, [vp, i64, i64, i32, vp, i64, vp, vp, i64, vp]),
    "dgrp_record_workspace_bytes": (i64, [vp, i64, i64, cint]),
    "dgrp_predict_record": (cint, [vp, vp, i64, i64, i64, cint, cint, cint, i64, i32, vp, i64, C.POINTER(i64), vp, i64, vp]),
    "dgrp_batch_workspace_bytes": (i64, [vp, i64, vp, i64]),
    "dgrp_predict_batch": (cint, [vp, vp, i64, vp, vp, vp, vp, i64, i64, cint, cint, vp, i64, C.POINTER(i64), vp, i64, vp]),
    "dgrp_batch_rows": (i64, [i64, vp]),
    "dgrp_predict_batch_probs": (cint, [vp, vp, i64, vp, vp, vp, vp, i64, i64, cint, cint, vp, i64, C.POINTER(i64), vp, i64, vp, vp]),
    "dgrp_confusion_matrix": (cint, [vp, vp, i64, cint, vp, vp, vp]),
    "dgrp_filter_segments": (cint, [vp, vp, i64, i64, vp]),
    "dgrp_eval_workspace_bytes": (i64, [i64, i64]),
    "dgrp_paint_rows_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_row_hits_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_row_scores_workspace_bytes": (i64, [i64, i64]),
    "dgrp_row_scores_batch": (cint, [vp, cint, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_prob_hist_workspace_bytes": (i64, [i64, cint, cint]),
    "dgrp_prob_hist_batch": (cint, [vp, cint, i64, vp, vp, vp, vp, cint, vp, vp, vp, i64, vp]),
    "dgrp_row_detect_workspace_bytes": (i64, [i64, i64]),
    "dgrp_paint_row_keys_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_row_detect_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_format_bed_bound": (i64, [i64, i64]),
    "dgrp_format_bed_rows": (cint, [vp, vp, i64, cint, vp, vp, i64, cint, vp, i64, C.POINTER(i64)]),
    "dgrp_bed_text_workspace_bytes": (i64, [i64, i64, i64]),
    "dgrp_bed_text_batch": (cint, [vp, vp, i64, cint, vp, vp, i64, cint, vp, i64, C.POINTER(i64), vp, i64, vp]),
    "dgrp_bed_index_workspace_bytes": (i64, [i64, i64, i64, i64]),
    "dgrp_bed_index_batch": (cint, [vp, vp, i64, cint, vp, vp, i64, cint, i64, vp, vp, i64, C.POINTER(i64), vp, i64, vp, vp, i64, vp]),
    "dgrp_bed_csi_workspace_bytes": (i64, [i64, i64, i64, i64, cint]),
    "dgrp_bed_csi_batch": (cint, [vp, vp, i64, cint, vp, vp, i64, cint, i64, vp, cint, vp, i64, C.POINTER(i64), vp, i64, vp, vp, i64, vp]),
    "dgrp_gff_text_workspace_bytes": (i64, [i64, i64, i64, i64, i64]),
    "dgrp_gff_text_batch": (cint, [vp, vp, i64, cint, vp, vp, i64, vp, vp, i64, cint, i64, vp, i64, C.POINTER(i64), C.POINTER(i64), vp, i64,
                                   vp]),
    "dgrp_gff_index_workspace_bytes": (i64, [i64, i64, i64, i64, i64, i64]),
    "dgrp_gff_index_batch": (cint, [vp, vp, i64, cint, vp, vp, i64, vp, vp, i64, cint, i64, i64, vp, vp, i64, C.POINTER(i64), vp, i64, vp, vp,
                                    i64, vp]),
    "dgrp_gff_csi_workspace_bytes": (i64, [i64, i64, i64, i64, i64, i64, cint]),
    "dgrp_gff_csi_batch": (cint, [vp, vp, i64, cint, vp, vp, i64, vp, vp, i64, cint, i64, i64, vp, cint, vp, i64, C.POINTER(i64), vp, i64, vp,
                                  vp, i64, vp]),
    "dgrp_rmout_text_workspace_bytes": (i64, [i64, i64, i64, i64, i64, i64]),
    "dgrp_rmout_text_batch": (cint, [vp, vp, i64, cint, vp, vp, i64, vp, vp, i64, cint, i64, vp, i64, i64, vp, i64, C.POINTER(i64),
                                     C.POINTER(i64), C.POINTER(i64), vp, i64, vp]),
    "dgrp_bed_blocks_workspace_bytes": (i64, [i64, i64, vp]),
    "dgrp_bed_blocks_batch": (cint, [cint, vp, vp, i64, cint, i64, vp, i64, vp, i64, C.POINTER(i64), vp, i64, C.POINTER(i64), C.POINTER(i64),
                                     vp, i64, vp]),
    "dgrp_bed_zoom_workspace_bytes": (i64, [i64, i64, vp]),
    "dgrp_bed_zoom_batch": (cint, [cint, vp, vp, i64, cint, i64, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp]),
    "dgrp_inflate_raw_host": (cint, [vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(cint)]),
    "dgrp_inflate_workspace_bytes": (i64, [i64]),
    "dgrp_inflate_batch": (cint, [vp, i64, i64, vp, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(cint), vp, i64, vp]),
    "dgrp_inflate_stream_host": (cint, [vp, i64, i64, i64, cint, vp, i64, C.POINTER(i64), C.POINTER(i64), vp, C.POINTER(cint)]),
    "dgrp_inflate_stream_workspace_bytes": (i64, [i64, i64]),
    "dgrp_inflate_stream_scan": (cint, [vp, i64, i64, i64, i64, cint, C.POINTER(i64), vp, C.POINTER(cint), vp, i64, vp]),
    "dgrp_inflate_stream_write": (cint, [vp, i64, i64, i64, vp, vp, i64, C.POINTER(C.c_uint32), C.POINTER(i64), C.POINTER(cint), vp, i64,
                                         vp]),
    "dgrp_bgzf_bound": (i64, [i64, cint]),
    "dgrp_bgzf_workspace_bytes": (i64, [i64]),
    "dgrp_bgzf_compress": (cint, [vp, i64, vp, i64, C.POINTER(i64), cint, vp, i64, vp]),
    "dgrp_bgzf_compress_host": (cint, [vp, i64, vp, i64, C.POINTER(i64), cint]),
    "dgrp_bgzf_workspace_bytes_level": (i64, [i64, cint]),
    "dgrp_bgzf_compress_level": (cint, [vp, i64, vp, i64, C.POINTER(i64), cint, cint, vp, i64, vp]),
    "dgrp_bgzf_compress_host_level": (cint, [vp, i64, vp, i64, C.POINTER(i64), cint, cint]),
    "dgrp_train_param_count": (i64, [cint, cint, cint]),
    "dgrp_train_workspace_bytes": (i64, [cint, cint, cint, cint, i64]),
    "dgrp_train_step": (cint, [cint, cint, cint, cint, vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp]),
    "dgrp_train_step_multi": (cint, [C.POINTER(TrainJob), cint, vp]),
    "dgrp_optimizer_step": (cint, [cint, vp, vp, vp, vp, i64, C.c_double, C.c_double, C.c_double, C.c_double, i64, vp]),
    "dgrp_truth_workspace_bytes": (i64, [i64, i64]),
    "dgrp_truth_multihot_batch": (cint, [vp, cint, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_class_starts_workspace_bytes": (i64, [i64, i64]),
    "dgrp_class_window_starts": (cint, [vp, i64, i64, vp, vp, cint, vp, i64, C.POINTER(i64), vp, i64, vp]),
    "dgrp_train_resolve_starts": (cint, [vp, i64, vp, vp, cint, vp, vp, i64, vp, vp]),
    "dgrp_rm_parse_workspace_bytes": (i64, [i64]),
    "dgrp_rm_parse": (cint, [vp, i64, vp, vp, cint, vp, cint, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp]),
    "dgrp_rm_parse_fields": (cint, [vp, i64, vp, vp, cint, vp, cint, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp]),
    "dgrp_paint_strata_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_prob_hist_strata_workspace_bytes": (i64, [i64]),
    "dgrp_prob_hist_strata_batch": (cint, [vp, cint, i64, vp, vp, vp, vp, cint, cint, vp, vp, vp, i64, vp]),
    "dgrp_rm_parse_all_workspace_bytes": (i64, [i64]),
    "dgrp_rm_parse_all": (cint, [vp, i64, vp, vp, cint, vp, cint, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp]),
    "dgrp_rows_parse_workspace_bytes": (i64, [i64]),
    "dgrp_rows_parse": (cint, [vp, i64, cint, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp]),
    "dgrp_gff_parse_workspace_bytes": (i64, [i64]),
    "dgrp_gff_parse": (cint, [vp, i64, vp, vp, vp, cint, vp, cint, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp]),
    "dgrp_token_ids_workspace_bytes": (i64, [i64, i64]),
    "dgrp_token_ids": (cint, [vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp]),
    "dgrp_paint_keys_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_key_crosstab_batch": (cint, [vp, vp, i64, cint, i64, vp, vp, vp]),
    "dgrp_row_key_classes_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_row_bounds_workspace_bytes": (i64, [i64, i64]),
    "dgrp_row_bounds_batch": (cint, [vp, i64, vp, vp, vp, vp, vp, cint, vp, vp, i64, vp]),
    "dgrp_bound_hist_workspace_bytes": (i64, [i64]),
    "dgrp_bound_hist_batch": (cint, [i64, vp, vp, vp, vp, vp, vp, vp, cint, cint, vp, vp, vp, vp, vp, i64, vp]),
    "dgrp_kernel_timer_enable": (cint, [cint]),
    "dgrp_kernel_timer_read": (cint, [C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64)]),
}

_lib = None


def lib() -> C.CDLL:
    """The loaded library; raises ImportError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C deepgrp_amd/csrc` (hipcc, gfx950) "
                "or `python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback.")
        # PyTorch-ROCm ships its own libamdhip64; it must be in the process BEFORE this library is
        # loaded so that both bind to the same HIP runtime (streams and device pointers are shared).
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        if L.dgrp_abi_version() != 1:
            raise ImportError("libdeepgrp_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().dgrp_last_error().decode("utf-8", "replace")
        raise DgrpError(f"{what or 'libdeepgrp_hip'} failed (code {rc}): {msg}")


def name_blob(names):
    """Names as the entries take them: str (UTF-8, surrogateescape) or bytes -> (the names as bytes, their bytes back to back,
    int64 offsets [len(names) + 1] into those)."""
    import numpy as np
    raw = [nm if isinstance(nm, bytes) else nm.encode("utf-8", "surrogateescape") for nm in names]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(x) for x in raw], out=off[1:])
    return raw, b"".join(raw), off


def exported_symbols():
    return sorted(_SIGNATURES)
