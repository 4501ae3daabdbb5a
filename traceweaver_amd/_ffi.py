"""ctypes declarations of include/traceweaver_amd.h.  The shared library must have been built by
`__graft_entry__.build()` (hipcc, gfx950); there is no fallback: a missing library is an error."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libtwgpu.so")

TW_MAX_EP = 8
TW_TOPK = 5
TW_MAX_COMP = 5

STATUS = {0: "TW_OK", -1: "TW_ERR_ARG", -2: "TW_ERR_UNSUPPORTED", -3: "TW_ERR_DEVICE", -4: "TW_ERR_STATE",
          -5: "TW_ERR_WINDOW_WIDTH", -6: "TW_ERR_WINDOW_SIZE", -7: "TW_ERR_NAN_PARAMS", -8: "TW_ERR_SKIP_PARAMS",
          -9: "TW_ERR_SKIP_REFERENCE_RAISES"}
TW_SKIP_BASE = 1024
TW_SKIP_STRIDE = 128

c_i32p = ctypes.POINTER(ctypes.c_int32)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_f64p = ctypes.POINTER(ctypes.c_double)


class Batch(ctypes.Structure):
    _fields_ = [
        ("n_units", ctypes.c_int32),
        ("unit_in_off", ctypes.c_void_p), ("unit_E", ctypes.c_void_p), ("ep_off", ctypes.c_void_p),
        ("dag", ctypes.c_void_p), ("key_rank", ctypes.c_void_p),
        ("in_start", ctypes.c_void_p), ("in_end", ctypes.c_void_p),
        ("out_start", ctypes.c_void_p), ("out_end", ctypes.c_void_p),
        ("batch_size", ctypes.c_int32), ("batch_size_mis", ctypes.c_int32), ("topk", ctypes.c_int32),
        ("unit_time_scale", ctypes.c_void_p),
        ("skip", ctypes.c_void_p),
        ("unit_part", ctypes.c_void_p),
    ]


class DeviceView(ctypes.Structure):
    _fields_ = [("parent", ctypes.c_void_p), ("parent_count", ctypes.c_int64), ("gaps", ctypes.c_void_p), ("gaps_count", ctypes.c_int64),
                ("device", ctypes.c_int32)]


class SkipUnit(ctypes.Structure):
    _fields_ = [("n_tw", ctypes.c_int32), ("tw_start", ctypes.c_void_p), ("pool", ctypes.c_void_p), ("dist", ctypes.c_void_p)]


class SpanTable(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("trace", "span_id", "service", "op_name", "parent", "start", "duration", "kind")]


class UnitSet(ctypes.Structure):
    _fields_ = [("n_units", ctypes.c_int32)] + [(k, ctypes.c_void_p) for k in (
        "unit_in_off", "unit_E", "ep_off", "dag", "key_rank", "in_start", "in_end", "out_start", "out_end",
        "true_child", "in_trace", "in_row", "out_row", "unit_service", "ep_name", "in_ep_name", "unit_order")] + [
        ("n_traces", ctypes.c_int64), ("skipped", ctypes.c_int32 * 4)]


class Results(ctypes.Structure):
    _fields_ = [
        ("parent", ctypes.c_void_p), ("topk_idx", ctypes.c_void_p), ("topk_score", ctypes.c_void_p),
        ("topk_n", ctypes.c_void_p), ("chosen", ctypes.c_void_p), ("leaves", ctypes.c_void_p),
        ("window_end", ctypes.c_void_p), ("unit_stats", ctypes.c_void_p),
    ]


class Stitched(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("root", "depth", "tree_off", "tree_rows", "tree_root", "tree_latency", "tree_flags")]


class AttrQuery(ctypes.Structure):
    _fields_ = [("percentile", ctypes.c_double), ("start_min", ctypes.c_int64), ("start_max", ctypes.c_int64),
                ("need_flags", ctypes.c_uint32), ("skip_flags", ctypes.c_uint32)]


class Attribution(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "link", "self_time", "path_time", "tree_top_group", "tree_selected", "tree_path_rows", "group_path_time", "group_path_rows",
        "group_self_time", "group_span_time", "group_span_rows", "group_trees", "group_top_trees")]


class ConfQuery(ctypes.Structure):
    _fields_ = [("threshold", ctypes.c_double), ("n_edges", ctypes.c_int32), ("edges", ctypes.c_void_p)]


class Confidence(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "rank", "list_n", "margin", "row_request", "tree_decisions", "tree_not_best", "tree_unassigned", "tree_min_margin",
        "tree_weakest_row", "tree_confident", "calib")]


class DistQuery(ctypes.Structure):
    _fields_ = [("n_q", ctypes.c_int32), ("probs", ctypes.c_void_p), ("n_edges", ctypes.c_int32), ("edges", ctypes.c_void_p)]


class Distributions(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("tree_cohort", "seg_count", "seg_sum", "seg_off", "values", "quantile", "hist")]


class CmpQuery(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int32), ("pairs", ctypes.c_void_p), ("n_q", ctypes.c_int32), ("probs", ctypes.c_void_p),
                ("n_perm", ctypes.c_int32), ("seed", ctypes.c_uint64), ("max_pool", ctypes.c_int64)]


class CohortComparison(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "n_a", "n_b", "ks_gap", "ks_at", "u2", "quantile_shift", "perm_ge_ks", "perm_ge_u", "perm_ge_q")]


class SigQuery(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("need_flags", ctypes.c_uint32), ("skip_flags", ctypes.c_uint32),
                ("keep_reference", ctypes.c_int32), ("compare", ctypes.c_int32)]


class Signatures(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "row_level", "tree_class", "tree_items", "tree_same", "class_rep", "class_trees", "class_latency_sum", "class_latency_min",
        "class_latency_max", "class_off", "class_entries")]


class ClassProfile(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "rows", "span_time", "span_min", "span_max", "self_time", "path_time", "path_rows", "path_trees", "offset",
        "class_counted", "class_latency", "class_path_time", "class_top_entry")]


class ClassCatalogue(ctypes.Structure):
    _fields_ = [("n_classes", ctypes.c_int64), ("n_entries", ctypes.c_int64), ("mode", ctypes.c_int32), ("n_groups", ctypes.c_int32)] + [
        (k, ctypes.c_void_p) for k in (
            "class_off", "class_entries", "trees", "latency_sum", "latency_min", "latency_max", "counted", "latency", "first_epoch", "last_epoch",
            "seen", "rows", "span_time", "span_min", "span_max", "self_time", "path_time", "path_rows", "path_trees", "offset", "class_path_time",
            "class_top_entry")]


class FilterClause(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("term", "subject", "group", "caller", "metric", "reduce", "negate")] + [
        ("lo", ctypes.c_int64), ("hi", ctypes.c_int64)]


class FilterQuery(ctypes.Structure):
    _fields_ = [("need_flags", ctypes.c_uint32), ("skip_flags", ctypes.c_uint32), ("n_clauses", ctypes.c_int32), ("clauses", ctypes.POINTER(FilterClause))]


class FilterResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("tree_match", "match_trees", "clause_value", "clause_trees", "term_trees")]


class ExtractQuery(ctypes.Structure):
    _fields_ = [("need_flags", ctypes.c_uint32), ("skip_flags", ctypes.c_uint32), ("mode", ctypes.c_int32), ("order", ctypes.c_int32), ("limit", ctypes.c_int64),
                ("n_probs", ctypes.c_int32), ("n_list", ctypes.c_int32), ("probs", ctypes.POINTER(ctypes.c_double)), ("list", ctypes.POINTER(ctypes.c_int32))]


class Extracted(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("sel_tree", "sel_root", "sel_latency", "sel_start", "sel_flags", "out_off", "row", "parent", "depth", "subtree",
                                               "kind", "group", "start", "end", "self_time", "path_time")]


TW_EXTR_MAX_PROBS = 32
TW_EXTR_MAX_LIST = 1 << 20
TW_TREE_CONFIDENT = 8
TW_TREE_MATCH = 16
TW_FILT_MAX_CLAUSES = 16
TW_FILT_MAX_TERMS = 8
TW_CONF_MAX_EDGES = 15
TW_DIST_MAX_Q = 32
TW_DIST_MAX_EDGES = 63
TW_CMP_MAX_Q = 8
TW_CMP_MAX_PAIRS = 64

EXPORTS = ["tw_create", "tw_destroy", "tw_last_error", "tw_load_batch", "tw_run_pass1", "tw_get_gaps", "tw_set_gaps",
           "tw_device_buffers", "tw_set_gaps_device", "tw_set_mixtures", "tw_fit_mixtures", "tw_fit_mixtures_seeded", "tw_set_fit_seed", "tw_fit_rows", "tw_fit_mixtures_tape", "tw_get_fit_order", "tw_get_mixtures", "tw_run_pass2", "tw_get_results", "tw_get_gauss_params", "tw_get_timing",
           "tw_assign_service", "tw_find_order", "tw_order_bound", "tw_order_stage", "tw_order_load", "tw_set_truth", "tw_evaluate", "tw_measure_hbm_copy", "tw_host_alloc", "tw_host_free", "tw_build_distributions", "tw_scale_load", "tw_run_baseline", "tw_wap5_delays", "tw_wap5_parents",
           "tw_set_span_rows", "tw_set_parents", "tw_stitch_traces", "tw_set_row_groups", "tw_attribute_traces",
           "tw_get_decisions", "tw_score_traces", "tw_set_row_cohorts", "tw_latency_distributions", "tw_compare_cohorts", "tw_trace_signatures", "tw_class_profiles", "tw_filter_traces", "tw_extract_traces", "tw_get_extracted",
           "tw_history_reset", "tw_history_push", "tw_history_merge", "tw_history_info", "tw_history_distributions", "tw_history_compare",
           "tw_class_history_reset", "tw_class_history_push", "tw_class_history_match", "tw_class_history_merge", "tw_class_history_info", "tw_class_history_get",
           "tw_corpus_create", "tw_corpus_destroy", "tw_corpus_last_error", "tw_corpus_add_files", "tw_corpus_set_callers", "tw_corpus_counts",
           "tw_corpus_string", "tw_corpus_loop_origin", "tw_corpus_trace_names", "tw_corpus_span_table", "tw_corpus_build_units"]


def load(path=None):
    path = path or DEFAULT_LIB
    # Hardware queues for the engine's class streams (tw_create has the measurements).  GPU_MAX_HW_QUEUES is read by the HIP
    # runtime when it initialises and holds for every HIP user of the process (torch, RCCL): loading this library does not
    # change it unless the host opts in with TW_SET_HW_QUEUES=1 (the applications of this repository -- bench.py, the
    # executor's command line -- export it themselves before anything touches the device).
    if os.environ.get("TW_SET_HW_QUEUES", "0") not in ("", "0"):
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    if not os.path.exists(path):
        raise ImportError(
            "traceweaver_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.tw_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    lib.tw_destroy.argtypes = [vp]
    lib.tw_destroy.restype = None
    lib.tw_last_error.argtypes = [vp]
    lib.tw_last_error.restype = ctypes.c_char_p
    lib.tw_load_batch.argtypes = [vp, ctypes.POINTER(Batch), ctypes.c_int]
    lib.tw_run_pass1.argtypes = [vp]
    lib.tw_get_gaps.argtypes = [vp, vp]
    lib.tw_set_gaps.argtypes = [vp, vp]
    lib.tw_run_baseline.argtypes = [vp, ctypes.c_int, vp]
    lib.tw_wap5_delays.argtypes = [vp, vp, vp, vp]
    lib.tw_wap5_parents.argtypes = [vp, vp, vp, vp]
    lib.tw_device_buffers.argtypes = [vp, ctypes.POINTER(DeviceView)]
    lib.tw_set_gaps_device.argtypes = [vp, vp]
    lib.tw_scale_load.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.tw_set_mixtures.argtypes = [vp, vp, vp]
    lib.tw_run_pass2.argtypes = [vp]
    lib.tw_fit_mixtures.argtypes = [vp]
    lib.tw_fit_mixtures_seeded.argtypes = [vp, vp]
    lib.tw_set_fit_seed.argtypes = [vp, ctypes.c_uint32]
    lib.tw_fit_rows.argtypes = [vp, vp]
    lib.tw_fit_mixtures_tape.argtypes = [vp, vp, ctypes.c_int64, vp]
    lib.tw_get_fit_order.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int32)]
    lib.tw_get_mixtures.argtypes = [vp, vp, vp]
    lib.tw_get_results.argtypes = [vp, ctypes.c_int, ctypes.POINTER(Results)]
    lib.tw_get_gauss_params.argtypes = [vp, vp]
    lib.tw_get_timing.argtypes = [vp, vp, ctypes.c_int32]
    lib.tw_assign_service.argtypes = [vp, ctypes.c_int32, vp, vp, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp,
                                      ctypes.POINTER(Results)]
    lib.tw_find_order.argtypes = [vp, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp]
    lib.tw_order_bound.argtypes = [vp, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.tw_order_stage.argtypes = [vp, ctypes.POINTER(Batch)]
    lib.tw_order_load.argtypes = [vp, ctypes.c_int32, vp, vp]
    lib.tw_set_truth.argtypes = [vp, vp, vp, ctypes.c_int64]
    lib.tw_evaluate.argtypes = [vp, vp, vp, vp]
    lib.tw_measure_hbm_copy.argtypes = [vp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]
    lib.tw_build_distributions.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, ctypes.c_int32, vp, vp]
    lib.tw_set_span_rows.argtypes = [vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp]
    lib.tw_set_parents.argtypes = [vp, vp]
    lib.tw_stitch_traces.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Stitched), vp, vp]
    lib.tw_set_row_groups.argtypes = [vp, ctypes.c_int32, vp]
    lib.tw_attribute_traces.argtypes = [vp, ctypes.POINTER(AttrQuery), ctypes.POINTER(Attribution), vp]
    lib.tw_get_decisions.argtypes = [vp, ctypes.c_int, vp, vp, vp]
    lib.tw_score_traces.argtypes = [vp, ctypes.POINTER(ConfQuery), ctypes.POINTER(Confidence), vp]
    lib.tw_set_row_cohorts.argtypes = [vp, ctypes.c_int32, vp]
    lib.tw_latency_distributions.argtypes = [vp, ctypes.POINTER(DistQuery), ctypes.POINTER(Distributions), vp]
    lib.tw_compare_cohorts.argtypes = [vp, ctypes.POINTER(CmpQuery), ctypes.POINTER(CohortComparison), vp]
    lib.tw_history_reset.argtypes = [vp]
    lib.tw_history_push.argtypes = [vp, ctypes.c_int32, vp, vp]
    lib.tw_history_merge.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp]
    lib.tw_history_info.argtypes = [vp, vp]
    lib.tw_history_distributions.argtypes = [vp, ctypes.POINTER(DistQuery), ctypes.POINTER(Distributions), vp]
    lib.tw_history_compare.argtypes = [vp, ctypes.POINTER(CmpQuery), ctypes.POINTER(CohortComparison), vp]
    lib.tw_class_history_reset.argtypes = [vp]
    lib.tw_class_history_push.argtypes = [vp, ctypes.c_int32, ctypes.c_int64, vp, vp]
    lib.tw_class_history_match.argtypes = [vp, vp, vp]
    lib.tw_class_history_merge.argtypes = [vp, ctypes.POINTER(ClassCatalogue), ctypes.c_int64, vp, vp]
    lib.tw_class_history_info.argtypes = [vp, vp]
    lib.tw_class_history_get.argtypes = [vp, ctypes.POINTER(ClassCatalogue), vp]
    lib.tw_trace_signatures.argtypes = [vp, ctypes.POINTER(SigQuery), ctypes.POINTER(Signatures), vp]
    lib.tw_class_profiles.argtypes = [vp, ctypes.POINTER(ClassProfile), vp]
    lib.tw_filter_traces.argtypes = [vp, ctypes.POINTER(FilterQuery), ctypes.POINTER(FilterResult), vp]
    lib.tw_extract_traces.argtypes = [vp, ctypes.POINTER(ExtractQuery), vp]
    lib.tw_get_extracted.argtypes = [vp, ctypes.POINTER(Extracted)]
    lib.tw_host_alloc.argtypes = [ctypes.c_int64, ctypes.POINTER(vp)]
    lib.tw_host_free.argtypes = [vp]
    lib.tw_host_free.restype = None
    lib.tw_corpus_create.argtypes = [ctypes.POINTER(vp)]
    lib.tw_corpus_destroy.argtypes = [vp]
    lib.tw_corpus_destroy.restype = None
    lib.tw_corpus_last_error.argtypes = [vp]
    lib.tw_corpus_last_error.restype = ctypes.c_char_p
    lib.tw_corpus_add_files.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    lib.tw_corpus_set_callers.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32]
    lib.tw_corpus_counts.argtypes = [vp, vp]
    lib.tw_corpus_string.argtypes = [vp, ctypes.c_int32]
    lib.tw_corpus_string.restype = ctypes.c_char_p
    lib.tw_corpus_loop_origin.argtypes = [vp, ctypes.c_char_p]
    lib.tw_corpus_loop_origin.restype = ctypes.c_char_p
    lib.tw_corpus_trace_names.argtypes = [vp, vp]
    lib.tw_corpus_span_table.argtypes = [vp, ctypes.POINTER(SpanTable)]
    lib.tw_corpus_build_units.argtypes = [vp, ctypes.POINTER(UnitSet)]
    for name in EXPORTS:
        if name not in ("tw_destroy", "tw_last_error", "tw_host_free", "tw_corpus_destroy", "tw_corpus_last_error", "tw_corpus_string", "tw_corpus_loop_origin"):
            getattr(lib, name).restype = ctypes.c_int
    return lib
