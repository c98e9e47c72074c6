"""ctypes binding of libchromegcn_hip.so -- the C ABI in include/chromegcn.h.

There is NO fallback: if the library is missing or a call fails, this raises.  torch is imported
first so that the HIP runtime already mapped by torch (soname libamdhip64.so.7) is the one the
library binds to; streams and device pointers are then interchangeable."""
import ctypes
import os

import torch  # must precede CDLL: shares torch's HIP runtime

from . import _build

_c_int = ctypes.c_int
_c_vp = ctypes.c_void_p
_c_sz = ctypes.c_size_t
_c_float = ctypes.c_float
_c_uint = ctypes.c_uint

# Every function of include/chromegcn.h: (return type, its parameters in header order, by their header names).  A bare
# name is a pointer (c_void_p); "name:t" has the type t of _TYPES ("zp": the size_t * results of
# cgcn_head_workspace_layout).  tests/test_lib_table.py checks this table against the header.
_TYPES = {"i": _c_int, "u": _c_uint, "ll": ctypes.c_longlong, "z": _c_sz, "f": _c_float, "zp": ctypes.POINTER(_c_sz)}
_HEADER = {
    "cgcn_abi_version": (_c_int, ""),
    "cgcn_strerror": (ctypes.c_char_p, "code:i"),
    "cgcn_spmm": (_c_int, "stream n_rows:i n_cols:i S:i d:i rowptr col val row_scale X Y aux"),
    "cgcn_layer_fwd": (_c_int, "stream n:i S:i d:i rowptr col val row_scale X W b wg cg Xn Z H gate dropout_p:f rng_state "
                               "stream_id:u H_in colstats colstats_rows:i aux"),
    "cgcn_layer_fwd_colstats_plan": (_c_int, "n:i S:i d:i mode:i rows_per_tile"),
    "cgcn_debug_set_fwd_split_bytes": (None, "bytes:ll"),
    "cgcn_debug_set_products": (None, "mode:i"),
    "cgcn_debug_get_products": (_c_int, ""),
    "cgcn_debug_layer_fwd_route": (_c_int, "n:i S:i d:i aux colstats_rows:i"),
    "cgcn_debug_layer_bwd_route": (_c_int, "n:i S:i d:i"),
    "cgcn_layer_bwd_workspace_bytes": (_c_sz, "n:i S:i d:i"),
    "cgcn_layer_bwd": (_c_int, "stream n:i S:i d:i rowptr_t col_t val_t row_scale X Z H gate W wg dXn dgate dX dHs dW db dwg "
                               "dcg accumulate:i in_dropout_p:f rng_state in_stream_id:u head workspace workspace_bytes:z "
                               "aux_stream sgd aux_t"),
    "cgcn_debug_layer_bwd_phases": (_c_int, "stream n:i S:i d:i rowptr_t col_t val_t row_scale X Z H gate W wg dXn dgate dX dHs "
                                            "dW db dwg dcg accumulate:i in_dropout_p:f rng_state in_stream_id:u head workspace "
                                            "workspace_bytes:z phases:i aux_t"),
    "cgcn_layer_bwd_co": (_c_int, "stream n:i S:i d:i rowptr_t col_t val_t row_scale X Z H gate W wg dXn dgate dX dHs dW db "
                                  "dwg dcg accumulate:i in_dropout_p:f rng_state in_stream_id:u head workspace "
                                  "workspace_bytes:z aux_stream sgd aux_t companion"),
    "cgcn_debug_layer_bwd_co_route": (_c_int, "n:i S:i d:i rowptr_t col_t val_t have_dX:i aux_t companion"),
    "cgcn_head_workspace_bytes": (_c_sz, "n:i S:i d:i C:i"),
    "cgcn_head_workspace_layout": (_c_int, "n:i S:i d:i C:i dym_offset:zp bnc_offset:zp part_offset:zp"),
    "cgcn_head_bwd_partials": (_c_int, "n:i"),
    "cgcn_head_fwd": (_c_int, "stream n:i S:i d:i C:i X bn_w bn_b run_mean run_var num_batches_tracked momentum:f eps:f "
                              "training:i W_out b_out target dropout_p:f rng_state probs loss dpred save_mean save_invstd "
                              "workspace workspace_bytes:z"),
    "cgcn_head_logits": (_c_int, "stream n:i S:i d:i C:i X bn_w bn_b run_mean run_var eps:f W_out b_out logits"),
    "cgcn_head_train": (_c_int, "stream n:i S:i d:i C:i X bn_w bn_b run_mean run_var num_batches_tracked momentum:f eps:f "
                                "W_out b_out target dropout_p:f rng_state probs loss save_mean save_invstd col_stats "
                                "col_stats_tiles:i col_stats_rows:i workspace workspace_bytes:z"),
    "cgcn_debug_head_train_phases": (_c_int, "stream n:i S:i d:i C:i X bn_w bn_b run_mean run_var num_batches_tracked "
                                             "momentum:f eps:f W_out b_out target dropout_p:f rng_state probs loss save_mean "
                                             "save_invstd col_stats col_stats_tiles:i col_stats_rows:i workspace "
                                             "workspace_bytes:z phases:i"),
    "cgcn_head_bwd": (_c_int, "stream n:i S:i d:i C:i X bn_w bn_b save_mean save_invstd W_out dpred dloss dropout_p:f "
                              "rng_state dX dW_out db_out dbn_w dbn_b accumulate:i workspace workspace_bytes:z"),
    "cgcn_sddmm": (_c_int, "stream n:i S:i d:i rowptr col A B out accumulate:i"),
    "cgcn_saliency_normalize": (_c_int, "stream n:i rowptr val raw out"),
    "cgcn_graph_count": (_c_int, "stream n:i adj_type:i rowptr_in col_in val_in row_counts rowptr_out"),
    "cgcn_graph_fill": (_c_int, "stream n:i adj_type:i rowptr_in col_in val_in rowptr_out col_out val_out row_scale "
                                "symmetric_flag"),
    "cgcn_metrics_workspace_bytes": (_c_sz, "n:ll C:i"),
    "cgcn_multilabel_metrics": (_c_int, "stream n:ll C:i probs targets fdr_cutoff:f out workspace workspace_bytes:z"),
    "cgcn_multilabel_metrics_nonneg": (_c_int, "stream n:ll C:i probs targets fdr_cutoff:f out bad workspace "
                                               "workspace_bytes:z"),
    "cgcn_sgd_step": (_c_int, "stream count:ll param grad momentum_buf lr:f momentum:f weight_decay:f nesterov:i "
                              "grad_scale:f rng_state"),
    "cgcn_adam_step": (_c_int, "stream count:ll param grad exp_avg exp_avg_sq step n_step:i ticket lr:f beta1:f beta2:f "
                               "eps:f weight_decay:f grad_scale:f rng_state"),
    "cgcn_ablation_prepare": (_c_int, "stream n:i C:i targets label_bits pos_lists pos_ranks pos_counts"),
    "cgcn_ablation_workspace_bytes": (_c_sz, "n_inst:i S:i d:i layers:i"),
    "cgcn_ablation_layer": (_c_int, "stream n:i S:i d:i rowptr col val row_scale X X_inst W b wg cg label_bits C:i pos_list "
                                    "pos_rank n_pos:i cols n_cols:i X_out removed"),
    "cgcn_ablation_head": (_c_int, "stream n:i S:i d:i C:i X X_inst bn_w bn_b run_mean run_var eps:f W_out b_out pos_lists "
                                   "pos_counts label:i n_pos:i cols n_cols:i removed base M"),
    "cgcn_ablation_mask": (_c_int, "stream n:i C:i rowptr col val row_scale label_bits label_i:i label_j:i val_out "
                                   "row_scale_out removed"),
    "cgcn_ablation_reduce": (_c_int, "stream n:i S:i C:i logits pos_lists pos_counts label:i col_label:i removed base M"),
    "cgcn_hic_workspace_bytes": (_c_sz, "M:ll N:i capacity:ll K:ll"),
    "cgcn_hic_count": (_c_int, "stream M:ll pos1 pos2 window_start N:i workspace workspace_bytes:z n_survivors"),
    "cgcn_hic_build": (_c_int, "stream M:ll pos1 pos2 count norm n_bins:ll resolution_bp:i window_start N:i K:ll capacity:ll "
                               "workspace workspace_bytes:z rowptr_out col_out nnz_out n_survivors"),
    "cgcn_hic_up_workspace_bytes": (_c_sz, "M:ll N:i capacity:ll K:ll resolution_bp:i window_bp:i n_window_bins:ll"),
    "cgcn_hic_count_up": (_c_int, "stream M:ll pos1 pos2 window_start N:i resolution_bp:i window_bp:i n_window_bins:ll workspace "
                                  "workspace_bytes:z n_survivors"),
    "cgcn_hic_build_up": (_c_int, "stream M:ll pos1 pos2 count norm n_bins:ll resolution_bp:i window_bp:i n_window_bins:ll "
                                  "window_start N:i K:ll capacity:ll workspace workspace_bytes:z rowptr_out col_out nnz_out "
                                  "n_survivors"),
    "cgcn_hic_count_dist": (_c_int, "stream M:ll pos1 pos2 window_start N:i min_distance_bp:ll workspace workspace_bytes:z "
                                    "n_survivors"),
    "cgcn_hic_build_dist": (_c_int, "stream M:ll pos1 pos2 count norm n_bins:ll resolution_bp:i window_start N:i K:ll "
                                    "capacity:ll min_distance_bp:ll expected n_expected:ll workspace workspace_bytes:z rowptr_out "
                                    "col_out nnz_out n_survivors"),
    "cgcn_hic_count_up_dist": (_c_int, "stream M:ll pos1 pos2 window_start N:i resolution_bp:i window_bp:i n_window_bins:ll "
                                       "min_distance_bp:ll workspace workspace_bytes:z n_survivors"),
    "cgcn_hic_build_up_dist": (_c_int, "stream M:ll pos1 pos2 count norm n_bins:ll resolution_bp:i window_bp:i n_window_bins:ll "
                                       "window_start N:i K:ll capacity:ll min_distance_bp:ll expected n_expected:ll workspace "
                                       "workspace_bytes:z rowptr_out col_out nnz_out n_survivors"),
    "cgcn_hicdist_workspace_bytes": (_c_sz, "M:ll n_bins:ll"),
    "cgcn_hicdist_sums": (_c_int, "stream M:ll pos1 pos2 count norm n_norm:ll resolution_bp:i n_bins:ll workspace "
                                  "workspace_bytes:z raw_out act_out sizes"),
    "cgcn_text_workspace_bytes": (_c_sz, "n_bytes:ll"),
    "cgcn_text_count": (_c_int, "stream text n_bytes:ll workspace workspace_bytes:z n_records"),
    "cgcn_text_parse": (_c_int, "stream text n_bytes:ll M:ll pos1_out pos2_out count_out flags flag_capacity:ll flag_totals "
                                "workspace workspace_bytes:z"),
    "cgcn_tsne_workspace_bytes": (_c_sz, "n:i"),
    "cgcn_tsne_sqdist": (_c_int, "stream n:i d:i ld:i X D"),
    "cgcn_tsne_affinities": (_c_int, "stream n:i ld:i D perplexity:f C beta"),
    "cgcn_tsne_symmetrize": (_c_int, "stream n:i ld:i C P workspace workspace_bytes:z"),
    "cgcn_tsne_gradient": (_c_int, "stream n:i ld:i P Y exaggeration:f grad want_kl:i workspace workspace_bytes:z"),
    "cgcn_tsne_update": (_c_int, "stream n:i Y update gains grad momentum:f learning_rate:f have_kl:i record workspace "
                                 "workspace_bytes:z"),
    "cgcn_curves_workspace_bytes": (_c_sz, "n:ll C:i"),
    "cgcn_curves_count": (_c_int, "stream n:ll C:i probs targets kind:i drop_intermediate:i offsets bad workspace "
                                  "workspace_bytes:z"),
    "cgcn_curves_fill": (_c_int, "stream n:ll C:i offsets capacity:ll tps fps thresholds workspace workspace_bytes:z"),
    "cgcn_curves_cutoff": (_c_int, "stream C:i offsets tps fps thresholds cutoffs"),
    "cgcn_threshold_workspace_bytes": (_c_sz, "n:ll C:i T:i"),
    "cgcn_debug_threshold_route": (_c_int, "n:ll C:i T:i"),
    "cgcn_threshold_counts": (_c_int, "stream n:ll C:i T:i probs targets thresholds pos tp pp exact rows tpsum workspace "
                                      "workspace_bytes:z"),
    "cgcn_hicnorm_workspace_bytes": (_c_sz, "M:ll n_bins:ll"),
    "cgcn_hicnorm_count": (_c_int, "stream M:ll pos1 pos2 count resolution_bp:i n_bins:ll workspace workspace_bytes:z sizes"),
    "cgcn_hicnorm_fill": (_c_int, "stream M:ll pos1 pos2 count resolution_bp:i n_bins:ll capacity:ll workspace "
                                  "workspace_bytes:z rowptr col val vc row_nnz sizes"),
    "cgcn_hicnorm_spmv": (_c_int, "stream n:i rowptr col val mask x p y long_row_nnz:i"),
    "cgcn_hicnorm_kr_state_bytes": (_c_sz, "n:i"),
    "cgcn_hicnorm_kr_step": (_c_int, "stream n:i op:i flag:i parity:i vc row_nnz state state_bytes:z"),
    "cgcn_hicnorm_vector": (_c_int, "stream n:i kind:i vc state out"),
    "cgcn_pairs_parse_workspace_bytes": (_c_sz, "n_bytes:ll"),
    "cgcn_pairs_parse": (_c_int, "stream text n_bytes:ll byte_base:ll names n_chroms:i resolution_bp:i binning:i min_diff:ll keys "
                                 "key_capacity:ll flags flag_capacity:ll totals chunk_totals workspace workspace_bytes:z"),
    "cgcn_pairs_reduce_workspace_bytes": (_c_sz, "n_keys:ll"),
    "cgcn_pairs_reduce": (_c_int, "stream n_keys:ll keys n_chroms:i resolution_bp:i pos1_out pos2_out count_out chrom_offsets "
                                  "n_records workspace workspace_bytes:z"),
    "cgcn_labelstats_workspace_bytes": (_c_sz, "n:i C:i"),
    "cgcn_labelstats_windows": (_c_int, "stream n:i C:i targets workspace workspace_bytes:z label_count labels_hist "
                                        "cooccurrence accumulate:i"),
    "cgcn_labelstats_graph": (_c_int, "stream n:i C:i nnz:ll rowptr col val label_bits label_bits_bytes:z degree_sum "
                                      "contact_pairs n_entries accumulate:i"),
    "cgcn_effects_workspace_bytes": (_c_sz, "n_inst:i S:i d:i layers:i"),
    "cgcn_effects_plan": (_c_int, "stream n:i rowptr_t col_t n_var:i windows counts diag_pos"),
    "cgcn_effects_rows1": (_c_int, "stream n:i S:i d:i rowptr_t col_t val_t row_scale X0 H1 windows alt offsets diag_pos "
                                   "n_var:i own:i n_inst:i H_inst X_inst rows"),
    "cgcn_effects_rows2": (_c_int, "stream n:i S:i d:i rowptr col val row_scale rowptr_t col_t X1 H2 windows offsets diag_pos "
                                   "n_var:i own:i n_inst:i X1_inst H_out X_res"),
    "cgcn_null_graph_workspace_bytes": (_c_sz, "n:i nnz:ll capacity:ll model:i"),
    "cgcn_null_graph": (_c_int, "stream n:i nnz:ll rowptr col model:i seed:ll rounds:i capacity:ll rowptr_out col_out sizes "
                                "workspace workspace_bytes:z"),
    "cgcn_bootstrap_workspace_bytes": (_c_sz, "n:ll C:i R:i"),
    "cgcn_bootstrap_sort": (_c_int, "stream n:ll C:i probs targets order bad workspace workspace_bytes:z"),
    "cgcn_bootstrap_weights": (_c_int, "stream n:ll rep0:ll R:i n_strata:i offsets block:i draws:ll seed:ll tile flags workspace "
                                       "workspace_bytes:z"),
    "cgcn_bootstrap_weights_in": (_c_int, "stream n:ll R:i weights tile flags"),
    "cgcn_bootstrap_sums": (_c_int, "stream n:ll C:i R:i order tile fdr_cutoff out"),
    "cgcn_hicinsul_sums": (_c_int, "stream n:i rowptr col val norm n_norm:ll n_windows:i windows out"),
    "cgcn_hiccomp_dense": (_c_int, "stream n:i rowptr col val norm n_norm:ll rank m:i ld:i B"),
    "cgcn_hiccomp_dist_sums": (_c_int, "stream n:i m:i ld:i B keep rank dsum"),
    "cgcn_hiccomp_oe_rows": (_c_int, "stream m:i ld:i B keep e n_e:i ignore_diags:i stages:i mean ss"),
    "cgcn_hiccomp_corr": (_c_int, "stream m:i ld:i Z C"),
    "cgcn_hiccomp_step": (_c_int, "stream m:i C v prev n_prev:i y v_next rec"),
    "cgcn_hicloops_band": (_c_int, "stream n:i rowptr col val width:i band"),
    "cgcn_hicloops_pass1": (_c_int, "stream n:i D:i width:i band vc norm n_norm:ll expected n_expected:ll p:i w:i ignore_diags:i "
                                    "min_dist:i bounds n_chunks:i W:i hist flags lambda_out"),
    "cgcn_hicloops_workspace_bytes": (_c_sz, "n:i D:i"),
    "cgcn_hicloops_count": (_c_int, "stream n:i D:i width:i band flags thr n_chunks:i W:i workspace workspace_bytes:z total"),
    "cgcn_hicloops_write": (_c_int, "stream n:i D:i width:i band vc norm n_norm:ll expected n_expected:ll p:i w:i ignore_diags:i "
                                    "flags thr n_chunks:i W:i capacity:ll workspace workspace_bytes:z pix_ij pix_val"),
    "cgcn_pileup_values": (_c_int, "stream n:i width:i band vc norm n_norm:ll expected n_expected:ll kind:i vband"),
    "cgcn_pileup_workspace_bytes": (_c_sz, "n_slices:ll w:i"),
    "cgcn_pileup_slices": (_c_int, "stream n:i width:i vband w:i n_slices:ll slice_off n_centres:ll ci cj workspace "
                                   "workspace_bytes:z"),
    "cgcn_pileup_fold": (_c_int, "stream n_groups:i w:i n_slices:ll group_off workspace workspace_bytes:z P N"),
    "cgcn_mapcmp_smooth": (_c_int, "stream n:i D:i h:i width:i band norm n_norm:ll ld:i S"),
    "cgcn_mapcmp_workspace_bytes": (_c_sz, "n:i D:i"),
    "cgcn_mapcmp_sums": (_c_int, "stream n:i D:i ld:i Sa Sb valid min_dist:i pass_no:i workspace workspace_bytes:z cells stats"),
}
_ABI = {fn: (res, tuple((p.partition(":")[0], _TYPES[p.partition(":")[2]] if ":" in p else _c_vp) for p in spec.split()))
        for fn, (res, spec) in _HEADER.items()}   # name: (restype, ((parameter name, ctypes type), ...))
_SIGNATURES = {fn: (res, [t for _, t in params]) for fn, (res, params) in _ABI.items()}   # name: (restype, argtypes)
# what query() needs per function, worked out once: the parameter names in order, the positions of the pointers and
# whether it takes a stream
_PLANS = {fn: (tuple(p for p, _ in params), tuple(i for i, (_, t) in enumerate(params) if t in (_c_vp, _TYPES["zp"])),
               any(p == "stream" for p, _ in params))
          for fn, (_, params) in _ABI.items()}
ABI_VERSION = 26
COLSTATS_RECORDS, COLSTATS_ACCUMULATE = 0, 1   # include/chromegcn.h: CGCN_COLSTATS_*
CURVE_ROC, CURVE_PR = 0, 1   # include/chromegcn.h: CGCN_CURVE_*
COLSTATS_ROWS_ACCUMULATE, COLSTATS_ROWS_ZERO_ONLY, COLSTATS_ROWS_ACCUMULATE_ZEROED = -1, -2, -3   # CGCN_COLSTATS_ROWS_*
_lib = None


class ChromeGCNLibraryError(RuntimeError):
    pass


def exported_symbols():
    return sorted(_SIGNATURES)


def load(build_if_missing=False):
    """Load (once) and return the ctypes handle.  Raises ChromeGCNLibraryError if the library is missing or was
    built from different sources than the tree holds.  Never compiles: building is explicit
    (`python -m chromegcn_amd._build` / `__graft_entry__.build()`), because this may run in a process that has
    already initialised the GPU, under a profiler, or as one of N ranks (chromegcn_amd/_build.py).
    `build_if_missing` is accepted for old callers and ignored."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("CHROMEGCN_LIB") or _build.LIB  # override: tuning experiments load a variant build
    if not os.path.exists(path):
        raise ChromeGCNLibraryError(
            "chromegcn_amd: %s is missing -- build it first: python -m chromegcn_amd._build (or "
            "__graft_entry__.build()).  There is no CPU/torch fallback for the HIP path." % path)
    if path == _build.LIB and _build.is_stale():
        raise ChromeGCNLibraryError(
            "chromegcn_amd: %s is stale (sources changed since it was built) -- rebuild: "
            "python -m chromegcn_amd._build" % path)
    _lib = open_library(path)
    return _lib


def open_library(path):
    """ctypes handle of the library at `path` with every signature of include/chromegcn.h set (not cached: tuning
    tools open a variant build beside the in-tree one)."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ChromeGCNLibraryError("chromegcn_amd: symbol %s missing from %s" % (name, path)) from e
        fn.restype = res
        fn.argtypes = args
    got = lib.cgcn_abi_version()
    if got != ABI_VERSION:
        raise ChromeGCNLibraryError("chromegcn_amd: ABI version %d != expected %d; rebuild" % (got, ABI_VERSION))
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().cgcn_strerror(rc).decode()
        raise RuntimeError("chromegcn_amd: %s failed: %s (code %d)" % (what, msg, rc))


def query(fn, **args):
    """Call the entry point `fn` with every parameter given by its header name; returns what it returns.  A pointer
    parameter takes a tensor (its data pointer), None (NULL), an int (an address), or a ctypes Structure or out-parameter
    (passed by reference).  `stream` defaults to torch's current stream."""
    names, pointers, has_stream = _PLANS[fn]
    if has_stream and "stream" not in args:
        args["stream"] = stream_ptr()
    try:
        vals = list(map(args.__getitem__, names))
    except KeyError as e:
        raise TypeError("%s: missing argument %s" % (fn, e.args[0])) from None
    if len(args) != len(names):
        raise TypeError("%s: unknown argument(s) %s" % (fn, ", ".join(sorted(set(args) - set(names)))))
    for i in pointers:   # the eager path makes ~8 of these calls per chromosome step: plain tensors take the short way
        v = vals[i]
        if v.__class__ is torch.Tensor:
            vals[i] = v.data_ptr()
        elif v is not None and v.__class__ is not int:
            vals[i] = v.data_ptr() if isinstance(v, torch.Tensor) else ctypes.byref(v)
    return getattr(load(), fn)(*vals)   # `args` keeps every tensor and struct alive until the call has returned


def call(fn, **args):
    """query() for an entry point that returns a status: raises unless it is CGCN_OK"""
    check(query(fn, **args), fn)


def _workspace(nbytes, device, what):
    if nbytes == 0:
        raise RuntimeError("chromegcn_amd: %s: unsupported shape" % what)
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


def workspace_for(fn, device, what, **sizes):
    """(uint8 workspace, its size in bytes) for the sizes the `*_workspace_bytes` function `fn` takes; `what` names the
    call in the unsupported-shape error"""
    nbytes = query(fn, **sizes)
    return _workspace(nbytes, device, what), nbytes


def head_workspace(n, S, d, C, device):
    """the uint8 workspace of cgcn_head_fwd / cgcn_head_train / cgcn_head_bwd"""
    return _workspace(query("cgcn_head_workspace_bytes", n=n, S=S, d=d, C=C), device,
                      "fused head, S=%d n=%d d=%d C=%d" % (S, n, d, C))


def layer_bwd_workspace(n, S, d, device):
    """the uint8 workspace of cgcn_layer_bwd"""
    return _workspace(query("cgcn_layer_bwd_workspace_bytes", n=n, S=S, d=d), device,
                      "layer backward, S=%d n=%d d=%d" % (S, n, d))


class HeadGrad(ctypes.Structure):
    """mirror of cgcn_head_grad (include/chromegcn.h)"""
    _fields_ = [("dym", _c_vp), ("bnc", _c_vp), ("save_mean", _c_vp), ("save_invstd", _c_vp), ("bn_w", _c_vp),
                ("dropout_p", _c_float), ("rng_state", _c_vp), ("part", _c_vp), ("n_partials", _c_int), ("C", _c_int),
                ("dW_out", _c_vp), ("db_out", _c_vp), ("accumulate", _c_int), ("dloss", _c_vp), ("dbn_w", _c_vp),
                ("dbn_b", _c_vp), ("stat_acc", _c_vp)]


class SgdFuse(ctypes.Structure):
    """mirror of cgcn_sgd_fuse (include/chromegcn.h)"""
    _fields_ = [("param", _c_vp), ("grad", _c_vp), ("momentum_buf", _c_vp), ("count", ctypes.c_longlong),
                ("lr", _c_float), ("momentum", _c_float), ("weight_decay", _c_float), ("grad_scale", _c_float),
                ("nesterov", _c_int), ("rng_state", _c_vp)]


class SpmmJob(ctypes.Structure):
    """mirror of cgcn_spmm_job (include/chromegcn.h)"""
    _fields_ = [("n", _c_int), ("S", _c_int), ("d", _c_int), ("rowptr", _c_vp), ("col", _c_vp), ("val", _c_vp),
                ("row_scale", _c_vp), ("X", _c_vp), ("H", _c_vp), ("aux", _c_vp)]


def ptr(t):
    """device pointer of a tensor (or None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


_aux_streams = {}


def aux_stream_ptr():
    """a per-device side stream for cgcn_layer_bwd's concurrent partial reduction.  OFF by default: measured on
    MI355X (chr21-like step, HIP graph) the fork/join edges cost more than the 7.5 us reduction they hide
    (0.295 ms with, 0.277 ms without).  CHROMEGCN_AUX_STREAM=1 turns it on."""
    if not os.environ.get("CHROMEGCN_AUX_STREAM"):
        return None
    dev = torch.cuda.current_device()
    s = _aux_streams.get(dev)
    if s is None:
        s = _aux_streams[dev] = torch.cuda.Stream(device=dev)
    return s.cuda_stream
