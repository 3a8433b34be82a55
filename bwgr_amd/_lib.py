"""ctypes binding of libbwgr_hip.so (include/bwgr.h).  Fails loudly: there is no CPU fallback."""
import ctypes as C
import os
import sys

from . import build as _build

_lib = None

c_f = C.POINTER(C.c_float)
c_d = C.POINTER(C.c_double)
P, vp, i64, u64, u32, i32, f32, f64 = C.POINTER, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint32, C.c_int, C.c_float, C.c_double

# The C ABI of include/bwgr.h, in the header's order: name -> argtypes (tests/test_abi_table_cpu.py holds the two against each other).
# A prototype's `T *` and `T x[N]` are pointers here; handles and untyped buffers are void pointers.
ABI = {
    "bwgr_abi_version": [],
    "bwgr_last_error": [],
    "bwgr_device_count": [P(i32)],
    "bwgr_panel_create": [P(vp), vp, i32, i32, i64, i64, i64, i32, i32, i32],
    "bwgr_panel_destroy": [vp],
    "bwgr_panel_set_stream": [vp, vp],
    "bwgr_panel_clone": [P(vp), vp],
    "bwgr_panel_max_concurrent": [vp, i32, P(i32)],
    "bwgr_panel_max_pairs": [vp, P(i32)],
    "bwgr_debug_occupancy_fits": [i32, i32, i32, i32, P(i32)],
    "bwgr_debug_stream3_dma": [i64, i64],
    "bwgr_debug_sweep3_kernel": [vp, P(i32)],
    "bwgr_panel_info": [vp, P(i64)],
    "bwgr_panel_pipeline": [vp, i32, P(i32)],
    "bwgr_panel_stats": [vp, c_f, c_f, c_f],
    "bwgr_kmup": [vp, c_f, c_f, c_f, c_f, c_f, f32, f32, u64, u32, i32],
    "bwgr_kmup2": [vp, P(i32), i64, c_f, c_f, c_f, c_f, c_f, c_f, f32, f32, u64, u32, i32],
    "bwgr_chain_create": [P(vp), vp, i32, vp, i32, f32, f32, f32, f32, f32, u64, i32],
    "bwgr_chain_destroy": [vp],
    "bwgr_chain_run": [vp, i32],
    "bwgr_chain_run_pair": [vp, vp, i32],
    "bwgr_chain_sync": [vp],
    "bwgr_chain_iterations": [vp, P(i32)],
    "bwgr_chain_result": [vp] + [c_f] * 10,
    "bwgr_chain_state": [vp] + [c_f] * 5,
    "bwgr_chain_sweep_ms": [vp, c_f, P(i32)],
    "bwgr_chain_redo_count": [vp, P(i32)],
    "bwgr_chain_create_sharded": [P(vp), vp, i32, vp, i32, f32, f32, f32, f32, f32, u64, i32, i64, i64, f32, vp],
    "bwgr_chain_sweep_blocks": [vp, i32, i32],
    "bwgr_chain_round_sweep": [vp, i32, i32, vp],
    "bwgr_chain_get_sums_dev": [vp, vp],
    "bwgr_chain_end_iteration_dev": [vp, vp],
    "bwgr_chain_round_apply": [vp, vp],
    "bwgr_chain_get_sums": [vp, c_d],
    "bwgr_chain_end_iteration": [vp, c_d],
    "bwgr_bayes": [vp, i32, c_f, f32, f32, f32, f32, f32, u64, i32] + [c_f] * 10,
    "bwgr_bayes2": [vp, vp, i32, c_f, f32, f32, f32, f32, f32, u64, i32] + [c_f] * 10,
    "bwgr_sample_rows": [u64, u32, i64, i64, i32, P(i32)],
    "bwgr_wgr": [vp, c_d, i32, i32, i32, i32, i32, f64, f64, f64, u64, i32] + [c_d] * 7,
    "bwgr_wgr_ex": [vp, c_d, i32, i32, i32, i32, i32, f64, f64, f64, u64, i32, c_d, c_d, i64, f64, i32] + [c_d] * 9,
    "bwgr_em": [vp, i32, c_f, f32, f32, f32, c_f, i32, P(f32), c_f, c_f, c_f, c_f, c_f, P(i32)],
    "bwgr_em_order": [i64, i32, P(i32)],
    "bwgr_mrr": [vp, c_d, i32, c_d, i32] + [c_d] * 11 + [P(i32)],
    "bwgr_debug_mrr_plan": [i32, i32, P(i32), P(i32), P(i64), P(i64)],
    "bwgr_mrr_dense": [i32, vp, i32, i64, i64, i64, c_d, i32, c_d, i32] + [c_d] * 11 + [P(i32)],
    "bwgr_debug_mrr_dense_plan": [i64, i64, i32, i32, P(i64)],
    "bwgr_mrr_svd_fit": [i32, vp, i32, i64, i64, i64, c_d, i32, i32, f64, i32] + [c_d] * 10 + [P(i32)],
    "bwgr_panel_xta": [vp, vp, i64, i64, i32, i32, vp, i64],
    "bwgr_debug_xta_plan": [i64, i64, i64, i64, P(i64)],
    "bwgr_project": [i32, vp, vp, i32, i64, i64, i64, c_d, i64, i64, vp, i32, i64],
    "bwgr_mlm": [i32, vp, vp, i32, i64, i64, i64, c_d, i64, i64, c_d, i32, i32, f64, f64, i32] + [c_d] * 8 + [P(i32)],
    "bwgr_debug_mlm_plan": [i64, i64, i64, i32, i32, P(i64)],
    "bwgr_debug_project_timing": [i32, c_d],
    "bwgr_uvbeta": [vp, c_d, i64, i32, i32, f64, f64, c_d, c_d, c_d, c_d, c_d, P(i32), c_d, c_d],
    "bwgr_debug_uvb_plan": [i64, i64, i64, P(i64)],
    "bwgr_uvbeta_dense": [i32, c_d, i64, i64, i64, c_d, i64, i32, i32, f64, f64, c_d, c_d, c_d, c_d, c_d, P(i32), c_d],
    "bwgr_debug_uvbd_plan": [i64, i64, i64, P(i64)],
    "bwgr_uvbeta2": [vp, c_d, i64, i64, c_d, i64, i32, f64, f64, c_d, c_d, c_d, c_d, c_d, c_d, c_d, P(i32), c_d],
    "bwgr_pegs": [i32, vp, i32, c_d, i64, i32, i32, f64, f64, f64, i32, i32, i32, c_d, vp, c_d, c_d, vp, c_d, P(i32), c_d],
    "bwgr_pegs_ex": [i32, vp, i32, c_d, i64, i32, i32, f64, f64, f64, i32, i32, i32, c_d, vp, c_d, c_d, vp, c_d, P(i32), c_d],
    "bwgr_debug_pegs_sparse_plan": [i64, i64, i64, i64, i32, i32, P(i64)],
    "bwgr_debug_pegs_plan": [i64, i64, i32, P(i64)],
    "bwgr_pegsx": [i32, vp, i32, c_d, i64, i32, c_d, i64, i32, i32, f64, f64, f64, f64, i32, i32, i32, i32, i32, c_d, c_d, vp, vp, vp, c_d, c_d, P(i32), c_d, c_d],
    "bwgr_pegsx_ex": [i32, vp, i32, c_d, i64, i32, c_d, i64, i32, i32, f64, f64, f64, f64, i32, i32, i32, i32, i32, c_d, c_d, vp, vp, vp, c_d, c_d, P(i32), c_d, c_d],
    "bwgr_debug_pegsx_plan": [i64, i32, i32, P(i64)],
    "bwgr_debug_pegs_launch_plan": [i64, i64, P(i64)],
    "bwgr_debug_pegsx_timing": [i32, c_d],
    "bwgr_panel_xb": [vp, c_d, i64, c_d],
    "bwgr_debug_panel_plan": [i32, i64, i64, i32, i32, i32, i32, i32, P(i64)],
    "bwgr_debug_sweep_plan": [i32, i64, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, P(i64)],
    "bwgr_debug_aux_plan": [i32, i64, i64, P(i64)],
    "bwgr_panel_crossprod": [vp, vp, i64, i32],
    "bwgr_panel_kernel": [vp, i32, f64, i32, vp, i64, i32],
    "bwgr_debug_xxt_plan": [i64, i64, i32, i64, P(i64)],
    "bwgr_panel_crossprod2": [vp, vp, vp, i64, i32],
    "bwgr_panel_kernel2": [vp, vp, i32, f64, vp, i64, vp, i64, i32],
    "bwgr_debug_xyt_plan": [i64, i64, i64, i32, i32, i64, P(i64)],
    "bwgr_synth_genotypes": [vp, i64, i64, i64, i64, u64, vp, i32, vp],
    "bwgr_group_create": [P(vp), i32, P(i32), vp, i32, i64, i64, i64, i32, c_f, i32, f32, f32, f32, f32, f32, u64, i32, i64],
    "bwgr_group_create_centred": [P(vp), i32, P(i32), vp, i32, i64, i64, i64, i32, c_f, i32, f32, f32, f32, f32, f32, u64, i32, i64, i32],
    "bwgr_group_run": [vp, i32],
    "bwgr_group_sync": [vp],
    "bwgr_group_info": [vp, P(i64)],
    "bwgr_group_sound": [vp, P(i32)],
    "bwgr_panel_centred": [vp, P(i32)],
    "bwgr_panel_set_centred": [vp, i32],
    "bwgr_group_result": [vp] + [c_f] * 10,
    "bwgr_group_destroy": [vp],
    "bwgr_debug_variates": [i32, u64, i32, f64, u32, u32, u32, i32, c_d],
    "bwgr_debug_withhold": [vp, i32],
    "bwgr_debug_last_redo": [P(i32)],
    "bwgr_debug_launch_plan": [i64, i64, i64, i64, P(i64)],
    "bwgr_debug_live": [P(i64)],
}
RESTYPE = {"bwgr_last_error": C.c_char_p}      # every other entry returns int
EXPORTS = list(ABI)


class BwgrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bwgr status %d: %s" % (code, msg))
        self.code = code


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if not os.path.exists(path):
        raise ImportError("libbwgr_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `python -m bwgr_amd.build`); bwgr_amd has no CPU fallback")
    # PyTorch bundles its own HIP runtime; if this library loads the system one first, a LATER `import torch` in the same process
    # finds "No HIP GPUs".  A caller that uses both imports torch first (bench.py, bwgr_amd.dist and bwgr_amd.synth do), or sets
    # BWGR_PRELOAD_TORCH=1 to have it imported here.  The library itself does not need torch.
    if "torch" not in sys.modules and os.environ.get("BWGR_PRELOAD_TORCH", "0") == "1":
        try:
            import torch  # noqa: F401
        except ImportError:   # a box without torch: the library does not need it
            pass
    L = C.CDLL(path)
    for name, argtypes in ABI.items():
        getattr(L, name).argtypes = argtypes
        getattr(L, name).restype = RESTYPE.get(name, C.c_int)
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise BwgrError(rc, lib().bwgr_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    lib().bwgr_device_count(C.byref(n))
    return n.value

