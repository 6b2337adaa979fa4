"""The library's dispatch options (PN2_OPTION_LIST of csrc/pn2_common.h) as the tests see them: the header's table parsed
without loading the library, an ``options(...)`` context manager, and LEDGER -- for EVERY option, where the kernels its
non-default values route to are checked.  tests/test_options_cpu.py holds the ledger to the header: an option cannot be
added (or dropped) without saying here where its alternative route is tested.

A ledger value is one of
  * a list of (value, test id) pairs: the test sets the option to that value and checks the result against a reference
    (a value of the form "a vs b" names the two settings one test compares);
  * ("threshold", test id): the option is a row / tile count at which one kernel family hands over to another; the test
    moves it, or runs at the value it reads from the library, so that both sides of the hand-over run;
  * "bit-equal pair tested in <test id>": both settings give the same bits, and that test says so.
A test id is "<module>::<function>" (parametrised cases are not spelled out).  Notes on single entries:
  NOTE_GRID     the option changes the launch grid (or a run-time argument) of the SAME template instantiation, so
                pn2_last_kernel() cannot tell the two settings apart and the test does not assert a name change;
  NOTE_FPS      pn2_fps does not record pn2_last_kernel(): that the route is taken rests on the dispatch code of
                csrc/geometry.hip (pn2_fps, launch_fps_pruned, fps_coop_plan), not on an assertion.
"""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pointnet12_amd", "csrc", "pn2_common.h")


def header_options(path=HEADER):
    """[(name, default text)] of PN2_OPTION_LIST in the order of the header; names without the PN2_ prefix."""
    text = open(path).read()
    m = re.search(r"#define PN2_OPTION_LIST\(X\)((?:[^\n]*\\\n)*[^\n]*\n)", text)
    assert m, "PN2_OPTION_LIST not found in %s" % path
    return re.findall(r"\bX\(\s*(\w+)\s*,\s*([^)]*?)\s*\)", m.group(1))


def header_defaults(path=HEADER):
    """{"PN2_<NAME>": default} as _lib.options() spells the names."""
    return {"PN2_" + name: int(value) for name, value in header_options(path)}


class options:
    """``with options(PN2_NAME=value, ...):`` library options for the block, restored afterwards (also when it raises)."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        from pointnet12_amd import _lib
        self.old = {k: _lib.options()[k] for k in self.values}
        for k, v in self.values.items():
            _lib.set_option(k, v)
        return self

    def __exit__(self, *exc):
        from pointnet12_amd import _lib
        for k, v in self.old.items():
            _lib.set_option(k, v)
        return False


NOTE_GRID = "grid only: same instantiation, no kernel-name assertion"
NOTE_FPS = "route by the dispatch code, not asserted (pn2_fps records no kernel name)"

_MLP, _GEO = "test_options_mlp_gpu", "test_options_geometry_gpu"
_NT = _MLP + "::test_few_row_nt_options_forward_and_data_gradient"
_TN = _MLP + "::test_tn_options_on_the_streamed_weight_gradient"
_WIDE = _MLP + "::test_wide_and_resident_options_at_their_row_thresholds"
_TWO = _MLP + "::test_two_phase_weight_gradient_flush_through_caller_scratch"
_SEAMS = "test_mlp_seams_gpu"
_CF = "test_mlp_cf_seams_gpu"

LEDGER = {
    # ---- csrc/geometry.hip
    "FPS_ROWS_MIN_PPT": [(16, _GEO + "::test_fps_rows_kernel_below_its_default_hand_over"),
                         (29, _GEO + "::test_fps_wave_level_pruned_kernel_above_its_default_hand_over"), NOTE_FPS],
    "FPS_ROWMAP": [(0, _GEO + "::test_fps_row_ownership_maps"), (1, _GEO + "::test_fps_row_ownership_maps"),
                   (2, _GEO + "::test_fps_row_ownership_maps"), NOTE_FPS],
    "FPS_SINGLE_MAX": [(28672, _GEO + "::test_fps_single_workgroup_kernel_at_28_points_per_thread"),
                       (16384, _GEO + "::test_fps_three_workgroup_cooperative_plan"), NOTE_FPS],
    "FPS_PIECE": [(1, _GEO + "::test_fps_sampling_chain_in_pieces"), (64, _GEO + "::test_fps_sampling_chain_in_pieces"),
                  (100, _GEO + "::test_fps_sampling_chain_in_pieces"), NOTE_FPS],
    "FPS_COOP": [(0, _GEO + "::test_fps_large_kernel_with_the_cooperative_plan_off"), NOTE_FPS],
    "FPS_PRUNE": [(0, _GEO + "::test_fps_single_workgroup_kernel_at_28_points_per_thread"),
                  (2, "test_geometry_gpu::test_fps_spatially_pruned_kernel_small_clouds_forced"), NOTE_FPS],
    "BQ_ORDER": [(0, "test_geometry_edges_gpu::test_ball_query_ordered_centres_batch_and_ragged")],
    # ---- csrc/mlp.hip, NT
    "FEWROW_MAX_TILES": [(0, _NT)],
    "FEWROW_MAX_TILES_DGRAD": [(0, _NT)],
    # (values outside {1, 2, 4} are left out: launch_fewrow sizes the grid by tiles * ks / 4 and falls to the one-wave kernel
    # for any other ks, which then leaves tiles uncomputed or runs past the last one)
    "FEWROW_KS": [(1, _NT), (2, _NT)],
    "NT_CFG": [(7, _NT), (8, _NT), (9, _MLP + "::test_nt_cfg_9_sends_96_columns_to_the_128_wide_tile")],
    "NT_SMALL_DEPTH": [(2, _NT), (3, _NT), (4, _NT)],
    "NT_NSPLIT": [(0, _MLP + "::test_nt_nsplit_off_runs_196_columns_in_one_launch")],
    # ---- csrc/mlp.hip, TN
    "TN_SPLITDIV": [(2, _TN), (8, _TN), NOTE_GRID],
    "TN_CFG": [(1, _TN), (3, _TN)],
    "TN_NARROW": [(0, _TN)],
    "TN_SMALLP": ("threshold", _TN),
    "TN_SMALL_DEPTH": [(1, _TN), (3, _TN)],
    "CF_WGS_PER_CU": [(1, _MLP + "::test_closed_form_first_layer_weight_gradient_workgroups_per_cu"),
                      (4, _MLP + "::test_closed_form_first_layer_weight_gradient_workgroups_per_cu"), NOTE_GRID],
    "WGRAD_SKINNY": [(0, _MLP + "::test_first_layer_weight_gradient_without_the_skinny_kernel")],
    "BWD_PAIR": [(0, _MLP + "::test_bwd_pair_in_one_launch_and_in_two_vs_fp64")],
    # ---- csrc/mlp_res.hip, csrc/mlp_wide.hip
    "RES": [(0, _WIDE), (0, _MLP + "::test_res_off_hands_the_fused_backward_to_the_streamed_pair")],
    "RES_MIN_ROWS": ("threshold", _SEAMS + "::test_forward_at_the_row_thresholds_and_ragged_tails"),
    "RES_HALF": [(0, _MLP + "::test_fused_backward_as_one_eight_wave_workgroup_per_cu")],
    "WIDE": [(0, _WIDE)],
    "WIDE_MIN_ROWS": ("threshold", _SEAMS + "::test_forward_at_the_row_thresholds_and_ragged_tails"),
    "SPLIT": [(0, _SEAMS + "::test_forward_of_the_fp32_register_stationary_kernel_with_a_ragged_tail"), (0, _WIDE)],
    "SPLIT_WGRAD": [(0, _WIDE)],
    "SPLIT_K256": [(0, _WIDE)],
    "SPLIT_NARROW": [(0, "test_mlp_gpu::test_pool_in_gemm_epilogue_equals_the_pooling_pass")],
    "SPLIT_RES": [(0, "test_mlp_gpu::test_bf16_split_kernels_against_the_fp32_pipe"), (2, _WIDE)],
    "FUSE_FIRST": [("0 vs 1", "test_mlp_gpu::test_shared_mlp_with_the_fused_first_layer_option"),
                   (1, _CF + "::test_fused_backward_with_the_first_layers_sums_at_its_seams")],
    "SPLIT_WG2": [(0, "test_geometry_gpu::test_fps_beside_the_pooled_split_forward_is_index_exact"), NOTE_GRID],
    "POOL_CF": [(0, "test_mlp_gpu::test_fused_backward_kernel_vs_fp64_on_fixed_operands"),
                (1, _CF + "::test_pooled_backward_from_the_input_with_pool_cf_1_takes_128x96_only"),
                (2, "test_mlp_gpu::test_shared_mlp_negative_and_zero_gamma"), (2, _CF + "::test_pooled_backward_from_the_input_at_its_seams")],
    "SPLIT_RES_MIN_TILES_128": ("threshold", _SEAMS + "::test_fused_backward_with_a_ragged_tail"),
    "SPLIT_MIN_ROWS_128": ("threshold", _SEAMS + "::test_forward_at_the_row_thresholds_and_ragged_tails"),
    "RING": "bit-equal pair tested in test_mlp_gpu::test_ring_forward_option_is_bit_equal",
    "WIDE_POOL": [(0, _MLP + "::test_wide_pool_off_makes_the_pooled_forward_refuse")],
    "WIDE_ADB196": [(0, _WIDE)],
    "WIDE_WGRAD": [(0, _WIDE)],
    "WIDE_WGRAD_MIN_ROWS": ("threshold", _SEAMS + "::test_wide_dgrad_and_wgrad_at_the_row_thresholds_and_ragged_tails"),
    "WGRAD_TWO_PHASE": [(1, _TWO), NOTE_GRID],
    "WGRAD_TWO_PHASE_ALL": [(1, _TWO), NOTE_GRID],
    # ---- csrc/scatter.hip, csrc/voxel_reduce.hip
    "SEG_CHUNK": [(16, "test_scatter_gpu::test_interp_bwd_constructed")],
    "SEGRED_COMBINE": [(0, "test_voxel_reduce_gpu::test_every_form_of_the_row_passes_against_the_restatement")],
    "SEGRED_LANES": [(0, "test_voxel_reduce_gpu::test_every_form_of_the_row_passes_against_the_restatement")],
}


def ledger_test_ids(ledger=LEDGER):
    """Every "<module>::<function>" the ledger names."""
    out = set()
    for value in ledger.values():
        if isinstance(value, str):
            out.update(re.findall(r"\b(test_\w+::test_\w+)", value))
        elif isinstance(value, tuple):
            if value[0] == "threshold":
                out.add(value[1])
        else:
            out.update(item[1] for item in value if isinstance(item, tuple))
    return out
