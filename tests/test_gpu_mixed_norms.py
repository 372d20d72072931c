"""GPU: every flow that forms or applies exp(G_t) on pulses whose slices differ widely in norm (tests/mixed_norm_cases.py):
within ONE pulse the squaring count (matrix flows: Taylor-8, s = squarings_for(bound)) or the Taylor degree and piece count
(vector flow) runs over its whole range, jumps between neighbouring slices, differs between slice t and its mirror N-1-t, and
an all-zero control column sits between two top-level slices -- the state a wave carries around the variable-length part
(prefetches, hazard padding, LDS images, the producer/consumer hand-over, the plan shared by the forward and the backward chain,
one s per packed tile, lanes of one wave with different s) is exercised the way a real pulse does.

One table, one row per flow; each row forces its flow with the knobs of that flow's own test file and asserts through
eng.info and eng.kernel_names() that the intended kernel ran.  Per row: every member's (F_k, g_k) and the ensemble (F, G)
against the oracle at PARITY_RTOL, a second evaluation bitwise, and -- where the flow forms propagators -- the last member's
P_t slice by slice against the oracle's at 1e-11 max(1, |P_ref|_inf) (asserted for Hermitian generators, printed otherwise).
Two cross-checks without a reference: the norm-chosen s against a uniform sufficient one (expm_squarings = s_top + 1) and
the time-reversed ramp.  test_mixed_norms_host.py proves, without a GPU, that the inputs of every row have the spread,
asymmetry and zeros claimed here and that the two CPU references agree on them three orders inside the bar."""
import functools

import numpy as np
import pytest

from conftest import assert_parity
import mixed_norm_cases as mn

pytestmark = pytest.mark.gpu

KNOBS = ("GRAPE_SMALL_KERNEL", "GRAPE_PAIR_VEC", "GRAPE_EXACT_W1", "GRAPE_HOIST", "GRAPE_HOIST2", "GRAPE_FORCE_FUSE",
         "GRAPE_NO_FUSE", "GRAPE_SPLIT_EXPM", "GRAPE_NO_TP", "GRAPE_NO_THIN", "GRAPE_TP_CHUNKS", "GRAPE_ACTION",
         "GRAPE_ACT_WHOLE", "GRAPE_THIN_DPP", "GRAPE_DPP_CHUNKS", "GRAPE_NO_COOP", "GRAPE_GRID", "GRAPE_CTRL_SCALE",
         "GRAPE_ACTION_MIN", "GRAPE_TILE_SPLIT_PERMILLE", "GRAPE_NO_SPARSE", "GRAPE_MAX_WORKSPACE_BYTES")

UG, ST, CT = "UnitaryGate", "StateTransfer", "CoherenceTransfer"
ROWS = {}


def row(rid, n, K, N, E, sys_type, herm, order, seed, *, env=None, flags=(), ekw=None, variants=(0, 1), mode="eval",
        objectives=("fom",), info=None, kernels=(), absent=(), props=True, forced=False, reverse=False, **case):
    """case: cols, shared_controls, zero_drift_member, rank_one, top_last, distinct_members of mixed_norm_cases.make_case"""
    assert rid not in ROWS, rid
    ROWS[rid] = dict(n=n, K=K, N=N, E=E, sys_type=sys_type, herm=herm, order=order, seed=seed, s_top=7 if herm else 5,
                     env=env or {}, flags=flags, ekw=ekw or {}, variants=variants, mode=mode, objectives=objectives,
                     info=info or {}, kernels=kernels, absent=absent, props=props, forced=forced, reverse=reverse, case=case)


# --- lane kernel, n = 2, 3, 4 (sweep_small.hip; knobs: test_gpu_random_shapes.py): lanes of one wave with different s ------------
LANE = dict(env={"GRAPE_SMALL_KERNEL": "lane"}, ekw={"slices_per_lane": 3}, kernels=("sweep_small_kernel",))
LANE_U = dict(LANE, info={"lane_pair": 0, "kernel_family": 0, "unitary_flow": 1, "slices_per_lane": 3})
LANE_G = dict(LANE, info={"lane_pair": 0, "kernel_family": 0, "unitary_flow": 0, "slices_per_lane": 3})
row("lane-n2-unitary-ramp", 2, 2, 40, 3, UG, True, "ramp", 1, forced=True, reverse=True, **LANE_U)
row("lane-n3-unitary-shuffled", 3, 2, 40, 3, UG, True, "shuffled", 2, **LANE_U)
row("lane-n4-unitary-ramp-zero-drift", 4, 2, 40, 3, UG, True, "ramp", 5, zero_drift_member=True, **LANE_U)
row("lane-n2-general-shuffled", 2, 2, 40, 3, ST, False, "shuffled", 5, **LANE_G)
row("lane-n3-general-ramp", 3, 2, 40, 3, ST, False, "ramp", 2, rank_one=False, **LANE_G)
row("lane-n4-general-shuffled", 4, 2, 40, 3, ST, False, "shuffled", 6, **LANE_G)
row("lane-n4-costates-shuffled", 4, 2, 40, 3, UG, True, "shuffled", 7, flags=("FLAG_KEEP_COSTATES",), **LANE_G)

# --- lane-pair kernel, n = 2, 4 (sweep_pair.hip; test_gpu_random_shapes.py): C3's flow is the first row ---------------------------
PAIR = dict(env={"GRAPE_SMALL_KERNEL": "pair"}, kernels=("sweep_pair_kernel",), absent=("sweep_pair_vec_kernel",))


def pair(W, unitary):
    return dict(PAIR, ekw={"waves_per_member": W}, info={"lane_pair": 1, "kernel_family": 0, "unitary_flow": unitary,
                                                         "waves_per_member": W})


row("pair-n4-unitary-W1-ramp", 4, 2, 65, 5, UG, True, "ramp", 1, forced=True, reverse=True, **pair(1, 1))
row("pair-n4-unitary-W3-shuffled", 4, 2, 65, 5, UG, True, "shuffled", 1, **pair(3, 1))
row("pair-n2-unitary-W3-spikes", 2, 2, 65, 5, UG, True, "spikes", 1, **pair(3, 1))
row("pair-n4-forced-general-W1-shuffled", 4, 2, 65, 5, UG, True, "shuffled", 7, flags=("FLAG_FORCE_GENERAL",), **pair(1, 0))
row("pair-n4-general-W3-ramp", 4, 2, 65, 5, UG, False, "ramp", 6, **pair(3, 0))
row("pair-n4-general-sandwich-W1-spikes", 4, 2, 65, 5, ST, False, "spikes", 1, **pair(1, 0))
row("pair-n2-general-sandwich-W1-shuffled", 2, 2, 65, 5, ST, False, "shuffled", 13, **pair(1, 0))
row("pair-n4-4x1-unitary-W1-ramp", 4, 2, 65, 5, UG, True, "ramp", 14, cols=1, **pair(1, 1))
row("pair-n4-4x2-general-W3-shuffled", 4, 2, 65, 5, UG, False, "shuffled", 6, cols=2, **pair(3, 0))

# --- sweep_pair_vec_kernel (test_gpu_pair_vec.py: 4 x 1 states, non-Hermitian generators; its smallest shape E = 1, N = 55, K = 1) --
row("pair-vec-4x1-shuffled", 4, 1, 55, 1, UG, False, "shuffled", 1, cols=1, kernels=("sweep_pair_vec_kernel",),
    info={"lane_pair": 1, "unitary_flow": 0})

# --- fom fast path (fom_small.hip; test_gpu_fom.py) ----------------------------------------------------------------------------------
FOM = dict(mode="fom", props=False)
row("fom-lane-n3-ramp", 3, 2, 40, 3, UG, True, "ramp", 2, ekw={"slices_per_lane": 3}, kernels=("fom_lane_kernel",), **FOM)
row("fom-lane-n3-general-spikes", 3, 2, 40, 3, ST, False, "spikes", 2, ekw={"slices_per_lane": 3}, kernels=("fom_lane_kernel",), **FOM)
row("fom-lane-n4-general-ramp", 4, 2, 40, 3, ST, False, "ramp", 1, env={"GRAPE_SMALL_KERNEL": "lane"}, ekw={"slices_per_lane": 3},
    kernels=("fom_lane_kernel",), **FOM)
row("fom-pair-n4-spikes", 4, 2, 65, 5, UG, True, "spikes", 1, kernels=("fom_pair_kernel",), **FOM)
row("fom-pair-n4-general-ramp", 4, 2, 65, 5, ST, False, "ramp", 6, kernels=("fom_pair_kernel",), **FOM)

# --- exact gradient, n <= 4 (exact_grad.hip; test_gpu_exact.py): lane, pair W1 flow, pair debug flow ---------------------------------
EX = dict(mode="exact", objectives=("fom", "c1"), props=False)
row("exact-lane-n2-shuffled", 2, 2, 24, 3, UG, True, "shuffled", 1, info={"lane_pair": 0}, kernels=("sweep_small_kernel", "exact_pair_kernel"), **EX)
row("exact-lane-n3-ramp", 3, 2, 24, 3, ST, True, "ramp", 2, info={"lane_pair": 0}, kernels=("sweep_small_kernel", "exact_grad_kernel"), **EX)
row("exact-lane-n4-general-shuffled", 4, 2, 24, 3, ST, False, "shuffled", 1, env={"GRAPE_SMALL_KERNEL": "lane"},
    info={"lane_pair": 0}, kernels=("sweep_small_kernel", "exact_pair_kernel"), **EX)
row("exact-pair-w1-n4-ramp", 4, 2, 24, 3, UG, True, "ramp", 1, variants=(0,), info={"lane_pair": 1, "unitary_flow": 1},
    kernels=("sweep_pair_kernel", "exact_pair_kernel"), **EX)
row("exact-pair-w1-n4-shuffled", 4, 2, 24, 3, UG, True, "shuffled", 1, variants=(0,), info={"lane_pair": 1, "unitary_flow": 1},
    kernels=("sweep_pair_kernel", "exact_pair_kernel"), **EX)
row("exact-pair-debug-n4-ramp", 4, 2, 24, 3, UG, True, "ramp", 3, variants=(0,), env={"GRAPE_EXACT_W1": "0"},
    info={"lane_pair": 1, "unitary_flow": 0}, kernels=("sweep_pair_kernel", "exact_pair_kernel"), **EX)
row("exact-pair-debug-n4-general-shuffled", 4, 2, 24, 3, ST, False, "shuffled", 1, info={"lane_pair": 1, "unitary_flow": 0},
    kernels=("sweep_pair_kernel", "exact_pair_kernel"), **EX)

# --- prop_tile_kernel, the per-member build (sweep_tile.hip; GRAPE_HOIST=0): n <= 8 packs two members of different d_k per tile ------
TILE = dict(info={"hoisted_controls": 0, "kernel_family": 1}, kernels=("prop_tile_kernel",), absent=("ctrl_sum_kernel",))
row("tile-n6-packed-shuffled", 6, 2, 24, 5, ST, True, "shuffled", 2, rank_one=False, env={"GRAPE_HOIST": "0"}, **TILE)
row("tile-n8-packed-ramp", 8, 2, 24, 5, UG, True, "ramp", 2, env={"GRAPE_HOIST": "0", "GRAPE_NO_TP": "1"}, forced=True, **TILE)
row("tile-n12-ramp", 12, 2, 24, 3, ST, True, "ramp", 1, rank_one=False, env={"GRAPE_HOIST": "0"}, **TILE)
row("tile-n16-shuffled", 16, 2, 24, 3, UG, True, "shuffled", 2, env={"GRAPE_HOIST": "0", "GRAPE_NO_TP": "1"}, **TILE)
row("tile-n24-general-shuffled", 24, 2, 24, 3, CT, False, "shuffled", 1, rank_one=False, env={"GRAPE_HOIST": "0"}, **TILE)
row("tile-n32-ramp", 32, 2, 24, 3, UG, True, "ramp", 1, env={"GRAPE_HOIST": "0", "GRAPE_NO_TP": "1"}, forced=True, **TILE)

# --- prop_hoist1_kernel / prop_hoist2_kernel (prop_hoist.hip; GRAPE_HOIST=1; test_gpu_hoist.py) -----------------------------------------
H1 = dict(info={"hoisted_controls": 1, "kernel_family": 1}, kernels=("ctrl_sum_kernel", "prop_hoist1_kernel"))
H2 = dict(info={"hoisted_controls": 1, "kernel_family": 1}, kernels=("ctrl_sum_kernel", "prop_hoist2_kernel"))
HOIST = {"GRAPE_HOIST": "1"}
HOIST_SEQ = {"GRAPE_HOIST": "1", "GRAPE_NO_TP": "1"}
row("hoist1-n9-ramp", 9, 2, 24, 8, ST, True, "ramp", 2, rank_one=False, env=HOIST, **H1)
row("hoist1-n16-unitary-ramp", 16, 2, 24, 8, UG, True, "ramp", 3, env=HOIST_SEQ, forced=True, reverse=True, **H1)
row("hoist1-n16-unitary-scaled-shuffled", 16, 2, 24, 8, UG, True, "shuffled", 1, shared_controls=False, env=HOIST_SEQ, **H1)
row("hoist1-n16-mixed-spikes", 16, 2, 24, 8, ST, True, "spikes", 1, rank_one=False, env=HOIST, **H1)
row("hoist1-n16-rank-one-fused-ramp", 16, 2, 24, 8, CT, False, "ramp", 3, env={"GRAPE_HOIST": "1", "GRAPE_FORCE_FUSE": "1"},
    **dict(H1, info={"hoisted_controls": 1, "rank_one_chain": 1, "fused_forward": 1}))
row("hoist1-n16-rank-one-unfused-shuffled", 16, 2, 24, 8, ST, True, "shuffled", 3, env={"GRAPE_HOIST": "1", "GRAPE_NO_FUSE": "1"},
    **dict(H1, info={"hoisted_controls": 1, "rank_one_chain": 1, "fused_forward": 0}))
row("hoist1-n16-split-chain-reads-propagators", 16, 2, 24, 8, CT, False, "shuffled", 3, rank_one=False,
    env={"GRAPE_HOIST": "1", "GRAPE_NO_TP": "1", "GRAPE_SPLIT_EXPM": "0"},
    **dict(H1, kernels=("ctrl_sum_kernel", "prop_hoist1_kernel", "chain_tile_split_kernel")))
row("hoist2-n17-scaled-shuffled", 17, 2, 24, 8, UG, True, "shuffled", 3, shared_controls=False, env=HOIST_SEQ, **H2)
row("hoist2-n32-unitary-ramp", 32, 2, 24, 8, UG, True, "ramp", 1, env=HOIST_SEQ, forced=True, **H2)      # C5's chain at test size
row("hoist2-n32-unitary-shuffled", 32, 2, 24, 8, UG, True, "shuffled", 1, env=HOIST, **H2)
row("hoist2-n32-mixed-scaled-spikes", 32, 2, 24, 8, ST, True, "spikes", 2, rank_one=False, shared_controls=False, env=HOIST_SEQ, **H2)

# --- the expm kernels when a wave WALKS several slices.  Below one round of resident workgroups (4 per compute unit, 3 for
# prop_hoist2_kernel) the launcher hands every wave of the unfused expm kernels ONE slice, so at E = 8, N = 24 only the fused row
# above carries a prefetch, an LDS image and the hazard padding from one slice into the next.  E x N beyond four rounds of a
# 256-unit device (4 x 1024, 4 x 768 slices) gives every wave two slices, four apart in a shuffled pulse.
row("tile-n16-waves-walk-slices", 16, 2, 24, 176, UG, True, "shuffled", 3, env={"GRAPE_HOIST": "0", "GRAPE_NO_TP": "1"}, variants=(0,),
    distinct_members=8, **TILE)
row("hoist1-n16-waves-walk-slices", 16, 2, 24, 176, UG, True, "shuffled", 3, env=HOIST_SEQ, variants=(0,), distinct_members=8, **H1)
row("hoist2-n32-waves-walk-slices", 32, 2, 24, 136, UG, True, "shuffled", 1, env=dict(HOIST_SEQ, GRAPE_HOIST2="1"), variants=(0,), distinct_members=8, **H2)

# --- expm inside the two-wave split chain (chain_tile_split_kernel<.., EXPM>; test_gpu_tile.py) ----------------------------------------
SPLIT = dict(env={"GRAPE_NO_TP": "1", "GRAPE_NO_THIN": "1"}, rank_one=False, info={"hoisted_controls": 1},
             kernels=("ctrl_sum_kernel", "chain_tile_split_kernel"), absent=("prop_hoist1_kernel", "prop_tile_kernel"))
row("split-expm-n16-ramp", 16, 2, 24, 8, CT, False, "ramp", 3, reverse=True, **SPLIT)
row("split-expm-n16-forced-general-shuffled", 16, 2, 24, 8, ST, True, "shuffled", 3, flags=("FLAG_FORCE_GENERAL",), forced=True, **SPLIT)

# --- chunked time axis (GRAPE_TP_CHUNKS; test_gpu_chunked.py, test_gpu_coop.py, test_gpu_action.py): N = 64 in 5 chunks of 13 ---------
# (the ragged last chunk, 12 slices, ends on the top level)
row("chunked-n16-rank-one-dpp-E1", 16, 2, 64, 1, CT, False, "shuffled", 1, top_last=True,
    env={"GRAPE_TP_CHUNKS": "5", "GRAPE_DPP_CHUNKS": "1"}, info={"time_chunks": 5, "rank_one_chain": 1, "prop_chain": 1},
    kernels=("chain_prop_kernel",))
row("chunked-n16-rank-one-thin-E2", 16, 2, 64, 2, ST, True, "shuffled", 1, top_last=True,
    env={"GRAPE_TP_CHUNKS": "3", "GRAPE_DPP_CHUNKS": "0"}, info={"time_chunks": 3, "rank_one_chain": 1, "prop_chain": 0},
    kernels=("chunk_product_thin_kernel", "chain_thin_kernel"))      # (chunks in multiples of 8 slices: 24 + 24 + 16)
row("chunked-n32-unitary-E2", 32, 2, 64, 2, UG, True, "shuffled", 1, top_last=True, env={"GRAPE_TP_CHUNKS": "5"},
    info={"time_chunks": 5, "unitary_flow": 1, "kernel_family": 1},
    kernels=("prop_hoist2_kernel", "coop_chunk_product_kernel", "chain_tile_unitary_kernel"))
row("chunked-n32-unitary-E1", 32, 2, 64, 1, UG, True, "shuffled", 2, top_last=True, env={"GRAPE_TP_CHUNKS": "7"},      # 6 x 10 + 4
    info={"time_chunks": 7, "unitary_flow": 1, "kernel_family": 1},
    kernels=("prop_hoist2_kernel", "coop_chunk_product_kernel", "chain_tile_unitary_kernel"))

# --- vector flow (action_thin.hip; GRAPE_ACTION=1; test_gpu_action.py): one plan serves slice i forward and N-1-i backward -----------
ACT_INFO = {"rank_one_chain": 1, "expm_action": 1, "time_chunks": 0}
PARTS = dict(props=False, info=ACT_INFO, kernels=("action_rows_kernel", "action_parts_kernel"))


def whole(flag):
    return {"GRAPE_ACTION": "1", "GRAPE_ACT_WHOLE": flag}


row("action-parts-n16-E3-N24-ramp", 16, 2, 24, 3, CT, False, "ramp", 2, env=whole("0"), reverse=True, **PARTS)      # C4's flow
row("action-whole-n16-E5-N25-ramp", 16, 2, 25, 5, CT, False, "ramp", 2, env=whole("1"), reverse=True, **PARTS)
row("action-parts-n12-nx1-E5-N25-ramp", 12, 2, 25, 5, UG, True, "ramp", 1, cols=1, env=whole("0"), reverse=True, **PARTS)
row("action-whole-n8-E3-N24-spikes", 8, 2, 24, 3, ST, True, "spikes", 3, env=whole("1"), **PARTS)
row("action-parts-n12-E3-N25-spikes", 12, 2, 25, 3, ST, False, "spikes", 3, env=whole("0"), **PARTS)
row("action-whole-n8-nx1-E5-N24-ramp", 8, 2, 24, 5, UG, False, "ramp", 3, cols=1, env=whole("1"), reverse=True, **PARTS)
row("action-scaled-controls-n16-E3-N25-ramp", 16, 2, 25, 3, CT, False, "ramp", 2, shared_controls=False, env={"GRAPE_ACTION": "1"},
    reverse=True, **PARTS)
row("action-own-controls-n16-E5-N24-ramp", 16, 2, 24, 5, ST, True, "ramp", 1, shared_controls=False,
    env={"GRAPE_ACTION": "1", "GRAPE_CTRL_SCALE": "0"}, reverse=True, props=False, info=dict(ACT_INFO, hoisted_controls=0),
    absent=("action_rows_kernel",))
THIN2 = dict(props=False, env={"GRAPE_ACTION": "1"}, info=dict(ACT_INFO, kernel_family=1), kernels=("action_thin2_kernel",))
row("action-thin2-n17-ramp", 17, 2, 12, 2, ST, True, "ramp", 1, reverse=True, **THIN2)
row("action-thin2-n32-nx1-ramp", 32, 2, 12, 2, UG, False, "ramp", 1, cols=1, reverse=True, **THIN2)
row("action-thin2-n32-spikes", 32, 2, 12, 2, CT, True, "spikes", 1, **THIN2)

# --- chain_prop_kernel on whole and on chunked time axes (GRAPE_THIN_DPP, GRAPE_DPP_CHUNKS; test_gpu_action.py) -------------------------
row("chain-prop-n16-shuffled", 16, 2, 24, 3, CT, False, "shuffled", 2,
    env={"GRAPE_ACTION": "0", "GRAPE_THIN_DPP": "1", "GRAPE_HOIST": "1"},
    info={"rank_one_chain": 1, "expm_action": 0, "time_chunks": 0, "fused_forward": 0}, kernels=("chain_prop_kernel",))
row("chain-prop-chunks-n16-shuffled", 16, 2, 64, 3, ST, True, "shuffled", 2, top_last=True,      # (this flow starts at 64 slices)
    env={"GRAPE_DPP_CHUNKS": "1", "GRAPE_TP_CHUNKS": "3"},
    info={"rank_one_chain": 1, "prop_chain": 1, "expm_action": 0, "time_chunks": 3}, kernels=("chunk_product_quad_kernel", "chain_prop_kernel"))

# --- exact_tile.hip (test_gpu_exact.py) ----------------------------------------------------------------------------------------------------
EXT = dict(mode="exact", objectives=("fom", "c1"), props=False, variants=(1,), info={"kernel_family": 1}, kernels=("exact_tile_kernel",))
row("exact-tile-n8-shuffled", 8, 2, 8, 2, ST, True, "shuffled", 1, **EXT)
row("exact-tile-n16-general-shuffled", 16, 2, 8, 2, CT, False, "shuffled", 1, rank_one=False, **EXT)
row("exact-tile-n32-shuffled", 32, 2, 8, 2, UG, True, "shuffled", 1, **EXT)

# --- grid family (sweep_grid.hip; test_gpu_grid.py): per-member and hoisted bound, the exact gradient at n = 33 ------------------------
GRID = dict(rank_one=False)
row("grid-n40-hoisted-ramp", 40, 2, 12, 2, UG, True, "ramp", 1, env={"GRAPE_HOIST": "1"}, forced=True, reverse=True,
    info={"kernel_family": 1, "hoisted_controls": 1}, kernels=("ctrl_sum_kernel", "grid_prop_kernel"), **GRID)
row("grid-n40-per-member-sequential-shuffled", 40, 2, 12, 2, ST, True, "shuffled", 1, env={"GRAPE_HOIST": "0", "GRAPE_NO_TP": "1"},
    info={"kernel_family": 1, "hoisted_controls": 0, "time_chunks": 0}, kernels=("grid_prop_kernel", "grid_chain_kernel"),
    absent=("ctrl_sum_kernel", "grid_chunk_product_kernel"), **GRID)
row("grid-n64-hoisted-shuffled", 64, 2, 12, 2, UG, True, "shuffled", 1, env={"GRAPE_HOIST": "1"},
    info={"kernel_family": 1, "hoisted_controls": 1}, kernels=("ctrl_sum_kernel", "grid_prop_kernel"), **GRID)
row("grid-n64-per-member-general-ramp", 64, 2, 12, 2, CT, False, "ramp", 1, env={"GRAPE_HOIST": "0"},
    info={"kernel_family": 1, "hoisted_controls": 0}, kernels=("grid_prop_kernel",), absent=("ctrl_sum_kernel",), **GRID)
row("grid-exact-n33-shuffled", 33, 2, 12, 2, UG, True, "shuffled", 2, mode="exact", objectives=("fom", "c1"), props=False,
    variants=(1,), kernels=("grid_exact_kernel",))

# --- sweep_any.hip (test_gpu_any.py) ------------------------------------------------------------------------------------------------------
row("any-n66-shuffled", 66, 2, 10, 2, UG, True, "shuffled", 1, forced=True, info={"kernel_family": 2, "states_stored": 1},
    kernels=("any_sweep_kernel",))


def case_of(rid):
    r = ROWS[rid]
    return mn.make_case(r["n"], r["K"], r["N"], r["E"], r["sys_type"], r["herm"], r["order"], r["s_top"], r["seed"], **r["case"])


@functools.lru_cache(maxsize=None)
def _case(rid):
    out = case_of(rid)
    for a in out[:-1]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(oracle, rid, variant, objective, reverse):
    """(F, G, foms, grads) of the oracle: computed once per (row, variant, objective, direction), read-only"""
    r = ROWS[rid]
    A, B, Xi, Xt, wts, x, T = _case(rid)
    x = np.ascontiguousarray(x[:, ::-1]) if reverse else x
    if r["mode"] == "exact":
        out = oracle.ensemble_exact(r["sys_type"], A, B, Xi, Xt, wts, x, T, variant=variant,
                                    objective=0 if objective == "fom" else 1, per_member=True)
    else:
        out = oracle.ensemble_eval(r["sys_type"], A, B, Xi, Xt, wts, x, T, variant=variant, per_member=True)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _reference_propagators(oracle, rid, variant, reverse):
    r = ROWS[rid]
    A, B, Xi, Xt, wts, x, T = _case(rid)
    x = np.ascontiguousarray(x[:, ::-1]) if reverse else x
    return oracle.member_eval(r["sys_type"], A[-1], B[-1], Xi[-1], Xt[-1], x, T, variant=variant, trajectory=True)[2]


def _engine(qoc, rid, variant, objective, **over):
    r = ROWS[rid]
    A, B, Xi, Xt, wts, x, T = _case(rid)
    flags = 0
    for name in r["flags"]:
        flags |= getattr(qoc.engine, name)
    kw = dict(r["ekw"], variant=variant, flags=flags, member_results=True)
    if r["mode"] == "exact":
        kw.update(gradient="exact", objective=objective)
    kw.update(over)
    return qoc.GrapeEngine(r["sys_type"], A, B, Xi, Xt, wts, T, r["N"], **kw)


def _assert_flow(r, info, names, what):
    for key, want in r["info"].items():
        assert info[key] == want, f"{what}: info[{key!r}] = {info[key]}, the row was written for {want} ({names})"
    for k in r["kernels"]:
        assert any(name == k or name.startswith(k) for name in names), f"{what}: {k} did not run: {names}"
    for k in r["absent"]:
        assert not any(name == k or name.startswith(k) for name in names), f"{what}: {k} ran: {names}"


def _set_env(monkeypatch, r):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)


def _check_propagators(oracle, eng, rid, variant, reverse, what):
    r = ROWS[rid]
    A, B, _, _, _, x, T = _case(rid)
    x = x[:, ::-1] if reverse else x
    P = eng.trajectory(r["E"] - 1, states=False)[0]
    P_ref = _reference_propagators(oracle, rid, variant, reverse)
    err = np.abs(P - P_ref).reshape(r["N"], -1).max(axis=1)
    tol = 1e-11 * max(1.0, np.abs(P_ref).max())
    t = int(np.argmax(err))
    s = [mn.squarings(b) for b in mn.slice_bounds(A[-1:], B[-1:], x, T / r["N"])[0]]
    msg = (f"{what}: propagators of member {r['E'] - 1}: worst slice t = {t} (squarings {s[t]}, neighbours "
           f"{s[max(t - 1, 0)]} / {s[min(t + 1, r['N'] - 1)]}), |P - P_ref|_inf = {err[t]:.3e}, bar {tol:.3e}; per slice "
           + " ".join(f"{e:.1e}" for e in err))
    print(msg)
    if r["herm"]:
        assert err[t] <= tol, msg


IDS = [(rid, v) for rid, r in ROWS.items() for v in r["variants"]]


@pytest.mark.parametrize("rid,variant", IDS, ids=[f"{rid}-v{v}" for rid, v in IDS])
def test_flow_on_a_mixed_norm_pulse(qoc, oracle, monkeypatch, rid, variant):
    r = ROWS[rid]
    x = _case(rid)[5]
    _set_env(monkeypatch, r)
    E, n = r["E"], r["n"]
    for objective in r["objectives"]:
        for reverse in ((False, True) if r["reverse"] else (False,)):
            what = f"{rid} v{variant} {objective}" + (" reversed" if reverse else "")
            xe = np.ascontiguousarray(x[:, ::-1]) if reverse else x
            F_ref, G_ref, foms_ref, grads_ref = _reference(oracle, rid, variant, objective, reverse)
            with _engine(qoc, rid, variant, objective) as eng:
                if r["mode"] == "fom":
                    F, mF = eng.fom(xe, members=True)
                    names, info = eng.kernel_names(), eng.info
                    assert eng.fom(xe) == F, f"{what}: a second call differs"
                    assert not any(k.startswith("sweep_") for k in names), names
                    _assert_flow(r, info, names, what)
                    for got, ref, tag in ((F, F_ref, "F"), (mF, foms_ref, "member F")):          # test_gpu_fom.py's bar
                        err = np.abs(np.asarray(got) - np.asarray(ref))
                        print(f"{what} {tag}: max |d| = {err.max():.3e}")
                        assert np.all(err <= 1e-10 * np.maximum(1.0, np.abs(ref))), f"{what} {tag}: |d| = {err.max():.3e}"
                    continue
                F, G = eng.eval(xe)
                foms, grads = eng.member_results()
                names, info = eng.kernel_names(), eng.info
                F2, G2 = eng.eval(xe)
                _assert_flow(r, info, names, what)
                if r["props"]:
                    _check_propagators(oracle, eng, rid, variant, reverse, what)
            assert F == F2 and np.array_equal(G, G2), f"{what}: a second evaluation differs"
            print(f"{what}: |F - F_ref| = {abs(F - F_ref):.3e}, |G - G_ref|_inf / |G_ref|_inf = "
                  f"{np.abs(G - G_ref).max() / np.abs(G_ref).max():.3e}")
            for k in range(E):
                assert_parity(foms[k], grads[k], foms_ref[k], grads_ref[k], n, what=f"{what} member {k}")
            assert_parity(F, G, F_ref, G_ref, n, what=f"{what} ensemble")


FORCED = [rid for rid, r in ROWS.items() if r["forced"]]


@pytest.mark.parametrize("rid", FORCED)
def test_norm_chosen_squarings_against_a_uniform_sufficient_count(qoc, monkeypatch, rid):
    """The same context with expm_squarings = s_top + 1 for every slice (sufficient everywhere: 6.9 / 2^8 < 0.08): the two runs
    of the library agree to the 1e-11 relative bar test_gpu_grid.py holds two of the library's own flows to."""
    r = ROWS[rid]
    assert r["herm"] and r["mode"] == "eval"
    x = _case(rid)[5]
    _set_env(monkeypatch, r)
    res = []
    for s in (-1, r["s_top"] + 1):
        with _engine(qoc, rid, 0, "fom", expm_squarings=s) as eng:
            res.append(eng.eval(x))
            names, info = eng.kernel_names(), eng.info
        _assert_flow(r, info, names, f"{rid} expm_squarings={s}")
    (F, G), (Fu, Gu) = res
    print(f"{rid}: |F - F_uniform| = {abs(F - Fu):.3e}, |G - G_uniform|_inf / |G_uniform|_inf = "
          f"{np.abs(G - Gu).max() / np.abs(Gu).max():.3e}")
    assert abs(F - Fu) <= 1e-11 * max(1.0, abs(Fu))
    assert np.abs(G - Gu).max() <= 1e-11 * np.abs(Gu).max()
