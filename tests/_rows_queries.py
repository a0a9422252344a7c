"""The sweep of the pure-host geometry queries behind tests/golden/rows_queries.json: shared by the
generator (tools/gen_golden_rows_queries.py, run on the commit BEFORE csrc/rows.h) and by
tests/test_host_api.py, so that both ask the same questions in the same order."""
import itertools

F32, BF16 = 0, 1
NS = (1, 2, 3)
MAPS = ((1, 1), (1, 7), (5, 3), (33, 65), (65, 129), (513, 1025))
# every cvb_log2 of both pickers, idle lanes included; 12 / 4 are off the bf16 vector
CS = (4, 8, 12, 24, 40, 72, 136, 264, 728, 2048)
DTYPES = (F32, BF16)
DW_GEOMS = ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (1, 100))  # (stride, dilation): every family
# out of contract: -1 (seg_skip_pool_bwd_rows: 0), never a division by zero
REJECTED = (
    ("seg_cg_joint_chunks", (0, 5, 3, 8)), ("seg_cg_joint_chunks", (1, 0, 3, 8)),
    ("seg_cg_joint_chunks", (1, 5, 3, 6)), ("seg_cg_joint_chunks", (1, 5, 3, 0)),
    ("seg_eesp_pyr_chunks", (0, 5, 3, 8, 1)), ("seg_eesp_pyr_chunks", (1, 5, 3, 8, 3)),
    ("seg_eesp_pyr_chunks", (1, 5, 3, 12, 1)), ("seg_eesp_pyr_chunks", (1, 5, 0, 8, 2)),
    ("seg_fpe_stage_rows", (2, 1, 5, 3, 8)), ("seg_fpe_stage_rows", (F32, 0, 5, 3, 8)),
    ("seg_fpe_stage_rows", (F32, 65536, 5, 3, 8)), ("seg_fpe_stage_rows", (BF16, 1, 5, 3, 6)),
    ("seg_fpe_stage_rows", (BF16, 1, 5, 3, 68)), ("seg_fpe_stage_rows", (BF16, 1, 0, 3, 8)),
    ("seg_meu_rows", (0, 5, 3, 8, 0)), ("seg_meu_rows", (1, 5, 3, 12, 1)),
    ("seg_meu_rows", (1, 5, 3, 136, 0)), ("seg_meu_rows", (1, 5, 0, 8, 1)),
    ("seg_apply_pool_chunks", (0, 15, 8)), ("seg_apply_pool_chunks", (1, 0, 8)),
    ("seg_apply_pool_chunks", (1, 15, 0)),
    ("seg_skip_pool_bwd_rows", (2, 1, 5, 3, 8)), ("seg_skip_pool_bwd_rows", (F32, 0, 5, 3, 8)),
    ("seg_skip_pool_bwd_rows", (F32, 1, 1, 3, 8)), ("seg_skip_pool_bwd_rows", (BF16, 1, 5, 3, 12)),
    ("seg_ew_geom_query", (F32, 6, 10, 0)), ("seg_ew_geom_query", (F32, 8, 10, 5)),
    ("seg_ew_geom_query", (BF16, 12, 10, 0)),
    ("seg_dwconv_grid_y", (BF16, 4, 1, 1, 1, 1, 1, 2)), ("seg_dwconv_grid_y", (F32, 6, 1, 9, 20, 3, 3, 0)),
    ("seg_dwconv_grid_y", (F32, 16, 0, 9, 20, 1, 1, 1)),
)


def calls():
    """-> [(query name, argument tuple), ...] in a fixed order."""
    out = []
    nmc = list(itertools.product(NS, MAPS, CS))
    out += [("seg_cg_joint_chunks", (N, H, W, C)) for N, (H, W), C in nmc]
    out += [("seg_eesp_pyr_chunks", (N, H, W, C, s)) for N, (H, W), C in nmc for s in (1, 2)]
    out += [("seg_fpe_stage_rows", (dt, N, H, W, C)) for dt in DTYPES for N, (H, W), C in nmc]
    out += [("seg_meu_rows", (N, H, W, C, high)) for N, (H, W), C in nmc for high in (0, 1)]
    out += [("seg_apply_pool_chunks", (N, H * W, C)) for N, (H, W), C in nmc]
    out += [("seg_adaptive_avgpool_chunks", (H, W, o)) for (H, W) in MAPS for o in (1, 2, 3, 6)]
    out += [("seg_skip_pool_bwd_rows", (dt, N, H, W, C)) for dt in DTYPES for N, (H, W), C in nmc]
    out += [("seg_ew_geom_query", (dt, C, N * H * W, what))
            for dt in DTYPES for N, (H, W), C in nmc for what in range(5)]
    out += [("seg_dwconv_grid_y", (dt, C, N, H, W, s, d, kind))
            for dt in DTYPES for N, (H, W), C in nmc for (s, d) in DW_GEOMS for kind in range(3)]
    out += list(REJECTED)
    return out


def sweep(query):
    """query(name, *args) -> int.  -> {query name: [value, ...]} over calls(), in order."""
    table = {}
    for name, args in calls():
        table.setdefault(name, []).append(int(query(name, *args)))
    return table
