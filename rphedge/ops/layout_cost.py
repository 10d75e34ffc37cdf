"""Constants of the scans under transaction costs (csrc/rph_types.h COST_NSTAT,
CostStat), compared by name with the native library's table of their own
(``rph_layout_consts_cost``) when it is loaded."""

COST_NSTAT = 8   # doubles per workgroup in the cost stats slab
CS_COST = 0      # sum of the cost carried to the horizon
CS_COST2 = 1     # sum of its square
CS_TURN = 2      # sum of the turnover
CS_TRADES = 3    # sum of the trade dates t >= 1
CS_COUNT = 4     # paths
