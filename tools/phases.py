"""Phase breakdown of ONE graph replay of the euro30 bench from a rocprofv3
results database: kernels of the first date's multi-start exploration (grid
y > 1), the first date's polish, and the later dates, with totals / counts /
means per kernel, and the idle time between kernels.
usage: python tools/phases.py RESULTS.db"""
import collections
import sqlite3
import sys


def main():
    c = sqlite3.connect(sys.argv[1])
    rows = list(c.execute("select s.kernel_name, d.start, d.end, d.grid_size_y from rocpd_kernel_dispatch d "
                          "join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start"))
    sims = [i for i, r in enumerate(rows) if "k_sim_scan" in r[0]]
    # the last replay: it opens with one k_sim_scan_pair (the main paths and the Gram subsample in one
    # launch), or with two k_sim_scan launches in a trace from before the merged launch
    start = sims[-1] if "k_sim_scan_pair" in rows[sims[-1]][0] else sims[-2]
    # ... and closes with the P&L: k_pnl_finish (folded into the evals), or the k_hedge_pnl scan
    end = next(i for i in range(start, len(rows)) if "k_pnl_finish" in rows[i][0] or "k_hedge_pnl" in rows[i][0])
    rep = rows[start:end + 1]
    # the first date ends with its k_hedge_eval, or - where that eval rides in the next fit's first solve launch
    # (k_lm_solve_eval) - before the pass two launches ahead of that solve
    first_eval = next(i - 2 if "k_lm_solve_eval" in r[0] else i for i, r in enumerate(rep)
                      if "k_hedge_eval" in r[0] or "k_lm_solve_eval" in r[0])
    agg, cnt = collections.defaultdict(float), collections.Counter()
    for i, (name, t0, t1, gy) in enumerate(rep):
        seg = "explore" if gy > 1 else ("first" if i < first_eval else "later")
        k = name.split("(")[0].replace("_ZN3rph", "").split("E")[0][:24]
        k = "15k_lm_solve_eval" if "k_lm_solve_eval" in name else k
        # (an exploration solve with a slice of the path scan riding in its launch)
        k = "14k_lm_solve_sim" if "k_lm_solve_sim" in name else k
        agg[(seg, k)] += (t1 - t0) / 1e3
        cnt[(seg, k)] += 1
    print(f"replay {(rep[-1][2] - rep[0][1]) / 1e3:.1f} us, {len(rep)} kernels, first date "
          f"{(rep[first_eval][1] - rep[0][1]) / 1e3:.1f} us, idle "
          f"{sum(max(0, rep[i + 1][1] - rep[i][2]) for i in range(len(rep) - 1)) / 1e3:.1f} us")
    # where the fits start: the head of the path scan (k_sim_scan_pair) and whatever else precedes the first
    # exploration pass, and the polish fit's first pass (grid y = 1), from the start of the replay
    p0 = next((r for r in rep if "k_lm_pass" in r[0]), None)
    p1 = next((r for r in rep if "k_lm_pass" in r[0] and r[3] == 1), None)
    print(f"head launch {(rep[0][2] - rep[0][1]) / 1e3:.1f} us, first k_lm_pass at "
          f"{(p0[1] - rep[0][1]) / 1e3 if p0 else float('nan'):.1f} us, first one-instance k_lm_pass at "
          f"{(p1[1] - rep[0][1]) / 1e3 if p1 else float('nan'):.1f} us")
    for k in sorted(agg):
        print(f"  {k[0]:8s} {k[1]:26s} n={cnt[k]:3d} total {agg[k]:8.1f} us  mean {agg[k] / cnt[k]:6.2f} us")


if __name__ == "__main__":
    main()
