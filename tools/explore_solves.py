"""Exploration solves (grid y > 1) of every replay in a rocprofv3 results db: count,
mean / min / max by kernel (k_lm_solve, or k_lm_solve_sim where a slice of the path
scan rides).  usage: python tools/explore_solves.py RESULTS.db"""
import collections, sqlite3, sys
c = sqlite3.connect(sys.argv[1])
rows = c.execute("select s.kernel_name, d.end - d.start from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s "
                 "on d.kernel_id = s.id where d.grid_size_y > 1 and s.kernel_name like '%k_lm_solve%'")
out = collections.defaultdict(list)
for n, dur in rows:
    out["k_lm_solve_sim" if "k_lm_solve_sim" in n else "k_lm_solve"].append(dur / 1e3)
for k, v in out.items():
    print(f"exploration {k:15s} n={len(v):4d} mean {sum(v) / len(v):6.2f} us  min {min(v):6.2f}  max {max(v):6.2f}")
