"""Launch the GBM scan (k_sim_scan) once per path statistic and scheme at the
euro30 shape - 2^20 paths, 30 dates x SUBSTEPS fine steps - 21 times each, for
a kernel trace of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o scan -- python tools/scan_time.py SUBSTEPS
  python tools/kstats.py OUT/scan_kernel_stats.csv k_sim_scan

The kernel names carry the template arguments <Real, ALIGNED, MODEL, STAT>
(MODEL 0 arithmetic / 1 log scheme; STAT 0 none, 1 mean, 2 geomean, 3 max, 4 min).
"""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402

from rphedge.ops import paths as P  # noqa: E402


def main():
    sub = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    dev = torch.device("cuda", 0)
    g = P.Grid(1.0, 1 / (30 * sub), 1 / 30)
    n = 1 << 20
    print(f"n_fine {g.n_fine} reduction {g.reduction} n_coarse {g.n_coarse}", flush=True)
    for scheme in ("log", "arith"):
        for stat in (None, "mean", "geomean", "max", "min"):
            if scheme == "arith" and stat == "geomean":
                continue
            kw = dict(scheme=scheme, norm=100.0, device=dev, path_stat=stat)
            p = P.simulate_gbm(g, n, 100.0, 0.08, 0.15, **kw)
            for _ in range(20):
                P.simulate_gbm(g, n, 100.0, 0.08, 0.15, out=p, **kw)
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
