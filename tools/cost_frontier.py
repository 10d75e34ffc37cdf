"""The cost / risk frontier of the no-trade band, and the cost scans timed
(BENCHMARKS.md "transaction costs"; raw output under profiles/costs/).

usage: python tools/cost_frontier.py frontier OUT.jsonl SEEDS [TEST_LOG2] [RATE] [BANDS]
       python tools/cost_frontier.py timing   OUT.jsonl [REPEATS]

frontier: euro30 (the bench.py preset), one training run per weight-init seed
  (SEEDS: a-b or a comma list), then HedgeRun.cost_frontier over BANDS (default
  0,0.01,0.02,0.05) at RATE (default 1e-3) on 2^TEST_LOG2 (default 22) fresh
  paths: mean cost, net P&L std and trades per path of the learnt hedge, with
  the Black-Scholes and the Leland delta hedges on 2^20 of those paths under
  the same costs beside them.
timing: 2^20 paths x 30 dates of one trained euro30 run: the materialised scan
  (backend.pnl on the training paths) and the fused out-of-sample scan, each
  plain and under costs, alternating in one process after a warm-up of each,
  timed with device events around the launch.
"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from rphedge.api import HedgeRun  # noqa: E402
from rphedge.engine import Costs, PnlData  # noqa: E402
from rphedge.ops import layout as L  # noqa: E402
from rphedge.ops import layout_cost as LC  # noqa: E402


def seeds(spec: str):
    if "-" in spec:
        a, b = spec.split("-")
        return list(range(int(a), int(b) + 1))
    return [int(x) for x in spec.split(",")]


def trained(seed: int):
    run = HedgeRun(bench.build_run(bench.parse(["--preset", "euro30", "--seed", str(seed)]), 1))
    return run, run.run()


def frontier(out: str, spec: str, test_log2: int = 22, rate: float = 1e-3, bands=(0.0, 0.01, 0.02, 0.05)):
    from rphedge import oos

    with open(out, "a") as f:
        for s in seeds(spec):
            run, res = trained(s)
            rows = run.cost_frontier(bands, rate=rate, paths_log2=test_log2)
            # the analytic hedges on 2^20 of the same test paths (materialised: they need the price table)
            p = run._simulate_paths(1 << min(test_log2, 20), 0, None, None, seeds=oos.table_seeds(oos.OOS_SEED))
            for row in rows:
                a = run.cost_anchors(Costs(rate, row["band"]), p.S, p.bond, run.grid.times())
                rec = dict(row, seed=s, rate=rate, n_test=1 << test_log2, V0=res.v0,
                           gross_pnl_std=res.self_financing_pnl["std"], **a)
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
            run.close()


def timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timing(out: str, repeats: int = 9):
    from rphedge import oos

    run, _ = trained(1)
    ind, be, dev = run.induction, run.backend, run.device
    n, nd = run.n_local, ind.n_dates
    costs = Costs(1e-3, 0.02)
    st = torch.zeros(be.pnl_wgs(), L.EVAL_NSTAT, dtype=torch.float64, device=dev)
    cst = torch.zeros(be.pnl_wgs(), LC.COST_NSTAT, dtype=torch.float64, device=dev)
    sim = oos._fused_scan(run, n, 0, oos.table_seeds(oos.OOS_SEED), None, False)[1]
    data = PnlData(n_dates=nd, features=None, prices=None, bond=ind.pnl_data.bond, fmu=ind.pnl_data.fmu,
                   fisd=ind.pnl_data.fisd, w0=None, wealth0=oos.fitted_v0(run), payoff=None)
    ost = torch.zeros(be.oos_wgs(n), L.EVAL_NSTAT, dtype=torch.float64, device=dev)
    ocst = torch.zeros(be.oos_wgs(n), LC.COST_NSTAT, dtype=torch.float64, device=dev)
    kind, strike = oos.payoff_code(run)
    fns = {"k_hedge_pnl": lambda: be.pnl(ind.snap, ind.pnl_data, st),
           "k_hedge_pnl_cost": lambda: be.pnl(ind.snap, ind.pnl_data, st, costs=costs, cost_stats=cst),
           "k_hedge_oos": lambda: be.oos(sim, ind.snap, data, ost, kind, strike),
           "k_hedge_oos_cost": lambda: be.oos(sim, ind.snap, data, ost, kind, strike, costs=costs, cost_stats=ocst)}
    for fn in fns.values():   # warm-up of each
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():   # alternating
            ms[k].append(timed(fn))
    rec = {"paths": n, "dates": nd, "repeats": repeats, "ms": ms,
           "median_ms": {k: sorted(v)[repeats // 2] for k, v in ms.items()}}
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    run.close()


if __name__ == "__main__":
    mode, out = sys.argv[1], sys.argv[2]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if mode == "frontier":
        frontier(out, sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 22,
                 float(sys.argv[5]) if len(sys.argv) > 5 else 1e-3,
                 tuple(float(x) for x in sys.argv[6].split(",")) if len(sys.argv) > 6 else (0.0, 0.01, 0.02, 0.05))
    elif mode == "timing":
        timing(out, int(sys.argv[3]) if len(sys.argv) > 3 else 9)
    else:
        sys.exit(__doc__)
