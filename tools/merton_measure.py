"""The Merton measurements of BENCHMARKS.md (raw output: profiles/merton/measure.jsonl).

usage: python tools/merton_measure.py OUT.jsonl [SEEDS]

scan_time: k_sim_scan (gbm_log) against k_sim_jump (J1 and lam = 0) at 2^20 paths,
  30 dates x 1 and x 10 fine steps; each sample is 50 launches between two device
  events, 7 samples per kernel, alternating, after a warm-up of each.
stress_quality: the euro30 preset of bench.py, seeds 1-4, 2^22 test paths: plain,
  sigma x 1.2 and the jump stress J1 = (1, -0.1, 0.15).
oos_route_time: that run's jump stress, fused against materialised, 5 alternating repeats.
training_quality: examples/merton_call_30.json, SEEDS (default 16) weight-init seeds:
  the net's self-financing P&L std against the Merton-delta hedge's on the same paths.
"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from rphedge.api import HedgeRun  # noqa: E402
from rphedge.config import parse_params  # noqa: E402
from rphedge.ops import paths as P  # noqa: E402

OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merton", "measure.jsonl")
J1 = dict(jump_intensity=1.0, jump_mean=-0.1, jump_std=0.15)
SEEDS = int(sys.argv[2]) if len(sys.argv) > 2 else 16


def emit(rec):
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def scan_time():
    dev = torch.device("cuda", 0)
    n = 1 << 20
    for sub in (1, 10):
        g = P.Grid(1.0, 1 / (30 * sub), 1 / 30)
        pg = P.simulate_gbm(g, n, 100.0, 0.08, 0.15, scheme="log", norm=100.0, device=dev)
        pm = P.simulate_merton(g, n, 100.0, 0.08, 0.15, 1.0, -0.1, 0.15, norm=100.0, device=dev)
        p0 = P.simulate_merton(g, n, 100.0, 0.08, 0.15, 0.0, -0.1, 0.15, norm=100.0, device=dev)
        fns = {"k_sim_scan gbm_log": lambda: P.simulate_gbm(g, n, 100.0, 0.08, 0.15, scheme="log", norm=100.0, device=dev, out=pg),
               "k_sim_jump J1": lambda: P.simulate_merton(g, n, 100.0, 0.08, 0.15, 1.0, -0.1, 0.15, norm=100.0, device=dev, out=pm),
               "k_sim_jump lam=0": lambda: P.simulate_merton(g, n, 100.0, 0.08, 0.15, 0.0, -0.1, 0.15, norm=100.0, device=dev, out=p0)}
        for fn in fns.values():
            timed(fn, 10)
        ms = {k: [] for k in fns}
        for _ in range(7):
            for k, fn in fns.items():   # alternating
                ms[k].append(timed(fn, 50))
        emit({"what": "scan_time", "n_paths": n, "n_fine": g.n_fine, "launches_per_sample": 50,
              "ms_median": {k: sorted(v)[3] for k, v in ms.items()}, "ms_min": {k: min(v) for k, v in ms.items()},
              "ms_max": {k: max(v) for k, v in ms.items()}})


def euro30(seed):
    return bench.build_run(bench.parse(["--preset", "euro30", "--seed", str(seed)]), 1)


def oos_time_and_stress_quality():
    for seed in range(1, 5):
        run = HedgeRun(euro30(seed))
        res = run.run()
        rows = {"plain": None, "sigma x 1.2": {"sigma": 1.2 * run.cfg.sigma}, "J1": J1}
        rec = {"what": "stress_quality", "config": "euro30", "seed": seed, "n_train": run.n_total, "n_test": 1 << 22,
               "V0": res.v0}
        for label, st in rows.items():
            o = run.out_of_sample(paths_log2=22, stress=st)
            rec[label] = {"route": o.route, "std": o.std, "mean": o.mean, "min": o.min, "max": o.max,
                          "std_ratio": o.std_ratio}
            rec["in_sample_std"] = o.in_sample["std"]
        emit(rec)
        if seed == 1:
            routes = {"fused": lambda: run.out_of_sample(paths_log2=22, stress=J1, fused=True),
                      "materialised": lambda: run.out_of_sample(paths_log2=22, stress=J1, fused=False)}
            std = {k: fn().std for k, fn in routes.items()}
            ms = {k: [] for k in routes}
            for _ in range(5):
                for k, fn in routes.items():
                    ms[k].append(timed(fn, 1))
            emit({"what": "oos_route_time", "config": "euro30 + J1 stress", "test_log2": 22, "ms": ms,
                  "ms_median": {k: sorted(v)[2] for k, v in ms.items()}, "std": std})
        run.close()


def training_quality():
    with open(os.path.join(ROOT, "examples", "merton_call_30.json")) as f:
        base = json.load(f)
    base.pop("oos_paths_log2", None)
    for seed in range(1, SEEDS + 1):
        run = HedgeRun(parse_params(dict(base, seed=seed, verbose=False, keep_paths=False)))
        res = run.run()
        s = res.summary
        emit({"what": "training_quality", "config": "merton_call_30", "seed": seed, "V0": res.v0,
              "analytic_price": s["analytic_price"], "mc_price": s["E_payoff"] * res.scale * float(run.paths.bond[0] / run.paths.bond[-1]),
              "net_pnl_std": res.self_financing_pnl["std"], "merton_delta_pnl_std": s["merton_delta_pnl_std"],
              "phi0": res.phi, "analytic_delta": s["analytic_delta"]})
        run.close()


if __name__ == "__main__":
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    scan_time()
    oos_time_and_stress_quality()
    training_quality()
