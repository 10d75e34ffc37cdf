"""In-sample vs out-of-sample hedge P&L, and the two out-of-sample routes timed
(BENCHMARKS.md "in-sample vs out-of-sample"; raw output under profiles/oos/).

usage: python tools/oos_bench.py quality OUT.jsonl SEEDS [TEST_LOG2]
       python tools/oos_bench.py timing  OUT.jsonl [REPEATS]

quality: euro30 and heston30 (the bench.py presets) and examples/asian_call_30.json,
  one training run per weight-init seed (SEEDS: a-b or a comma list, as
  tools/config_seeds.py), the self-financing P&L std in sample and on 2^TEST_LOG2
  (default 22) fresh paths; euro30 also with the test paths simulated at
  sigma x 1.2 (the misspecified-model row).
timing: one trained run per configuration, then out_of_sample(fused=True) and
  out_of_sample(fused=False) at 2^22 and 2^24 test paths, alternating in one
  process after a warm-up of each, timed with device events around the call
  (simulation, hedge, statistics and their reduction).
"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from rphedge.api import HedgeRun  # noqa: E402
from rphedge.config import parse_params  # noqa: E402

CONFIGS = ("euro30", "heston30", "asian_call_30")


def seeds(spec: str):
    if "-" in spec:
        a, b = spec.split("-")
        return list(range(int(a), int(b) + 1))
    return [int(x) for x in spec.split(",")]


def config(name: str, seed: int):
    if name in bench.PRESETS:
        return bench.build_run(bench.parse(["--preset", name, "--seed", str(seed)]), 1)
    with open(os.path.join(ROOT, "examples", name + ".json")) as f:
        return parse_params(dict(json.load(f), seed=seed, verbose=False, keep_paths=False))


def trained(name: str, seed: int):
    run = HedgeRun(config(name, seed))
    res = run.run()
    return run, res


def quality(out: str, spec: str, test_log2: int = 22):
    with open(out, "a") as f:
        for name in CONFIGS:
            for s in seeds(spec):
                run, res = trained(name, s)
                rows = [(None, run.out_of_sample(paths_log2=test_log2))]
                if name == "euro30":
                    rows.append(("sigma x 1.2", run.out_of_sample(paths_log2=test_log2,
                                                                  stress={"sigma": 1.2 * run.cfg.sigma})))
                for label, o in rows:
                    rec = {"config": name, "seed": s, "stress": o.stress, "label": label, "route": o.route,
                           "n_train": run.n_total, "n_test": o.n_paths, "oos_seed": o.seed,
                           "in_sample_std": o.in_sample["std"], "oos_std": o.std, "std_ratio": o.std_ratio,
                           "in_sample_mean": o.in_sample["mean"], "oos_mean": o.mean, "oos_min": o.min,
                           "oos_max": o.max, "V0": res.v0, "oos_seconds": o.seconds}
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


def timing(out: str, repeats: int = 5):
    with open(out, "a") as f:
        for name in CONFIGS:
            run, _ = trained(name, 1)
            for log2 in (22, 24):
                routes = {"fused": lambda: run.out_of_sample(paths_log2=log2, fused=True),
                          "materialised": lambda: run.out_of_sample(paths_log2=log2, fused=False)}
                std = {k: fn().std for k, fn in routes.items()}   # warm-up of each (tables, allocator)
                ms = {k: [] for k in routes}
                for _ in range(repeats):
                    for k, fn in routes.items():   # alternating
                        ms[k].append(timed(fn))
                peak = {}
                for k, fn in routes.items():
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    fn()
                    peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                rec = {"config": name, "test_log2": log2, "repeats": repeats,
                       "fused_ms": ms["fused"], "materialised_ms": ms["materialised"],
                       "fused_ms_median": sorted(ms["fused"])[repeats // 2],
                       "materialised_ms_median": sorted(ms["materialised"])[repeats // 2],
                       "fused_peak_mib": peak["fused"], "materialised_peak_mib": peak["materialised"],
                       "fused_std": std["fused"], "materialised_std": std["materialised"]}
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
            run.close()


if __name__ == "__main__":
    mode, out = sys.argv[1], sys.argv[2]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if mode == "quality":
        quality(out, sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 22)
    elif mode == "timing":
        timing(out, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        sys.exit(__doc__)
