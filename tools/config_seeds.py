"""Seed sweep of a params JSON (examples/*.json) in ONE process: the run is
captured into its hipGraph and replayed like bench.py does; one JSON line per
seed with the time per replay and the quality fields.  tools/seeds.py sweeps
bench.py presets; this is the same loop for any configuration bench.py has no
preset for (the path-dependent options).

usage: python tools/config_seeds.py OUT.jsonl SEEDS CONFIG.json [key=value ...]
  SEEDS: comma list or a-b range, e.g. 1-16
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402

from rphedge.__main__ import _coerce  # noqa: E402
from rphedge.api import HedgeRun  # noqa: E402
from rphedge.config import parse_params  # noqa: E402


def seeds(spec: str):
    if "-" in spec:
        a, b = spec.split("-")
        return list(range(int(a), int(b) + 1))
    return [int(x) for x in spec.split(",")]


def main(warmup: int = 2, steps: int = 5):
    out, spec, config, rest = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
    with open(config) as f:
        base = json.load(f)
    base.update({k: _coerce(v) for k, v in (kv.split("=", 1) for kv in rest)})
    base.update(verbose=False, keep_paths=False)
    with open(out, "a") as f:
        for s in seeds(spec):
            t0 = time.perf_counter()
            run = HedgeRun(parse_params(dict(base, seed=s)))
            run.build()
            run.capture(include_simulation=True)
            for _ in range(warmup):
                run.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(steps):
                run.replay()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t1) / steps * 1e3
            res = run.collect()
            run.close()
            sm = res.summary
            rec = {"seed": s, "config": os.path.basename(config), "args": " ".join(rest), "ms": ms,
                   "pnl": sm["self_financing_pnl_std"], "pnl_mean": (res.self_financing_pnl or {}).get("mean"),
                   "resid": sm["terminal_residual_std"], "V0": res.v0, "analytic_price": sm.get("analytic_price"),
                   "bs_price": sm.get("bs_price"), "nin": run.spec.nin, "wall_s": time.perf_counter() - t0}
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
