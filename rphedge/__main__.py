"""Command line interface: ``python -m rphedge <command>``.

  run        --config cfg.json [--set key=value ...]   any params dict (pension, SV, European, basket)
  european   [--paths N] [--parity] [--payoff NAME] ...   European Options notebook driver (NAME: asian_call ...)
             [--exercise bermudan [--exercise-every K]]   ... with the right to exercise at every K-th rebalancing date
  run / european also take the out-of-sample test of the trained hedge:
             [--oos-paths-log2 M] [--oos-seed S] [--oos-stress key=value ...]   2^M fresh paths (stress: sigma=0.18 ...;
                                                    jumps: jump_intensity=1,jump_mean=-0.1,jump_std=0.15)
  Merton jump-diffusion: --set model=merton jump_intensity=1 jump_mean=-0.1 jump_std=0.15 (examples/merton_call_30.json)
  run / european also take proportional transaction costs and a no-trade band (RunResult.costs):
             [--cost-rate R] [--rebalance-band B] [--cost-unwind]   a trade of |dh| at S costs R |dh| S
  sts                                                    Single Time Step notebook driver
  sweep      [--sigmas .05,.1,...]                       volatility sweep (Multi Time Step)
  calibrate  --csv prices.csv | --synthetic               CIR calibration (Extra: Stochastic Volatility)
  sanity     --config cfg.json                           notebook sanity checks
  info                                                   device + native library info
Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N -m rphedge run ...``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def _coerce(v: str):
    for f in (int, float):
        try:
            return f(v)
        except ValueError:
            pass
    if v.lower() in ("true", "false"):
        return v.lower() == "true"
    return v


def _summary(res) -> dict:
    out = {"phi0": res.phi, "psi0": res.psi, "V0": res.v0, "terminal_pnl": res.terminal_pnl, "VaR": res.var,
           "summary": {k: v for k, v in res.summary.items() if not isinstance(v, list)},
           "timings": res.timings}
    if res.costs is not None:
        out["costs"] = res.costs
    if res.out_of_sample is not None:
        out["out_of_sample"] = res.out_of_sample.as_dict()
    return out


def _oos_args(p):
    p.add_argument("--oos-paths-log2", type=int, default=None,
                   help="out-of-sample test of the trained hedge on 2^M fresh paths (0: off)")
    p.add_argument("--oos-seed", type=int, default=None, help="Sobol scramble seed of the test paths")
    p.add_argument("--oos-stress", nargs="*", default=None, metavar="key=value",
                   help="simulate the test paths under other model parameters (sigma=0.18, xi=0.4 ...; gbm_log / merton: "
                        "jump_intensity=1,jump_mean=-0.1,jump_std=0.15 makes the test paths jump)")


def _cost_args(p):
    p.add_argument("--cost-rate", type=float, default=None,
                   help="proportional transaction cost per unit of traded value (the hedge is scanned under it)")
    p.add_argument("--rebalance-band", type=float, default=None,
                   help="no-trade band: rebalance only where the target leaves the held position by more than this")
    p.add_argument("--cost-unwind", action="store_true", help="also sell the final position at the horizon")


def _cost_params(a) -> dict:
    out = {}
    if a.cost_rate is not None:
        out["cost_rate"] = a.cost_rate
    if a.rebalance_band is not None:
        out["rebalance_band"] = a.rebalance_band
    if a.cost_unwind:
        out["cost_unwind"] = True
    return out


def _oos_params(a) -> dict:
    out = {}
    if a.oos_paths_log2 is not None:
        out["oos_paths_log2"] = a.oos_paths_log2
    if a.oos_seed is not None:
        out["oos_seed"] = a.oos_seed
    if a.oos_stress:
        out["oos_stress"] = ",".join(a.oos_stress)
    return out


def _plots(res, out_dir):
    if not out_dir:
        return
    from .utils.reports import plot_run

    os.makedirs(out_dir, exist_ok=True)
    res.summary["figures"] = plot_run(res, out_prefix=os.path.join(out_dir, "rphedge"))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="rphedge", description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--config", required=True)
    r.add_argument("--set", nargs="*", default=[])
    r.add_argument("--sv", action="store_true")
    r.add_argument("--out", default=None)
    r.add_argument("--plots", default=None, help="directory for the report figures (C26-C32)")
    _oos_args(r)
    _cost_args(r)
    e = sub.add_parser("european")
    e.add_argument("--paths", type=int, default=3000)
    e.add_argument("--rebalancing", type=float, default=1 / 52)
    e.add_argument("--parity", action="store_true")
    e.add_argument("--payoff", default=None,
                   help="path-dependent option instead of the call: asian_call, geo_asian_call, lookback_call, ...")
    e.add_argument("--exercise", default=None, choices=["european", "bermudan", "american"],
                   help="bermudan: the holder may exercise at the rebalancing dates (american: at every one)")
    e.add_argument("--exercise-every", type=int, default=None, help="bermudan: every K-th rebalancing date")
    e.add_argument("--set", nargs="*", default=[])
    e.add_argument("--plots", default=None, help="directory for the report figures (C26-C32)")
    _oos_args(e)
    _cost_args(e)
    sub.add_parser("sts").add_argument("--no-parity", action="store_true")
    s = sub.add_parser("sweep")
    s.add_argument("--sigmas", default="0.05,0.10,0.15,0.20,0.30")
    s.add_argument("--set", nargs="*", default=[])
    c = sub.add_parser("calibrate")
    c.add_argument("--csv", default=None)
    c.add_argument("--synthetic", action="store_true")
    c.add_argument("--window", type=int, default=40)
    sa = sub.add_parser("sanity")
    sa.add_argument("--config", required=True)
    sub.add_parser("info")
    a = ap.parse_args(argv)

    if a.cmd == "run":
        from .api import run_params

        with open(a.config) as f:
            params = json.load(f)
        params.update({k: _coerce(v) for k, v in (kv.split("=", 1) for kv in a.set)})
        if a.out:
            params["save_dir"] = a.out
        params.update(_oos_params(a))
        params.update(_cost_params(a))
        res = run_params(params, sv=a.sv)
        _plots(res, a.plots)
        print(json.dumps(_summary(res), default=float, indent=1))
    elif a.cmd == "european":
        from .api import european_option

        extra = {k: _coerce(v) for k, v in (kv.split("=", 1) for kv in a.set)}
        if a.payoff:
            extra["payoff"] = a.payoff
        if a.exercise:
            extra["exercise"] = a.exercise
        if a.exercise_every is not None:
            extra["exercise_every"] = a.exercise_every
        extra.update(_oos_params(a))
        extra.update(_cost_params(a))
        res = european_option(N_paths=a.paths, rebalancing_frequency=a.rebalancing, parity=a.parity, **extra)
        _plots(res, a.plots)
        print(json.dumps(_summary(res), default=float, indent=1))
    elif a.cmd == "sts":
        from .experiments import single_time_step

        out = single_time_step(parity=not a.no_parity)
        out.pop("result")
        print(json.dumps(out, default=float, indent=1))
    elif a.cmd == "sweep":
        from .experiments import volatility_sweep

        extra = {k: _coerce(v) for k, v in (kv.split("=", 1) for kv in a.set)}
        rows = volatility_sweep(sigmas=[float(x) for x in a.sigmas.split(",")], **extra)
        print(json.dumps(rows, default=float, indent=1))
    elif a.cmd == "calibrate":
        from . import calib

        prices = calib.load_prices(a.csv) if a.csv else calib.synthetic_prices()
        out = calib.calibrate(prices, window=a.window)
        out.pop("volatility")
        print(json.dumps(out, indent=1))
    elif a.cmd == "sanity":
        from .experiments import sanity_checks

        with open(a.config) as f:
            print(json.dumps(sanity_checks(json.load(f)), default=float, indent=1))
    elif a.cmd == "info":
        import torch

        from .ops import native

        info = {"torch": torch.__version__, "hip": torch.version.hip, "gpu": torch.cuda.is_available(),
                "native": str(native._LIB_PATH), "native_loaded": native.available()}
        if torch.cuda.is_available():
            info.update(native.device_info(0))
        print(json.dumps(info, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
