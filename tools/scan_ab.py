"""The plain scan kernels of two builds compared: outputs bit for bit, and timing.

usage: python tools/scan_ab.py dump OUT.npz          every output array of rph_pnl / rph_oos on fixed inputs
       python tools/scan_ab.py compare A.npz B.npz   exit 1 unless every array of A equals B's bit for bit
       python tools/scan_ab.py timing OUT.jsonl [REPEATS]   k_hedge_pnl / k_hedge_oos at 2^20 paths x 30 dates

k_hedge_pnl and k_hedge_oos are instantiations of shared scan bodies
(csrc/pnl_scan.h, csrc/oos_scan.h); their machine code is not instruction for
instruction that of the commit before the bodies were shared.  This tool is
how their outputs were shown to be unchanged, and how the "parent" column of
BENCHMARKS.md "Transaction costs" was measured: it uses only HipBackend.pnl /
.oos without costs, so the same file runs in a checkout of an earlier commit
(copy it there, build that checkout, `dump` / `timing`), and `compare` takes
the two files.  RPH_NATIVE_LIB=<path>.so selects another library in one
checkout where that library exports every symbol the bindings ask for.

dump: rph_pnl on the twelve network shapes (synthetic tables of
tests/test_gpu_pnl.py; n = 2500 x 7 dates and 1025 x 2; the one-network shapes
also with the stopping rule of an exercise run): per-path P&L and statistics
rows; rph_oos on the five families of tests/test_gpu_oos.py (n = 2500 at an
unaligned offset, 2048 aligned; one and two networks): per-path P&L,
statistics rows and the price trace.
"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

SHAPES = [((1, 8, 2, 0), False), ((1, 8, 1, 1), False), ((3, 8, 2, 0), True), ((5, 8, 6, 0), False),
          ((2, 8, 2, 0), False), ((4, 8, 2, 0), False), ((6, 8, 7, 0), True), ((1, 32, 1, 1), False),
          ((1, 32, 2, 0), False), ((2, 32, 2, 0), True), ((3, 32, 2, 0), False), ((5, 32, 6, 0), False)]


def dump(out: str):
    import test_gpu_oos as T
    import torch
    from test_gpu_eval import make_spec
    from test_gpu_pnl import HOLD_C, make_tables

    from rphedge.engine import Exercise, HipBackend, PnlData, TrainConfig
    from rphedge.ops import layout as L

    dev = torch.device("cuda", 0)
    arrays = {}
    for shape, has_b in SHAPES:
        spec = make_spec(shape)
        for n, nd in ((2500, 7), (1025, 2)):
            tb = make_tables(spec, n, nd, has_b, seed=1000 * nd + n)
            be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
            feats = [f.to(dev) for f in tb["feats"]]
            prices = [p.to(dev) for p in tb["prices"]]
            data = PnlData(n_dates=nd, features=lambda t: [f[t] for f in feats], prices=lambda t: [p[t] for p in prices],
                           bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev), fisd=tb["fisd"].to(dev),
                           w0=tb["w0"].to(dev), payoff=tb["payoff"].to(dev))
            for ex in ((None,) if has_b else (None, Exercise("put", 1.0, 1))):
                slab = torch.zeros(be.pnl_wgs(), L.EVAL_NSTAT, dtype=torch.float64, device=dev)
                pnl = torch.empty(n, device=dev)
                tau = torch.empty(n, dtype=torch.int32, device=dev) if ex else None
                be.pnl(tb["snap"].to(dev), data, slab, has_b=has_b, hold_c=HOLD_C if has_b else 0.0, pnl_out=pnl,
                       exercise=ex, tau_out=tau)
                torch.cuda.synchronize()
                k = f"pnl{shape}{n}_{nd}_{ex is not None}"
                arrays[k], arrays[k + "s"] = pnl.cpu().numpy(), slab.cpu().numpy()
    for fam in T.FAMILIES:
        model, stat, shape, kind = fam
        spec = make_spec(shape)
        for n, off in ((2500, 37), (2048, 0)):
            for has_b in (False, True):
                g = T.mini_grid(18, 4)
                nd = g.n_coarse - 1
                tb = T.make_tables(spec, nd, has_b, "variance" if model == "heston" else "stat")
                tr = T.launch(dev, spec, T.sim_desc(g, n, off, model, stat, dev), tb, nd, has_b, kind)
                k = f"oos{fam}{n}_{has_b}"
                arrays[k], arrays[k + "s"], arrays[k + "t"] = tr["pnl"], tr["raw"], tr["s"]
    np.savez(out, **arrays)
    print(f"{len(arrays)} arrays -> {out}")


def compare(a: str, b: str) -> int:
    x, y = np.load(a), np.load(b)
    bad = [k for k in x.files if k not in y.files or not np.array_equal(x[k], y[k], equal_nan=True)]
    print(f"arrays {len(x.files)}, differing {len(bad)}: {bad[:10]}")
    return 1 if bad or set(x.files) != set(y.files) else 0


def timing(out: str, repeats: int = 9):
    import torch

    import bench
    from rphedge import oos
    from rphedge.api import HedgeRun
    from rphedge.engine import PnlData
    from rphedge.ops import layout as L

    run = HedgeRun(bench.build_run(bench.parse(["--preset", "euro30", "--seed", "1"]), 1))
    run.run()
    ind, be, dev = run.induction, run.backend, run.device
    n, nd = run.n_local, ind.n_dates
    st = torch.zeros(be.pnl_wgs(), L.EVAL_NSTAT, dtype=torch.float64, device=dev)
    sim = oos._fused_scan(run, n, 0, oos.table_seeds(oos.OOS_SEED), None, False)[1]
    data = PnlData(n_dates=nd, features=None, prices=None, bond=ind.pnl_data.bond, fmu=ind.pnl_data.fmu,
                   fisd=ind.pnl_data.fisd, w0=None, wealth0=oos.fitted_v0(run), payoff=None)
    ost = torch.zeros(be.oos_wgs(n), L.EVAL_NSTAT, dtype=torch.float64, device=dev)
    kind, strike = oos.payoff_code(run)
    fns = {"k_hedge_pnl": lambda: be.pnl(ind.snap, ind.pnl_data, st),
           "k_hedge_oos": lambda: be.oos(sim, ind.snap, data, ost, kind, strike)}
    for fn in fns.values():   # warm-up of each
        fn()
    torch.cuda.synchronize()

    def timed(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():   # alternating
            ms[k].append(timed(fn))
    rec = {"library": os.environ.get("RPH_NATIVE_LIB", "") or "this checkout", "paths": n, "dates": nd, "ms": ms,
           "median_ms": {k: sorted(v)[repeats // 2] for k, v in ms.items()}}
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    run.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "dump" and len(sys.argv) == 3:
        dump(sys.argv[2])
    elif mode == "compare" and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif mode == "timing" and len(sys.argv) >= 3:
        timing(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 9)
    else:
        sys.exit(__doc__)
