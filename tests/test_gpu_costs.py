"""k_hedge_pnl_cost / k_hedge_oos_cost (HipBackend.pnl / .oos with ``costs``:
the forward scans under proportional transaction costs and a no-trade band)
on an MI355X.

A. k_hedge_pnl_cost against the fp64 recursion (test_costs_cpu.cost_recursion)
   on the synthetic tables of test_gpu_pnl.  u = 2^-24, na = traded assets.
   - The band decision ``|target - held| > band`` is an fp32 threshold: a path
     whose fp64 difference comes within MARGIN of the band at any date may
     decide differently and is left out - those paths only.  MARGIN: the scan
     test's committed summary measures at most 7.9 u max|ref| per date between
     the fp32 and the fp64 recursion for the 8-unit nets (test_gpu_pnl.py);
     the holdings are one part of that date's roundings, so 7.9 u hmax bounds
     their difference, times a safety factor 8 = 64 u hmax for each of target
     and held position: MARGIN = 128 u hmax (hmax = max |holding|, about 8e-6).
     The left-out share is asserted <= 2 %.  Measured on the CPU from the fp64
     reference alone over every case below: 0.0 % at band 0 (no decision), at
     most 0.10 % at band 0.03 (1 of 1000 paths: (2, 8, 2, 0) at 2 dates, the
     5-asset net at 2 and at 5 dates); the band holds back 0 - 13 % of the trades.
   - P&L: the scan test's ``32 nd u max|ref|`` plus the fp32 bound of the
     accumulated cost, tol_c below.  cost_T and turnover: (na + 8)(nd + 1) u max
     (per date na + 1 roundings of the sum, the rate, the carry factor and its
     fma, the accumulation) plus the holdings' own error through MARGIN.
     ``trades_out`` exactly.  The cstats rows against fp64 sums of the
     kernel's own per-path outputs (rel 1e-12; counts exactly).
B. Bitwise: rate = 0, band = 0 is rph_pnl / rph_oos on the same inputs, P&L and
   statistics rows; two launches of one descriptor are identical.
C. k_hedge_oos_cost against the materialised cost route on its own trace
   (k_payoff, then k_hedge_pnl_cost): the agreement test_gpu_oos establishes
   for the frictionless kernels (64 nd u max|pnl|; trade counts exactly).
D. The launchers reject every bad descriptor before any launch.
E. End to end: a 2^12-path euro call with costs, captured and replayed; against
   the torch backend; against the run without costs.  Two ranks on one card.

Measured on an MI355X.  A: the largest error over the 120 cases is 0.11 of the
P&L tolerance, 0.05 of the cost and of the turnover tolerance; at most 0.10 %
of the paths left out; the trade counts of all the others exact.  B: bitwise on
every shape.  C: fused and materialised agree on every path (0 u) in P&L, cost
and turnover for the four families, both launch geometries.  E: the LM run's
cost scan is within 3.3e-7 per path of the oracle's scan of the same hedge
(sums to rel 4e-7 at worst, the same trades per path); on two ranks every key of
``costs`` printed equal to the one-rank run's to the last digit.
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_costs_cpu import cost_recursion
from test_gpu_dp import _port
from test_gpu_eval import U, check_guards, guarded, make_spec
from test_gpu_kernels import dev  # noqa: F401  (fixture)
from test_gpu_pnl import HOLD_C, make_tables

pytestmark = pytest.mark.gpu

RATE = 2e-3
# (1, 8, 1, COMPLEMENT), (1, 8, 2, FREE), (2, 8, 2, FREE), the pension net with two networks, the 5-asset basket net
CASES = [((1, 8, 1, 1), False), ((1, 8, 2, 0), False), ((2, 8, 2, 0), False), ((3, 8, 2, 0), True),
         ((5, 8, 6, 0), False)]
MARGIN_U = 128.0
EXCLUDED_CAP = 0.02


def _seed(n, nd):
    return 1000 * nd + n


def _data(tb, nd, dev, w0=True):  # noqa: F811
    from rphedge.engine import PnlData

    feats = [f.to(dev) for f in tb["feats"]]
    prices = [p.to(dev) for p in tb["prices"]]
    return PnlData(n_dates=nd, features=lambda t: [f[t] for f in feats], prices=lambda t: [p[t] for p in prices],
                   bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev), fisd=tb["fisd"].to(dev),
                   w0=tb["w0"].to(dev) if w0 else None, payoff=tb["payoff"].to(dev))


def _scan(be, dev, tb, nd, has_b, costs, n):  # noqa: F811
    """One launch of HipBackend.pnl (costs None: the plain scan); host arrays, guards checked."""
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC

    wgs = be.pnl_wgs()
    slab = torch.full((wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    bufs = {"pnl": guarded(n, dev)}
    kw = {}
    if costs is not None:
        bufs.update(cost=guarded(n, dev), turn=guarded(n, dev))
        tbuf = torch.full((n + 128,), -7, dtype=torch.int32, device=dev)
        cslab = torch.full((wgs, LC.COST_NSTAT), float("nan"), dtype=torch.float64, device=dev)
        kw = dict(costs=costs, cost_stats=cslab, cost_out=bufs["cost"][1], turn_out=bufs["turn"][1],
                  trades_out=tbuf[64:64 + n])
    be.pnl(tb["snap"].to(dev), _data(tb, nd, dev), slab, has_b=has_b, hold_c=HOLD_C if has_b else 0.0,
           pnl_out=bufs["pnl"][1], **kw)
    torch.cuda.synchronize()
    out = {}
    for k, (buf, v) in bufs.items():
        check_guards(k, buf)
        out[k] = v.cpu().numpy()
    out["stats"] = slab.cpu().numpy()
    if costs is not None:
        t = tbuf.cpu().numpy()
        assert np.all(t[:64] == -7) and np.all(t[64 + n:] == -7), "trades_out: guard band overwritten"
        out["trades"], out["cstats"] = t[64:64 + n], cslab.cpu().numpy()
    return out


# ---------------------------------------------------------------------------
# A. against the fp64 recursion
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [1, 2, 5])
@pytest.mark.parametrize("n", [1000, 1025])
@pytest.mark.parametrize("shape,has_b", CASES)
def test_pnl_cost_vs_fp64_recursion(dev, shape, has_b, n, nd):  # noqa: F811
    from rphedge.engine import Costs, HipBackend, TrainConfig, reduce_cost_stats
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC

    spec = make_spec(shape)
    na = spec.nhold - 1
    tb = make_tables(spec, n, nd, has_b, seed=_seed(n, nd))
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    wgs = (n + 1023) // 1024
    smax = max(float(p.max()) for p in tb["prices"])
    to_end = float(tb["bond"][nd] / tb["bond"][0])
    for band in (0.0, 0.03):
        for unwind in (False, True):
            tag = f"pnl_cost {shape} n={n} nd={nd} band={band} unwind={unwind}"
            ref = cost_recursion(spec, tb, nd, has_b, RATE, band, unwind, hold_c=HOLD_C if has_b else 0.0)
            margin = MARGIN_U * U * ref["hmax"]
            keep = ref["gap"] > margin
            share = float((~keep).mean())
            print(f"EXCLUDED {tag}: {100 * share:.2f} % (cap {100 * EXCLUDED_CAP:.0f} %)")
            assert share <= EXCLUDED_CAP, tag
            got = _scan(be, dev, tb, nd, has_b, Costs(RATE, band, unwind), n)
            assert np.array_equal(got["trades"][keep], ref["trades"][keep]), tag
            R = (na + 8) * (nd + 1) * U
            tol_t = R * float(ref["turn"].max()) + (nd + 1) * na * margin * smax
            tol_c = R * float(ref["cost"].max()) + (nd + 1) * na * margin * smax * RATE * to_end
            tol_p = 32 * nd * U * float(np.abs(ref["pnl"]).max()) + tol_c
            for name, tol in (("pnl", tol_p), ("cost", tol_c), ("turn", tol_t)):
                err = float(np.abs(got[name] - ref[name])[keep].max())
                print(f"ERR {tag} {name}: {err:.3e} (tol {tol:.3e})")
                assert err <= tol, f"{tag} {name}: {err:.3e} > {tol:.3e}"
            if band == 0.0:
                assert np.all(got["trades"] == nd - 1), tag
            # the cost rows: fp64 sums of the kernel's own per-path outputs, per workgroup
            cs = got["cstats"]
            assert cs.shape == (wgs, LC.COST_NSTAT) and not np.isnan(cs).any(), tag
            for w in range(wgs):
                sl = slice(1024 * w, min(n, 1024 * (w + 1)))
                c64, t64 = got["cost"][sl].astype(np.float64), got["turn"][sl].astype(np.float64)
                assert cs[w, LC.CS_COUNT] == sl.stop - sl.start and cs[w, LC.CS_TRADES] == got["trades"][sl].sum(), tag
                assert cs[w, LC.CS_COST] == pytest.approx(c64.sum(), rel=1e-12), tag
                assert cs[w, LC.CS_COST2] == pytest.approx((c64 * c64).sum(), rel=1e-12), tag
                assert cs[w, LC.CS_TURN] == pytest.approx(t64.sum(), rel=1e-12), tag
            assert np.all(cs[:, LC.CS_COUNT + 1:] == 0.0), tag
            assert reduce_cost_stats(torch.from_numpy(cs))[LC.CS_COUNT] == n
            # the P&L rows are the eval-stats rows of the net P&L
            st = got["stats"]
            assert not np.isnan(st).any() and st[:, L.ES_COUNT].sum() == n, tag
            assert st[:, L.ES_RES].sum() == pytest.approx(got["pnl"].astype(np.float64).sum(), rel=1e-9, abs=1e-9), tag


# ---------------------------------------------------------------------------
# B. bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,has_b", CASES)
def test_zero_costs_are_the_plain_scan_bitwise(dev, shape, has_b):  # noqa: F811
    from rphedge.engine import Costs, HipBackend, TrainConfig

    spec = make_spec(shape)
    for n, nd in ((1025, 5), (1000, 1)):
        tb = make_tables(spec, n, nd, has_b, seed=_seed(n, nd))
        be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
        plain = _scan(be, dev, tb, nd, has_b, None, n)
        zero = _scan(be, dev, tb, nd, has_b, Costs(0.0, 0.0), n)
        assert np.array_equal(plain["pnl"], zero["pnl"]), (shape, n, nd)
        assert np.array_equal(plain["stats"], zero["stats"]), (shape, n, nd)
        assert np.all(zero["cost"] == 0) and np.all(zero["trades"] == nd - 1) and np.all(zero["turn"] > 0)
        a = _scan(be, dev, tb, nd, has_b, Costs(RATE, 0.03, True), n)
        b = _scan(be, dev, tb, nd, has_b, Costs(RATE, 0.03, True), n)
        for k in a:
            assert np.array_equal(a[k], b[k]), (shape, n, nd, k)
        assert not np.array_equal(a["pnl"], plain["pnl"])


# ---------------------------------------------------------------------------
# C. the fused kernel against the materialised cost route
# ---------------------------------------------------------------------------
def _oos_launch(dev, spec, sim, tb, nd, kind, costs, wgs):  # noqa: F811
    """One traced k_hedge_oos(_cost) launch -> device tensors."""
    import test_gpu_oos as T

    from rphedge.engine import HipBackend, PnlData, TrainConfig
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC

    n, nc = int(sim.n_local), int(sim.n_coarse)
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    wgs = be.oos_wgs(n) if wgs is None else wgs
    o = {k: torch.full((sz,), float("nan"), device=dev) for k, sz in (("s", nc * n), ("x", nc * n), ("fin", n),
                                                                       ("fin2", n), ("pay", n), ("pnl", n),
                                                                       ("cost", n), ("turn", n))}
    o["trades"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
    sim.out, sim.out2 = o["s"].data_ptr(), o["x"].data_ptr()
    sim.final_out, sim.final2_out = o["fin"].data_ptr(), o["fin2"].data_ptr()
    o["stats"] = torch.full((wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    data = PnlData(n_dates=nd, features=None, prices=None, bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev),
                   fisd=tb["fisd"].to(dev), w0=None, payoff=None, wealth0=0.25)
    kw = {}
    if costs is not None:
        o["cstats"] = torch.full((wgs, LC.COST_NSTAT), float("nan"), dtype=torch.float64, device=dev)
        kw = dict(costs=costs, cost_stats=o["cstats"], cost_out=o["cost"], turn_out=o["turn"], trades_out=o["trades"])
    be.oos(sim, tb["snap"].to(dev), data, o["stats"], kind, T.STRIKE, pnl_out=o["pnl"], payoff_out=o["pay"], **kw)
    torch.cuda.synchronize()
    return be, data, o


OOS_FAMILIES = [("gbm", None, (1, 8, 2, 0), 2), ("gbm_log", None, (1, 8, 1, 1), 1), ("gbm_log", "mean", (2, 8, 2, 0), 4),
                ("heston", None, (2, 8, 2, 0), 1)]


@pytest.mark.parametrize("n,offset,wgs", [(1000, 37, None), (512, 0, 1)])
@pytest.mark.parametrize("fam", OOS_FAMILIES)
def test_oos_cost_matches_the_materialised_cost_route(dev, fam, n, offset, wgs):  # noqa: F811
    """(1000 paths at an unaligned offset: a partial last tile; 512 aligned on ONE
    workgroup: it loops over two tiles and starts each path's position afresh)"""
    import test_gpu_oos as T

    from rphedge.engine import Costs, PnlData
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC
    from rphedge.ops import native

    model, stat, shape, kind = fam
    spec = make_spec(shape)
    g = T.mini_grid(18, 4)
    nd = g.n_coarse - 1
    tb = T.make_tables(spec, nd, False, "variance" if model == "heston" else "stat")
    plain = _oos_launch(dev, spec, T.sim_desc(g, n, offset, model, stat, dev), tb, nd, kind, None, wgs)[2]
    zero = _oos_launch(dev, spec, T.sim_desc(g, n, offset, model, stat, dev), tb, nd, kind, Costs(0.0, 0.0), wgs)[2]
    assert torch.equal(plain["pnl"], zero["pnl"]) and torch.equal(plain["stats"], zero["stats"])   # bitwise rph_oos
    assert torch.all(zero["cost"] == 0) and torch.all(zero["trades"] == nd - 1)
    for band, unwind in ((0.0, False), (0.03, True)):
        costs = Costs(RATE, band, unwind)
        be, data, o = _oos_launch(dev, spec, T.sim_desc(g, n, offset, model, stat, dev), tb, nd, kind, costs, wgs)
        assert torch.equal(o["s"], plain["s"]) and torch.equal(o["pay"], plain["pay"])
        # the materialised route on the trace: k_payoff on the terminal state, then k_hedge_pnl_cost
        S, X = o["s"].view(nd + 1, n), o["x"].view(nd + 1, n)
        pay = torch.empty(n, device=dev)
        if kind <= 2:
            native.payoff(kind, o["fin2"] if stat is not None else o["fin"], pay, T.STRIKE)
        else:
            native.payoff(kind, o["fin"], pay, T.STRIKE, x=o["fin2"])
        assert torch.equal(pay, o["pay"])
        md = PnlData(n_dates=nd, features=(lambda t: [S[t], X[t]]) if spec.nin == 2 else (lambda t: [S[t]]),
                     prices=lambda t: [S[t]], bond=data.bond, fmu=data.fmu, fisd=data.fisd, w0=None, wealth0=0.25,
                     payoff=pay)
        mw = be.pnl_wgs(n)
        m = dict(pnl=torch.empty(n, device=dev), cost=torch.empty(n, device=dev), turn=torch.empty(n, device=dev),
                 trades=torch.empty(n, dtype=torch.int32, device=dev),
                 stats=torch.zeros(mw, L.EVAL_NSTAT, dtype=torch.float64, device=dev),
                 cstats=torch.zeros(mw, LC.COST_NSTAT, dtype=torch.float64, device=dev))
        be.pnl(tb["snap"].to(dev), md, m["stats"], pnl_out=m["pnl"], n_local=n, costs=costs, cost_stats=m["cstats"],
               cost_out=m["cost"], turn_out=m["turn"], trades_out=m["trades"])
        torch.cuda.synchronize()
        tag = f"oos_cost {fam} n={n} band={band}"
        assert torch.equal(o["trades"], m["trades"]), tag
        for name in ("pnl", "cost", "turn"):
            a, b = o[name].double().cpu().numpy(), m[name].double().cpu().numpy()
            scale = float(np.abs(b).max())
            err = float(np.abs(a - b).max())
            print(f"ROUTES {tag} {name}: fused - materialised {err / (U * scale):.2f} u max (bound {64 * nd})")
            assert err <= 64 * nd * U * scale, tag
        fs, ms = o["cstats"].sum(0).cpu().numpy(), m["cstats"].sum(0).cpu().numpy()
        assert fs[LC.CS_COUNT] == n == ms[LC.CS_COUNT] and fs[LC.CS_TRADES] == ms[LC.CS_TRADES]
        np.testing.assert_allclose(fs, ms, rtol=64 * nd * U)
        G = o["cstats"].shape[0]
        cnt = np.bincount((np.arange(n) // 256) % G, minlength=G)
        assert np.array_equal(o["cstats"][:, LC.CS_COUNT].cpu().numpy(), cnt.astype(np.float64))
        if band > 0:
            assert 0 < float(o["trades"].float().mean()) < nd - 1    # the band holds some trades back, not all


# ---------------------------------------------------------------------------
# D. host validation
# ---------------------------------------------------------------------------
def test_launchers_reject_bad_descriptors_before_any_launch(dev, monkeypatch):  # noqa: F811
    import test_gpu_oos as T

    from rphedge.engine import Costs, HipBackend, PnlData, TrainConfig
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC
    from rphedge.ops import native

    # the descriptors HipBackend would launch, captured instead of launched
    n, nd, spec = 1025, 2, make_spec((1, 8, 2, 0))
    tb = make_tables(spec, n, nd, False, seed=5)
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    st = torch.full((2, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    cst = torch.full((2, LC.COST_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    got = []
    real_pnl_cost, real_oos_cost = native.pnl_cost, native.oos_cost
    monkeypatch.setattr(native, "pnl_cost", lambda d, s=None: got.append(d))
    monkeypatch.setattr(native, "oos_cost", lambda d, s=None: got.append(d))
    data = _data(tb, nd, dev)
    snap = tb["snap"].to(dev)
    be.pnl(snap, data, st, costs=Costs(RATE, 0.03), cost_stats=cst)
    g = T.mini_grid(15, 2)
    otb = T.make_tables(spec, g.n_coarse - 1, False, "stat")
    okeep = [otb[k].to(dev) for k in ("snap", "bond", "fmu", "fisd")]
    odata = PnlData(n_dates=g.n_coarse - 1, features=None, prices=None, bond=okeep[1], fmu=okeep[2], fisd=okeep[3],
                    w0=None, payoff=None, wealth0=0.25)
    be.oos(T.sim_desc(g, 512, 0, "gbm_log", None, dev), okeep[0], odata, st, 1, 1.0, costs=Costs(RATE, 0.03),
           cost_stats=cst)
    pd, od = got
    assert isinstance(pd, native.CostPnlDesc) and isinstance(od, native.CostOosDesc)
    bad = [("c.cost_rate", float("nan"), "cost_rate must be finite and >= 0"),
           ("c.cost_rate", float("inf"), "cost_rate must be finite and >= 0"),
           ("c.cost_rate", -1e-3, "cost_rate must be finite and >= 0"),
           ("c.cost_rate", 1.5, "cost_rate must be <= 1"),
           ("c.band", float("nan"), "band must be finite and >= 0"),
           ("c.band", -0.01, "band must be finite and >= 0"),
           ("c.cstats", None, "null cstats")]
    for which, base, check, launch, extra in (
            ("rph_pnl_cost", pd, native.pnl_cost_check, real_pnl_cost,
             [("p.ex_kind", 1, "ex_kind with costs"), ("p.stats", None, "bad P&L descriptor"),
              ("p.num_wgs", 1, "num_wgs does not match"), ("p.h", 16, "unsupported network shape")]),
            ("rph_oos_cost", od, native.oos_cost_check, real_oos_cost,
             [("o.stats", None, "null snapshot or statistics pointer"), ("o.num_wgs", 3, "num_wgs must be in"),
              ("o.nin", 3, "unsupported network shape")])):
        for field, value, msg in bad + extra:
            d = type(base).from_buffer_copy(base)
            obj, name = field.split(".")
            setattr(getattr(d, obj), name, value)
            if field == "p.ex_kind":
                d.p.ex_every, d.p.ex_strike = 1, 1.0
            fns = (launch,) if field in ("p.h",) else (check, launch)   # (rph_pnl_cost's shape table is the launcher's)
            for fn in fns:
                with pytest.raises(RuntimeError, match=msg) as e:
                    fn(d)
                assert f"{which} failed with code -22" in str(e.value), (field, str(e.value))
    torch.cuda.synchronize()
    assert torch.isnan(st).all() and torch.isnan(cst).all()          # nothing was launched
    real_pnl_cost(pd)                                                # the captured descriptor itself runs
    torch.cuda.synchronize()
    assert float(st[:, L.ES_COUNT].sum()) == n and float(cst[:, LC.CS_COUNT].sum()) == n
    st.fill_(float("nan"))
    cst.fill_(float("nan"))
    real_oos_cost(od)
    torch.cuda.synchronize()
    assert float(st[:, L.ES_COUNT].sum()) == 512 and float(cst[:, LC.CS_COUNT].sum()) == 512
    # the Python front end refuses mis-sized buffers and stray cost outputs
    with pytest.raises(ValueError, match="cost_stats must be float64"):
        be.pnl(snap, data, st, costs=Costs(RATE), cost_stats=cst[:1])
    with pytest.raises(ValueError, match="trades_out must be"):
        be.pnl(snap, data, st, costs=Costs(RATE), cost_stats=cst, trades_out=torch.empty(n, device=dev))
    with pytest.raises(ValueError, match="cost outputs without costs"):
        be.pnl(snap, data, st, cost_stats=cst)


# ---------------------------------------------------------------------------
# E. end to end
# ---------------------------------------------------------------------------
E2E_RTOL = 2e-2   # test_gpu_exercise.test_e2e_matches_torch
FRICTIONLESS = ("terminal_pnl", "self_financing_pnl", "terminal_residual", "v0", "phi", "psi")


def euro_params(**kw):
    p = dict(Y=100, K=100, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.125, N=1, P=1, x=0, l0=0, c=0, ita=0,
             dt=0.125 / 4, n_paths=12, payoff="call", option_type="CALL", model="gbm_log", mortality=False, q99=False,
             optimizer="lm", lm_passes_first=80, lm_passes_rest=3, early_stopping=False, verbose=False,
             cost_rate=1e-3, rebalance_band=0.02)
    p.update(kw)
    return p


@pytest.fixture(scope="module")
def euro_run(dev):  # noqa: F811
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(euro_params(device=str(dev))))
    res = run.run()
    yield run, res
    run.close()


def test_e2e_graph_replay_bitwise(euro_run):
    run, res = euro_run
    eager = [res.induction.values.clone(), res.induction.pnl_paths.clone(), res.induction.cost_pnl_paths.clone()]
    run.capture(include_simulation=True)
    costs = []
    for _ in range(2):
        run.replay()
        r = run.collect()
        for a, b in zip(eager, [r.induction.values, r.induction.pnl_paths, r.induction.cost_pnl_paths]):
            assert torch.equal(a, b)
        costs.append(r.costs)
    assert costs[0] == costs[1] == res.costs and res.costs["mean_cost"] > 0


def test_e2e_frictionless_fields_unchanged(euro_run, dev):  # noqa: F811
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run, res = euro_run
    free_run = HedgeRun(parse_params(euro_params(device=str(dev), cost_rate=0.0, rebalance_band=0.0)))
    free = free_run.run()
    assert free.costs is None
    for k in FRICTIONLESS:
        assert getattr(res, k) == getattr(free, k), k
    assert torch.equal(res.induction.pnl_paths, free.induction.pnl_paths)
    assert torch.equal(res.induction.values, free.induction.values)
    assert res.costs["gross_pnl_std"] == free.self_financing_pnl["std"]
    # out of sample: both routes, the frontier
    o = run.out_of_sample(paths_log2=12)
    m = run.out_of_sample(paths_log2=12, fused=False)
    assert o.route == "fused" and m.route == "materialised"
    for k in ("net_pnl_std", "mean_cost", "mean_turnover"):
        assert o.costs[k] == pytest.approx(m.costs[k], rel=1e-5), k
    assert o.costs["trades_per_path"] == m.costs["trades_per_path"]
    assert o.std == free_run.out_of_sample(paths_log2=12).std
    rows = run.cost_frontier([0.0, 0.02, 0.1], paths_log2=12)
    assert rows[0]["mean_cost"] > rows[1]["mean_cost"] > rows[2]["mean_cost"]
    assert rows[1]["mean_cost"] == o.costs["mean_cost"]
    free_run.close()


def test_e2e_lm_cost_scan_matches_the_oracle_scan(euro_run):
    """The LM run's cost figures against the oracle on the SAME hedge: the torch
    backend scans the run's own paths with the run's fitted snapshots under the
    run's costs.  Per path the two differ by fp32 rounding (the bound of A: about
    32 nd u = 1.5e-5 of max|P&L|) except where the band decision falls within
    128 u hmax of the band - about 1e-5 / 0.02 of the decisions, each moving one
    trade: means and std to rel 1e-4, trades per path to 5e-3."""
    from rphedge.engine import PnlData, TorchBackend, TrainConfig, reduce_cost_stats, reduce_stats
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC

    run, res = euro_run
    ind, n = run.induction, run.n_local
    pd = ind.pnl_data
    data = PnlData(n_dates=pd.n_dates, features=lambda t: [f.cpu() for f in pd.features(t)],
                   prices=lambda t: [p.cpu() for p in pd.prices(t)], bond=pd.bond.cpu(), fmu=pd.fmu.cpu(),
                   fisd=pd.fisd.cpu(), w0=pd.w0.cpu(), payoff=pd.payoff.cpu())
    be = TorchBackend(run.spec, n, TrainConfig(batch_size=n))
    st = torch.zeros(1, L.EVAL_NSTAT, dtype=torch.float64)
    cst = torch.zeros(1, LC.COST_NSTAT, dtype=torch.float64)
    pnl = torch.empty(n)
    be.pnl(ind.snap.cpu(), data, st, hold_c=ind.hold_c, pnl_out=pnl, costs=run.costs, cost_stats=cst)
    got, gc = reduce_stats(ind.cost_pnl_stats), reduce_cost_stats(ind.cost_stats)
    want, wc = st[0].numpy(), cst[0].numpy()
    assert gc[LC.CS_COUNT] == wc[LC.CS_COUNT] == n
    for name, a, b in (("mean cost", gc[LC.CS_COST], wc[LC.CS_COST]), ("turnover", gc[LC.CS_TURN], wc[LC.CS_TURN]),
                       ("cost^2", gc[LC.CS_COST2], wc[LC.CS_COST2]), ("net P&L^2", got[L.ES_RES2], want[L.ES_RES2]),
                       ("wealth", got[L.ES_V], want[L.ES_V])):
        print(f"ORACLE {name}: hip {a / n!r} torch {b / n!r}")
        assert a == pytest.approx(b, rel=1e-4), name
    assert abs(got[L.ES_RES] - want[L.ES_RES]) / n <= 1e-4 * float(np.sqrt(want[L.ES_RES2] / n)), "net P&L mean"
    assert abs(gc[LC.CS_TRADES] - wc[LC.CS_TRADES]) / n <= 5e-3
    err = float((ind.cost_pnl_paths.cpu() - pnl).abs().max())
    print(f"ORACLE per path: max |hip - torch| {err:.3e}, trades/path {gc[LC.CS_TRADES] / n:.4f} vs {wc[LC.CS_TRADES] / n:.4f}")


ADAM = dict(optimizer="adam", deterministic=True, batch_size=1 << 12, epochs_first=300, epochs_rest=40,
            lr_schedule_first=False, lr=1e-2)


def test_e2e_matches_torch(dev):  # noqa: F811
    """HIP against the torch backend (same Sobol paths, same initial weights) on
    every figure of ``costs``, to the tolerance of test_gpu_exercise.test_e2e_matches_torch
    (rel 2e-2).  The pair runs full-batch Keras-Adam with the fixed-order
    reduction: there the two backends take the same steps, so the fitted hedges
    - and with them every cost figure - are the same hedge.  (The LM run of the
    other end-to-end tests is no such pair: the backends' LM fits end 5.6 % apart
    in the FRICTIONLESS P&L std at 2^12 paths - 1.751 hip vs 1.658 torch - and
    the cost figures follow the hedge: net P&L std 1.775 vs 1.673, mean cost
    0.1614 vs 0.1530; the analytic anchors agree to 2e-7.)"""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(euro_params(device=str(dev), **ADAM)))
    res = run.run()
    run.close()
    rt = HedgeRun(parse_params(euro_params(device="cpu", backend="torch", **ADAM)))
    rest = rt.run()
    rt.close()
    print(f"E2E hip {res.costs} | torch {rest.costs}")
    assert res.v0 == pytest.approx(rest.v0, rel=E2E_RTOL)
    for k in ("net_pnl_std", "gross_pnl_std", "mean_cost", "mean_turnover", "trades_per_path", "cost_share_of_v0",
              "bs_net_pnl_std", "bs_mean_cost", "leland_net_pnl_std"):
        assert res.costs[k] == pytest.approx(rest.costs[k], rel=E2E_RTOL), k
    for k in ("rate", "band", "unwind"):
        assert res.costs[k] == rest.costs[k]


def _dp_worker(rank, world, port, n, nd, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from rphedge.engine import Costs, HipBackend, TrainConfig, reduce_cost_stats, reduce_stats
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC

    d = torch.device("cuda", 0)
    torch.cuda.set_device(d)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    spec = make_spec((1, 8, 2, 0))
    tb = make_tables(spec, n, nd, False, seed=9)
    per = n // world
    sl = slice(rank * per, (rank + 1) * per)
    loc = dict(tb, feats=[f[:, sl].contiguous() for f in tb["feats"]], prices=[p[:, sl].contiguous() for p in tb["prices"]],
               w0=tb["w0"][sl].contiguous(), payoff=tb["payoff"][sl].contiguous())
    be = HipBackend(spec, per, TrainConfig(batch_size=n), device=d, world=world, rank=rank)
    st = torch.zeros(be.pnl_wgs(), L.EVAL_NSTAT, dtype=torch.float64, device=d)
    cst = torch.zeros(be.pnl_wgs(), LC.COST_NSTAT, dtype=torch.float64, device=d)
    be.pnl(loc["snap"].to(d), _data(loc, nd, d), st, costs=Costs(RATE, 0.03, True), cost_stats=cst)
    torch.cuda.synchronize()
    np.save(out + f".{rank}.npy", np.concatenate([reduce_stats(st, world), reduce_cost_stats(cst, world)]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_card_pool_the_cost_slab(dev):  # noqa: F811
    """Each rank scans its shard; the pooled statistics (reduce_stats / reduce_cost_stats
    over the ranks) are the one-rank result on the same global paths."""
    from rphedge.engine import Costs, HipBackend, TrainConfig, reduce_cost_stats, reduce_stats
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC

    n, nd, world = 4096, 5, 2
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "s")
        ctx = mp.get_context("spawn")
        port = _port()
        procs = [ctx.Process(target=_dp_worker, args=(r, world, port, n, nd, out)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        r0, r1 = np.load(out + ".0.npy"), np.load(out + ".1.npy")
    assert np.array_equal(r0, r1)
    spec = make_spec((1, 8, 2, 0))
    tb = make_tables(spec, n, nd, False, seed=9)
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    st = torch.zeros(be.pnl_wgs(), L.EVAL_NSTAT, dtype=torch.float64, device=dev)
    cst = torch.zeros(be.pnl_wgs(), LC.COST_NSTAT, dtype=torch.float64, device=dev)
    be.pnl(tb["snap"].to(dev), _data(tb, nd, dev), st, costs=Costs(RATE, 0.03, True), cost_stats=cst)
    torch.cuda.synchronize()
    one = np.concatenate([reduce_stats(st), reduce_cost_stats(cst)])
    # (the same per-path fp32 values summed in fp64 in another grouping)
    np.testing.assert_allclose(r0, one, rtol=1e-12, atol=1e-12)
    assert r0[L.ES_COUNT] == n and r0[L.EVAL_NSTAT + LC.CS_COUNT] == n
    assert r0[L.EVAL_NSTAT + LC.CS_TRADES] == one[L.EVAL_NSTAT + LC.CS_TRADES]


# --- the whole run on two ranks (the harness of test_gpu_dp.test_pension_both_fits_lm_world_invariant) ---
def _euro_dp_run(di):
    """The 2^14-path euro call with costs in leaf mode (LM pass leaves of 256
    paths: the data-parallel fits are bitwise the one-rank fits), then its
    out-of-sample test: (record of the cost figures, weight snapshots)."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    cfg = parse_params(euro_params(n_paths=14, device="cuda:0", lm_leaf_paths=256))
    run = HedgeRun(cfg, dist_info=di) if di is not None else HedgeRun(cfg)
    res = run.run()
    torch.cuda.synchronize()
    o = run.out_of_sample(paths_log2=13)
    rows = run.cost_frontier([0.0, 0.05], paths_log2=13)
    snap = run.induction.snap.cpu().numpy().copy()
    rec = dict(v0=res.v0, costs=res.costs, gross=res.self_financing_pnl, oos=o.costs, oos_std=o.std, route=o.route,
               frontier=rows, n_local=run.n_local)
    run.close()
    return rec, snap


def _worker_euro_dp(rank, world, port, out):
    import json

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    from rphedge.parallel import dist as D

    di = D.init()
    rec, snap = _euro_dp_run(di)
    np.save(out + f".{rank}.npy", snap)
    with open(out + f".{rank}.json", "w") as fh:
        json.dump(rec, fh)
    D.barrier()
    D.shutdown()


def _same_costs(tag, got, want):
    """Key by key: the settings and the trade counts (integer sums) exactly, every
    pooled fp64 moment to rel 1e-9 (the same per-path fp32 values summed in
    another grouping, as test_pension_both_fits_lm_world_invariant allows)."""
    assert set(got) == set(want), tag
    for k, v in want.items():
        if k == "in_sample":
            if v is None:
                assert got[k] is None, tag
            else:
                _same_costs(tag + ".in_sample", got[k], v)
        elif k in ("rate", "band", "unwind", "trades_per_path", "net_pnl_min", "net_pnl_max"):
            assert got[k] == v, (tag, k, got[k], v)
        elif v is None:
            assert got[k] is None, (tag, k)
        else:
            assert got[k] == pytest.approx(v, rel=1e-9, abs=1e-12), (tag, k, got[k], v)


def test_euro_run_with_costs_two_ranks_one_card():
    """The euro run with cost_rate / rebalance_band data parallel on one card:
    each rank scans its shard, the cost slab is pooled with the other
    statistics, and ``RunResult.costs`` - the BS / Leland anchors' pooled
    moments included -, ``OosResult.costs`` with its in-sample block and the
    frontier rows equal the one-rank run's on the same global paths."""
    import json

    world = 2
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "e")
        ctx = mp.get_context("spawn")
        port = _port()
        procs = [ctx.Process(target=_worker_euro_dp, args=(r, world, port, out)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        recs = [json.load(open(out + f".{r}.json")) for r in range(world)]
        snaps = [np.load(out + f".{r}.npy") for r in range(world)]
    ref, snap1 = _euro_dp_run(None)
    assert ref["costs"] is not None and ref["costs"]["mean_cost"] > 0 and ref["oos"]["in_sample"] is not None
    for r in range(world):
        rec = recs[r]
        print(f"DP rank {r}: costs {rec['costs']} | one rank {ref['costs']}")
        assert rec["n_local"] * world == ref["n_local"]
        assert np.array_equal(snaps[r], snap1), np.abs(snaps[r] - snap1).max()
        assert rec["v0"] == pytest.approx(ref["v0"], rel=1e-9)
        _same_costs(f"rank {r} costs", rec["costs"], ref["costs"])
        assert rec["gross"]["std"] == pytest.approx(ref["gross"]["std"], rel=1e-9)
        assert rec["route"] == ref["route"] == "fused"
        _same_costs(f"rank {r} oos", rec["oos"], ref["oos"])
        assert rec["oos_std"] == pytest.approx(ref["oos_std"], rel=1e-9)
        for a, b in zip(rec["frontier"], ref["frontier"]):
            _same_costs(f"rank {r} frontier", a, b)
    _same_costs("ranks", recs[0]["costs"], recs[1]["costs"])
