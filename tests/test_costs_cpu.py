"""Proportional transaction costs and the no-trade band, without a GPU: the
``Costs`` / config validation, the torch oracle (``TorchBackend.pnl(costs=...)``)
against the plain fp64 numpy recursion below, its identities, the BS / Leland
delta hedges under costs, the layout table of the cost descriptors, the host
checks of the two launchers and the feature end to end on the torch backend.

Semantics (csrc/rph_types.h CostTerms): per asset the held position starts at
0 and follows the network's target where ``t == 0``, ``band == 0`` or
``|target - held| > band``; date t costs ``rate sum_a |dh_a| S_a,t``, taken off
the wealth before the scan's update; ``unwind`` sells the final position at the
horizon.  By-products per path: the cost carried to the horizon, the turnover,
the dates ``t >= 1`` with a trade.
"""
import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from test_pnl import _np_forward

U = 2.0 ** -24
HOLD_C = 0.1
GOLDEN = Path(__file__).parent / "golden" / "bs_delta_hedge_parent.json"


def f32(x) -> float:
    return float(np.float32(x))


def make_spec(shape, alpha=0.3):
    from rphedge.models.hedge_mlp import NetSpec

    nin, h, nout, head = shape
    return NetSpec(nin=nin, hidden=h, nout=nout, head=head, alpha=alpha)


def hand_tables(spec, n, nd, has_b, seed):
    """Hand-made ``[nd + 1, n]`` feature / price tables, per-date snapshots,
    standardisation and bond (the construction of test_gpu_pnl.make_tables with
    plain N(0, 0.5) weights)."""
    from rphedge.engine import MAXIN
    from rphedge.ops import layout as L

    g = torch.Generator().manual_seed(seed)
    na = spec.nhold - 1
    feats = [(f + 1) * (0.75 + 0.5 * torch.rand(nd + 1, n, generator=g)) for f in range(spec.nin)]
    prices = [(k + 1) * (0.8 + 0.4 * torch.rand(nd + 1, n, generator=g)) for k in range(na)]
    fmu, fisd = torch.zeros(nd, MAXIN), torch.ones(nd, MAXIN)
    for t in range(nd):
        for f in range(spec.nin):
            fmu[t, f] = (f + 1) * (1.0 + 0.02 * t)
            fisd[t, f] = (1.0 + 0.1 * f + 0.05 * t) / ((f + 1) * 0.15)
    snap = torch.zeros(nd, 2, L.NETW_FLOATS)
    ws = np.zeros((nd, 2, spec.nparams), np.float32)
    for t in range(nd):
        for k in range(2 if has_b else 1):
            ws[t, k] = (0.5 * torch.randn(spec.nparams, generator=g)).numpy()
            snap[t, k, :spec.nparams] = torch.from_numpy(ws[t, k])
    bond = torch.tensor([1.03 ** (0.7 * t) for t in range(nd + 1)], dtype=torch.float64)
    w0 = 0.8 + 0.4 * torch.rand(n, generator=g)
    payoff = torch.rand(n, generator=g)
    return dict(feats=feats, prices=prices, fmu=fmu, fisd=fisd, snap=snap, ws=ws, bond=bond, w0=w0, payoff=payoff)


def cost_recursion(spec, tb, nd, has_b, rate, band, unwind, hold_c=HOLD_C, w0=None):
    """The semantics in fp64 (numpy); ``rate`` / ``band`` enter as the fp32
    values of a descriptor.  Returns a dict: W, pnl, cost, turn, trades, and
    ``gap`` = per path the smallest ``| |target - held| - band |`` over the band
    decisions taken (dates >= 1; inf without one) and ``hmax`` = max |holding|."""
    na = spec.nhold - 1
    n = tb["payoff"].numel()
    W = (tb["w0"].double().numpy().copy() if w0 is None else np.full(n, f32(w0), np.float64))
    bond = tb["bond"].numpy()
    alpha, rate, band = f32(spec.alpha), f32(rate), f32(band)
    held = np.zeros((n, na))
    cost, turn, trades = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    gap = np.full(n, np.inf)
    hmax = 0.0
    S = [np.stack([p[t].double().numpy() for p in tb["prices"]], axis=1) for t in range(nd + 1)]
    for t in range(nd):
        X = np.stack([f[t].double().numpy() for f in tb["feats"]], axis=1)
        X = (X - tb["fmu"][t, :spec.nin].double().numpy()) * tb["fisd"][t, :spec.nin].double().numpy()
        h = _np_forward(spec, tb["ws"][t, 0].astype(np.float64), X, alpha)
        if has_b:
            hb = _np_forward(spec, tb["ws"][t, 1].astype(np.float64), X, alpha)
            h = h + f32(hold_c) * (hb - h)
        target = h[:, :na]
        hmax = max(hmax, float(np.abs(target).max()))
        d = np.abs(target - held)
        if t == 0 or band == 0.0:
            tr = np.ones_like(d, bool)
        else:
            tr = d > band
            gap = np.minimum(gap, np.abs(d - band).min(axis=1))
        new = np.where(tr, target, held)
        dv = (np.abs(new - held) * S[t]).sum(axis=1)
        c = rate * dv
        W = W - c
        cost += c * f32(bond[nd] / bond[t])
        turn += dv
        if t > 0:
            trades += tr.any(axis=1)
        held = new
        grow = f32(bond[t + 1] / bond[t])
        W = W * grow + (held * (S[t + 1] - S[t] * grow)).sum(axis=1)
    if unwind:
        dv = (np.abs(held) * S[nd]).sum(axis=1)
        W, cost, turn = W - rate * dv, cost + rate * dv, turn + dv
    return dict(W=W, pnl=W - tb["payoff"].double().numpy(), cost=cost, turn=turn, trades=trades, gap=gap, hmax=hmax,
                held=held)


def pnl_data(tb, nd, dev="cpu"):
    from rphedge.engine import PnlData

    feats = [f.to(dev) for f in tb["feats"]]
    prices = [p.to(dev) for p in tb["prices"]]
    return PnlData(n_dates=nd, features=lambda t: [f[t] for f in feats], prices=lambda t: [p[t] for p in prices],
                   bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev), fisd=tb["fisd"].to(dev), w0=tb["w0"].to(dev),
                   payoff=tb["payoff"].to(dev))


def oracle(spec, tb, nd, has_b, costs):
    """TorchBackend.pnl on the tables -> dict of numpy arrays and the two statistics rows."""
    from rphedge.engine import TorchBackend, TrainConfig
    from rphedge.ops import layout as L
    from rphedge.ops import layout_cost as LC

    n = tb["payoff"].numel()
    be = TorchBackend(spec, n, TrainConfig(batch_size=n))
    st = torch.zeros(1, L.EVAL_NSTAT, dtype=torch.float64)
    out = dict(pnl=torch.empty(n))
    kw = {}
    if costs is not None:
        out.update(cost=torch.empty(n), turn=torch.empty(n), trades=torch.empty(n, dtype=torch.int32))
        cst = torch.zeros(1, LC.COST_NSTAT, dtype=torch.float64)
        kw = dict(costs=costs, cost_stats=cst, cost_out=out["cost"], turn_out=out["turn"], trades_out=out["trades"])
    be.pnl(tb["snap"], pnl_data(tb, nd), st, has_b=has_b, hold_c=HOLD_C if has_b else 0.0, pnl_out=out["pnl"], **kw)
    res = {k: v.numpy() for k, v in out.items()}
    res["stats"] = st[0].numpy()
    if costs is not None:
        res["cstats"] = cst[0].numpy()
    return res


# ---------------------------------------------------------------------------
# configuration
# ---------------------------------------------------------------------------
def test_costs_validation():
    from rphedge.engine import Costs

    k = Costs(rate=1e-3)
    assert (k.rate, k.band, k.unwind, k.active) == (1e-3, 0.0, False, True)
    assert not Costs(rate=0.0).active and Costs(rate=0.0, band=0.1).active and Costs(rate=1.0).active
    for bad in (dict(rate=-1e-3), dict(rate=float("nan")), dict(rate=float("inf")), dict(rate=1.0001),
                dict(rate=1e-3, band=-0.1), dict(rate=1e-3, band=float("nan")), dict(rate=1e-3, band=float("inf")),
                dict(rate="1e-3"), dict(rate=None), dict(rate=True)):
        with pytest.raises(ValueError, match="cost (rate|band) must be"):
            Costs(**bad)


def _euro_params(**kw):
    p = dict(Y=100, K=100, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.125, N=1, P=1, x=0, l0=0, c=0, ita=0,
             dt=0.125 / 4, n_paths=10, payoff="call", option_type="CALL", model="gbm_log", mortality=False, q99=False,
             verbose=False, device="cpu", backend="torch", epochs_first=20, epochs_rest=5)
    p.update(kw)
    return p


def test_config_validation():
    from rphedge.api import HedgeRun
    from rphedge.config import RunConfig, parse_params

    c = RunConfig()
    assert (c.cost_rate, c.rebalance_band, c.cost_unwind) == (0.0, 0.0, False)
    assert HedgeRun(parse_params(_euro_params())).costs is None
    k = HedgeRun(parse_params(_euro_params(cost_rate=2e-3, rebalance_band=0.05, cost_unwind=True))).costs
    assert (k.rate, k.band, k.unwind) == (2e-3, 0.05, True)
    assert HedgeRun(parse_params(_euro_params(rebalance_band=0.05))).costs.rate == 0.0   # a band alone is a scan too
    for bad in (dict(cost_rate=-1e-3), dict(cost_rate=float("nan")), dict(cost_rate=1.5), dict(rebalance_band=-0.01),
                dict(rebalance_band=float("inf")), dict(cost_rate="x")):
        with pytest.raises(ValueError, match="cost_rate / rebalance_band"):
            HedgeRun(parse_params(_euro_params(**bad)))
    with pytest.raises(ValueError, match="cost_unwind"):
        HedgeRun(parse_params(_euro_params(cost_unwind=True)))
    with pytest.raises(ValueError, match="cost_unwind must be a bool"):
        HedgeRun(parse_params(_euro_params(cost_rate=1e-3, cost_unwind="yes")))
    with pytest.raises(KeyError, match="unknown params key"):
        parse_params(_euro_params(cost_band=0.1))
    # early exercise with costs is out of scope: a clear error at config time
    for ex in ("bermudan", "american"):
        with pytest.raises(ValueError, match="early exercise with transaction costs is not supported"):
            HedgeRun(parse_params(_euro_params(payoff="put", option_type="PUT", exercise=ex, cost_rate=1e-3)))


def test_backends_refuse_costs_with_exercise():
    from rphedge.engine import Costs, Exercise

    spec = make_spec((1, 8, 2, 0))
    tb = hand_tables(spec, 16, 2, False, 1)
    from rphedge.engine import TorchBackend, TrainConfig
    from rphedge.ops import layout as L

    be = TorchBackend(spec, 16, TrainConfig(batch_size=16))
    st = torch.zeros(1, L.EVAL_NSTAT, dtype=torch.float64)
    with pytest.raises(ValueError, match="costs with exercise"):
        be.pnl(tb["snap"], pnl_data(tb, 2), st, exercise=Exercise("put", 1.0), costs=Costs(1e-3),
               cost_stats=torch.zeros(1, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="cost outputs without costs"):
        be.pnl(tb["snap"], pnl_data(tb, 2), st, cost_out=torch.empty(16))


# ---------------------------------------------------------------------------
# the oracle against the fp64 recursion
# ---------------------------------------------------------------------------
ORACLE_SHAPES = [((1, 8, 2, 0), False), ((5, 8, 6, 0), False)]


@pytest.mark.parametrize("nd", [1, 2, 5])
@pytest.mark.parametrize("shape,has_b", ORACLE_SHAPES)
def test_oracle_vs_fp64_recursion(shape, has_b, nd):
    """n = 257.  Tolerances (u = 2^-24): the P&L ``32 nd u max|ref|`` of the
    scan tests plus the cost's own roundings, ``(na + 8)(nd + 1) u max cost``;
    cost and turnover ``(na + 8)(nd + 1) u max``.  Paths whose fp64 band
    decision comes within ``256 u hmax`` of the band may decide differently in
    fp32 and are left out (at most 2 %); the trade counts of the others are exact."""
    from rphedge.engine import Costs
    from rphedge.ops import layout_cost as LC

    n, spec = 257, make_spec(shape)
    na = spec.nhold - 1
    tb = hand_tables(spec, n, nd, has_b, seed=10 * nd + na)
    for band in (0.0, 0.03, 0.3):
        for unwind in (False, True):
            rate = 2e-3
            ref = cost_recursion(spec, tb, nd, has_b, rate, band, unwind, hold_c=HOLD_C if has_b else 0.0)
            got = oracle(spec, tb, nd, has_b, Costs(rate, band, unwind))
            keep = ref["gap"] > 256 * U * ref["hmax"]
            assert (~keep).mean() <= 0.02
            R = (na + 8) * (nd + 1) * U
            tol_c, tol_t = R * float(ref["cost"].max()), R * float(ref["turn"].max())
            tol_p = 32 * nd * U * float(np.abs(ref["pnl"]).max()) + tol_c
            assert np.abs(got["pnl"] - ref["pnl"])[keep].max() <= tol_p
            assert np.abs(got["cost"] - ref["cost"])[keep].max() <= tol_c
            assert np.abs(got["turn"] - ref["turn"])[keep].max() <= tol_t
            assert np.array_equal(got["trades"][keep], ref["trades"][keep])
            if band == 0.0:
                assert np.all(got["trades"] == nd - 1)
            cs = got["cstats"]
            assert cs[LC.CS_COUNT] == n and cs[LC.CS_TRADES] == got["trades"].sum()
            assert cs[LC.CS_COST] == pytest.approx(got["cost"].astype(np.float64).sum(), rel=1e-12)
            assert cs[LC.CS_COST2] == pytest.approx((got["cost"].astype(np.float64) ** 2).sum(), rel=1e-12)
            assert cs[LC.CS_TURN] == pytest.approx(got["turn"].astype(np.float64).sum(), rel=1e-12)
            assert np.all(cs[LC.CS_COUNT + 1:] == 0)


@pytest.mark.parametrize("shape,has_b", ORACLE_SHAPES + [((3, 8, 2, 0), True)])
def test_oracle_identities(shape, has_b):
    from rphedge.engine import Costs

    n, nd, spec = 257, 5, make_spec(shape)
    na = spec.nhold - 1
    tb = hand_tables(spec, n, nd, has_b, seed=77)
    plain = oracle(spec, tb, nd, has_b, None)
    # rate = 0, band = 0: the plain scan, bit for bit
    zero = oracle(spec, tb, nd, has_b, Costs(0.0, 0.0))
    assert np.array_equal(zero["pnl"], plain["pnl"]) and np.array_equal(zero["stats"], plain["stats"])
    assert np.all(zero["cost"] == 0) and np.all(zero["trades"] == nd - 1)
    # band = 0: the hedge is the frictionless one, so net = gross - cost_T up to fp32 rounding.  The cost c_t
    # leaves the wealth at date t and grows to c_t B_n / B_t: with the nd factors g_s rounded to fp32 and one
    # rounding per wealth update, |net - (gross - cost_T)| <= 4 (nd + 1) u (max|W| + max cost_T) - every one of
    # the (nd + 1) steps rounds the wealth (relative u, magnitude <= max|W|) at most 3 times in either scan and
    # the carried cost once
    rate = 2e-3
    b0 = oracle(spec, tb, nd, has_b, Costs(rate, 0.0))
    wmax = float(np.abs(plain["pnl"] + tb["payoff"].numpy()).max())
    bound = 4 * (nd + 1) * U * (wmax + float(b0["cost"].max()))
    assert np.abs(b0["pnl"].astype(np.float64) - (plain["pnl"].astype(np.float64) - b0["cost"])).max() <= bound
    assert b0["cost"].min() > 0
    # band = +large: one purchase at date 0, then a frozen hedge
    big = oracle(spec, tb, nd, has_b, Costs(rate, 1e6))
    ref = cost_recursion(spec, tb, 1, has_b, rate, 0.0, False, hold_c=HOLD_C if has_b else 0.0)   # date 0's trade
    assert np.all(big["trades"] == 0)
    # turnover = |phi*_0| S_0: the fp32 holdings are within 256 u hmax of the fp64 ones (the band margin above)
    smax = max(float(p[0].max()) for p in tb["prices"])
    np.testing.assert_allclose(big["turn"], ref["turn"], rtol=(na + 8) * U, atol=na * 256 * U * ref["hmax"] * smax)
    frozen = cost_recursion(spec, tb, nd, has_b, rate, 1e6, False, hold_c=HOLD_C if has_b else 0.0)
    assert np.array_equal(frozen["held"], ref["held"])    # (the recursion's own hedge stays date 0's)
    tol = 32 * nd * U * float(np.abs(frozen["pnl"]).max()) + (na + 8) * (nd + 1) * U * float(frozen["cost"].max())
    assert np.abs(big["pnl"] - frozen["pnl"]).max() <= tol
    # unwinding adds the sale of the final position
    un = oracle(spec, tb, nd, has_b, Costs(rate, 0.0, True))
    # (a final position near zero sells for nothing: >= per path, > on the whole)
    assert np.all(un["cost"] >= b0["cost"]) and np.all(un["turn"] >= b0["turn"]) and np.all(un["pnl"] <= b0["pnl"])
    assert un["cost"].sum() > b0["cost"].sum() and un["turn"].sum() > b0["turn"].sum()


# ---------------------------------------------------------------------------
# analytic anchors
# ---------------------------------------------------------------------------
def _bs_grid():
    from rphedge.ops import paths as P

    g = P.Grid(1.0, 1.0 / 13, 1.0 / 13)
    p = P.simulate_gbm(g, 1 << 10, 100.0, 0.08, 0.15, scheme="log", norm=100.0, device="cpu")
    return g, p


def test_bs_delta_hedge_defaults_unchanged():
    """Bitwise against the values the parent commit's bs_delta_hedge returned on this grid (tests/golden)."""
    from rphedge import analytic

    g, p = _bs_grid()
    a = analytic.bs_delta_hedge(p.S, g.bond(0.08), 1.0, 0.08, 0.15, 1.0, g.times())
    want = json.loads(GOLDEN.read_text())
    assert set(a) == set(want["call"])
    for k, v in want["call"].items():
        assert a[k] == float.fromhex(v) if isinstance(v, str) else a[k] == v, k
    b = analytic.bs_delta_hedge(p.S, g.bond(0.08), 1.0, 0.08, 0.15, 1.0, g.times(), "PUT")
    for k, v in want["put"].items():
        assert b[k] == float.fromhex(v) if isinstance(v, str) else b[k] == v, k


def test_bs_delta_hedge_with_costs_vs_recursion():
    from rphedge import analytic

    g, p = _bs_grid()
    S, B, tt = p.S.double().numpy(), np.asarray(g.bond(0.08), np.float64), np.asarray(g.times())
    rate, band, sig, r, k = 1e-3, 0.05, 0.15, 0.08, 1.0
    nc, n = S.shape

    def delta(s, tau, sigma):
        d1 = (np.log(s / k) + (r + 0.5 * sigma * sigma) * tau) / (sigma * math.sqrt(tau))
        return np.array([0.5 * math.erfc(-x / math.sqrt(2.0)) for x in d1])

    for sh, unwind in ((None, False), (analytic.leland_sigma(sig, rate, 1.0 / 13), True)):
        a = analytic.bs_delta_hedge(p.S, B, k, r, sig, 1.0, tt, cost_rate=rate, band=band, unwind=unwind,
                                    sigma_hedge=sh)
        w = np.full(n, a["price"])
        held, cost, turn, trades = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        for t in range(nc - 1):
            dl = delta(S[t], 1.0 - tt[t], sig if sh is None else sh)
            tr = np.ones(n, bool) if t == 0 else np.abs(dl - held) > band
            new = np.where(tr, dl, held)
            dv = np.abs(new - held) * S[t]
            gr = B[t + 1] / B[t]
            w = (w - rate * dv) * gr + new * (S[t + 1] - S[t] * gr)
            cost += rate * dv * B[-1] / B[t]
            turn += dv
            trades += tr if t > 0 else 0
            held = new
        if unwind:
            dv = np.abs(held) * S[-1]
            w, cost, turn = w - rate * dv, cost + rate * dv, turn + dv
        pnl = w - np.maximum(S[-1] - k, 0)
        assert a["pnl_mean"] == pytest.approx(pnl.mean(), abs=1e-12)
        assert a["pnl_std"] == pytest.approx(pnl.std(ddof=1), rel=1e-10)
        assert a["mean_cost"] == pytest.approx(cost.mean(), rel=1e-10)
        assert a["mean_turnover"] == pytest.approx(turn.mean(), rel=1e-10)
        assert a["trades_per_path"] == pytest.approx(trades.mean(), rel=1e-12)
        assert 0 < a["trades_per_path"] < nc - 2
    free = analytic.bs_delta_hedge(p.S, B, k, r, sig, 1.0, tt)
    assert "mean_cost" not in free
    with pytest.raises(ValueError, match="cost_rate must be finite"):
        analytic.bs_delta_hedge(p.S, B, k, r, sig, 1.0, tt, cost_rate=-1.0)


def test_leland_sigma_hand_value():
    from rphedge.analytic import leland_sigma

    # sigma 0.2, rate 0.01, dt 0.04: sqrt(8/pi) = 1.5957691216..., 0.01 / (0.2 * 0.2) = 0.25
    # -> 0.2 sqrt(1 + 0.3989422804) = 0.2 * 1.1827689040 = 0.2365537808
    assert leland_sigma(0.2, 0.01, 0.04) == pytest.approx(0.2365537808, abs=1e-9)
    assert leland_sigma(0.2, 0.0, 0.04) == 0.2
    with pytest.raises(ValueError):
        leland_sigma(0.0, 0.01, 0.04)


# ---------------------------------------------------------------------------
# layout and host checks of the launchers
# ---------------------------------------------------------------------------
def test_cost_layout_table():
    from rphedge.ops import layout_cost as LC
    from rphedge.ops import native

    lib = native.load(required=True)
    fields, consts = native.native_layout_cost(lib)
    classes = (native.CostTerms,) + native.DESCRIPTORS_COST
    assert native.DESCRIPTORS_COST == (native.CostPnlDesc, native.CostOosDesc)
    assert native.layout_mismatches(fields, consts, classes=classes, layout=LC) == []
    assert dict(consts) == {"COST_NSTAT": 8, "CS_COST": 0, "CS_COST2": 1, "CS_TURN": 2, "CS_TRADES": 3, "CS_COUNT": 4}
    assert {s for s, _, _, _ in fields} == {"CostTerms", "CostPnlDesc", "CostOosDesc"}
    assert C.sizeof(native.CostPnlDesc) == C.sizeof(native.PnlDesc) + C.sizeof(native.CostTerms)
    assert C.sizeof(native.CostOosDesc) == C.sizeof(native.OosDesc) + C.sizeof(native.CostTerms)
    f = list(native.CostTerms._fields_)
    i, j = [x[0] for x in f].index("cost_rate"), [x[0] for x in f].index("band")
    g = list(f)
    g[i], g[j] = g[j], g[i]
    swapped = type("CostTerms", (C.Structure,), {"_fields_": g})
    bad = native.layout_mismatches(fields, consts, classes=(swapped,), layout=LC)
    assert len(bad) == 2 and any("CostTerms.cost_rate" in b for b in bad) and any("CostTerms.band" in b for b in bad)
    dropped = type("CostTerms", (C.Structure,), {"_fields_": [x for x in f if x[0] != "trades_out"]})
    bad = native.layout_mismatches(fields, consts, classes=(dropped,), layout=LC)
    assert any("CostTerms.trades_out" in b and "not in ctypes" in b for b in bad)
    assert any(b.startswith("CostTerms: native size") for b in bad)
    import types

    off = types.SimpleNamespace(**{**{k: v for k, v in vars(LC).items() if k.isupper()}, "CS_TURN": 5})
    assert native.layout_mismatches(fields, consts, classes=classes, layout=off) == ["layout.CS_TURN: native 2, python 5"]
    # the earlier tables are as they were
    assert native.DESCRIPTORS_EXT == (native.OosDesc,) and len(native.DESCRIPTORS) == 7


def _fake(n=4):
    """A live host buffer to point descriptor fields at (the checks never dereference them)."""
    return (C.c_double * n)()


def _valid_pnl_cost(keep):
    from rphedge.ops import native

    d = native.CostPnlDesc()
    p = d.p
    buf = _fake()
    keep.append(buf)
    a = C.addressof(buf)
    p.feat[0], p.price[0], p.feat_ts[0], p.price_ts[0] = a, a, 8, 8
    p.snap = p.fmu = p.fisd = p.bond = p.payoff = p.stats = a
    p.alpha, p.n_local, p.n_dates, p.num_wgs = 0.3, 8, 2, 1
    p.nin, p.h, p.nout, p.head = 1, 8, 2, 0
    d.c.cost_rate, d.c.band, d.c.cstats = 1e-3, 0.02, a
    return d


def test_pnl_cost_check_rejects_each_bad_field():
    from rphedge.ops import native

    keep = []
    native.pnl_cost_check(_valid_pnl_cost(keep))
    bad = [("c.cost_rate", float("nan"), "cost_rate must be finite and >= 0"),
           ("c.cost_rate", float("inf"), "cost_rate must be finite and >= 0"),
           ("c.cost_rate", -1e-3, "cost_rate must be finite and >= 0"),
           ("c.cost_rate", 1.5, "cost_rate must be <= 1"),
           ("c.band", float("nan"), "band must be finite and >= 0"),
           ("c.band", float("inf"), "band must be finite and >= 0"),
           ("c.band", -0.01, "band must be finite and >= 0"),
           ("c.cstats", None, "null cstats"),
           ("p.ex_kind", 1, "ex_kind with costs"),
           ("p.snap", None, "bad P&L descriptor"),            # the embedded descriptor's own checks come first
           ("p.num_wgs", 2, "num_wgs does not match"),
           ("p.h", 16, r"unsupported network shape")]
    for field, value, msg in bad:
        d = _valid_pnl_cost(keep)
        obj, name = field.split(".")
        setattr(getattr(d, obj), name, value)
        if field == "p.ex_kind":
            d.p.ex_every, d.p.ex_strike = 1, 1.0
        fn = native.pnl_cost if field == "p.h" else native.pnl_cost_check   # (the shape table is the launcher's)
        with pytest.raises(RuntimeError, match=msg) as e:
            fn(d, 0) if field == "p.h" else fn(d)
        assert "rph_pnl_cost failed with code -22" in str(e.value), (field, str(e.value))


def test_oos_cost_check_rejects_each_bad_field():
    from rphedge.ops import layout as L
    from rphedge.ops import native

    keep = []

    def valid():
        d = native.CostOosDesc()
        o, s = d.o, d.o.sim
        buf = _fake()
        keep.append(buf)
        a = C.addressof(buf)
        s.model, s.n_local, s.n_fine, s.reduction, s.n_coarse, s.na = L.SIM_GBM_LOG, 512, 15, 2, 8, 1
        s.sv1 = s.shift1 = a
        s.dims1 = 15
        o.snap = o.fmu = o.fisd = o.bond = o.stats = a
        o.alpha, o.wealth0, o.strike, o.payoff_kind, o.n_dates, o.num_wgs = 0.3, 0.25, 1.0, 1, 7, 2
        o.nin, o.h, o.nout, o.head = 1, 8, 2, 0
        d.c.cost_rate, d.c.band, d.c.cstats = 1e-3, 0.02, a
        return d

    native.oos_cost_check(valid())
    bad = [("c.cost_rate", float("nan"), "cost_rate must be finite and >= 0"),
           ("c.cost_rate", -1e-3, "cost_rate must be finite and >= 0"),
           ("c.cost_rate", 1.0001, "cost_rate must be <= 1"),
           ("c.band", float("inf"), "band must be finite and >= 0"),
           ("c.band", -0.01, "band must be finite and >= 0"),
           ("c.cstats", None, "null cstats"),
           ("o.stats", None, "null snapshot or statistics pointer"),
           ("o.payoff_kind", 3, "payoff_kind must be 1, 2, 4 or 5")]
    for field, value, msg in bad:
        d = valid()
        obj, name = field.split(".")
        setattr(getattr(d, obj), name, value)
        with pytest.raises(RuntimeError, match=msg) as e:
            native.oos_cost_check(d)
        assert "rph_oos_cost failed with code -22" in str(e.value), (field, str(e.value))


# ---------------------------------------------------------------------------
# end to end on the torch backend
# ---------------------------------------------------------------------------
FRICTIONLESS = ("terminal_pnl", "self_financing_pnl", "terminal_residual", "v0", "phi", "psi")


@pytest.fixture(scope="module")
def euro_runs():
    """The 2^10-path euro call without costs and under rate 1e-3 at three bands (torch backend)."""
    from rphedge.api import european_option

    kw = dict(n_paths=10, backend="torch", device="cpu", verbose=False, rebalancing_frequency=1 / 8, dt=1 / 32,
              epochs_first=20, epochs_rest=5)
    free = european_option(**kw)
    return free, [european_option(cost_rate=1e-3, rebalance_band=b, **kw) for b in (0.0, 0.02, 0.1)]


def test_e2e_torch_costs(euro_runs):
    free, runs = euro_runs
    assert free.costs is None
    keys = {"rate", "band", "unwind", "net_pnl_mean", "net_pnl_std", "net_pnl_min", "net_pnl_max", "gross_pnl_std",
            "mean_cost", "cost_share_of_v0", "mean_turnover", "trades_per_path", "bs_net_pnl_std", "bs_mean_cost",
            "leland_net_pnl_std", "leland_mean_cost"}
    for r, band in zip(runs, (0.0, 0.02, 0.1)):
        c = r.costs
        assert set(c) == keys and c["rate"] == 1e-3 and c["band"] == band and c["unwind"] is False
        assert all(math.isfinite(c[k]) for k in keys - {"unwind"})
        assert c["mean_cost"] > 0 and 0 < c["cost_share_of_v0"] < 0.2 and c["net_pnl_min"] <= c["net_pnl_max"]
        assert c["gross_pnl_std"] == free.self_financing_pnl["std"]
        # every frictionless field is the run's without costs
        for k in FRICTIONLESS:
            assert getattr(r, k) == getattr(free, k), k
        assert r.summary["terminal_pnl_std"] == free.summary["terminal_pnl_std"]
        assert torch.equal(r.induction.pnl_paths, free.induction.pnl_paths)
    assert runs[0].costs["trades_per_path"] == 7.0          # band 0 trades at every date after the first
    t = [r.costs["trades_per_path"] for r in runs]
    m = [r.costs["mean_cost"] for r in runs]
    assert t[0] > t[1] > t[2] and m[0] > m[1] > m[2]


def test_out_of_sample_costs_cpu_route():
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params
    from rphedge.engine import Costs

    run = HedgeRun(parse_params(_euro_params(cost_rate=1e-3, rebalance_band=0.02)))
    res = run.run()
    o = run.out_of_sample(paths_log2=9)
    assert o.route == "materialised" and o.costs["rate"] == 1e-3 and o.costs["band"] == 0.02
    assert o.costs["gross_pnl_std"] == o.std and o.costs["mean_cost"] > 0
    ins = o.costs["in_sample"]
    for k in ("net_pnl_std", "mean_cost", "trades_per_path", "mean_turnover"):
        assert ins[k] == pytest.approx(res.costs[k], rel=1e-12), k
    assert run.out_of_sample(paths_log2=9, costs=False).costs is None
    a = run.out_of_sample(paths_log2=9, costs=Costs(2e-3, 0.0))
    b = run.out_of_sample(paths_log2=9, costs={"rate": 2e-3})
    assert a.costs["rate"] == 2e-3 and a.costs["band"] == 0.0 and a.costs["trades_per_path"] == 7.0
    assert {k: v for k, v in a.costs.items()} == {k: v for k, v in b.costs.items()}
    assert a.std == o.std and a.mean == o.mean           # the result's own figures stay frictionless
    with pytest.raises(ValueError, match="costs dict takes"):
        run.out_of_sample(paths_log2=9, costs={"band": 0.1})
    with pytest.raises(ValueError, match="costs must be"):
        run.out_of_sample(paths_log2=9, costs=0.001)
    rows = run.cost_frontier([0.0, 0.02, 0.1, 0.5], paths_log2=9)
    assert [r["band"] for r in rows] == [0.0, 0.02, 0.1, 0.5]
    assert set(rows[0]) == {"band", "mean_cost", "net_pnl_std", "net_pnl_mean", "trades_per_path"}
    cost = [r["mean_cost"] for r in rows]
    assert all(x > y for x, y in zip(cost, cost[1:]))      # monotone in cost
    assert rows[0]["mean_cost"] == pytest.approx(o.costs["in_sample"]["mean_cost"], rel=0.5)
    tr = [r["trades_per_path"] for r in rows]
    assert all(x >= y for x, y in zip(tr, tr[1:]))
    with pytest.raises(ValueError, match="cost_frontier needs a cost rate > 0"):
        run.cost_frontier([0.0, 0.1], rate=0.0, paths_log2=9)
    with pytest.raises(ValueError, match="bands must be finite and >= 0"):
        run.cost_frontier([0.0, -0.1], paths_log2=9)
    run.close()
