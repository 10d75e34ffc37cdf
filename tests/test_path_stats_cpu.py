"""Path-dependent options on the host: the fp64 numpy twin of the scan's
running statistics (ops.paths._cpu_gbm), the geometric Asian closed form and
the public entry point.

* the twin's recursion (running sum / extreme) against independent formulas
  (``cumsum`` / ``maximum.accumulate`` over the full fine matrix rebuilt from
  the same Sobol normals): both fp64, so 1e-12 relative;
* grid A (T=1, dt=1/32, rebalancing=1/8) ends its coarse grid on the last
  fine point; grid B (dt=1/30, rebalancing=1/4: 31 fine points, reduction 7)
  ends it at fine point 28 != 30, so ``stat_final`` is not ``stat[-1]``;
* m <= G <= A <= M on every path and date, all equal S_0 at date 0;
* Monte-Carlo price of the geometric Asian call within ONE iid standard error
  of the closed form that is exact for the log-Euler scheme (Sobol points:
  measured 0.04 standard errors at 2^14 paths).
"""
import math

import numpy as np
import pytest

from rphedge.ops import paths as P

GRID_A = dict(T=1.0, dt=1 / 32, rebalancing=1 / 8)
GRID_B = dict(T=1.0, dt=1 / 30, rebalancing=1 / 4)
S0, MU, SIGMA = 1.0, 0.08, 0.15
STATS = ("mean", "geomean", "max", "min")


def _fine(grid, n, scheme, s0=S0):
    """The full fine matrix [n, n_fine] in closed form (no recursion over t)."""
    W = P._normals(grid.n_fine, P.SEED_W1, n, 0, grid.n_fine)[:, 1:]
    if scheme == "log":
        inc = (MU - 0.5 * SIGMA ** 2) * grid.dt + SIGMA * math.sqrt(grid.dt) * W
        S = s0 * np.exp(np.cumsum(inc, axis=1))
    else:
        S = s0 * np.cumprod(1.0 + MU * grid.dt + SIGMA * math.sqrt(grid.dt) * W, axis=1)
    return np.concatenate([np.full((n, 1), s0), S], axis=1)


def _stat_fine(S, stat):
    """The statistic at every fine point [n, n_fine] from the fine matrix."""
    j = np.arange(1, S.shape[1])
    out = np.empty_like(S)
    out[:, 0] = S[:, 0]
    if stat == "mean":
        out[:, 1:] = np.cumsum(S[:, 1:], axis=1) / j
    elif stat == "geomean":
        out[:, 1:] = np.exp(np.cumsum(np.log(S[:, 1:]), axis=1) / j)
    elif stat == "max":
        out = np.maximum.accumulate(S, axis=1)
    else:
        out = np.minimum.accumulate(S, axis=1)
    return out


def _cases():
    return [(s, st) for s in ("log", "arith") for st in STATS if not (s == "arith" and st == "geomean")]


def test_grids_are_what_the_cases_assume():
    a, b = P.Grid(**GRID_A), P.Grid(**GRID_B)
    assert (a.n_fine, a.reduction, a.n_coarse) == (33, 4, 9)
    assert (a.n_coarse - 1) * a.reduction == a.n_fine - 1
    assert (b.n_fine, b.reduction, b.n_coarse) == (31, 7, 5)
    assert (b.n_coarse - 1) * b.reduction == 28


@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["A", "B"])
@pytest.mark.parametrize("scheme,stat", _cases())
def test_twin_vs_independent_formulas(grid, scheme, stat):
    g = P.Grid(**grid)
    n = 64
    S, fin, A, afin = P._cpu_gbm(g, n, S0, MU, SIGMA, scheme, 0, P.SEED_W1, path_stat=stat)
    S0_, fin0 = P._cpu_gbm(g, n, S0, MU, SIGMA, scheme, 0, P.SEED_W1)
    assert np.array_equal(S, S0_) and np.array_equal(fin, fin0)  # the statistic does not touch the price
    F = _fine(g, n, scheme)
    ref = _stat_fine(F, stat)
    coarse = np.arange(g.n_coarse) * g.reduction
    np.testing.assert_allclose(S, F[:, coarse].T, rtol=1e-12)
    np.testing.assert_allclose(A, ref[:, coarse].T, rtol=1e-12)
    np.testing.assert_allclose(afin, ref[:, -1], rtol=1e-12)
    if coarse[-1] != g.n_fine - 1:  # grid B: the payoff's statistic is not the last coarse one
        assert np.all(afin != A[-1]) if stat in ("mean", "geomean") else np.any(afin != A[-1])
    else:
        assert np.array_equal(afin, A[-1])
    # the simulator of the torch / CPU backend returns the same numbers (fp32, normalised)
    p = P.simulate_gbm(g, n, 100.0 * S0, MU, SIGMA, scheme=scheme, norm=100.0, device="cpu", path_stat=stat)
    assert p.kind == "gbm_stat" and p.stat_kind == stat
    assert p.stat.shape == (g.n_coarse, n) and p.stat_final.shape == (n,)
    np.testing.assert_allclose(p.stat.numpy(), A, rtol=3e-7)
    np.testing.assert_allclose(p.stat_final.numpy(), afin, rtol=3e-7)
    f = p.features(2)
    assert len(f) == 2 and f[0] is not None and np.array_equal(f[1].numpy(), p.stat[2].numpy())
    assert len(p.prices(2)) == 1


@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["A", "B"])
def test_orderings(grid):
    g = P.Grid(**grid)
    n = 64
    r = {st: P._cpu_gbm(g, n, S0, MU, SIGMA, "log", 0, P.SEED_W1, path_stat=st) for st in STATS}
    m, G, A, M = (r[k][2] for k in ("min", "geomean", "mean", "max"))
    tiny = 1e-14  # (G <= A by AM-GM; equal up to rounding where one point is monitored)
    assert np.all(m <= G * (1 + tiny)) and np.all(G <= A * (1 + tiny)) and np.all(A <= M * (1 + tiny))
    mf, Gf, Af, Mf = (r[k][3] for k in ("min", "geomean", "mean", "max"))
    assert np.all(mf <= Gf * (1 + tiny)) and np.all(Gf <= Af * (1 + tiny)) and np.all(Af <= Mf * (1 + tiny))
    for k in STATS:
        assert np.all(r[k][2][0] == S0)
    ar = {st: P._cpu_gbm(g, n, S0, MU, SIGMA, "arith", 0, P.SEED_W1, path_stat=st) for st in ("min", "mean", "max")}
    assert np.all(ar["min"][2] <= ar["mean"][2] * (1 + tiny)) and np.all(ar["mean"][2] <= ar["max"][2] * (1 + tiny))
    for k in ar:
        assert np.all(ar[k][2][0] == S0)


def test_geo_asian_price_vs_closed_form():
    from rphedge.analytic import geo_asian_price

    g = P.Grid(**GRID_A)
    n, r, K = 1 << 14, 0.08, 1.0
    p = P.simulate_gbm(g, n, S0, r, SIGMA, scheme="log", device="cpu", path_stat="geomean")
    pay = P.payoff("geo_asian_call", p, K).double().numpy() * math.exp(-r * (g.n_fine - 1) * g.dt)
    mc, se = pay.mean(), pay.std(ddof=1) / math.sqrt(n)
    cf = geo_asian_price(S0, K, r, SIGMA, g.dt, g.n_fine - 1, "CALL")
    print(f"geo asian call: MC {mc:.6f}, closed form {cf:.6f}, {abs(mc - cf) / se:.3f} standard errors")
    assert abs(mc - cf) <= se
    # the put by parity: C - P = e^{-rT} (E[G] - K), E[G] from the same lognormal
    put = geo_asian_price(S0, K, r, SIGMA, g.dt, g.n_fine - 1, "PUT")
    G = p.stat_final.double().numpy()
    se_f = G.std(ddof=1) / math.sqrt(n) * math.exp(-r)
    assert abs((cf - put) - math.exp(-r) * (G.mean() - K)) <= se_f
    # one monitoring point: the geometric Asian is the European option on S_dt
    from rphedge.analytic import black_scholes

    assert abs(geo_asian_price(100.0, 95.0, 0.05, 0.2, 0.5, 1) - black_scholes(100.0, 95.0, 0.05, 0.2, 0.5, "CALL")[0]) < 1e-10


def test_payoff_names_cpu():
    g = P.Grid(**GRID_B)
    n, K = 256, 1.02
    by = {st: P.simulate_gbm(g, n, S0, MU, SIGMA, scheme="log", device="cpu", path_stat=st) for st in STATS}
    for name, (st, _) in P.PATH_PAYOFFS.items():
        p = by[st]
        s, x = p.S_final.numpy(), p.stat_final.numpy()
        want = {"asian_call": x - K, "geo_asian_call": x - K, "lookback_call": x - K,
                "asian_put": K - x, "geo_asian_put": K - x, "lookback_put": K - x,
                "asian_strike_call": s - x, "lookback_float_call": s - x,
                "asian_strike_put": x - s, "lookback_float_put": x - s}[name]
        got = P.payoff(name, p, K).numpy()
        assert np.array_equal(got, np.maximum(want, 0).astype(np.float32)), name
    assert np.all(P.payoff("lookback_float_call", by["min"], K).numpy() == (by["min"].S_final - by["min"].stat_final).numpy())
    with pytest.raises(ValueError):
        P.payoff("asian_call", by["max"], K)
    with pytest.raises(ValueError):
        P.simulate_gbm(g, n, S0, MU, SIGMA, scheme="arith", device="cpu", path_stat="geomean")
    with pytest.raises(ValueError):
        P.simulate_gbm(g, n, S0, MU, SIGMA, scheme="log", device="cpu", path_stat="median")


def _hedge_run(**extra):
    """The HedgeRun of european_option(**extra)'s parameters (the entry point returns only its result)."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    params = dict(Y=100.0, K=100.0, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=1 / 8, N=1, P=1.0, x=0.0,
                  l0=0.0, c=0.0, ita=0.0, dt=1 / 32, n_paths=12, option_type="CALL", model="gbm_log",
                  mortality=False, q99=False, verbose=False, device="cpu")
    params.update(extra)
    return HedgeRun(parse_params(params))


def test_api_geo_asian_cpu():
    import rphedge
    from rphedge.analytic import geo_asian_price

    kw = dict(N_paths=1 << 12, dt=1 / 32, rebalancing_frequency=1 / 8, epochs_first=4, epochs_rest=2,
              batch_size=512, verbose=False, device="cpu")
    run = _hedge_run(payoff="geo_asian_call")
    assert run.kind == "european" and (run.spec.nin, run.spec.nout) == (2, 2)
    assert _hedge_run(payoff="geo_asian_call", path_feature=False).spec.nin == 1
    assert _hedge_run(payoff="lookback_float_put", model="gbm").spec.nin == 2
    res = rphedge.european_option(payoff="geo_asian_call", **kw)
    assert res.holdings0.shape == (2,) and res.config["path_feature"] is True
    assert math.isfinite(res.v0) and math.isfinite(res.phi) and math.isfinite(res.psi)
    assert math.isfinite(res.terminal_pnl["std"])
    s = res.summary
    assert "bs_price" not in s and "bs_delta" not in s
    assert s["analytic_price"] == pytest.approx(geo_asian_price(100.0, 100.0, 0.08, 0.15, 1 / 32, 32, "CALL"))
    assert 0.0 < s["p_oom"] < 1.0
    pay = res.paths
    assert pay.kind == "gbm_stat" and pay.stat_kind == "geomean"
    zero = float((np.maximum(pay.stat_final.numpy() - 1.0, 0) == 0).mean())
    assert s["p_oom"] == pytest.approx(zero)
    # the discounted mean payoff is the closed form within 3 standard errors (0.12 measured at 2^12)
    disc = math.exp(-0.08)
    v = np.maximum(pay.stat_final.double().numpy() - 1.0, 0) * 100.0 * disc
    assert abs(v.mean() - s["analytic_price"]) <= 3 * v.std(ddof=1) / math.sqrt(v.size)
    # the ablation: same payoff, the net sees S alone
    res1 = rphedge.european_option(payoff="geo_asian_call", path_feature=False, **kw)
    assert math.isfinite(res1.v0) and len(res1.paths.features(1)) == 1 and len(res.paths.features(1)) == 2
    assert res1.summary["E_payoff"] == s["E_payoff"]
    # a plain call keeps its Black-Scholes anchors and gets no analytic_price
    res2 = rphedge.european_option(**kw)
    assert "bs_price" in res2.summary and "analytic_price" not in res2.summary


@pytest.mark.parametrize("extra", [dict(model="heston"), dict(model="basket"), dict(complement_head=True),
                                   dict(mortality=True), dict(payoff="geo_asian_put", model="gbm")])
def test_api_rejects(extra):
    import rphedge

    kw = dict(payoff="asian_call", N_paths=256, dt=1 / 8, rebalancing_frequency=1 / 4, verbose=False, device="cpu")
    kw.update(extra)
    with pytest.raises(ValueError):
        rphedge.european_option(**kw)
