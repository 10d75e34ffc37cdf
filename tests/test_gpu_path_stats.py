"""Path-dependent options on the GPU: the running statistics of k_sim_scan
(SimDesc.path_stat), the floating-strike payoff kinds 4 / 5, and Asian /
lookback hedges end to end.

Tolerances of the scan test are the ones ``test_gbm_paths_vs_numpy`` applies
to ``S`` (rtol 2e-6 with an fp64 recursion, 5e-5 in fp32): the statistic is a
mean of, or a choice among, at most N <= 32 such values, and a sequential
fp32 sum of N terms adds at most N 2^-24 ~ 2e-6.

The end-to-end caps (P&L std with the statistic as an input <= 0.70 x / 0.85 x
the std of the same net fed S alone) come from a host proxy on these exact
paths - a cubic least-squares hedge per date, no network: 0.445 (Asian),
0.438 (geometric Asian), 0.663 (lookback).

Measured on an MI355X: statistics at most 1.2e-7 relative off the twin with the
fp64 recursion, 2.8e-6 in fp32; geometric Asian V0 0.09 standard errors from
the closed form, P&L mean 1e-5; P&L std ratio 0.417 (Asian), 0.664 (lookback);
graph replay V0 equal to the eager run's to the last bit.
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_eval import check_guards, guarded
from test_gpu_kernels import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GRID_A = dict(T=1.0, dt=1 / 32, rebalancing=1 / 8)   # last coarse point = last fine point
GRID_B = dict(T=1.0, dt=1 / 30, rebalancing=1 / 4)   # 31 fine points, reduction 7: coarse grid ends at 28 != 30
S0, MU, SIGMA, NORM = 100.0, 0.08, 0.15, 100.0
CASES = [(s, st) for s in ("log", "arith") for st in ("mean", "geomean", "max", "min")
         if not (s == "arith" and st == "geomean")]

_TWIN = {}


def _twin(grid_key, n, scheme, stat):
    """fp64 host twin (computed once per case, read-only)."""
    from rphedge.ops import paths as P

    key = (grid_key, n, scheme, stat)
    if key not in _TWIN:
        g = P.Grid(**(GRID_A if grid_key == "A" else GRID_B))
        r = tuple(np.asarray(a) / NORM for a in P._cpu_gbm(g, n, S0, MU, SIGMA, scheme, 0, P.SEED_W1, path_stat=stat))
        for a in r:
            a.setflags(write=False)
        _TWIN[key] = r
    return _TWIN[key]


def _guarded_paths(P, g, n, dev, stat):  # noqa: F811
    """A Paths whose statistic buffers sit between guard bands."""
    sbuf, s2 = guarded(g.n_coarse * n, dev)
    fbuf, f2 = guarded(n, dev)
    p = P.Paths(kind="gbm_stat", grid=g, n_local=n, path_offset=0,
                S=torch.empty(g.n_coarse, n, dtype=torch.float32, device=dev), bond=g.bond(0.0),
                S_final=torch.empty(n, dtype=torch.float32, device=dev), norm=NORM,
                stat=s2.view(g.n_coarse, n), stat_final=f2, stat_kind=stat)
    return p, sbuf, fbuf


@pytest.mark.parametrize("grid_key", ["A", "B"])
@pytest.mark.parametrize("n", [1, 255, 257, 4096])
def test_scan_statistics_vs_twin(dev, n, grid_key):  # noqa: F811
    from rphedge.ops import paths as P

    g = P.Grid(**(GRID_A if grid_key == "A" else GRID_B))
    kw = dict(norm=NORM, device=dev)
    for scheme in ("log", "arith"):
        plain = {f: P.simulate_gbm(g, n, S0, MU, SIGMA, scheme=scheme, fp64=f, **kw) for f in (True, False)}
        for stat in [st for s, st in CASES if s == scheme]:
            S, fin, A, afin = _twin(grid_key, n, scheme, stat)
            for fp64, rtol in ((True, 2e-6), (False, 5e-5)):
                out, sbuf, fbuf = _guarded_paths(P, g, n, dev, stat)
                p = P.simulate_gbm(g, n, S0, MU, SIGMA, scheme=scheme, fp64=fp64, path_stat=stat, out=out, **kw)
                torch.cuda.synchronize()
                assert p is out
                check_guards(f"stat {stat}", sbuf)
                check_guards(f"stat_final {stat}", fbuf)
                tag = f"{scheme} {stat} fp64={fp64} n={n} grid {grid_key}"
                # the price is the plain run's, bit for bit
                assert torch.equal(p.S, plain[fp64].S) and torch.equal(p.S_final, plain[fp64].S_final), tag
                got, gfin = p.stat.cpu().numpy().astype(np.float64), p.stat_final.cpu().numpy().astype(np.float64)
                err = max(np.abs(got / A - 1).max(), np.abs(gfin / afin - 1).max())
                print(f"{tag}: max rel err {err:.2e} (bound {rtol:.0e})")
                np.testing.assert_allclose(got, A, rtol=rtol, err_msg=tag)
                np.testing.assert_allclose(gfin, afin, rtol=rtol, err_msg=tag)
                assert np.all(got[0] == np.float32(S0) * np.float32(1.0 / NORM))
                if grid_key == "B" and n > 1 and stat in ("mean", "geomean"):
                    assert not np.array_equal(gfin, got[-1])
    # a fresh allocation (no out=) gives the same numbers as the guarded buffers
    a = P.simulate_gbm(g, n, S0, MU, SIGMA, scheme="log", path_stat="mean", **kw)
    b, _, _ = _guarded_paths(P, g, n, dev, "mean")
    P.simulate_gbm(g, n, S0, MU, SIGMA, scheme="log", path_stat="mean", out=b, **kw)
    assert a.kind == "gbm_stat" and torch.equal(a.stat, b.stat) and torch.equal(a.stat_final, b.stat_final)


def test_simulate_rejects_bad_statistics(dev):  # noqa: F811
    from rphedge.ops import layout as L
    from rphedge.ops import native
    from rphedge.ops import paths as P
    from rphedge.ops.sobol import device_table

    g = P.Grid(**GRID_A)
    n = 256
    S = torch.empty(g.n_coarse, n, device=dev)
    A = torch.empty(g.n_coarse, n, device=dev)
    fin = torch.empty(n, device=dev)
    sv, sh, dims = device_table(g.n_fine, P.SEED_W1, dev)

    def desc(model, stat, out2=True):
        d = P._desc(model, n, 0, g, False, False)
        d.sv1, d.shift1, d.dims1 = sv.data_ptr(), sh.data_ptr(), dims
        d.sv2, d.shift2, d.dims2 = sv.data_ptr(), sh.data_ptr(), dims
        d.s0[0], d.mu[0], d.sigma[0], d.inv_norm[0] = 1.0, MU, SIGMA, 1.0
        d.v0, d.kappa, d.theta, d.xi, d.rho = 0.04, 2.0, 0.04, 0.3, -0.5
        d.out, d.final_out = S.data_ptr(), fin.data_ptr()
        if out2:
            d.out2 = A.data_ptr()
        d.path_stat = stat
        return d

    for d, what in ((desc(L.SIM_GBM_LOG, 5), "0..4"), (desc(L.SIM_GBM_LOG, -1), "0..4"),
                    (desc(L.SIM_HESTON, 1), "GBM"), (desc(L.SIM_GBM_LOG, 3, out2=False), "out2"),
                    (desc(L.SIM_GBM_ARITH, 2), "geomean")):
        with pytest.raises(RuntimeError, match=what):
            native.simulate(d)
    native.simulate(desc(L.SIM_GBM_ARITH, 1))  # the same descriptor, valid: runs
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="x array"):
        native.payoff(4, fin, torch.empty(n, device=dev), 0.0)


def test_statistics_shards_and_index_map_bitwise(dev):  # noqa: F811
    from rphedge.engine import gram_subsample
    from rphedge.ops import paths as P
    from rphedge.ops.paths import path_indices

    g = P.Grid(**GRID_B)
    kw = dict(norm=NORM, device=dev)
    n = 8192
    ns, blk, stride = gram_subsample(n, 2048)
    idx = torch.as_tensor(path_indices(ns, 0, (blk, stride)).astype(np.int64), device=dev)
    assert ns < n
    for scheme, stat in CASES:
        full = P.simulate_gbm(g, n, S0, MU, SIGMA, scheme=scheme, path_stat=stat, **kw)
        a = P.simulate_gbm(g, n // 2, S0, MU, SIGMA, scheme=scheme, path_stat=stat, offset=0, **kw)
        b = P.simulate_gbm(g, n // 2, S0, MU, SIGMA, scheme=scheme, path_stat=stat, offset=n // 2, **kw)
        assert torch.equal(torch.cat([a.stat, b.stat], 1), full.stat), (scheme, stat)
        assert torch.equal(torch.cat([a.stat_final, b.stat_final]), full.stat_final), (scheme, stat)
        assert torch.equal(torch.cat([a.S, b.S], 1), full.S)
        sub = P.simulate_gbm(g, ns, S0, MU, SIGMA, scheme=scheme, path_stat=stat, index_map=(blk, stride), **kw)
        assert torch.equal(sub.stat, full.stat[:, idx]) and torch.equal(sub.stat_final, full.stat_final[idx])
        assert torch.equal(sub.S, full.S[:, idx]) and torch.equal(sub.S_final, full.S_final[idx])


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_payoff_floating_strike_kinds(dev, n):  # noqa: F811
    from rphedge.ops import native

    rng = np.random.default_rng(n)
    if n >= 3:
        x = (0.5 + rng.random(n)).astype(np.float32)
        s = (0.5 + rng.random(n)).astype(np.float32)
        ties = [(i * 97) % n for i in range(3)]
        s[ties[0]] = x[ties[0]]
        s[ties[1]] = np.nextafter(x[ties[1]], np.float32(np.inf))
        s[ties[2]] = np.nextafter(x[ties[2]], np.float32(-np.inf))
        variants = [(s, x, ties[0])]
    else:
        k = np.float32(1.1)
        variants = [(np.full(n, v, np.float32), np.full(n, k, np.float32), 0 if v == k else None)
                    for v in (k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf)))]
    for s, x, tie in variants:
        sd, xd = torch.from_numpy(s).to(dev), torch.from_numpy(x).to(dev)
        s64, x64 = s.astype(np.float64), x.astype(np.float64)
        for kind, ref in ((4, np.maximum(s64 - x64, 0.0)), (5, np.maximum(x64 - s64, 0.0))):
            buf, out = guarded(n, dev)
            native.payoff(kind, sd, out, 123.0, x=xd)  # (the fixed strike is not read)
            torch.cuda.synchronize()
            check_guards(f"payoff kind {kind}", buf)
            got = out.cpu().numpy()
            ulp = np.spacing(np.maximum(ref, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(got.astype(np.float64) - ref) <= ulp), (kind, n)
            assert np.all(got >= 0)
            if tie is not None:
                assert got[tie] == 0.0 and not np.signbit(got[tie])
            if n >= 3:
                assert (got == 0).any() and (got > 0).any()


def _cfg(payoff, n_log2=14, path_feature=True, Y=100.0):
    from rphedge.config import ParityFlags, RunConfig, TrainingParams

    tr = TrainingParams(batch_size=1 << n_log2, epochs_first=1, epochs_rest=1, early_stopping=False, q99=False,
                        lr_schedule_first=False, chunk_log2=6, optimizer="lm", lm_passes_first=60,
                        lm_passes_rest=3, lm_lam_carry=3.0, lm_out_fix=True)
    return RunConfig(Y=Y, K=Y, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=1 / 8, dt=1 / 32, n_paths=n_log2,
                     payoff=payoff, option_type="CALL", model="gbm_log", mortality=False, N=1, P=1.0,
                     path_feature=path_feature, keep_paths=False, verbose=False, train=tr, parity=ParityFlags(),
                     device="cuda:0")


def test_graph_resimulates_statistics(dev):  # noqa: F811
    from rphedge.api import HedgeRun

    run = HedgeRun(_cfg("asian_call", n_log2=13))
    assert (run.spec.nin, run.spec.nout) == (2, 2)
    run.build()
    r_eager = run.run()
    p = run.paths
    keep = [t.clone() for t in (p.S, p.stat, p.stat_final, run.v_terminal)]
    assert float(keep[1].abs().sum()) > 0 and float(keep[3].abs().sum()) > 0
    run.capture(include_simulation=True)
    for t in (p.S, p.stat, p.stat_final, run.v_terminal):
        t.zero_()
    run.replay()
    r_graph = run.collect()
    run.close()
    for t, k, name in zip((p.S, p.stat, p.stat_final, run.v_terminal), keep, ("S", "stat", "stat_final", "v_T")):
        assert torch.equal(t, k), name
    print(f"asian_call V0 eager {r_eager.v0!r} graph {r_graph.v0!r}")
    assert r_graph.v0 == pytest.approx(r_eager.v0, rel=1e-6)


_E2E = {}


def _e2e(payoff, path_feature=True):
    """One LM run at 2^14 paths on grid A (shared between the tests below)."""
    from rphedge.api import HedgeRun

    key = (payoff, path_feature)
    if key not in _E2E:
        run = HedgeRun(_cfg(payoff, path_feature=path_feature))
        res = run.run()
        disc = math.exp(-0.08)
        pay = run.v_terminal.double() * 100.0 * disc
        _E2E[key] = dict(v0=res.v0, pnl_mean=res.self_financing_pnl["mean"], pnl_std=res.self_financing_pnl["std"],
                         pay_std=float(pay.std()), pay_mean=float(pay.mean()), nin=run.spec.nin,
                         summary=res.summary, n=run.n_total)
        run.close()
    return _E2E[key]


def test_e2e_geo_asian_price_and_pnl(dev):  # noqa: F811
    from rphedge.analytic import geo_asian_price

    r = _e2e("geo_asian_call")
    cf = geo_asian_price(100.0, 100.0, 0.08, 0.15, 1 / 32, 32, "CALL")
    se = r["pay_std"] / math.sqrt(r["n"])
    print(f"geo_asian_call: V0 {r['v0']:.5f} closed form {cf:.5f} ({abs(r['v0'] - cf) / se:.2f} se), "
          f"P&L mean {r['pnl_mean']:.5f} std {r['pnl_std']:.5f} (payoff std {r['pay_std']:.4f})")
    assert r["nin"] == 2
    assert r["summary"]["analytic_price"] == pytest.approx(cf) and "bs_price" not in r["summary"]
    assert abs(r["v0"] - cf) <= 3 * se
    assert abs(r["pnl_mean"]) <= 3 * r["pnl_std"] / math.sqrt(r["n"])
    assert r["pnl_std"] < r["pay_std"]


@pytest.mark.parametrize("payoff,cap", [("asian_call", 0.70), ("lookback_call", 0.85)])
def test_e2e_statistic_input_beats_price_alone(dev, payoff, cap):  # noqa: F811
    a, b = _e2e(payoff, True), _e2e(payoff, False)
    print(f"{payoff}: P&L std {a['pnl_std']:.5f} with the statistic, {b['pnl_std']:.5f} with S alone "
          f"(ratio {a['pnl_std'] / b['pnl_std']:.3f}, cap {cap}); payoff std {a['pay_std']:.4f}")
    assert (a["nin"], b["nin"]) == (2, 1)
    assert a["pay_std"] == b["pay_std"]
    assert a["pnl_std"] <= cap * b["pnl_std"]
    assert a["pnl_std"] < a["pay_std"] and b["pnl_std"] < b["pay_std"]
