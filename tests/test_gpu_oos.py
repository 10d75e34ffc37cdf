"""k_hedge_oos (HipBackend.oos: the fused simulate-and-hedge kernel of the
out-of-sample test) on synthetic snapshots, standardisation and bond tables.

A. Hedge arithmetic.  The kernel is launched with its trace on; the P&L is
   recomputed in fp64 from the TRACED prices / statistics (the fp32 values the
   nets consumed) with the recursion of test_gpu_pnl.reference, the payoff
   from the traced finals.  Per path ``|pnl - ref| <= 32 n_dates u max|ref| +
   2 u max|payoff|`` (u = 2^-24; the P&L scan's bound plus the payoff's two
   roundings); the statistics as test_gpu_pnl bounds them, the count exactly,
   per workgroup (persistent workgroups: row w sums the tiles w, w + G, ...).
B. Simulation.  The traced arrays against the fp64 twins under the bounds the
   fp32 scan tests use (GBM: rtol 5e-5, test_gpu_path_stats; Heston: 4 x the
   float32 emulation's error, test_gpu_path_scans), and bitwise against
   native.simulate on the same descriptor inputs (both run sim_step.h).
C. Route equivalence through the API: fused against materialised per path
   within ``64 n_dates u max|pnl|`` (each is within 32 of the fp64 recursion),
   and the training seed and window against the in-sample folded P&L.
D. Host validation of rph_oos.

Grids are (n_fine, reduction); (18, 4) is the one that leaves fine steps after
the last coarse date (fine 16 of 0..17) - (17, 4) ends on it.

Measured on an MI355X (profiles/oos/pytest_gpu_oos.log).  A: the largest
per-path error over the cases with more than one path is 3.7 u max|ref| per
date (bound 32; Heston, n = 2500, the single-date grid).  With n = 1 max|ref|
is that one path's own P&L, which can nearly cancel (|P&L| << |payoff|): the
worst single-path case is 61.8 u |P&L| per date (GBM + max, grid (18, 4), two
networks), inside the bound through its payoff term.  B: GBM prices and
statistics at most 2.9e-6 relative off the twin (bound 5e-5); Heston within
the emulation's own error (S 7.97e-5 vs e_max 8.01e-5 at xi 0.9; 99.97 % of
the points inside 4 e_99.9); every traced array equals the scan's bit for bit.
C: fused and materialised P&L equal on every path (0 u) for the three
families; the fused kernel on the training paths is within 9.6 u max|pnl| of
the in-sample folded P&L (bound 448).
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_eval import GUARD, SENTINEL, U, check_guards, f32, guarded, make_spec, make_weights  # noqa: F401
from test_gpu_kernels import dev  # noqa: F401  (fixture)
from test_pnl import _np_forward

pytestmark = pytest.mark.gpu

HOLD_C = 0.1
S0, MU, SIGMA, NORM = 100.0, 0.08, 0.15, 100.0
HESTON = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
OFFSET = 37   # nonzero, not a multiple of 64
GRIDS = [(2, 1), (8, 1), (15, 2), (17, 4), (18, 4)]
NS = [1, 255, 256, 257, 2500]
# (model, path statistic, network shape, k_payoff kind)
FAMILIES = [("gbm_log", None, (1, 8, 1, 1), 1), ("gbm", None, (1, 8, 2, 0), 2), ("gbm_log", "mean", (2, 8, 2, 0), 4),
            ("gbm", "max", (2, 8, 2, 0), 1), ("heston", None, (2, 8, 2, 0), 1)]
STRIKE = 1.02
MAX_ULPS = [0.0]


def mini_grid(n_fine, reduction, dt=None):
    """The fields of ops.paths.Grid the descriptors and the twins read."""
    return SimpleNamespace(n_fine=n_fine, reduction=reduction, n_coarse=-(-n_fine // reduction),
                           dt=1.0 / (n_fine - 1) if dt is None else dt)


def sim_desc(g, n, offset, model, stat, dev, scheme="qe", heston=None, mu=MU):  # noqa: F811
    from rphedge.ops import paths as P

    if model == "heston":
        h = dict(HESTON, **(heston or {}))
        return P.sv_desc(g, n, S0, mu, h["v0"], "heston", 0.0, 0.0, 0.0, h["kappa"], h["theta"], h["xi"], h["rho"], NORM,
                         dev, offset, False, False, P.SEED_W1, P.SEED_W2, scheme, 0.0, True)
    return P.gbm_desc(g, n, S0, mu, SIGMA, "arith" if model == "gbm" else "log", NORM, dev, offset, False, P.SEED_W1,
                      None, stat)


def make_tables(spec, nd, has_b, second):
    """Synthetic snapshots (NaN outside w[0][:P]), standardisation and bond of ``nd`` dates."""
    from rphedge.engine import MAXIN
    from rphedge.ops import layout as L

    fmu, fisd = torch.zeros(nd, MAXIN), torch.ones(nd, MAXIN)
    for t in range(nd):
        fmu[t, 0], fisd[t, 0] = 1.0 + 0.02 * t, (1.0 + 0.05 * t) / 0.15
        if spec.nin == 2:   # the running statistic (near S) or the variance (near 0.04)
            fmu[t, 1], fisd[t, 1] = (0.04, 1.0 / 0.02) if second == "variance" else (1.0 + 0.01 * t, 1.0 / 0.1)
    snap = torch.full((nd, 2, L.NETW_FLOATS), float("nan"))
    ws = np.zeros((nd, 2, spec.nparams), np.float32)
    for t in range(nd):
        for k in range(2 if has_b else 1):
            ws[t, k] = make_weights(spec, 100 + 2 * t + k)
            snap[t, k, :spec.nparams] = torch.from_numpy(ws[t, k])
    bond = torch.tensor([1.03 ** (0.7 * t) for t in range(nd + 1)], dtype=torch.float64)
    return dict(fmu=fmu, fisd=fisd, snap=snap, ws=ws, bond=bond)


def launch(dev, spec, sim, tb, nd, has_b, kind, wgs=None, wealth0=0.25):  # noqa: F811
    """One traced k_hedge_oos launch; returns the host arrays and the raw statistics rows."""
    from rphedge.engine import HipBackend, PnlData, TrainConfig
    from rphedge.ops import layout as L

    n, nc = int(sim.n_local), int(sim.n_coarse)
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    wgs = be.oos_wgs(n) if wgs is None else wgs
    assert 1 <= wgs <= (n + 255) // 256
    bufs = {k: guarded(sz, dev) for k, sz in (("s", nc * n), ("x", nc * n), ("fin", n), ("fin2", n), ("pay", n),
                                              ("pnl", n))}
    sim.out, sim.out2 = bufs["s"][1].data_ptr(), bufs["x"][1].data_ptr()
    sim.final_out, sim.final2_out = bufs["fin"][1].data_ptr(), bufs["fin2"][1].data_ptr()
    slab = torch.full((wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    data = PnlData(n_dates=nd, features=None, prices=None, bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev),
                   fisd=tb["fisd"].to(dev), w0=None, payoff=None, wealth0=wealth0)
    be.oos(sim, tb["snap"].to(dev), data, slab, kind, STRIKE, has_b=has_b, hold_c=HOLD_C if has_b else 0.0,
           pnl_out=bufs["pnl"][1], payoff_out=bufs["pay"][1])
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        check_guards(k, buf)
    out = {k: v.cpu().numpy().astype(np.float64) for k, (_, v) in bufs.items()}
    out["s"], out["x"] = out["s"].reshape(nc, n), out["x"].reshape(nc, n)
    out["raw"] = slab.cpu().numpy()
    out["slab"], out["wgs"] = slab, wgs
    return out


def reference(spec, tb, tr, nd, has_b, kind, stat, wealth0):
    """fp64 recursion of test_gpu_pnl.reference on the traced fp32 values, payoff from the traced finals."""
    W = np.full(tr["s"].shape[1], f32(wealth0), np.float64)
    bond = tb["bond"].numpy()
    alpha = f32(spec.alpha)
    for t in range(nd):
        X = np.stack([tr["s"][t]] + ([tr["x"][t]] if spec.nin == 2 else []), axis=1)
        X = (X - tb["fmu"][t, :spec.nin].double().numpy()) * tb["fisd"][t, :spec.nin].double().numpy()
        h = _np_forward(spec, tb["ws"][t, 0].astype(np.float64), X, alpha)
        if has_b:
            hb = _np_forward(spec, tb["ws"][t, 1].astype(np.float64), X, alpha)
            h = h + f32(HOLD_C) * (hb - h)
        grow = f32(bond[t + 1] / bond[t])
        W = W * grow + h[:, 0] * (tr["s"][t + 1] - tr["s"][t] * grow)
    k, s, x = f32(STRIKE), tr["fin"], tr["fin2"]
    u = x if (stat is not None and kind <= 2) else s
    pay = {1: np.maximum(u - k, 0), 2: np.maximum(k - u, 0), 4: np.maximum(s - x, 0), 5: np.maximum(x - s, 0)}[kind]
    return W, pay, W - pay


def check_case(dev, fam, n, grid, has_b, wgs=None):  # noqa: F811
    from rphedge.engine import reduce_stats
    from rphedge.ops import layout as L

    model, stat, shape, kind = fam
    spec = make_spec(shape)
    g = mini_grid(*grid)
    nd = g.n_coarse - 1
    tb = make_tables(spec, nd, has_b, "variance" if model == "heston" else "stat")
    sim = sim_desc(g, n, OFFSET, model, stat, dev)
    wealth0 = 0.25
    tr = launch(dev, spec, sim, tb, nd, has_b, kind, wgs=wgs, wealth0=wealth0)
    tag = f"oos {model} {stat} {shape} n={n} grid={grid} has_b={has_b} wgs={tr['wgs']}"
    # the trace is what the scan stores: S_0 on row 0, finite, positive prices
    assert np.all(tr["s"][0] == np.float32(S0) * np.float32(1.0 / NORM)), tag
    assert np.all(np.isfinite(tr["s"])) and np.all(tr["s"] > 0) and np.all(np.isfinite(tr["fin"])), tag
    if (g.n_coarse - 1) * g.reduction == g.n_fine - 1:
        assert np.array_equal(tr["fin"], tr["s"][-1]), tag
    elif n > 1:
        assert not np.array_equal(tr["fin"], tr["s"][-1]), tag
    W, pay, pnl = reference(spec, tb, tr, nd, has_b, kind, stat, wealth0)
    # the payoff itself: one subtraction of two fp32 values
    assert np.abs(tr["pay"] - pay).max() <= U * max(float(np.abs(pay).max()), 1e-30), tag
    scale, pscale = float(np.abs(pnl).max()), float(np.abs(pay).max())
    F = 32.0 * nd
    tol_p = F * U * scale + 2 * U * pscale
    tol_w = F * U * float(np.abs(W).max())
    err = float(np.abs(tr["pnl"] - pnl).max())
    MAX_ULPS[0] = max(MAX_ULPS[0], err / (U * scale * nd))
    print(f"ULPS {tag}: {err / (U * scale):.3f} u max|ref| (bound {F:.0f} + payoff); per date so far max "
          f"{MAX_ULPS[0]:.3f}")
    assert err <= tol_p, f"{tag}: max err {err:.3e} = {err / (U * scale):.2f} u max|ref| > {F:.0f}"
    raw = tr["raw"]
    assert not np.isnan(raw).any(), f"{tag}: statistics rows not overwritten"
    G = tr["wgs"]
    cnt = np.bincount((np.arange(n) // 256) % G, minlength=G)
    assert np.array_equal(raw[:, L.ES_COUNT], cnt.astype(np.float64)), tag
    st = reduce_stats(tr["slab"])
    assert st[L.ES_COUNT] == n

    def lin(x, tol):
        return float(x.sum()), n * tol + 8 * U * float(np.abs(x).sum())

    def sq(x, tol):
        return float((x * x).sum()), n * (2 * float(np.abs(x).max()) * tol + tol * tol) + 8 * U * float((x * x).sum())

    want = {L.ES_V: lin(W, tol_w), L.ES_V2: sq(W, tol_w), L.ES_RES: lin(pnl, tol_p), L.ES_RES2: sq(pnl, tol_p),
            L.ES_ABSRES: lin(np.abs(pnl), tol_p)}
    for idx, (ref, tol) in want.items():
        assert abs(st[idx] - ref) <= tol, f"{tag}: statistic {idx}: {st[idx]!r} vs {ref!r} (tol {tol:.3e})"
    assert abs(st[L.ES_RESMIN] - pnl.min()) <= tol_p and abs(st[L.ES_RESMAX] - pnl.max()) <= tol_p
    others = [c for c in range(L.EVAL_NSTAT) if c not in (*want, L.ES_COUNT, L.ES_RESMIN, L.ES_RESMAX)]
    assert np.all(raw[:, others] == 0.0)


# ---------------------------------------------------------------------------
# A. hedge arithmetic
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", NS)
def test_hedge_arithmetic_vs_fp64_recursion_of_the_trace(dev, n, grid):  # noqa: F811
    for fam in FAMILIES:
        for has_b in (False, True):
            check_case(dev, fam, n, grid, has_b)


@pytest.mark.parametrize("grid", GRIDS)
def test_one_workgroup_loops_over_the_tiles(dev, grid):  # noqa: F811
    """n = 2500 is ten tiles: one persistent workgroup takes them all, three take 4 / 3 / 3."""
    for fam in FAMILIES:
        check_case(dev, fam, 2500, grid, True, wgs=1)
    check_case(dev, FAMILIES[2], 2500, grid, False, wgs=3)


# ---------------------------------------------------------------------------
# B. simulation
# ---------------------------------------------------------------------------
def _launch_sim_only(dev, g, n, offset, model, stat, **kw):  # noqa: F811
    shape = (1, 8, 2, 0) if (stat is None and model != "heston") else (2, 8, 2, 0)
    spec = make_spec(shape)
    nd = g.n_coarse - 1
    tb = make_tables(spec, nd, False, "variance" if model == "heston" else "stat")
    sim = sim_desc(g, n, offset, model, stat, dev, **kw)
    return launch(dev, spec, sim, tb, nd, False, 1)


GBM_GRID = dict(T=1.0, dt=1 / 30, rebalancing=1 / 4)   # test_gpu_path_stats GRID_B: coarse grid ends at fine 28 of 30


@pytest.mark.parametrize("n,offset", [(257, 37), (2048, 128), (2500, 0)])
@pytest.mark.parametrize("scheme", ["log", "arith"])
def test_gbm_trace_vs_twin_and_scan(dev, scheme, n, offset):  # noqa: F811
    from rphedge.ops import paths as P

    g = P.Grid(**GBM_GRID)
    assert (g.n_coarse - 1) * g.reduction == 28 and g.n_fine == 31
    model = "gbm" if scheme == "arith" else "gbm_log"
    for stat in (None, "mean", "geomean", "max", "min"):
        if stat == "geomean" and scheme == "arith":
            continue
        tr = _launch_sim_only(dev, g, n, offset, model, stat, mu=MU)
        ref = P._cpu_gbm(g, n, S0, MU, SIGMA, scheme, offset, P.SEED_W1, path_stat=stat)
        tag = f"{scheme} {stat} n={n} offset={offset}"
        pairs = [("S", tr["s"], ref[0]), ("S_final", tr["fin"], ref[1])]
        if stat is not None:
            pairs += [("stat", tr["x"], ref[2]), ("stat_final", tr["fin2"], ref[3])]
        for name, got, want in pairs:
            err = float(np.abs(got / (want / NORM) - 1).max())
            print(f"{tag} {name}: max rel err {err:.2e} (bound 5e-05)")
            np.testing.assert_allclose(got, want / NORM, rtol=5e-5, err_msg=f"{tag} {name}")
        # the scan itself, bit for bit
        p = P.simulate_gbm(g, n, S0, MU, SIGMA, scheme=scheme, norm=NORM, device=dev, offset=offset, path_stat=stat)
        torch.cuda.synchronize()
        assert np.array_equal(tr["s"], p.S.cpu().numpy().astype(np.float64)), tag
        assert np.array_equal(tr["fin"], p.S_final.cpu().numpy().astype(np.float64)), tag
        if stat is not None:
            assert np.array_equal(tr["x"], p.stat.cpu().numpy().astype(np.float64)), tag
            assert np.array_equal(tr["fin2"], p.stat_final.cpu().numpy().astype(np.float64)), tag


@pytest.mark.parametrize("case", ["heston_euler", "heston_qe_xi03", "heston_qe_xi09"])
def test_heston_trace_vs_twin_and_scan(dev, case):  # noqa: F811
    import test_gpu_path_scans as T

    from rphedge.ops import paths as P

    model, v0, kw = T.SV_CASES[case]
    g = T.grid("GA")   # 101 fine points, reduction 12: the coarse grid ends at 96
    emu_s, emu_v, got_s, got_v = [], [], [], []
    for rk in ("R4", "R9"):   # (2051, 37) unaligned and (2048, 0) aligned
        n, off, m = T.RANGES[rk]
        assert m is None
        ref = T._sv_twin(case, "GA", rk)
        hz = dict(v0=v0, kappa=kw["kappa"], theta=kw["theta"], xi=kw["xi"], rho=kw["rho"])
        tr = _launch_sim_only(dev, g, n, off, "heston", None, scheme=kw["scheme"], heston=hz, mu=T.MU)
        ks, kv = T._errors(tr["s"], tr["x"], tr["fin"], ref)
        es, ev = T._sv_emu_errors(case, "GA", rk)
        emu_s.append(es), emu_v.append(ev), got_s.append(ks), got_v.append(kv)
        # the scan itself, bit for bit
        p = P.simulate_sv(g, n, T.S0, T.MU, v0, model="heston", norm=T.NORM, device=dev, offset=off, **kw)
        torch.cuda.synchronize()
        for name, a, b in (("S", tr["s"], p.S), ("variance", tr["x"], p.vol), ("S_final", tr["fin"], p.S_final)):
            assert np.array_equal(a, b.cpu().numpy().astype(np.float64)), (case, rk, name)
    for name, emu, got in (("S rel", emu_s, got_s), ("variance abs", emu_v, got_v)):
        emu, got = np.concatenate(emu), np.concatenate(got)
        e_max, e_999 = float(emu.max()), float(np.quantile(emu, 0.999))
        inside = float(np.mean(got <= 4 * e_999))
        print(f"FP32 {case} {name}: kernel max {got.max():.2e} | emulation e_max {e_max:.2e} e_99.9 {e_999:.2e}, "
              f"{100 * inside:.3f} % inside")
        assert got.max() <= 4 * e_max, (case, name, got.max(), e_max)
        assert inside >= 0.999, (case, name, inside)


# ---------------------------------------------------------------------------
# C. route equivalence through the API
# ---------------------------------------------------------------------------
def _api_cfg(family):
    from rphedge.config import ParityFlags, RunConfig, TrainingParams

    tr = TrainingParams(batch_size=1 << 11, epochs_first=1, epochs_rest=1, early_stopping=False, q99=False,
                        lr_schedule_first=False, chunk_log2=6, optimizer="lm", lm_passes_first=20, lm_passes_rest=2)
    kw = dict(payoff="call", model="gbm_log")
    if family == "asian":
        kw = dict(payoff="asian_call", model="gbm_log")
    elif family == "heston":
        kw = dict(payoff="call", model="heston", v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
    # 29 fine points, reduction 4: 8 coarse points = 7 dates (every number exact in binary)
    return RunConfig(Y=100.0, K=100.0, T=0.875, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.125, dt=1 / 32, n_paths=11,
                     option_type="CALL", mortality=False, N=1, P=1.0, verbose=False, train=tr, parity=ParityFlags(),
                     device="cuda:0", **kw)


@pytest.mark.parametrize("family", ["gbm", "asian", "heston"])
def test_fused_route_matches_the_materialised_one(dev, family):  # noqa: F811
    from rphedge import oos
    from rphedge.api import HedgeRun
    from rphedge.engine import PnlData
    from rphedge.ops import layout as L
    from rphedge.ops.paths import SEED_W1

    run = HedgeRun(_api_cfg(family))
    res = run.run()
    ind, be = run.induction, run.backend
    nd, n = ind.n_dates, run.n_local
    assert nd == 7 and n == 2048 and oos.fused_unsupported(run) is None
    assert run.out_of_sample().route == "fused"          # the auto-selected route
    o = run.out_of_sample(fused=True, keep_paths=True, keep_pnl=True, offset=4096 + 37)
    assert o.route == "fused" and o.n_paths == n and o.stats[L.ES_COUNT] == n
    # the returned paths through the materialised route: backend.pnl
    data = PnlData(n_dates=nd, features=o.paths.features, prices=o.paths.prices, bond=ind.pnl_data.bond,
                   fmu=ind.pnl_data.fmu, fisd=ind.pnl_data.fisd, w0=None, wealth0=oos.fitted_v0(run),
                   payoff=run._payoff(o.paths))
    slab = torch.zeros(be.pnl_wgs(n), L.EVAL_NSTAT, dtype=torch.float64, device=run.device)
    pnl_m = torch.empty(n, dtype=torch.float32, device=run.device)
    be.pnl(ind.snap, data, slab, pnl_out=pnl_m, n_local=n)
    torch.cuda.synchronize()
    a, b = o.pnl.double().cpu().numpy(), pnl_m.double().cpu().numpy()
    scale = float(np.abs(b).max())
    err = float(np.abs(a - b).max())
    print(f"ROUTES {family}: fused - materialised {err / (U * scale):.2f} u max|pnl| (bound {64 * nd})")
    assert err <= 64 * nd * U * scale
    # and the whole API route: the same window, materialised, gives the same statistics within that bound
    m = run.out_of_sample(fused=False, offset=4096 + 37)
    assert m.route == "materialised" and abs(m.std - o.std) <= 2 * 64 * nd * U * scale * run.scale
    # the training seed and window: the in-sample (folded) P&L
    t = run.out_of_sample(fused=True, seed=SEED_W1, offset=0, keep_pnl=True)
    c = res.induction.pnl_paths.double().cpu().numpy()
    scale = float(np.abs(c).max())
    err = float(np.abs(t.pnl.double().cpu().numpy() - c).max())
    print(f"ROUTES {family}: fused on the training paths - in-sample folded P&L {err / (U * scale):.2f} u max|pnl| "
          f"(bound {64 * nd}); std ratio {t.std_ratio:.6f}")
    assert err <= 64 * nd * U * scale
    run.close()


# ---------------------------------------------------------------------------
# D. host validation
# ---------------------------------------------------------------------------
def test_rph_oos_rejects_bad_descriptors_before_any_launch(dev):  # noqa: F811
    from rphedge.engine import HipBackend, PnlData, TrainConfig
    from rphedge.ops import layout as L
    from rphedge.ops import native

    n, g = 512, mini_grid(15, 2)
    nd = g.n_coarse - 1
    spec = make_spec((1, 8, 2, 0))
    tb = make_tables(spec, nd, False, "stat")
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    keep = [tb["snap"].to(dev), tb["bond"].to(dev), tb["fmu"].to(dev), tb["fisd"].to(dev),
            torch.full((2, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)]

    def desc(**edit):
        d = native.OosDesc()
        d.sim = sim_desc(g, n, 0, "gbm_log", None, dev)
        d.snap, d.bond, d.fmu, d.fisd, d.stats = (t.data_ptr() for t in keep)
        d.alpha, d.wealth0, d.strike, d.payoff_kind, d.n_dates, d.num_wgs = 0.3, 0.25, 1.0, 1, nd, 2
        d.nin, d.h, d.nout, d.head = 1, 8, 2, 0
        for k, v in edit.items():
            obj, name = (d.sim, k[4:]) if k.startswith("sim_") else (d, k)
            setattr(obj, name, v)
        return d

    bad = [(dict(snap=None), "null snapshot or statistics pointer"),
           (dict(stats=None), "null snapshot or statistics pointer"),
           (dict(nin=3), r"unsupported network shape \(nin 3, h 8, nout 2, head 0\)"),
           (dict(h=32), r"unsupported network shape \(nin 1, h 32, nout 2, head 0\)"),
           (dict(nin=2), r"unsupported network shape \(nin 2"),          # two inputs need a statistic / Heston
           (dict(sim_path_stat=1), r"unsupported network shape \(nin 1"),  # ... and a statistic needs two
           (dict(sim_n_coarse=g.n_coarse + 1), "n_coarse / n_dates inconsistent with n_fine and reduction"),
           (dict(n_dates=nd - 1), "n_coarse / n_dates inconsistent with n_fine and reduction"),
           (dict(sim_reduction=3), "n_coarse / n_dates inconsistent with n_fine and reduction"),
           (dict(sim_path_offset=(1 << 30) - n + 1), r"path range leaves the 30-bit Sobol index space \[0, 2\^30\)"),
           (dict(sim_path_offset=-1), r"path range leaves the 30-bit Sobol index space"),
           (dict(num_wgs=3), "num_wgs must be in"), (dict(num_wgs=0), "num_wgs must be in"),
           (dict(payoff_kind=3), "payoff_kind must be 1, 2, 4 or 5"),
           (dict(payoff_kind=4), "floating-strike payoff without a path statistic"),
           (dict(sim_model=L.SIM_BASKET), "model must be"), (dict(sim_fp64=1), "fp32, one asset"),
           (dict(sim_dims1=g.n_fine - 1), "Sobol table 1")]
    for edit, msg in bad:
        for fn in (native.oos_check, native.oos):
            with pytest.raises(RuntimeError, match=msg) as e:
                fn(desc(**edit))
            assert "rph_oos failed with code -22" in str(e.value), (edit, str(e.value))
    torch.cuda.synchronize()
    assert torch.isnan(keep[4]).all()                 # nothing was launched
    native.oos_check(desc(sim_path_offset=(1 << 30) - n))   # the last window that fits
    native.oos(desc())                                # the same descriptor, valid: runs
    torch.cuda.synchronize()
    assert not torch.isnan(keep[4]).any() and float(keep[4][:, L.ES_COUNT].sum()) == n
    assert be.oos_wgs(1) == 1 and be.oos_wgs(1 << 30) == L.OOS_WGS_PER_CU * torch.cuda.get_device_properties(
        dev).multi_processor_count
    # the Python front end refuses mis-sized buffers
    data = PnlData(n_dates=nd, features=None, prices=None, bond=keep[1], fmu=keep[2], fisd=keep[3], w0=None,
                   payoff=None, wealth0=0.25)
    with pytest.raises(ValueError, match="pnl_out must be float32"):
        be.oos(sim_desc(g, n, 0, "gbm_log", None, dev), keep[0], data, keep[4], 1, 1.0,
               pnl_out=torch.empty(n - 1, device=dev))


def test_measured_ulps_summary():
    """(last: prints the largest per-date error of the arithmetic cases run in this session)"""
    print(f"MAX ULPS per date over the hedge-arithmetic cases: {MAX_ULPS[0]:.3f} (bound 32)")
