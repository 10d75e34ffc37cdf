"""Early exercise on the GPU: the exercise variants of k_hedge_eval and
k_hedge_pnl against the fp64 recursions of test_exercise_cpu.py, and the
end-to-end Bermudan put (hip backend, LM fits).

Bounds (u = 2^-24; derivations in test_gpu_eval.py / test_gpu_pnl.py):

* eval, per path: ``|got - ref| <= F u max|ref|`` with the suite's factor
  ``F = test_gpu_eval.ulp_factor``: 32 for the 8-unit nets, and for H = 32 the
  same 32 scaled by the number of sequential roundings, 32 (nin + 2 H + nhold
  + 4) / (nin + 16 + nhold + 4) ~ 99 - the bound test_gpu_eval.py holds the
  plain kernel to ("32 u max|ref|, the suite's bound");
* eval, decision: read bitwise from the stored value (it is the plain
  kernel's V or the fp32 intrinsic value) and equal to the fp64 reference's on
  every path that is no near tie; on a near tie either value may be stored;
* eval: holdings, pred1, the residual and their statistics are bitwise the
  plain kernel's on the same inputs (test_gpu_eval.py holds those to fp64);
* eval, new columns: ES_EXER exact up to the number of near ties; ES_EXVAL and
  ES_CONT within the suite's bound of a summed statistic (``n x`` the per-path
  tolerance ``+ 8 u sum|terms|``) plus the near ties' own terms;
* P&L scan: ``tau_out`` exact and ``|pnl - ref| <= 32 n_dates u max|ref|`` on
  the paths that met no near tie; ES_EXER / ES_TAU are exactly the sums of
  ``tau_out``, ES_EXVAL the fp64 sum of the amounts paid at those dates.

Quality (ATM put, 8 dates, 2^16 paths, 8 weight seeds on an MI355X; the seed
log is profiles/early_exercise/quality_seeds.json, bounds 1.5 x the worst
seed): |V0 - tree| <= 0.2151 (worst 0.1434; the tree is 3.4304, the European
put 2.7012), tree - policy_value <= 0.0239 (worst 0.0159), |P&L mean| <=
0.2058 (worst 0.1372).  V0 scatters on both sides of the tree with the weight
seed (3.287 .. 3.549, mean 3.425) while the policy's own price stays within
0.016 below it: the scatter is the value fits' (three LM trial points per later
date), not the exercise rule's.
"""
import numpy as np
import pytest
import torch

from test_exercise_cpu import (KINDS, SHAPES, eval_case, eval_ex_reference, intrinsic64, near_tie, pnl_case)
from test_gpu_eval import (BOND_NEXT, BOND_NOW, GUARD, SENTINEL, U, check_guards, guarded, stat_terms,  # noqa: F401
                           ulp_factor)
from test_gpu_kernels import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _backend(dev, spec, n):  # noqa: F811
    from rphedge.engine import HipBackend, TrainConfig

    return HipBackend(spec, n, TrainConfig(batch_size=max(n, 1)), device=dev)


def run_eval_exercise(dev, be, spec, inp, w, strike, kind, alias, tag):  # noqa: F811
    """One exercise-date eval call; every output and statistic is checked.
    Returns (pairs, exercised pairs, near ties) of the reference."""
    from rphedge.engine import DateData, Exercise, reduce_stats
    from rphedge.ops import layout as L

    n = inp["feats"][0].numel()
    na = spec.nhold - 1
    feats = [f.to(dev) for f in inp["feats"]]
    data = DateData(feats=feats, prices_next=[p.to(dev) for p in inp["nxt"]], bond_next=BOND_NEXT,
                    target=inp["target"].to(dev), prices_now=feats[:na] if alias else [p.to(dev) for p in inp["now"]],
                    bond_now=BOND_NOW, fmu=inp["fmu"], fisd=inp["fisd"])
    bufs = {k: guarded(n, dev) for k in ("v", "res", "pred1")}
    hold_bufs = [guarded(n, dev) for _ in range(spec.nhold)]
    snap_a = torch.full((L.NETW_FLOATS,), SENTINEL, dtype=torch.float32, device=dev)
    slab = torch.full((be.eval_wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    be.eval(be.new_weights(w), data, slab, v_out=bufs["v"][1], hold_out=[b[1] for b in hold_bufs],
            resid_out=bufs["res"][1], pred1_out=bufs["pred1"][1], snap_a=snap_a,
            exercise=Exercise(kind=kind, strike=strike))
    # the same call without the right: holdings, pred1, the residual and their statistics must not change
    plain = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in ("v", "res", "pred1")}
    plain_hold = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(spec.nhold)]
    slab0 = torch.full((be.eval_wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    be.eval(be.new_weights(w), data, slab0, v_out=plain["v"], hold_out=plain_hold, resid_out=plain["res"],
            pred1_out=plain["pred1"])
    torch.cuda.synchronize()

    ref = eval_ex_reference(spec, inp, w, alias, kind, strike)
    F = ulp_factor(spec)
    near, ex, x, cont = ref["near"], ref["ex"], ref["x"], ref["cont"]
    off = ~near
    for k, (buf, _) in bufs.items():
        check_guards(f"{tag} {k}", buf)
    for k, b in enumerate(hold_bufs):
        check_guards(f"{tag} hold[{k}]", b[0])
        assert torch.equal(b[1], plain_hold[k]), f"{tag}: hold[{k}] differs from the plain kernel's"
    assert torch.equal(bufs["res"][1], plain["res"]), f"{tag}: residual differs from the plain kernel's"
    assert torch.equal(bufs["pred1"][1], plain["pred1"]), f"{tag}: pred1 differs from the plain kernel's"
    # ... and the stored value is, bitwise, the plain kernel's V or the fp32 intrinsic value
    x32 = Exercise(kind=kind, strike=strike).intrinsic(data.prices_now[0])
    is_c, is_x = bufs["v"][1] == plain["v"], bufs["v"][1] == x32
    assert bool(torch.all(is_c | is_x)), f"{tag}: a stored value is neither the continuation nor the intrinsic value"
    # the stored value: the bound is taken over max(|X|, |C|) of the case (both enter every decision)
    got_v = bufs["v"][1].cpu().numpy().astype(np.float64)
    scale = max(float(np.abs(ref["v"]).max()), 0.0)
    tol_v = F * U * scale
    err = np.abs(got_v - ref["v"])
    print(f"ULPS {tag} v: {float(err[off].max(initial=0.0)) / (U * scale) if scale > 0 else 0.0:.3f} (bound {F:.1f})")
    assert np.all(err[off] <= tol_v), f"{tag}: value off a near tie: max err {err[off].max():.3e} > {tol_v:.3e}"
    tol_c = F * U * float(np.abs(cont).max())
    # the kernel's decision, bitwise: the path stores X and not C; where the two are the same fp32 number
    # the rule X > 0 && X >= C exercises exactly when X > 0.  Off near ties it is the fp64 reference's.
    took_x = torch.where(is_x & is_c, x32 > 0, is_x).cpu().numpy()
    assert np.array_equal(took_x[off], ex[off]), \
        f"{tag}: exercise decision differs off a near tie on paths {np.nonzero(off & (took_x != ex))[0][:8]}"
    # a near tie stores either one
    either = np.minimum(np.abs(got_v - x), np.abs(got_v - cont))
    assert np.all(either[near] <= tol_v + tol_c), tag
    P = spec.nparams
    sa = snap_a.cpu().numpy()
    assert np.array_equal(sa[:P].view(np.uint32), np.asarray(w, np.float32).view(np.uint32)), tag
    assert np.all(sa[P:] == SENTINEL), tag

    # statistics: the suite's bounds for the existing columns, the exercised value in ES_V
    raw = slab.cpu().numpy()
    assert not np.isnan(raw).any(), f"{tag}: statistics rows not overwritten"
    wgs = be.eval_wgs
    cnt = np.bincount((np.arange(n) // 256) % wgs, minlength=wgs)
    assert np.array_equal(raw[:, L.ES_COUNT], cnt.astype(np.float64)), tag
    st = reduce_stats(slab)
    st0 = reduce_stats(slab0)
    same = [c for c in range(L.ES_EXER) if c not in (L.ES_V, L.ES_V2)]
    assert np.array_equal(st[same], st0[same]), f"{tag}: an existing statistic differs from the plain kernel's"
    assert np.array_equal(raw[:, same], slab0.cpu().numpy()[:, same]), tag
    assert np.all(st0[L.ES_EXER:] == 0.0)
    tols = {"v": tol_v}
    n_near = int(near.sum())
    slack = float(np.abs(x - cont)[near].sum())                   # a near tie may store the other value
    slack2 = float((np.abs(x * x - cont * cont))[near].sum())
    vt = stat_terms(spec, {"v": ref["v"], "res": ref["res"], "pred1": ref["pred1"]},
                    {"v": tol_v, "res": 0.0, "pred1": 0.0}, n)
    want = {L.ES_V: (vt[L.ES_V][0], vt[L.ES_V][1] + slack), L.ES_V2: (vt[L.ES_V2][0], vt[L.ES_V2][1] + slack2)}

    def lin(v, tol):
        return float(v.sum()), n * tol + 8 * U * float(np.abs(v).sum())

    want[L.ES_CONT] = lin(cont, tol_c)
    xv, xt = lin(np.where(ex, x, 0.0), F * U * float(np.abs(x).max()))
    want[L.ES_EXVAL] = (xv, xt + float(np.maximum(np.abs(x), np.abs(cont))[near].sum()))
    for idx, (w_, tol) in want.items():
        print(f"STAT {tag} [{idx}]: got {st[idx]:.9g} ref {w_:.9g} err {abs(st[idx] - w_):.3e} tol {tol:.3e}")
        assert abs(st[idx] - w_) <= tol, f"{tag}: statistic {idx}: {st[idx]!r} vs {w_!r} (tol {tol:.3e})"
    assert abs(st[L.ES_EXER] - float(ex.sum())) <= n_near, (tag, st[L.ES_EXER], ex.sum(), n_near)
    assert st[L.ES_EXER] == round(st[L.ES_EXER])
    assert np.all(st[[L.ES_TAU, 30, 31]] == 0.0)
    return n, int(ex.sum()), n_near


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_eval_exercise_vs_fp64(dev, shape, kind):  # noqa: F811
    """All 12 shapes x put / call at 1, 255, 256 and 1000 paths, prices aliased
    to the features (PA = true) and separate (PA = false)."""
    pairs = exd = near = 0
    for n in (1, 255, 256, 1000):
        for alias in (True, False):
            spec, inp, w, strike = eval_case(shape, kind, n, alias)
            be = _backend(dev, spec, n)
            a, b, c = run_eval_exercise(dev, be, spec, inp, w, strike, kind, alias,
                                        f"ex {shape} {kind} n={n} {'alias' if alias else 'separate'} k={strike}")
            pairs, exd, near = pairs + a, exd + b, near + c
    assert near <= 0.005 * pairs and 0.1 <= exd / pairs <= 0.9, (pairs, exd, near)


@pytest.mark.parametrize("shape", [(1, 8, 2, 0), (2, 8, 2, 0), (5, 8, 6, 0), (3, 32, 2, 0)])
def test_eval_exercise_unaligned_grid(dev, monkeypatch, shape):  # noqa: F811
    """Three workgroups walking 1636 paths: two or three trips each round the
    load ring, the last one partial."""
    monkeypatch.setenv("RPH_EVAL_WGS", "3")
    n = 3 * 256 * 2 + 100
    for kind in KINDS:
        spec, inp, w, strike = eval_case(shape, kind, n, False)
        be = _backend(dev, spec, n)
        assert be.eval_wgs == 3
        run_eval_exercise(dev, be, spec, inp, w, strike, kind, False, f"ex {shape} {kind} 3 wgs k={strike}")


def test_eval_exercise_launcher_rejects(dev):  # noqa: F811
    """The exercise variant takes one network and needs price_t[0]."""
    from rphedge.engine import DateData, Exercise

    spec, inp, w, strike = eval_case((1, 8, 2, 0), "put", 256, True)
    be = _backend(dev, spec, 256)
    feats = [f.to(dev) for f in inp["feats"]]
    data = DateData(feats=feats, prices_next=[p.to(dev) for p in inp["nxt"]], bond_next=BOND_NEXT,
                    target=inp["target"].to(dev), prices_now=feats[:1], bond_now=BOND_NOW, fmu=inp["fmu"],
                    fisd=inp["fisd"])
    wa, ex = be.new_weights(w), Exercise(kind="put", strike=strike)
    with pytest.raises(RuntimeError, match=r"rph_eval failed \(-22\): wb with ex_kind"):
        be.eval(wa, data, be.new_stats(), wts_b=be.new_weights(w), exercise=ex)
    with pytest.raises(RuntimeError, match=r"rph_eval failed \(-22\): g_base with ex_kind"):
        be.eval(wa, data, be.new_stats(), g_base=inp["g_base"].to(dev), exercise=ex)
    d = be.native.EvalDesc()
    d.wa, d.stats, d.n_local, d.num_wgs = wa.data_ptr(), be.new_stats().data_ptr(), 256, 1
    d.nin, d.h, d.nout, d.head = be.shape
    d.alpha, d.feat[0], d.ex_kind, d.ex_strike = 0.3, feats[0].data_ptr(), 1, 1.0
    with pytest.raises(RuntimeError, match=r"rph_eval failed \(-22\): price_t\[0\] is null with ex_kind"):
        be.native.eval_(d, be.stream)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("nd", [1, 2, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_pnl_stopping_vs_fp64_recursion(dev, shape, nd, every):  # noqa: F811
    from rphedge.engine import Exercise, HipBackend, PnlData, TrainConfig, reduce_stats
    from rphedge.ops import layout as L

    pairs = exd = near = 0
    for kind in KINDS:
        for n in (1023, 1025):
            spec, tb, strike, ref = pnl_case(shape, kind, n, nd, every)
            be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
            feats = [f.to(dev) for f in tb["feats"]]
            prices = [p.to(dev) for p in tb["prices"]]
            data = PnlData(n_dates=nd, features=lambda t: [f[t] for f in feats],
                           prices=lambda t: [p[t] for p in prices], bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev),
                           fisd=tb["fisd"].to(dev), w0=tb["w0"].to(dev), payoff=tb["payoff"].to(dev))
            wgs = (n + 1023) // 1024
            slab = torch.full((wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
            buf, out = guarded(n, dev)
            tbuf = torch.full((n + 2 * GUARD,), -77, dtype=torch.int32, device=dev)
            be.pnl(tb["snap"].to(dev), data, slab, pnl_out=out, exercise=Exercise(kind=kind, strike=strike, every=every),
                   tau_out=tbuf[GUARD:GUARD + n])
            torch.cuda.synchronize()

            tag = f"pnl-ex {shape} {kind} n={n} nd={nd} every={every} k={strike}"
            check_guards(tag, buf)
            tb_c = tbuf.cpu()
            assert torch.all(tb_c[:GUARD] == -77) and torch.all(tb_c[-GUARD:] == -77), f"{tag}: tau guard overwritten"
            tau = tb_c[GUARD:GUARD + n].numpy().astype(np.int64)
            got = out.cpu().numpy().astype(np.float64)
            ok = ~ref["amb"]
            assert np.array_equal(tau[ok], ref["tau"][ok]), f"{tag}: tau differs off a near tie"
            assert np.all((tau >= 0) & (tau <= nd)) and np.all((tau[tau < nd] % every) == 0)
            F = 32.0 * nd
            scale = float(np.abs(ref["pnl"]).max())
            err = float(np.abs(got - ref["pnl"])[ok].max(initial=0.0))
            print(f"ULPS {tag}: {err / (U * scale):.3f} u max|ref| (bound {F:.0f})")
            assert err <= F * U * scale, f"{tag}: max err {err:.3e} = {err / (U * scale):.2f} u max|ref| > {F:.0f}"

            raw = slab.cpu().numpy()
            assert not np.isnan(raw).any(), f"{tag}: statistics rows not overwritten"
            st = reduce_stats(slab)
            assert st[L.ES_COUNT] == n
            assert st[L.ES_TAU] == float(tau.sum()) and st[L.ES_EXER] == float((tau < nd).sum())
            # the amounts paid at the kernel's own exercise dates, in fp64
            bond = tb["bond"].numpy()
            s0 = np.stack([tb["prices"][0][t].double().numpy() for t in range(nd)], axis=0)
            xt = intrinsic64(kind, strike, s0[np.minimum(tau, nd - 1), np.arange(n)])
            paid = np.where(tau < nd, xt * (bond[0] / bond[np.minimum(tau, nd - 1)]),
                            tb["payoff"].double().numpy() * (bond[0] / bond[nd]))
            assert abs(st[L.ES_EXVAL] - paid.sum()) <= 4 * U * np.abs(paid).sum(), (tag, st[L.ES_EXVAL], paid.sum())
            # the other columns are the fp64 sums of the kernel's own per-path P&L
            assert abs(st[L.ES_RES] - got.sum()) <= 1e-12 * np.abs(got).sum() + 1e-300
            assert abs(st[L.ES_RES2] - (got * got).sum()) <= 1e-12 * (got * got).sum() + 1e-300
            assert st[L.ES_RESMIN] == got.min() and st[L.ES_RESMAX] == got.max()
            tol_w = F * U * float(np.abs(ref["W"]).max())
            amb_slack = float(np.abs(ref["W"])[~ok].sum()) * 2 + float(np.abs(got)[~ok].sum())
            assert abs(st[L.ES_V] - ref["W"].sum()) <= n * tol_w + 8 * U * np.abs(ref["W"]).sum() + amb_slack
            assert np.all(raw[:, [L.ES_APE, L.ES_PRED1, L.ES_CONT, 30, 31]] == 0.0)
            assert np.all(raw[:, L.ES_HOLD:L.ES_RESMIN] == 0.0)
            pairs, exd, near = pairs + ref["pairs"], exd + ref["exercised"], near + ref["near"]
    assert near <= 0.005 * pairs and 0.1 <= exd / pairs <= 0.9, (pairs, exd, near)


def test_pnl_stopping_launcher_rejects(dev):  # noqa: F811
    from rphedge.engine import Exercise, HipBackend, PnlData, TrainConfig

    spec, tb, strike, _ = pnl_case((1, 8, 2, 0), "put", 1023, 2, 1)
    n, nd = 1023, 2
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    feats = [f.to(dev) for f in tb["feats"]]
    prices = [p.to(dev) for p in tb["prices"]]
    data = PnlData(n_dates=nd, features=lambda t: [f[t] for f in feats], prices=lambda t: [p[t] for p in prices],
                   bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev), fisd=tb["fisd"].to(dev), w0=tb["w0"].to(dev),
                   payoff=tb["payoff"].to(dev))
    snap = tb["snap"].to(dev)
    with pytest.raises(RuntimeError, match=r"rph_pnl failed \(-22\): has_b with ex_kind"):
        be.pnl(snap, data, be.new_pnl_stats(), has_b=True, exercise=Exercise(kind="put", strike=strike))
    with pytest.raises(RuntimeError, match=r"rph_pnl failed \(-22\): tau_out without ex_kind"):
        be.pnl(snap, data, be.new_pnl_stats(), tau_out=torch.zeros(n, dtype=torch.int32, device=dev))


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def put_params(n_paths=14, **kw):
    p = dict(Y=100, K=100, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.125, N=1, P=1, x=0, l0=0, c=0, ita=0,
             dt=0.125 / 4, n_paths=n_paths, payoff="put", option_type="PUT", model="gbm_log", mortality=False,
             q99=False, optimizer="lm", lm_passes_first=80, lm_passes_rest=3, early_stopping=False, verbose=False,
             exercise="bermudan")
    p.update(kw)
    return p


@pytest.fixture(scope="module")
def put_run(dev):  # noqa: F811
    """The 2^14-path x 8-date Bermudan put on the hip backend: the run object
    (built, run eagerly once) and its result, shared by the end-to-end tests."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(put_params(device=str(dev))))
    res = run.run()
    yield run, res
    run.close()


def test_e2e_tau_matches_kept_values(put_run):
    """tau of the P&L scan = the first exercise date at which the kept value
    of the path is its intrinsic value, values[t] == X_t > 0 - off near ties."""
    from rphedge.engine import Exercise

    run, res = put_run
    ind, paths = res.induction, res.paths
    nd = paths.n_coarse - 1
    ex = Exercise(kind="put", strike=1.0)
    n = ind.values.shape[1]
    first = np.full(n, nd, np.int64)
    amb = np.zeros(n, bool)
    pairs = near = 0
    for t in range(nd - 1, -1, -1):
        s = paths.prices(t)[0]
        x = ex.intrinsic(s)
        v = ind.values[t]
        hit = ((x > 0) & (v == x)).cpu().numpy()
        first = np.where(hit, t, first)
        # near ties of the date: the continuation value from the kept holdings of the date
        c = (ind.holdings[t, 0].double() * s.double() + ind.holdings[t, 1].double() * float(np.float32(paths.bond[t])))
        xd = x.double().cpu().numpy()
        nt = (xd > 0) & near_tie(xd, c.cpu().numpy())
        amb |= nt
        pairs += n
        near += int(nt.sum())
    assert near <= 0.005 * pairs, (near, pairs)
    tau = ind.tau.cpu().numpy().astype(np.int64)
    assert np.array_equal(tau[~amb], first[~amb])
    share = float((tau < nd).mean())
    assert 0.1 <= share <= 0.9 and res.exercise_share == pytest.approx(share, abs=1e-12)
    assert res.mean_exercise_date == pytest.approx(float(tau.mean()) * paths.grid.dt_coarse, rel=1e-12)


def test_e2e_graph_replay_bitwise(put_run):
    run, res = put_run
    eager = [res.induction.values.clone(), res.induction.pnl_paths.clone(), res.induction.tau.clone()]
    run.capture(include_simulation=True)
    run.replay()
    r2 = run.collect()
    for a, b in zip(eager, [r2.induction.values, r2.induction.pnl_paths, r2.induction.tau]):
        assert torch.equal(a, b)
    assert r2.v0 == res.v0 and r2.exercise_share == res.exercise_share and r2.policy_value == res.policy_value


def test_e2e_matches_torch(put_run, dev):  # noqa: F811
    """HIP against the torch backend (the CPU oracle: same Sobol paths, same
    initial weights) on V0 and the exercised shares, to the tolerance of the
    end-to-end LM comparison test_gpu_lm.test_lm_fit_matches_torch_and_is_deterministic
    (rel 2e-2)."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run, res = put_run
    rt = HedgeRun(parse_params(put_params(device="cpu", backend="torch")))
    rest = rt.run()
    rt.close()
    print(f"E2E hip V0 {res.v0:.6f} share {res.exercise_share:.5f} policy {res.policy_value:.6f} | torch V0 "
          f"{rest.v0:.6f} share {rest.exercise_share:.5f} policy {rest.policy_value:.6f} | tree {res.tree_price:.6f}")
    assert res.v0 == pytest.approx(rest.v0, rel=E2E_RTOL)
    assert res.exercise_share == pytest.approx(rest.exercise_share, abs=E2E_SHARE_ATOL)
    for a, b in zip(res.summary["exercise_dates"], rest.summary["exercise_dates"]):
        assert a["date"] == b["date"] and a["share"] == pytest.approx(b["share"], abs=E2E_SHARE_ATOL)


E2E_RTOL = 2e-2
E2E_SHARE_ATOL = 2e-2

# Quality bounds: 1.5 x the worst of the 8 weight seeds measured on an MI355X
# (profiles/early_exercise/quality_seeds.json); the V0 bound must stay < 0.25.
# Worst seeds: |V0 - tree| 0.14340 (seed 1235), tree - policy_value 0.01592 (1235), |P&L mean| 0.13717 (1238).
Q_V0_TREE = 0.2151
Q_TREE_POLICY = 0.0239
Q_PNL_MEAN = 0.2058


def test_quality_bermudan_put(dev):  # noqa: F811
    """ATM put, 8 dates, 2^16 paths, 8 weight seeds: |V0 - tree|, tree -
    policy_value and |P&L mean| within 1.5 x the worst seed recorded."""
    from rphedge.api import run_params

    rows = []
    for seed in range(1234, 1242):
        r = run_params(put_params(n_paths=16, device=str(dev), seed=seed, keep_paths=False))
        rows.append((seed, r.v0, r.tree_price, r.policy_value, r.self_financing_pnl["mean"], r.exercise_share))
        print(f"QUALITY seed {seed}: V0 {r.v0:.5f} tree {r.tree_price:.5f} policy {r.policy_value:.5f} "
              f"pnl_mean {r.self_financing_pnl['mean']:+.5f} share {r.exercise_share:.4f}")
    assert Q_V0_TREE < 0.25   # a third of the early-exercise premium: beyond it the scheme is not working
    for seed, v0, tree, pol, pm, _ in rows:
        assert abs(v0 - tree) <= Q_V0_TREE, (seed, v0, tree)
        assert tree - pol <= Q_TREE_POLICY, (seed, tree, pol)
        assert abs(pm) <= Q_PNL_MEAN, (seed, pm)
