"""The self-financing P&L folded into the backward induction: k_hedge_eval
accumulating R_t per path (EvalDesc.pnl_acc) from date nd - 1 down to 0, then
k_pnl_finish - against the fp64 forward recursion of test_gpu_pnl on its
synthetic tables and NaN-padded snapshots, with that file's bounds (u = 2^-24):
per path ``|pnl - ref| <= 32 n_dates u max|ref|``, the statistics ``n x`` the
per-path tolerance ``+ 8 u sum|terms|``, ES_COUNT exact, the other columns 0.

Every sequence runs twice into one accumulator that starts as NaN: the first
accumulated date must write R, not add to it, and both runs must agree bitwise.

Largest per-path error measured on an MI355X over every case below, in
u max|ref| per date (bound 32): 2.9 (the forward scan: 7.9, test_gpu_pnl).  The
driver case measured 8.4 u max|scan| over its 4 dates (bound 256).

The driver cases: a 2^12-path, 4-date LM run's folded P&L against the forward
scan (HipBackend.pnl) on the same snapshots and paths - two results within the
bound of the exact one are within twice the bound of each other - and an
early-exercise run, which keeps the forward scan.
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from test_gpu_eval import GUARD, SENTINEL, U, check_guards, guarded, make_spec  # noqa: F401
from test_gpu_kernels import dev  # noqa: F401  (fixture)
from test_gpu_pnl import HOLD_C, make_tables, reference

pytestmark = pytest.mark.gpu

# (shape, two networks per date)
CASES = [((1, 8, 2, 0), False), ((1, 8, 1, 1), False), ((5, 8, 6, 0), False), ((3, 8, 2, 0), True),
         ((1, 32, 2, 0), False)]
MAX_ULPS = [0.0]


def fold(be, spec, tb, nd, has_b, dev, acc, slab, out, alias=False):  # noqa: F811
    """The driver's sequence: the final eval of every date nd - 1 .. 0 with the accumulator, then the finish."""
    from rphedge.engine import DateData, pnl_fold_factors
    from rphedge.ops import layout as L

    grow, carry, carry_all = pnl_fold_factors(tb["bond"].numpy())
    feats = [f.to(dev) for f in tb["feats"]]
    prices = feats[:spec.nhold - 1] if alias else [p.to(dev) for p in tb["prices"]]
    snap = tb["snap"].to(dev)
    bond = tb["bond"].numpy()
    es = torch.empty(be.eval_wgs, L.EVAL_NSTAT, dtype=torch.float64, device=dev)
    for t in range(nd - 1, -1, -1):
        data = DateData(feats=[f[t] for f in feats], prices_next=[p[t + 1] for p in prices], bond_next=float(bond[t + 1]),
                        target=None, prices_now=[p[t] for p in prices], bond_now=float(bond[t]),
                        fmu=tuple(float(x) for x in tb["fmu"][t, :spec.nin]),
                        fisd=tuple(float(x) for x in tb["fisd"][t, :spec.nin]))
        kw = dict(wts_b=snap[t, 1], hold_c=HOLD_C) if has_b else {}
        be.eval(snap[t, 0], data, es, pnl_acc=acc, pnl_grow=float(grow[t]), pnl_carry=float(carry[t]),
                pnl_first=t == nd - 1, **kw)
    be.pnl_finish(acc, tb["w0"].to(dev), tb["payoff"].to(dev), float(carry_all), slab, pnl_out=out)


# separate price tables (test_gpu_pnl.make_tables as it builds them) at every size; the price-alias form at the
# sizes where max|ref| is a maximum over many paths
SIZES = [(False, n) for n in (1, 255, 256, 257, 2500)] + [(True, n) for n in (257, 2500)]


@pytest.mark.parametrize("nd", [1, 2, 7])
@pytest.mark.parametrize("alias,n", SIZES)
@pytest.mark.parametrize("shape,has_b", CASES)
def test_fold_vs_fp64_recursion(dev, shape, has_b, alias, n, nd):  # noqa: F811
    """``alias``: the traded prices ARE the leading features (the price-alias
    instantiation of the eval, the GBM / basket runs' form: the same
    arithmetic, the prices taken from the feature registers); else separate
    tables.  The bounds scale with max|ref| over the paths, which presumes a
    population: with ONE path it is that path's own cancellation residue, not
    the magnitude of the terms that were rounded.  The separate-table cases keep
    n = 1 as test_gpu_pnl has it; the alias tables are not run there ((5,8,6,0),
    n = 1, nd = 2 gave W = 0.03875 from terms of magnitude 1..6 with an error
    of 2.6e-7: 0.7 u of the largest price, 101 u of |W|, bound 64)."""
    from rphedge.engine import HipBackend, TrainConfig, reduce_stats
    from rphedge.ops import layout as L

    spec = make_spec(shape)
    tb = make_tables(spec, n, nd, has_b, seed=1000 * nd + n)
    if alias:
        tb["prices"] = tb["feats"][:spec.nhold - 1]
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    wgs = (n + 1023) // 1024
    assert be.pnl_wgs() == wgs
    runs = []
    abuf, acc = guarded(n, dev)
    acc.fill_(float("nan"))
    for _ in range(2):
        slab = torch.full((wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
        buf, out = guarded(n, dev)
        fold(be, spec, tb, nd, has_b, dev, acc, slab, out, alias=alias)
        torch.cuda.synchronize()
        runs.append((buf.cpu().numpy().copy(), slab.cpu().numpy().copy(), abuf.cpu().numpy().copy()))
    tag = f"pnl fold {shape} alias={alias} n={n} nd={nd}"
    for a, b in zip(*runs):  # the second run saw the first run's R: the first date must not read it
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{tag}: the second run differs"
    check_guards(tag, buf)
    check_guards(tag + " acc", abuf)

    W, pnl = reference(spec, tb, nd, has_b)
    F = 32.0 * nd
    got = out.cpu().numpy().astype(np.float64)
    scale = float(np.abs(pnl).max())
    tol_p, tol_w = F * U * scale, F * U * float(np.abs(W).max())
    err = float(np.abs(got - pnl).max())
    MAX_ULPS[0] = max(MAX_ULPS[0], err / (U * scale * nd))
    print(f"ULPS {tag}: {err / (U * scale):.3f} u max|ref| (bound {F:.0f}); per date so far max {MAX_ULPS[0]:.3f}")
    assert err <= tol_p, f"{tag}: max err {err:.3e} = {err / (U * scale):.2f} u max|ref| > {F:.0f}"

    raw = slab.cpu().numpy()
    assert not np.isnan(raw).any(), f"{tag}: statistics rows not overwritten"
    cnt = np.bincount(np.arange(n) // 1024, minlength=wgs)
    assert np.array_equal(raw[:, L.ES_COUNT], cnt.astype(np.float64))
    st = reduce_stats(slab)
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


@pytest.mark.parametrize("shape,has_b", CASES)
def test_eval_outputs_do_not_depend_on_the_fold(dev, shape, has_b):  # noqa: F811
    """pnl_acc=None (with the other new arguments set) is the call without
    them, byte for byte; and an accumulating call writes the same values,
    holdings, residuals and statistics beside its R."""
    from rphedge.engine import DateData, HipBackend, TrainConfig
    from rphedge.ops import layout as L

    spec = make_spec(shape)
    n, nd = 1500, 2
    tb = make_tables(spec, n, nd, has_b, seed=77)
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    feats = [f.to(dev) for f in tb["feats"]]
    prices = [p.to(dev) for p in tb["prices"]]
    snap = tb["snap"].to(dev)
    data = DateData(feats=[f[0] for f in feats], prices_next=[p[1] for p in prices], bond_next=1.07,
                    target=tb["payoff"].to(dev), prices_now=[p[0] for p in prices], bond_now=1.03,
                    fmu=tuple(float(x) for x in tb["fmu"][0, :spec.nin]),
                    fisd=tuple(float(x) for x in tb["fisd"][0, :spec.nin]))
    kw = dict(wts_b=snap[0, 1], hold_c=HOLD_C, g_base=tb["w0"].to(dev), blend_c=0.1) if has_b else {}

    def call(**extra):
        bufs = [guarded(n, dev) for _ in range(3 + spec.nhold)]
        slab = torch.full((be.eval_wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
        be.eval(snap[0, 0], data, slab, v_out=bufs[0][1], resid_out=bufs[1][1], pred1_out=bufs[2][1],
                hold_out=[b[1] for b in bufs[3:]], **kw, **extra)
        torch.cuda.synchronize()
        return [b[0].cpu().numpy().view(np.uint32) for b in bufs] + [slab.cpu().numpy().view(np.uint64)]

    plain = call()
    off = call(pnl_acc=None, pnl_grow=1.03, pnl_carry=0.9, pnl_first=True)
    abuf, acc = guarded(n, dev)
    on = call(pnl_acc=acc, pnl_grow=1.03, pnl_carry=0.9, pnl_first=True)
    for a, b, c in zip(plain, off, on):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    check_guards("acc", abuf)
    assert torch.isfinite(acc).all() and float(acc.abs().max()) > 0


def test_fold_rejects_what_it_cannot_accumulate(dev):  # noqa: F811
    from rphedge.engine import DateData, Exercise, HipBackend, TrainConfig
    from rphedge.ops import layout as L

    spec = make_spec((1, 8, 2, 0))
    n = 300
    tb = make_tables(spec, n, 1, False, seed=3)
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    f, snap = [x.to(dev) for x in tb["feats"]], tb["snap"].to(dev)
    slab = torch.zeros(be.eval_wgs, L.EVAL_NSTAT, dtype=torch.float64, device=dev)
    acc = torch.zeros(n, dtype=torch.float32, device=dev)
    no_next = DateData(feats=[f[0][0]], prices_next=[], bond_next=1.0, target=None, prices_now=[f[0][0]], bond_now=1.0)
    with pytest.raises(RuntimeError, match=r"rph_eval failed \(-22\): pnl_acc needs price_t and price_t1"):
        be.eval(snap[0, 0], no_next, slab, pnl_acc=acc, pnl_first=True)
    full = DateData(feats=[f[0][0]], prices_next=[f[0][1]], bond_next=1.0, target=None, prices_now=[f[0][0]],
                    bond_now=1.0)
    with pytest.raises(RuntimeError, match=r"rph_eval failed \(-22\): pnl_acc with ex_kind"):
        be.eval(snap[0, 0], full, slab, pnl_acc=acc, pnl_first=True, exercise=Exercise(kind="put", strike=1.0))
    with pytest.raises(ValueError, match="pnl_acc must be float32"):
        be.eval(snap[0, 0], full, slab, pnl_acc=acc[:-1], pnl_first=True)
    assert float(acc.abs().max()) == 0.0


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def call_params(**kw):
    p = dict(Y=100, K=100, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.25, N=1, P=1, x=0, l0=0, c=0, ita=0,
             dt=0.125, n_paths=12, payoff="call", option_type="CALL", model="gbm_log", mortality=False, q99=False,
             optimizer="lm", lm_passes_first=30, lm_passes_rest=2, early_stopping=False, verbose=False, seed=1234)
    p.update(kw)
    return p


def test_driver_fold_matches_forward_scan(dev):  # noqa: F811
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params
    from rphedge.engine import reduce_stats
    from rphedge.ops import layout as L

    run = HedgeRun(parse_params(call_params(device=str(dev))))
    try:
        res = run.run()
        drv, be = run.induction, run.backend
        nd, n = drv.n_dates, 4096
        assert nd == 4 and drv.pnl_fold and res.induction.pnl.count == n
        folded = res.induction.pnl_paths.clone()
        stats = np.asarray(res.induction.pnl.stats, np.float64).copy()
        # the forward scan over the same snapshots, paths, V_0 and payoff
        slab = be.new_pnl_stats()
        scan = torch.empty(n, dtype=torch.float32, device=dev)
        be.pnl(drv.snap, drv.pnl_data, slab, has_b=False, hold_c=drv.hold_c, pnl_out=scan)
        torch.cuda.synchronize()
        ref = scan.double().cpu().numpy()
        tol = 2 * 32.0 * nd * U * float(np.abs(ref).max())
        err = float(np.abs(folded.double().cpu().numpy() - ref).max())
        print(f"driver fold vs scan: {err / (U * np.abs(ref).max()):.3f} u max|scan| (bound {2 * 32 * nd})")
        assert err <= tol
        st = reduce_stats(slab)
        assert stats[L.ES_COUNT] == st[L.ES_COUNT] == n
        assert abs(stats[L.ES_RES] - st[L.ES_RES]) <= n * tol
        assert abs(stats[L.ES_RESMIN] - st[L.ES_RESMIN]) <= tol and abs(stats[L.ES_RESMAX] - st[L.ES_RESMAX]) <= tol
        # a captured graph replays the fold from scratch every time (nothing carried over in R)
        run.capture(include_simulation=True)
        for _ in range(2):
            run.replay()
            assert torch.equal(run.collect().induction.pnl_paths, folded)
    finally:
        run.close()


def test_driver_exercise_run_keeps_the_forward_scan(dev):  # noqa: F811
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    params = json.loads((Path(__file__).resolve().parent.parent / "examples" / "bermudan_put_30.json").read_text())
    params.update(rebalancing=0.25, dt=0.25, n_paths=12, batch_size=4096, verbose=False, device=str(dev))
    run = HedgeRun(parse_params(params))
    try:
        res = run.run()
        assert run.induction.n_dates == 4 and not run.induction.pnl_fold
        tau = res.induction.tau
        assert tau is not None and tau.dtype == torch.int32 and int(tau.min()) >= 0 and int(tau.max()) <= 4
        share = float((tau < 4).double().mean())
        assert 0.0 < share < 1.0 and res.exercise_share == pytest.approx(share, abs=1e-12)
        assert res.mean_exercise_date == pytest.approx(float(tau.double().mean()) * 0.25, rel=1e-12)
    finally:
        run.close()
