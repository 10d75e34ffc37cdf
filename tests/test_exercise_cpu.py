"""Early exercise (exercise="bermudan") on the CPU: the binomial-tree anchor,
TorchBackend.eval / TorchBackend.pnl with the exercise right against an fp64
numpy recursion on synthetic tables, the end-to-end run on the torch backend,
the rejected configurations, the CLI / example config and a two-rank gloo run.

The fp64 references and the case tables below are shared with
test_gpu_exercise.py (the same recursion checks k_hedge_eval / k_hedge_pnl).

Decision rule (both kernels, both backends): a path exercises at a date where
``X > 0 and X >= C``, X the intrinsic value of traded asset 0, C the
continuation value of the date's network.  A (path, date) pair is a *near tie*
when ``|X - C| <= 32 u max(1, |X|, |C|)`` in the fp64 reference (u = 2^-24):
fp32 and fp64 may decide those differently, every other pair must agree.  The
strikes below are chosen so that the reference alone has at most 0.5 % near
ties and 10 - 90 % of the pairs exercise (test_reference_cases_are_balanced).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_eval import (BOND_NOW, U, f32, make_inputs, make_spec, make_weights)
from test_gpu_eval import reference as eval_reference
from test_gpu_pnl import make_tables
from test_pnl import _np_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 32.0 * U
SHAPES = [(1, 8, 1, 1), (1, 8, 2, 0), (2, 8, 2, 0), (3, 8, 2, 0), (4, 8, 2, 0), (5, 8, 6, 0), (6, 8, 7, 0),
          (1, 32, 1, 1), (1, 32, 2, 0), (2, 32, 2, 0), (3, 32, 2, 0), (5, 32, 6, 0)]
KINDS = ("put", "call")


def near_tie(x, c):
    return np.abs(x - c) <= NEAR * np.maximum(1.0, np.maximum(np.abs(x), np.abs(c)))


def intrinsic64(kind, strike, s):
    """fp64 intrinsic value of fp32 prices, the strike rounded to fp32 first (a descriptor field)."""
    k = f32(strike)
    return np.maximum(k - s, 0.0) if kind == "put" else np.maximum(s - k, 0.0)


# ---------------------------------------------------------------------------
# eval: one date
# ---------------------------------------------------------------------------
EVAL_SEED_W, EVAL_SEED_IN = 21, 31


STRIKE_GRID = np.arange(0, 257, dtype=np.float64) / 64.0  # candidate strikes 0, 1/64 ... 4 (exact in fp32)


def pick_strike(kind, s, c, target):
    """The candidate strike whose share of exercised pairs, ``X > 0 and X >=
    C`` over the pooled fp64 reference prices ``s`` / continuation values
    ``c``, is nearest ``target`` (the smallest such candidate).  The nets of
    these tests are random, so their value level is arbitrary (negative, or far
    above any intrinsic value at a strike near the prices); choosing the strike
    from the reference keeps both outcomes frequent in every case."""
    best, best_d = 0.0, 2.0
    for k in STRIKE_GRID:
        x = np.maximum(k - s, 0.0) if kind == "put" else np.maximum(s - k, 0.0)
        d = abs(float(((x > 0.0) & (x >= c)).mean()) - target)
        if d < best_d - 1e-12:
            best, best_d = float(k), d
    return best


def eval_strike(spec, inp, w, alias, kind):
    ref = eval_reference(spec, inp, w, None, alias=alias)
    s = (inp["feats"][0] if alias else inp["now"][0]).double().numpy()
    return pick_strike(kind, s, ref["v"], 0.5)


def eval_ex_reference(spec, inp, w, alias, kind, strike):
    """fp64 outputs of an exercise date: reference() of test_gpu_eval plus the
    continuation / intrinsic values, the decision and the near ties."""
    ref = eval_reference(spec, inp, w, None, alias=alias)
    s = (inp["feats"][0] if alias else inp["now"][0]).double().numpy()
    cont = ref["v"]
    x = intrinsic64(kind, strike, s)
    ex = (x > 0.0) & (x >= cont)
    out = dict(ref)
    out.update(cont=cont, x=x, ex=ex, near=near_tie(x, cont) & (x > 0.0), v=np.where(ex, x, cont))
    return out


# ---------------------------------------------------------------------------
# P&L scan with the stopping rule
# ---------------------------------------------------------------------------
def pnl_forward(spec, tb, nd):
    """Per date: fp64 holdings of the date's network, prices at t and t + 1."""
    alpha = f32(spec.alpha)
    out = []
    for t in range(nd):
        X = np.stack([f[t].double().numpy() for f in tb["feats"]], axis=1)
        X = (X - tb["fmu"][t, :spec.nin].double().numpy()) * tb["fisd"][t, :spec.nin].double().numpy()
        h = _np_forward(spec, tb["ws"][t, 0].astype(np.float64), X, alpha)
        S0 = np.stack([p[t].double().numpy() for p in tb["prices"]], axis=1)
        S1 = np.stack([p[t + 1].double().numpy() for p in tb["prices"]], axis=1)
        out.append((h, S0, S1))
    return out


def pnl_continuation(spec, tb, fw, t):
    h, S0, _ = fw[t]
    na = spec.nhold - 1
    return (h[:, :na] * S0).sum(axis=1) + h[:, na] * f32(tb["bond"].numpy()[t])


def pnl_strike(spec, tb, fw, nd, kind, every):
    """About a quarter of the pooled (path, exercise date) pairs exercise."""
    dates = [t for t in range(nd) if t % every == 0]
    s = np.concatenate([fw[t][1][:, 0] for t in dates])
    c = np.concatenate([pnl_continuation(spec, tb, fw, t) for t in dates])
    return pick_strike(kind, s, c, 0.25)


def pnl_ex_reference(spec, tb, nd, kind, strike, every, fw=None):
    """fp64 recursion of test_gpu_pnl.reference with the stopping rule.
    Returns W (terminal-equivalent wealth), pnl, tau, paid (discounted to date
    0), ``amb`` (paths that met a near tie while alive: their later course is
    either one), and the numbers of live pairs, exercised pairs and near ties."""
    na = spec.nhold - 1
    n = tb["w0"].numel()
    W = tb["w0"].double().numpy().copy()
    bond = tb["bond"].numpy()
    fw = fw if fw is not None else pnl_forward(spec, tb, nd)
    tau = np.full(n, nd, np.int64)
    pnl_ex = np.zeros(n)
    paid = np.zeros(n)
    amb = np.zeros(n, bool)
    pairs = exercised = near = 0
    for t in range(nd):
        h, S0, S1 = fw[t]
        grow = f32(bond[t + 1] / bond[t])
        alive = tau == nd
        if t % every == 0:
            c = pnl_continuation(spec, tb, fw, t)
            x = intrinsic64(kind, strike, S0[:, 0])
            ex = alive & (x > 0.0) & (x >= c)
            nt = alive & ~amb & (x > 0.0) & near_tie(x, c)
            pairs += int((alive & ~amb).sum())
            exercised += int((ex & ~amb).sum())
            near += int(nt.sum())
            amb |= nt
            to_end = f32(bond[nd] / bond[t])
            pnl_ex = np.where(ex, (W - x) * to_end, pnl_ex)
            paid = np.where(ex, x * (bond[0] / bond[t]), paid)
            W = np.where(ex, W * to_end, W)
            tau = np.where(ex, t, tau)
            alive = tau == nd
        Wn = W * grow + (h[:, :na] * (S1 - S0 * grow)).sum(axis=1)
        W = np.where(alive, Wn, W)
    payoff = tb["payoff"].double().numpy()
    pnl = np.where(tau < nd, pnl_ex, W - payoff)
    paid = np.where(tau < nd, paid, payoff * (bond[0] / bond[nd]))
    return dict(W=W, pnl=pnl, tau=tau, paid=paid, amb=amb, pairs=pairs, exercised=exercised, near=near)


def _no_cancellation(spec, inp, w, alias):
    """The fp64 continuation value of every path is at least half the sum of
    its terms |h_k p_k|: ``max|ref|`` then is the magnitude the roundings act
    on, which the bound ``32 u max|ref|`` takes for granted (with many paths
    the largest value sees to that; a single path is all there is)."""
    ref = eval_reference(spec, inp, w, None, alias=alias)
    na = spec.nhold - 1
    p0 = inp["feats"][:na] if alias else inp["now"]
    terms = sum(np.abs(ref["hold"][:, k] * p0[k].double().numpy()) for k in range(na))
    terms = terms + np.abs(ref["hold"][:, na] * f32(BOND_NOW))
    return bool(np.all(np.abs(ref["v"]) >= 0.5 * terms))


def eval_case(shape, kind, n, alias):
    spec = make_spec(shape)
    w = make_weights(spec, EVAL_SEED_W)
    seed = EVAL_SEED_IN + n
    inp = make_inputs(spec, n, seed=seed)
    while n == 1 and not (_no_cancellation(spec, inp, w, True) and _no_cancellation(spec, inp, w, False)):
        seed += 100  # the single-path case: the first input seed whose reference value is well conditioned
        inp = make_inputs(spec, n, seed=seed)
    strike = eval_strike(spec, inp, w, alias, kind)
    return spec, inp, w, strike


def pnl_case(shape, kind, n, nd, every):
    spec = make_spec(shape)
    tb = make_tables(spec, n, nd, False, seed=7000 + 1000 * nd + n)
    fw = pnl_forward(spec, tb, nd)
    strike = pnl_strike(spec, tb, fw, nd, kind, every)
    return spec, tb, strike, pnl_ex_reference(spec, tb, nd, kind, strike, every, fw)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
ATM = dict(S0=100.0, K=100.0, r=0.08, sigma=0.15, T=1.0)
EURO_PUT, TREE_8 = 2.7012452750135054, 3.4303501009318516   # Black-Scholes; the tree with 8 exercise dates


def test_tree_european_equals_black_scholes():
    """CRR converges at O(1 / steps): 800 steps are 2.0e-3 off, every doubling
    halves it - 3200 steps within 1e-3 (doubling 100 steps per date moves the
    put by less than 1e-3, the issue's criterion for the default)."""
    from rphedge.analytic import bermudan_tree_price, black_scholes

    a = dict(S0=100.0, K=100.0, r=0.08, sigma=0.15, T=1.0, n_dates=8, exercise_every=1)
    for ot in ("PUT", "CALL"):
        bs = black_scholes(100.0, 100.0, 0.08, 0.15, 1.0, ot)[0]
        p400, bnd = bermudan_tree_price(option_type=ot, steps_per_date=400, exercise="european", **a)
        assert abs(p400 - bs) < 1e-3 and np.all(np.isnan(bnd))
    p100 = bermudan_tree_price(option_type="PUT", steps_per_date=100, exercise="european", **a)[0]
    p200 = bermudan_tree_price(option_type="PUT", steps_per_date=200, exercise="european", **a)[0]
    assert abs(p200 - p100) < 1e-3
    assert bermudan_tree_price(option_type="PUT", **a)[0] == pytest.approx(TREE_8, abs=1e-9)
    assert bermudan_tree_price(100, 100, 0.08, 0.15, 1.0, 30, 1, "PUT")[0] == pytest.approx(3.501, abs=1e-3)


def test_tree_put_monotone_in_exercise_dates_and_call_is_european():
    from rphedge.analytic import bermudan_tree_price

    # exercise dates {0}, {0, 4}, {0, 2, 4, 6}, {0 .. 7}: nested sets, so the price cannot fall
    p = [bermudan_tree_price(100, 100, 0.08, 0.15, 1.0, 8, k, "PUT")[0] for k in (8, 4, 2, 1)]
    assert p[0] == pytest.approx(bermudan_tree_price(100, 100, 0.08, 0.15, 1.0, 8, 1, "PUT", exercise="european")[0],
                                 abs=1e-12)   # the right at date 0 alone is worthless at the money
    assert p[0] < p[1] < p[2] < p[3]
    price, bnd = bermudan_tree_price(100, 100, 0.08, 0.15, 1.0, 8, 1, "PUT")
    assert np.isnan(bnd[0]) and np.all(np.diff(bnd[1:]) >= 0) and np.all(bnd[1:] < 100.0)
    # no dividends: a call is never exercised early
    c, cb = bermudan_tree_price(100, 100, 0.08, 0.15, 1.0, 8, 1, "CALL")
    ce = bermudan_tree_price(100, 100, 0.08, 0.15, 1.0, 8, 1, "CALL", exercise="european")[0]
    assert c == pytest.approx(ce, abs=1e-12) and np.all(np.isnan(cb))


def test_reference_cases_are_balanced():
    """The fp64 reference alone: at most 0.5 % near ties and 10 - 90 % of the
    pairs exercising in every group of cases the GPU tests assert on."""
    for shape in SHAPES:
        for kind in KINDS:
            pairs = exd = near = 0
            for n in (1, 255, 256, 1000):
                for alias in (True, False):
                    spec, inp, w, k = eval_case(shape, kind, n, alias)
                    r = eval_ex_reference(spec, inp, w, alias, kind, k)
                    pairs, exd, near = pairs + n, exd + int(r["ex"].sum()), near + int(r["near"].sum())
            assert near <= 0.005 * pairs and 0.1 <= exd / pairs <= 0.9, (shape, kind, pairs, exd, near)
    for shape in SHAPES:
        for nd in (1, 2, 7):
            for every in (1, 3):
                pairs = exd = near = 0
                for kind in KINDS:
                    for n in (1023, 1025):
                        r = pnl_case(shape, kind, n, nd, every)[3]
                        pairs, exd, near = pairs + r["pairs"], exd + r["exercised"], near + r["near"]
                assert near <= 0.005 * pairs and 0.1 <= exd / pairs <= 0.9, (shape, nd, every, pairs, exd, near)


CPU_SHAPES = [(1, 8, 2, 0), (2, 8, 2, 0), (1, 8, 1, 1)]


def _torch_backend(spec, n):
    from rphedge.engine import TorchBackend, TrainConfig

    return TorchBackend(spec, n, TrainConfig(batch_size=n))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_torch_eval_exercise_vs_fp64(shape, kind):
    """TorchBackend.eval with the exercise right (fp32) against the fp64
    reference: values within 32 u max|ref| and the decision identical off near
    ties, the new columns within the statistics bound of test_gpu_eval."""
    from rphedge.engine import DateData, Exercise
    from rphedge.ops import layout as L

    pairs = exd = near_n = 0
    for n, alias in ((1000, True), (257, False)):
        spec, inp, w, strike = eval_case(shape, kind, n, alias)
        na = spec.nhold - 1
        be = _torch_backend(spec, n)
        data = DateData(feats=inp["feats"], prices_next=inp["nxt"], bond_next=1.07, target=inp["target"],
                        prices_now=inp["feats"][:na] if alias else inp["now"], bond_now=BOND_NOW, fmu=inp["fmu"],
                        fisd=inp["fisd"])
        v, vc = torch.empty(n), torch.empty(n)
        st = be.new_stats()
        be.eval(be.new_weights(w), data, st, v_out=v, exercise=Exercise(kind=kind, strike=strike))
        be.eval(be.new_weights(w), data, be.new_stats(), v_out=vc)
        ref = eval_ex_reference(spec, inp, w, alias, kind, strike)
        near, off = ref["near"], ~ref["near"]
        tol = 32 * U * float(np.abs(ref["v"]).max())
        tol_c = 32 * U * float(np.abs(ref["cont"]).max())
        got = v.double().numpy()
        assert np.all(np.abs(got - ref["v"])[off] <= tol)
        # the decision, read bitwise: the stored value is the fp32 continuation value or the fp32 intrinsic one
        x32 = Exercise(kind=kind, strike=strike).intrinsic(data.prices_now[0])
        is_c, is_x = v == vc, v == x32
        assert bool(torch.all(is_c | is_x))
        took_x = torch.where(is_x & is_c, x32 > 0, is_x).numpy()
        assert np.array_equal(took_x[off], ref["ex"][off])
        assert np.all(np.minimum(np.abs(got - ref["x"]), np.abs(got - ref["cont"]))[near] <= tol + tol_c)
        s = st[0].numpy()
        assert abs(s[L.ES_EXER] - ref["ex"].sum()) <= near.sum()
        slack = float(np.maximum(np.abs(ref["x"]), np.abs(ref["cont"]))[near].sum())
        assert abs(s[L.ES_CONT] - ref["cont"].sum()) <= n * tol_c + 8 * U * np.abs(ref["cont"]).sum()
        xs = np.where(ref["ex"], ref["x"], 0.0)
        assert abs(s[L.ES_EXVAL] - xs.sum()) <= n * 32 * U * np.abs(ref["x"]).max() + 8 * U * xs.sum() + slack
        assert abs(s[L.ES_V] - ref["v"].sum()) <= n * tol + 8 * U * np.abs(ref["v"]).sum() + slack
        pairs, exd, near_n = pairs + n, exd + int(ref["ex"].sum()), near_n + int(near.sum())
        # without the right: the plain path, new columns zero
        st0 = be.new_stats()
        be.eval(be.new_weights(w), data, st0, v_out=v)
        assert np.all(np.abs(v.double().numpy() - ref["cont"]) <= tol_c) and np.all(st0[0].numpy()[26:] == 0.0)
    assert near_n <= 0.005 * pairs and 0.1 <= exd / pairs <= 0.9


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("nd", [1, 3, 8])
@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_torch_pnl_stopping_vs_fp64(shape, nd, every):
    from rphedge.engine import Exercise, PnlData
    from rphedge.ops import layout as L

    pairs = exd = near = 0
    for kind in KINDS:
        n = 1025
        spec, tb, strike, ref = pnl_case(shape, kind, n, nd, every)
        be = _torch_backend(spec, n)
        data = PnlData(n_dates=nd, features=lambda t: [f[t] for f in tb["feats"]],
                       prices=lambda t: [p[t] for p in tb["prices"]], bond=tb["bond"], fmu=tb["fmu"],
                       fisd=tb["fisd"], w0=tb["w0"], payoff=tb["payoff"])
        snap = torch.nan_to_num(tb["snap"], nan=0.0)
        st, out, tau = be.new_pnl_stats(), torch.empty(n), torch.empty(n, dtype=torch.int32)
        be.pnl(snap, data, st, pnl_out=out, exercise=Exercise(kind=kind, strike=strike, every=every), tau_out=tau)
        ok = ~ref["amb"]
        t = tau.numpy().astype(np.int64)
        assert np.array_equal(t[ok], ref["tau"][ok])
        F = 32.0 * nd
        scale = float(np.abs(ref["pnl"]).max())
        assert np.abs(out.double().numpy() - ref["pnl"])[ok].max() <= F * U * scale
        s = st[0].numpy()
        assert s[L.ES_EXER] == (t < nd).sum() and s[L.ES_TAU] == t.sum() and s[L.ES_COUNT] == n
        if not ref["amb"].any():
            assert s[L.ES_EXVAL] == pytest.approx(ref["paid"].sum(), rel=4 * U)
        pairs, exd, near = pairs + ref["pairs"], exd + ref["exercised"], near + ref["near"]
        with pytest.raises(ValueError, match="has_b with exercise"):
            be.pnl(snap, data, st, has_b=True, exercise=Exercise(kind=kind, strike=strike))
    assert near <= 0.005 * pairs and 0.1 <= exd / pairs <= 0.9


def put_params(n_paths=14, **kw):
    p = dict(Y=100, K=100, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.125, N=1, P=1, x=0, l0=0, c=0, ita=0,
             dt=0.125 / 4, n_paths=n_paths, payoff="put", option_type="PUT", model="gbm_log", mortality=False,
             q99=False, optimizer="lm", lm_passes_first=80, lm_passes_rest=3, early_stopping=False, verbose=False,
             exercise="bermudan", device="cpu", backend="torch")
    p.update(kw)
    return p


@pytest.fixture(scope="module")
def cpu_put():
    """(run, result) of the ATM Bermudan put: 8 dates, 2^14 paths, LM, torch backend."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(put_params()))
    return run, run.run()


def test_e2e_cpu_bermudan_put(cpu_put):
    from test_gpu_exercise import Q_V0_TREE

    run, res = cpu_put
    ind, paths = res.induction, res.paths
    nd = paths.n_coarse - 1
    assert nd == 8 and res.tree_price == pytest.approx(TREE_8, abs=1e-9)
    assert res.summary["bs_price"] == pytest.approx(EURO_PUT, abs=1e-9)
    print(f"CPU put: V0 {res.v0:.5f} tree {res.tree_price:.5f} policy {res.policy_value:.5f} "
          f"pnl mean {res.self_financing_pnl['mean']:+.5f} share {res.exercise_share:.4f}")
    assert abs(res.v0 - TREE_8) < abs(res.v0 - EURO_PUT)
    assert abs(res.v0 - TREE_8) <= Q_V0_TREE < 0.25
    # the policy's own price: the mean of the discounted amounts paid, recomputed from tau and the paths
    tau = ind.tau.numpy().astype(np.int64)
    bond = np.asarray(paths.bond, np.float64)
    s = np.stack([paths.prices(t)[0].double().numpy() for t in range(nd)], axis=0)
    x = np.maximum(1.0 - s[np.minimum(tau, nd - 1), np.arange(tau.size)], 0.0)
    paid = np.where(tau < nd, x * bond[0] / bond[np.minimum(tau, nd - 1)],
                    ind.values[nd].double().numpy() * bond[0] / bond[nd]) * res.scale
    assert res.policy_value == pytest.approx(paid.mean(), rel=1e-6)
    se = paid.std(ddof=1) / math.sqrt(paid.size)
    assert res.policy_value <= TREE_8 + 4 * se
    assert res.exercise_share == pytest.approx((tau < nd).mean(), abs=1e-12) and 0.1 < res.exercise_share < 0.9
    assert res.mean_exercise_date == pytest.approx(tau.mean() * paths.grid.dt_coarse, rel=1e-9)
    # the unstopped scan keeps hedging exercised paths: its mean is the early-exercise premium it never paid
    be, bi = run.backend, run.induction
    st = be.new_pnl_stats()
    be.pnl(bi.snap, bi.pnl_data, st)
    from rphedge.ops import layout as L

    spurious = float(st[0, L.ES_RES] / st[0, L.ES_COUNT]) * res.scale
    print(f"CPU put: unstopped P&L mean {spurious:+.5f}")
    assert abs(res.self_financing_pnl["mean"]) < abs(spurious) and spurious > 0.5
    # per-date report and boundary
    dates = res.summary["exercise_dates"]
    assert [d["date"] for d in dates] == list(range(7, -1, -1)) and dates[-1]["share"] == 0.0
    assert all(0.0 <= d["share"] <= 1.0 and d["mean_continuation"] > 0 for d in dates)
    from rphedge.utils.reports import exercise_boundary

    eb = exercise_boundary(res)
    assert eb["dates"] == list(range(8)) and math.isnan(eb["boundary"][0])
    b, tr = np.asarray(eb["boundary"][1:]), np.asarray(eb["tree"][1:])
    assert np.all(b < 100.0) and np.all(np.abs(b - tr) < 3.0)   # within 3 % of the strike of the tree's boundary


# The European put of put_params() on the commit before the exercise keys existed, one torch thread (the
# CPU reductions depend on the thread count in their last bits): V0, P&L std, sha256 of values / pnl_paths
PARENT_EURO = ("0x1.59178e0000000p+1", "0x1.b8c057b2e75b4p+0",
               "a7f681d703889c003847886cf85c46e23be38950bbe5b29a6cdebb804e3c367b",
               "744097b20e676251a76faf24f2056ea2cc2882f3e06e714e3f13b4352651c4b9")


def test_e2e_cpu_european_unchanged(cpu_put):
    """exercise="european" is bitwise the run of the parent commit (recorded
    above under one thread), and bitwise the run without the key."""
    import hashlib

    from rphedge.api import run_params

    def sha(t):
        return hashlib.sha256(t.numpy().tobytes()).hexdigest()

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        a = run_params(put_params(exercise="european"))
        kw = put_params()
        del kw["exercise"]
        b = run_params(kw)
    finally:
        torch.set_num_threads(threads)
    got = (float(a.v0).hex(), float(a.self_financing_pnl["std"]).hex(), sha(a.induction.values),
           sha(a.induction.pnl_paths))
    assert got == PARENT_EURO
    assert torch.equal(a.induction.values, b.induction.values)
    assert torch.equal(a.induction.pnl_paths, b.induction.pnl_paths) and a.v0 == b.v0
    assert a.induction.tau is None and a.exercise_share is None and a.tree_price is None
    assert "exercise" not in a.summary
    assert a.v0 < 2.75 < cpu_put[1].v0


def test_plot_run_draws_exercise_boundary(cpu_put, tmp_path):
    from rphedge.utils.reports import plot_run

    files = plot_run(cpu_put[1], out_prefix=str(tmp_path / "put"))
    fig = str(tmp_path / "put_exercise_boundary.png")
    assert fig in files and os.path.getsize(fig) > 0
    # a European run has no such figure
    from rphedge.api import run_params

    e = run_params(put_params(exercise="european", n_paths=10, lm_passes_first=10))
    assert not any("exercise_boundary" in f for f in plot_run(e, out_prefix=str(tmp_path / "euro")))


# worst of seeds 1234 .. 1241 on the torch backend (2^14 paths, 8 dates): |V0 - European V0| 0.00473,
# exercised share 0.00415 (a call without dividends is never worth exercising; the net's fit error near the
# strike exercises a few deep in-the-money paths); bounds 1.5 x the worst seed
CALL_V0_DIFF, CALL_SHARE = 0.0071, 0.0063


@pytest.mark.parametrize("seed", [1234, 1238])
def test_e2e_cpu_bermudan_call_is_european(seed):
    from rphedge.api import run_params

    kw = dict(payoff="call", option_type="CALL", seed=seed, keep_paths=False)
    a = run_params(put_params(**kw))
    b = run_params(put_params(exercise="european", **kw))
    print(f"CPU call seed {seed}: V0 {a.v0:.5f} European {b.v0:.5f} share {a.exercise_share:.5f}")
    assert abs(a.v0 - b.v0) <= CALL_V0_DIFF and a.exercise_share <= CALL_SHARE
    assert a.tree_price == pytest.approx(a.summary["bs_price"], abs=3e-3)


@pytest.mark.parametrize("kw,msg", [
    (dict(payoff="basket_call", model="basket", n_assets=3), "basket, pension or mortality"),
    (dict(payoff="guarantee", mortality=True, model="gbm"), "basket, pension or mortality"),
    (dict(payoff="guarantee", mortality=False, model="gbm"), "basket, pension or mortality"),
    (dict(payoff="asian_put"), "path-dependent payoff 'asian_put'"),
    (dict(payoff="lookback_call", option_type="CALL"), "path-dependent payoff 'lookback_call'"),
    (dict(q99=True), "q99=True"),
    (dict(parity=True), "parity=True"),
    (dict(model="sv_ref"), "model 'sv_ref'"),
    (dict(exercise="bermudan", exercise_every=0), "exercise_every must be >= 1"),
    (dict(exercise="american", exercise_every=2), "exercise='american' is exercise='bermudan' with exercise_every=1"),
    (dict(exercise="asian"), "exercise must be european"),
])
def test_rejected_combinations(kw, msg):
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    with pytest.raises(ValueError, match=msg):
        HedgeRun(parse_params(put_params(**kw)))


def test_second_network_rejected_by_backend_and_driver():
    from rphedge.engine import DateData, Exercise

    spec, inp, w, strike = eval_case((1, 8, 2, 0), "put", 256, True)
    be = _torch_backend(spec, 256)
    data = DateData(feats=inp["feats"], prices_next=inp["nxt"], bond_next=1.07, target=inp["target"],
                    prices_now=inp["feats"][:1], bond_now=BOND_NOW, fmu=inp["fmu"], fisd=inp["fisd"])
    ex = Exercise(kind="put", strike=strike)
    with pytest.raises(ValueError, match="wb / g_base with exercise"):
        be.eval(be.new_weights(w), data, be.new_stats(), wts_b=be.new_weights(w), exercise=ex)
    with pytest.raises(ValueError, match="wb / g_base with exercise"):
        be.eval(be.new_weights(w), data, be.new_stats(), g_base=inp["g_base"], exercise=ex)
    with pytest.raises(ValueError, match="kind must be 'put' or 'call'"):
        Exercise(kind="straddle", strike=1.0)


def test_american_alias_heston_and_saved_config(tmp_path):
    """"american" = bermudan with k = 1; a Heston run takes the 2-input shape
    (no tree price); the saved run config carries the keys."""
    from rphedge.api import run_params

    small = dict(n_paths=11, lm_passes_first=20, lm_passes_rest=2)
    a = run_params(put_params(exercise="american", **small))
    b = run_params(put_params(exercise="bermudan", exercise_every=1, **small))
    assert a.v0 == b.v0 and a.exercise_share == b.exercise_share and a.summary["exercise"] == "bermudan"
    h = run_params(put_params(model="heston", save_dir=str(tmp_path / "run"), **small))
    assert h.tree_price is None and h.exercise_share is not None and h.induction.weights_snapshots.shape[0] == 8
    saved = json.load(open(tmp_path / "run" / "config.json"))["config"]
    assert saved["exercise"] == "bermudan" and saved["exercise_every"] == 1 and saved["model"] == "heston"


def test_cli_and_example_config(capsys):
    from rphedge.__main__ import main

    assert main(["european", "--paths", "2048", "--rebalancing", "0.125", "--exercise", "bermudan",
                 "--exercise-every", "2", "--set", "OPTION_TYPE=PUT", "dt=0.03125", "device=cpu", "verbose=false",
                 "optimizer=lm", "lm_passes_first=20", "lm_passes_rest=2", "early_stopping=false"]) == 0
    out = json.loads(capsys.readouterr().out)
    s = out["summary"]
    assert s["exercise"] == "bermudan" and s["exercise_every"] == 2 and 0.0 <= s["exercise_share"] <= 1.0
    assert s["tree_price"] == pytest.approx(3.3366, abs=1e-3) and s["policy_value"] > 0
    cfg = json.load(open(os.path.join(ROOT, "examples", "bermudan_put_30.json")))
    ref = json.load(open(os.path.join(ROOT, "examples", "euro_call_30_lm.json")))
    assert {k: v for k, v in cfg.items() if k not in ("payoff", "option_type", "exercise", "exercise_every")} == \
        {k: v for k, v in ref.items() if k not in ("payoff", "option_type")}
    assert main(["run", "--config", os.path.join(ROOT, "examples", "bermudan_put_30.json"), "--set", "n_paths=11",
                 "device=cpu", "verbose=false", "lm_passes_first=20", "batch_size=2048"]) == 0
    s = json.loads(capsys.readouterr().out)["summary"]
    assert s["exercise"] == "bermudan" and s["n_dates"] == 30 and s["tree_price"] == pytest.approx(3.501, abs=1e-3)


def _dp_cfg():
    from rphedge.config import parse_params

    # full-batch gradient descent (batch = all paths, no shuffle): the two-rank gradient is the one-rank gradient
    return parse_params(put_params(n_paths=11, optimizer="adam", batch_size=2048, epochs_first=12, epochs_rest=4,
                                   early_stopping=False, lr_schedule_first=False, shuffle=False, lr=5e-3))


def _dp_worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from rphedge.api import HedgeRun
    from rphedge.parallel import dist as D

    di = D.init(device="cpu")
    res = HedgeRun(_dp_cfg(), dist_info=di).run()
    if rank == 0:
        with open(out, "w") as f:
            json.dump({"v0": res.v0, "share": res.exercise_share, "policy": res.policy_value,
                       "tau_mean": res.mean_exercise_date, "dates": res.summary["exercise_dates"]}, f)
    D.shutdown()


def test_dp_two_ranks_reproduce_one_process(tmp_path):
    import torch.multiprocessing as mp

    from test_distributed_cpu import _free_port

    world, port, out = 2, _free_port(), str(tmp_path / "dp.json")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    dp = json.load(open(out))
    from rphedge.api import HedgeRun
    from rphedge.parallel import dist as D

    ref = HedgeRun(_dp_cfg(), dist_info=D.DistInfo(device=torch.device("cpu"))).run()
    # values agree to 2e-4 (test_distributed_cpu); a decision flips only where |X - C| is below that, a
    # fraction of a percent of the paths
    assert dp["v0"] == pytest.approx(ref.v0, rel=1e-3)
    assert dp["share"] == pytest.approx(ref.exercise_share, abs=5e-3)
    assert dp["policy"] == pytest.approx(ref.policy_value, rel=5e-3)
    for a, b in zip(dp["dates"], ref.summary["exercise_dates"]):
        assert a["date"] == b["date"] and a["share"] == pytest.approx(b["share"], abs=5e-3)
