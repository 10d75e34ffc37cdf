"""Merton jump-diffusion on the CPU: the jump-count thresholds, the fp64 numpy
twin ``_cpu_merton`` against Merton's series, the series itself, the config
surface (``model="merton"``, every rejection) and the torch-backend runs (a
Merton run end to end; a gbm_log hedge stressed with jumps out of sample).

Jump sets (lam, mu_J, sigma_J): J1 = (1, -0.1, 0.15), J5 = (5, -0.05, 0.1),
J8 = (8, 0.02, 0.05).  Grids GB = Grid(1, 1/32, 1/8), GN = Grid(2, 0.25, 0.5);
path ranges R1-R9 of tests/test_gpu_path_scans.py.

Census of the count uniforms (``SEED_W1``, the nine ranges pooled), asserted in
``test_counts_census_and_no_uniform_near_a_threshold``: GN x J8 (lam dt = 2)
reaches the 8-jump cap on 49 draws; GB x J5 has 2186 double and 110 triple
jumps; no count uniform of any range x grid x set lies within 2 of a threshold
below 2^30 - so the GPU comparison of tests/test_gpu_merton.py leaves out no
path.

Twin against the series (2^14 paths, S0 = K = 100, r = 0.05, sigma = 0.2,
T = 1, GB), discounted call payoff: J1 12.804 against 12.761, J5 14.819
against 14.766 - both 0.3 standard errors off (bound: 4).
"""
import math

import numpy as np
import pytest

END = 1 << 30
RANGES = {
    "R1": (1, 0, None), "R2": (257, 64, None), "R3": (512, 37, None), "R4": (2051, 37, None),
    "R5": (512, 0, (64, 1024)), "R6": (300, 0, (50, 1000)), "R7": (512, END - 512, None),
    "R8": (300, END - 300, None), "R9": (2048, 0, None),
}
GRIDS = {"GB": (1.0, 1 / 32, 1 / 8), "GN": (2.0, 0.25, 0.5)}
JUMPS = {"J1": (1.0, -0.1, 0.15), "J5": (5.0, -0.05, 0.1), "J8": (8.0, 0.02, 0.05)}


def grid(key):
    from rphedge.ops.paths import Grid

    return Grid(*GRIDS[key])


def count_uniforms(gk, rk):
    """The raw 30-bit count uniforms [n, n_fine] of a range: dimensions [nf, 2 nf) of the 3 nf-dimensional sequence."""
    from rphedge.ops import paths as P

    g = grid(gk)
    n, off, m = RANGES[rk]
    nf = g.n_fine
    return P._u30(3 * nf, P.SEED_W1, n, off, 3 * nf, m)[:, nf:2 * nf]


# ---------------------------------------------------------------------------
# thresholds and counts
# ---------------------------------------------------------------------------
def test_thresholds():
    from scipy.stats import poisson

    from rphedge.ops import layout as L
    from rphedge.ops.paths import merton_counts, merton_thresholds

    assert L.JUMP_MAX == 8 and L.SIM_MERTON == 6
    z = merton_thresholds(0.0)
    assert z.dtype == np.uint32 and z.shape == (8,) and np.all(z == END)
    for lam_dt in (1 / 32, 5 / 32, 0.25, 1.0, 2.0):
        t = merton_thresholds(lam_dt).astype(np.int64)
        assert np.all(np.diff(t) >= 0) and t.max() <= END, lam_dt
        assert t[0] == math.floor(math.exp(-lam_dt) * 2.0 ** 30)
        # the Poisson CDF by another route: floor(F 2^30) up to the CDF's own rounding
        want = np.minimum(np.floor(poisson.cdf(np.arange(8), lam_dt) * 2.0 ** 30), END)
        assert np.all(np.abs(t - want) <= 1), (lam_dt, t, want)
    # lam dt = 2: the mass past the cap is 1 - F_7 = 1.1e-3, so the last threshold is well below 2^30
    t2 = merton_thresholds(2.0).astype(np.int64)
    assert t2[-1] < END and (END - t2[-1]) / END == pytest.approx(1 - poisson.cdf(7, 2.0), rel=1e-6)
    # lam dt = 1 (the config's bound): the draws that the cap truncates, N >= 9 counted as 8, have mass < 1.2e-6
    assert 1.1e-6 < poisson.sf(8, 1.0) < 1.2e-6
    assert 1 - merton_thresholds(1.0)[-1] / END == pytest.approx(poisson.sf(7, 1.0), rel=1e-3)
    # counts: an integer comparison
    t = merton_thresholds(0.25).astype(np.int64)
    u = np.array([0, t[0] - 1, t[0], t[1] - 1, t[1], END - 1])
    assert merton_counts(u, t).tolist() == [0, 0, 1, 1, 2, int((END - 1 >= t).sum())]
    assert merton_counts(np.array([0, END - 1]), z).tolist() == [0, 0]
    for bad in (-0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="lam \\* dt"):
            merton_thresholds(bad)


def test_counts_census_and_no_uniform_near_a_threshold():
    from rphedge.ops.paths import merton_counts, merton_thresholds

    near = 0
    census = {}
    for gk in GRIDS:
        g = grid(gk)
        U = np.concatenate([count_uniforms(gk, rk)[:, 1:].ravel() for rk in RANGES])   # (step 0 draws nothing)
        assert U.min() >= 0 and U.max() < END
        for jk, (lam, _, _) in JUMPS.items():
            thr = merton_thresholds(lam * g.dt).astype(np.int64)
            live = thr[thr < END]   # (a threshold of 2^30 is above every uniform: no jump, nothing to flip)
            near += int((np.abs(U[:, None] - live[None, :]) <= 2).sum())
            census[gk, jk] = np.bincount(merton_counts(U, thr), minlength=9)
    assert near == 0
    assert census["GN", "J8"][8] == 49                       # the 8-jump cap is reached (lam dt = 2)
    assert census["GB", "J5"][2] == 2186 and census["GB", "J5"][3] == 110
    assert all(c[1] > 0 for c in census.values())            # every case jumps


# ---------------------------------------------------------------------------
# the twin against the series; the series
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("jk", ["J1", "J5"])
def test_twin_against_the_series(jk):
    from rphedge import analytic
    from rphedge.ops import paths as P

    s0 = k = 100.0
    r, sig, T, n = 0.05, 0.2, 1.0, 1 << 14
    lam, mj, sj = JUMPS[jk]
    counts = []
    S, fin = P._cpu_merton(grid("GB"), n, s0, r, sig, lam, mj, sj, 0, P.SEED_W1, counts=counts)
    assert S.shape == (9, n) and np.all(S[0] == s0) and np.array_equal(S[-1], fin)   # (GB ends on a coarse date)
    assert counts[0].shape == (n, 33) and counts[0][:, 1:].sum() > 0
    pay = math.exp(-r * T) * np.maximum(fin - k, 0.0)
    mc, se = pay.mean(), pay.std(ddof=1) / math.sqrt(n)
    want = analytic.merton_price(s0, k, r, sig, T, lam, mj, sj, "CALL")
    print(f"{jk}: twin {mc:.3f} series {want:.3f} ({(mc - want) / se:+.2f} se)")
    assert abs(mc - want) < 4 * se
    assert want == pytest.approx({"J1": 12.761, "J5": 14.766}[jk], abs=5e-4)
    fse = fin.std(ddof=1) / math.sqrt(n)
    assert abs(fin.mean() - s0 * math.exp(r * T)) < 4 * fse      # the compensated drift: a martingale after discounting


def test_twin_without_jumps_is_the_gbm_twin():
    from rphedge.ops import paths as P

    g = grid("GB")
    nf = g.n_fine
    # lam = 0: the log-Euler recursion on the first n_fine dimensions of the 3 n_fine-dimensional sequence
    S, fin = P._cpu_merton(g, 300, 100.0, 0.05, 0.2, 0.0, -0.1, 0.15, 37, P.SEED_W1)
    W = P.ndtri_u30_f64(P._u30(3 * nf, P.SEED_W1, 300, 37, nf))
    y = math.log(100.0) + np.cumsum((0.05 - 0.5 * 0.2 ** 2) * g.dt + 0.2 * math.sqrt(g.dt) * W[:, 1:], axis=1)
    np.testing.assert_allclose(fin, np.exp(y[:, -1]), rtol=1e-13)
    np.testing.assert_allclose(S[1:], np.exp(y[:, g.reduction - 1::g.reduction]).T, rtol=1e-13)


def test_series_sanity():
    from rphedge import analytic
    from rphedge.utils.reports import black_scholes

    for typ in ("CALL", "PUT"):
        for (s, k, r, sig, T) in ((100.0, 100.0, 0.05, 0.2, 1.0), (90.0, 100.0, 0.08, 0.15, 0.5)):
            p, d = black_scholes(s, k, r, sig, T, typ)
            assert analytic.merton_price(s, k, r, sig, T, 0.0, -0.1, 0.15, typ) == pytest.approx(p, abs=1e-12)
            assert analytic.merton_delta(s, k, r, sig, T, 0.0, -0.1, 0.15, typ) == pytest.approx(d, abs=1e-12)
    for lam, mj, sj in JUMPS.values():
        for (s, k, r, sig, T) in ((100.0, 100.0, 0.05, 0.2, 1.0), (90.0, 100.0, 0.08, 0.15, 0.5)):
            c = analytic.merton_price(s, k, r, sig, T, lam, mj, sj, "CALL")
            p = analytic.merton_price(s, k, r, sig, T, lam, mj, sj, "PUT")
            assert c - p == pytest.approx(s - k * math.exp(-r * T), abs=1e-10)
            dc = analytic.merton_delta(s, k, r, sig, T, lam, mj, sj, "CALL")
            dp = analytic.merton_delta(s, k, r, sig, T, lam, mj, sj, "PUT")
            assert dc - dp == pytest.approx(1.0, abs=1e-10) and 0 < dc < 1
            # the delta is the price's derivative
            h = 1e-4 * s
            fd = (analytic.merton_price(s + h, k, r, sig, T, lam, mj, sj) -
                  analytic.merton_price(s - h, k, r, sig, T, lam, mj, sj)) / (2 * h)
            assert dc == pytest.approx(fd, abs=1e-6)
            assert c > black_scholes(s, k, r, sig, T)[0]     # jumps add variance
    with pytest.raises(ValueError, match="merton_price"):
        analytic.merton_price(100.0, 100.0, 0.05, 0.2, 1.0, -1.0, 0.0, 0.1)


def test_merton_delta_hedge_on_jumpless_paths_is_the_bs_hedge():
    import torch

    from rphedge import analytic
    from rphedge.ops import paths as P

    g = grid("GB")
    p = P.simulate_gbm(g, 512, 100.0, 0.05, 0.2, scheme="log", norm=100.0, device="cpu")
    B = g.bond(0.05)
    a = analytic.bs_delta_hedge(p.S, B, 1.0, 0.05, 0.2, 1.0, g.times())
    m = analytic.merton_delta_hedge(p.S, B, 1.0, 0.05, 0.2, 1.0, g.times(), 0.0, -0.1, 0.15)
    assert m["price"] == pytest.approx(a["price"], abs=1e-12) and m["pnl_std"] == pytest.approx(a["pnl_std"], rel=1e-9)
    # on paths that jump the model delta leaves more P&L than the BS hedge leaves without jumps
    q = P.simulate_merton(g, 512, 100.0, 0.05, 0.2, *JUMPS["J1"], norm=100.0, device="cpu")
    assert q.kind == "gbm" and len(q.features(0)) == 1 and q.S.dtype == torch.float32
    j = analytic.merton_delta_hedge(q.S, B, 1.0, 0.05, 0.2, 1.0, g.times(), *JUMPS["J1"])
    assert j["price"] == pytest.approx(analytic.merton_price(1.0, 1.0, 0.05, 0.2, 1.0, *JUMPS["J1"]), abs=1e-12)
    assert j["pnl_std"] > 1.5 * a["pnl_std"] and abs(j["pnl_mean"]) < 4 * j["pnl_std"] / math.sqrt(512)


def test_simulate_merton_cpu_surface():
    import torch

    from rphedge.ops import paths as P

    g = grid("GN")
    lam, mj, sj = JUMPS["J8"]
    a = P.simulate_merton(g, 300, 100.0, 0.05, 0.2, lam, mj, sj, norm=100.0, device="cpu", offset=0, index_map=(50, 1000))
    S, fin = P._cpu_merton(g, 300, 100.0, 0.05, 0.2, lam, mj, sj, 0, P.SEED_W1, (50, 1000))
    assert torch.equal(a.S, torch.from_numpy((S / 100.0).astype(np.float32)))
    assert torch.equal(a.S_final, torch.from_numpy((fin / 100.0).astype(np.float32)))
    assert a.meta["index_map"] == (50, 1000)
    # out=: the same buffers, refilled
    b = P.simulate_merton(g, 300, 100.0, 0.05, 0.2, lam, mj, sj, norm=100.0, device="cpu", offset=64, out=a)
    assert b is a and not torch.equal(a.S_final, torch.from_numpy((fin / 100.0).astype(np.float32)))
    with pytest.raises(ValueError, match="jump_std"):
        P.simulate_merton(g, 8, 100.0, 0.05, 0.2, 1.0, 0.0, -0.1, device="cpu")
    with pytest.raises(ValueError, match="jump_intensity"):
        P.simulate_merton(g, 8, 100.0, 0.05, 0.2, -1.0, 0.0, 0.1, device="cpu")


# ---------------------------------------------------------------------------
# config and runs (torch backend)
# ---------------------------------------------------------------------------
def params(**kw):
    p = dict(Y=100.0, K=100.0, T=1.0, mu=0.05, r=0.05, sigma=0.2, rebalancing=1 / 6, N=1, P=1.0, x=0.0, l0=0.0,
             c=0.0, ita=0.0, dt=0.05, n_paths=9, payoff="call", option_type="CALL", model="merton",
             jump_intensity=1.0, jump_mean=-0.1, jump_std=0.15, mortality=False, q99=False, device="cpu",
             backend="torch", verbose=False, optimizer="lm", lm_passes_first=12, lm_passes_rest=2,
             early_stopping=False, batch_size=512)
    p.update(kw)
    return p


def test_config_parsing_and_rejections():
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    cfg = parse_params(params())
    assert (cfg.model, cfg.jump_intensity, cfg.jump_mean, cfg.jump_std) == ("merton", 1.0, -0.1, 0.15)
    d = cfg.to_dict()
    assert d["jump_intensity"] == 1.0 and d["jump_std"] == 0.15
    run = HedgeRun(cfg)
    assert run.kind == "european" and (run.spec.nin, run.spec.nout) == (1, 2)
    HedgeRun(parse_params(params(option_type="PUT", payoff="put")))
    HedgeRun(parse_params(params(jump_intensity=0.0)))            # no jumps: still the Merton scan
    HedgeRun(parse_params(params(cost_rate=1e-3, rebalance_band=0.02)))
    HedgeRun(parse_params(params(jump_intensity=20.0)))           # lam dt = 1: the bound itself
    bad = [
        (dict(jump_intensity=20.5), "jump_intensity \\* dt = 1.025 > 1"),
        (dict(jump_intensity=-1.0), "jump_intensity must be finite and >= 0"),
        (dict(jump_std=-0.1), "jump_std must be finite and >= 0"),
        (dict(jump_mean=math.nan), "jump_mean finite"),
        (dict(exercise="bermudan"), "early exercise under jumps"),
        (dict(exercise="american"), "early exercise under jumps"),
        (dict(payoff="asian_call"), "path-dependent payoff 'asian_call'"),
        (dict(payoff="lookback_put"), "path-dependent payoff 'lookback_put'"),
        (dict(parity=True), "parity=True"),
        (dict(payoff="guarantee", mortality=True), "pension or mortality liability"),
        (dict(payoff="guarantee"), "pension or mortality liability"),
        (dict(payoff="basket_call", n_assets=2), "basket, pension or mortality liability"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            HedgeRun(parse_params(params(**kw)))
    # the jump keys belong to the jump model
    with pytest.raises(ValueError, match="need model='merton'"):
        HedgeRun(parse_params(params(model="gbm_log")))
    HedgeRun(parse_params(params(model="gbm_log", jump_intensity=0.0, jump_mean=0.0, jump_std=0.0)))


@pytest.fixture(scope="module")
def merton_run():
    from rphedge.api import european_option

    return european_option(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, N_paths=512, dt=0.05,
                           rebalancing_frequency=1 / 6, model="merton", jump_intensity=1.0, jump_mean=-0.1,
                           jump_std=0.15, device="cpu", backend="torch", verbose=False, optimizer="lm",
                           lm_passes_first=12, lm_passes_rest=2, early_stopping=False, batch_size=512)


def test_merton_run_end_to_end(merton_run):
    from rphedge import analytic

    res = merton_run
    s = res.summary
    assert s["n_paths"] == 512 and res.config["model"] == "merton"
    sf = res.self_financing_pnl
    assert all(np.isfinite(sf[k]) for k in ("mean", "std", "min", "max")) and sf["std"] > 0
    assert np.isfinite(res.v0) and res.v0 > 0
    assert s["analytic_price"] == pytest.approx(analytic.merton_price(100.0, 100.0, 0.05, 0.2, 1.0, 1.0, -0.1, 0.15))
    assert s["analytic_price"] == pytest.approx(12.761, abs=5e-4)
    assert 0 < s["analytic_delta"] < 1 and "bs_price" not in s
    assert np.isfinite(s["merton_delta_pnl_std"]) and s["merton_delta_pnl_std"] > 0
    # the paths jump: the largest one-date log return is far outside the diffusion's
    S = res.paths.S.double()
    lr = (S[1:] / S[:-1]).log().abs().max()
    assert float(lr) > 6 * 0.2 * math.sqrt(res.paths.grid.dt_coarse)


def test_merton_run_out_of_sample_and_stress(merton_run):
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(params()))
    run.run()
    o = run.out_of_sample()
    assert o.route == "materialised" and np.isfinite(o.std) and o.std > 0
    calm = run.out_of_sample(stress={"jump_intensity": 0.0})
    wild = run.out_of_sample(stress={"jump_intensity": 5.0, "jump_std": 0.3})
    assert calm.std < o.std < wild.std
    with pytest.raises(ValueError, match="jump_intensity \\* dt"):
        run.out_of_sample(stress={"jump_intensity": 25.0})
    with pytest.raises(ValueError, match="unknown out-of-sample stress key 'kappa'"):
        run.out_of_sample(stress={"kappa": 1.0})


def test_jump_stress_of_a_gbm_log_hedge():
    import torch

    from rphedge import oos
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    assert oos.stress_keys("gbm_log") == ("sigma", "mu", "r", "jump_intensity", "jump_mean", "jump_std")
    assert oos.stress_keys("merton") == oos.stress_keys("gbm_log")
    assert oos.stress_keys("gbm") == ("sigma", "mu", "r") and oos.stress_keys("heston") == oos.HESTON_STRESS
    assert oos.parse_stress("jump_intensity=1,jump_mean=-0.1,jump_std=0.15") == {
        "jump_intensity": 1.0, "jump_mean": -0.1, "jump_std": 0.15}
    run = HedgeRun(parse_params(params(model="gbm_log", jump_intensity=0.0, jump_mean=0.0, jump_std=0.0, n_paths=10,
                                       batch_size=1024)))
    run.run()
    j1 = dict(jump_intensity=1.0, jump_mean=-0.1, jump_std=0.15)
    base = run.out_of_sample(keep_pnl=True, keep_paths=True)
    hit = run.out_of_sample(stress=j1, keep_pnl=True, keep_paths=True)
    assert hit.route == base.route == "materialised" and hit.stress == j1
    assert hit.std > base.std and hit.min < base.min
    # the nets, the strike, the bond grid and V0 stay the run's: only the paths changed
    assert np.array_equal(hit.paths.bond, run.paths.bond) and torch.equal(hit.paths.S[0], run.paths.S[0])
    assert hit.in_sample == base.in_sample
    # jump sizes without an intensity: no jump, but the Merton scan's 3 n_fine-dimensional sequence is not drawn
    none = run.out_of_sample(stress=dict(jump_mean=-0.1, jump_std=0.15), keep_pnl=True)
    assert torch.equal(none.pnl, base.pnl)
    # the arithmetic scheme has no jump scan
    arith = HedgeRun(parse_params(params(model="gbm", jump_intensity=0.0, jump_mean=0.0, jump_std=0.0)))
    with pytest.raises(ValueError, match="unknown out-of-sample stress key 'jump_intensity' for model 'gbm'"):
        arith._sim_params(j1)
    with pytest.raises(ValueError, match="jump_std must be finite and >= 0"):
        run.out_of_sample(stress=dict(jump_intensity=1.0, jump_std=-0.2))
    # the jump scan has no path statistic, and there is no early exercise under jumps
    plain = dict(model="gbm_log", jump_intensity=0.0, jump_mean=0.0, jump_std=0.0)
    for kw in (dict(payoff="asian_call"), dict(exercise="bermudan", payoff="put", option_type="PUT")):
        other = HedgeRun(parse_params(params(**dict(plain, **kw))))
        with pytest.raises(ValueError, match="jump_intensity > 0 needs a European call \\| put"):
            other._sim_params(j1)
        other._sim_params(dict(jump_mean=-0.1))      # (no intensity: no jump)
