"""The eval ride end to end (driver.BackwardInduction.enqueue, TrainingParams.
eval_ride): 8 dates on 2^14 paths with the euro30 and the Heston bench
configurations at that size, the route on against the route off, eager and as
a captured graph.  Values, weights, date statistics, P&L statistics and
V0 / phi0 / psi0 are equal BYTE FOR BYTE, and the graph has dates - 1 fewer
nodes (every later date's eval rides in the next fit's first solve launch)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DATES = 8
COMMON = dict(Y=100, K=100, T=1.0, N=1, P=1, x=0, l0=0, c=0, ita=0, rebalancing=1.0 / DATES, n_paths=14,
              payoff="call", option_type="CALL", mortality=False, q99=False, batch_size=1 << 14, chunk_log2=6,
              early_stopping=False, verbose=False, seed=1234, optimizer="lm", lm_passes_rest=1, lm_lam_carry=3.0,
              lm_out_fix=True, feature_norm="horizon", feature_norm_floor=0.1, lm_lam0_first=16.384000778198242,
              lm_starts=4, lm_explore_passes=10, lm_explore_log2=12, keep_paths=True)
CONFIGS = {
    # bench.py PRESETS["euro30"] / ["heston30"] with 8 dates, 2^14 paths and a shorter first date
    "euro": dict(COMMON, model="gbm_log", mu=0.08, r=0.08, sigma=0.15, dt=1.0 / DATES, lm_passes_first=25,
                 init="spread"),
    "heston": dict(COMMON, model="heston", mu=0.05, r=0.05, sigma=0.2, kappa=2.0, theta=0.04, xi=0.5, rho=-0.7,
                   v0=0.04, dt=1.0 / (DATES * 10), lm_passes_first=35),
}


def _outputs(run, res):
    from rphedge.engine import reduce_stats

    ind = run.induction
    torch.cuda.synchronize()
    out = dict(values=ind.values.cpu().numpy().tobytes(), weights=ind.snap.cpu().numpy().tobytes(),
               holdings=ind.holdings.cpu().numpy().tobytes(), residuals=ind.residuals.cpu().numpy().tobytes(),
               pnl_paths=ind.pnl_paths.cpu().numpy().tobytes(), pnl_stats=ind.pnl_stats.cpu().numpy().tobytes(),
               date_stats=b"".join(np.asarray(reduce_stats(s[1]), np.float64).tobytes() for s in ind.stats),
               slabs=b"".join(s[1].cpu().numpy().tobytes() for s in ind.stats),
               fits=b"".join(f[0].cpu().numpy().tobytes() for f in ind.fits),
               v0=np.float64(res.v0).tobytes(), hold0=np.asarray(res.induction.holdings0, np.float64).tobytes())
    assert np.isfinite(np.frombuffer(out["values"], np.float32)).all()
    return out


def _run(name, ride, dev):
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(dict(CONFIGS[name], eval_ride=ride, device=str(dev))))
    try:
        res = run.run()
        rides = run.induction.eval_rides
        eager = _outputs(run, res)
        run.capture(include_simulation=True)
        run.replay()
        run.replay()
        graph = _outputs(run, run.collect())
        return eager, graph, int(run.graph.num_nodes), rides, run.induction.n_dates
    finally:
        run.close()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_route_on_is_bytewise_route_off(name):
    dev = torch.device("cuda", 0)
    e_off, g_off, nodes_off, rides_off, nd = _run(name, False, dev)
    e_on, g_on, nodes_on, rides_on, _ = _run(name, True, dev)
    assert nd == DATES and rides_off == 0 and rides_on == DATES - 1
    for k in e_off:
        assert e_off[k] == e_on[k], ("eager", k)
        assert g_off[k] == g_on[k], ("graph", k)
        assert e_on[k] == g_on[k], ("eager vs graph", k)
    assert nodes_on == nodes_off - (DATES - 1)
