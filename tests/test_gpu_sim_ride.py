"""The sim ride on the GPU (SimRideDesc, k_lm_solve_sim, TrainingParams.sim_ride).

Every comparison is BYTE FOR BYTE, and every buffer a split simulation writes
is NaN-filled first, so a block nobody simulated shows.

* a scan cut into a head launch and a remainder launch (the WIDE step code:
  sobol_point_wide one step ahead, a counter for the coarse dates), each block
  followed by its payoff epilogue, against the plain scan (the per-bit Sobol
  fold) + k_payoff: every stored float of every date, the fine terminal values
  and the payoff (both destinations), with the upper Gray bits set and clear;
* a 6-date run whose first date explores, captured and replayed twice, with
  the ride (a few riders, the backend's own count, explorations too short to
  carry every block) and without: paths, payoff, values, exploration states,
  selection block, fitted networks, statistics and V0."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ---------------------------------------------------------------------------
# scan cut + payoff epilogue
# ---------------------------------------------------------------------------
def _simulate(model, grid, n, offset, dev, defer=None, index_map=None):
    from rphedge.ops import paths as P

    kw = dict(device=dev, offset=offset, defer=defer, index_map=index_map)
    if model in ("log", "arith"):
        return P.simulate_gbm(grid, n, 100.0, 0.08, 0.15, scheme=model, norm=100.0, **kw)
    return P.simulate_sv(grid, n, 100.0, 0.05, 0.04, model="heston", kappa=2.0, theta=0.04, xi=0.5, rho=-0.7,
                         norm=100.0, scheme=model.split("_")[1], **kw)


def _buffers(p):
    return [t for t in (p.S, p.S_final, p.vol, p.stat, p.stat_final) if t is not None]


# (the scans a run can split: the ones with a rider - GBM arithmetic / log and both Heston schemes)
PAYOFFS = {"log": "call", "arith": "put", "heston_qe": "call", "heston_euler": "put"}


@pytest.mark.parametrize("fine", [1, 4])
@pytest.mark.parametrize("offset", [0, (1 << 20) + 64])
@pytest.mark.parametrize("n", [1 << 12, (1 << 12) + 256])
@pytest.mark.parametrize("model", list(PAYOFFS))
def test_cut_scan_with_payoff_is_the_plain_scan_and_payoff(model, n, offset, fine):
    from rphedge.ops import native
    from rphedge.ops import paths as P

    dev = torch.device("cuda", 0)
    grid = P.Grid(1.0, 1.0 / (30 * fine), 1.0 / 30)
    ref = _simulate(model, grid, n, offset, dev)
    name, strike = PAYOFFS[model], 1.02
    v_ref = P.payoff(name, ref, strike)
    defer = []
    cut = _simulate(model, grid, n, offset, dev, defer=defer)
    for t in _buffers(cut):
        t.fill_(NAN)
    v, v2 = (torch.full((n,), NAN, device=dev) for _ in range(2))
    r = native.SimRideDesc()
    r.sim = defer[0]
    r.pay_out, r.pay_out2, r.strike = v.data_ptr(), v2.data_ptr(), strike
    r.pay_kind = {"call": 1, "put": 2}[name]
    r.b0, r.b1, r.per_rider = 3, n // 256, 1
    native.sim_ride_head(r, None)
    torch.cuda.synchronize()
    # the head wrote its blocks and nothing else
    assert torch.isnan(cut.S[:, 3 * 256:]).all() and torch.isnan(v[3 * 256:]).all()
    assert torch.equal(cut.S[:, :3 * 256], ref.S[:, :3 * 256]) and torch.equal(v[:3 * 256], v_ref[:3 * 256])
    native.sim_ride_rest(r, 5)
    torch.cuda.synchronize()
    assert torch.isnan(cut.S[:, 3 * 256:5 * 256]).all() and torch.isnan(v2[3 * 256:5 * 256]).all()
    native.sim_ride_rest(r)
    torch.cuda.synchronize()
    for a, b in zip(_buffers(cut), _buffers(ref)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert v.cpu().numpy().tobytes() == v_ref.cpu().numpy().tobytes() == v2.cpu().numpy().tobytes()


def test_head_carries_the_gram_subsample_like_the_pair_launch():
    from rphedge.ops import native
    from rphedge.ops import paths as P

    dev = torch.device("cuda", 0)
    grid, n = P.Grid(1.0, 1.0 / 30, 1.0 / 30), 1 << 13
    ra, rb = [], []
    a = _simulate("log", grid, n, 0, dev, defer=ra)
    b = _simulate("log", grid, 512, 0, dev, defer=rb, index_map=(64, 1024))
    assert native.simulate_pair(ra[0], rb[0])
    v_ref = P.payoff("call", a, 1.0)
    torch.cuda.synchronize()
    want = [t.clone() for t in _buffers(a) + _buffers(b)]
    for t in _buffers(a) + _buffers(b):
        t.fill_(NAN)
    v = torch.full((n,), NAN, device=dev)
    r = native.SimRideDesc()
    r.sim = ra[0]
    r.pay_out, r.pay_out2, r.strike, r.pay_kind, r.b0, r.b1, r.per_rider = v.data_ptr(), None, 1.0, 1, 4, n // 256, 1
    native.sim_ride_head(r, rb[0])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_buffers(b), want[len(_buffers(a)):]))  # the whole subsample
    assert torch.isnan(a.S[:, 1024:]).all()
    native.sim_ride_rest(r)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_buffers(a), want)) and torch.equal(v, v_ref)
    # descriptors the launchers refuse: nothing reaches the GPU
    from rphedge.ops import layout as L

    for field, val, msg in [("b1", n // 256 + 1, "block range"), ("b0", -1, "block range"), ("per_rider", 0, "per rider"),
                            ("pay_kind", 3, "payoff kinds"), ("pay_kind", 4, "payoff kinds"), ("pay_out", None, "null")]:
        bad = type(r).from_buffer_copy(r)
        setattr(bad, field, val)
        with pytest.raises(RuntimeError, match=msg):
            native.sim_ride_rest(bad)
    for field, val in [("model", L.SIM_SV_REF), ("path_stat", L.STAT_MEAN)]:  # (scans without a rider)
        bad = type(r).from_buffer_copy(r)
        setattr(bad.sim, field, val)
        with pytest.raises(RuntimeError, match="path statistic"):
            native.sim_ride_rest(bad)


# ---------------------------------------------------------------------------
# the ride, end to end
# ---------------------------------------------------------------------------
DATES = 6
EURO = dict(Y=100, K=100, T=1.0, N=1, P=1, x=0, l0=0, c=0, ita=0, rebalancing=1.0 / DATES, n_paths=13,
            payoff="call", option_type="CALL", mortality=False, q99=False, batch_size=1 << 13, chunk_log2=6,
            early_stopping=False, verbose=False, seed=1234, optimizer="lm", lm_passes_rest=1, lm_lam_carry=3.0,
            lm_out_fix=True, feature_norm="horizon", feature_norm_floor=0.1, lm_lam0_first=16.384000778198242,
            lm_explore_log2=10, keep_paths=False, model="gbm_log", mu=0.08, r=0.08, sigma=0.15, dt=1.0 / DATES,
            lm_passes_first=12, init="spread")
HESTON = dict({k: v for k, v in EURO.items() if k != "init"}, model="heston", mu=0.05, r=0.05, sigma=0.2, kappa=2.0,
              theta=0.04, xi=0.5, rho=-0.7, v0=0.04, dt=1.0 / (DATES * 10))
BLOCKS = (1 << 13) // 256 - (1 << 10) // 256  # blocks the head launch leaves


def _outputs(run):
    from rphedge.engine import reduce_stats

    res = run.collect()
    ind, x = run.induction, run.backend.lm_explore_last
    out = dict(values=ind.values, snap=ind.snap, v_terminal=run.v_terminal, pnl_stats=ind.pnl_stats,
               explore_state=x["state"], sel=x["sel"], gram=run.gpaths.S,
               **{f"paths{i}": t for i, t in enumerate(_buffers(run.paths))})
    out = {k: v.cpu().numpy().tobytes() for k, v in out.items()}
    out["date_stats"] = b"".join(np.asarray(reduce_stats(s[1]), np.float64).tobytes() for s in ind.stats)
    out["v0"] = np.float64(res.v0).tobytes()
    out["pnl_std"] = np.float64(res.terminal_pnl["std"]).tobytes()
    assert np.isfinite(np.frombuffer(out["values"], np.float32)).all()
    assert np.isfinite(np.frombuffer(out["paths0"], np.float32)).all()
    return out


def _replays(cfg, K, passes, ride, riders, monkeypatch):
    """Outputs of an eager run and of two replays of its captured graph (every buffer the simulation, the
    payoff and the induction write NaN-filled before each), and the graph's node count."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    monkeypatch.setenv("RPH_SIM_RIDE_STEPS", "100000")  # (correctness: Heston's 120-point blocks ride too)
    if riders is not None:
        monkeypatch.setenv("RPH_SIM_RIDERS", str(riders))
    else:
        monkeypatch.delenv("RPH_SIM_RIDERS", raising=False)
    run = HedgeRun(parse_params(dict(cfg, lm_starts=K, lm_explore_passes=passes, sim_ride=ride, device="cuda:0")))
    try:
        run.run()
        outs = [_outputs(run)]
        run.capture(include_simulation=True)
        for _ in range(2):
            torch.cuda.synchronize()
            for t in _buffers(run.paths) + _buffers(run.gpaths) + [run.v_terminal, run.induction.values]:
                t.fill_(NAN)
            run.replay()
            outs.append(_outputs(run))
        assert run.sim_ride is None
        return outs, int(run.graph.num_nodes)
    finally:
        run.close()


@functools.lru_cache(maxsize=None)
def _reference(name, K, passes):
    mp = pytest.MonkeyPatch()
    try:
        return _replays(dict(euro=EURO, heston=HESTON)[name], K, passes, False, None, mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("name,K,passes,riders", [("euro", 4, 1, 3), ("euro", 4, 20, 7), ("euro", 16, 20, None),
                                                  ("euro", 16, 1, None), ("heston", 4, 1, 7), ("heston", 4, 20, 3)])
def test_ride_on_is_bytewise_ride_off(name, K, passes, riders, monkeypatch):
    off, nodes_off = _reference(name, K, passes)
    on, nodes_on = _replays(dict(euro=EURO, heston=HESTON)[name], K, passes, True, riders, monkeypatch)
    for i, (a, b) in enumerate(zip(off, on)):
        for k in a:
            assert a[k] == b[k], (("eager", "replay 1", "replay 2")[i], k)
    for k in on[0]:
        assert on[0][k] == on[1][k] == on[2][k], ("eager vs replays", k)
    # the ride took place: no payoff launch and no copy into values[-1]; one plain launch for the blocks the
    # exploration's passes + 1 solves could not carry
    carried = (riders if riders is not None else 10 ** 6) * (passes + 1)
    assert nodes_on == nodes_off - 2 + (1 if carried < BLOCKS else 0), (nodes_on, nodes_off)
