"""Out-of-sample test of a trained hedge (HedgeRun.out_of_sample) on the torch
backend: the materialised route (fresh Paths -> payoff -> backend.pnl).

The run is tiny: 2^10 paths, T = 1, dt = 1/20, rebalancing 1/6 - 21 fine
points, 7 coarse points (fine 0, 3 .. 18), so the last coarse point is NOT the
last fine point and the payoff comes from the fine-grid end.

With the training seed and window the test paths ARE the training paths: the
snapshots, the standardisation, the recursion and the scalar V0 (date-0 inputs
are the same on every path) are the in-sample ones, so every statistic is
reproduced exactly.
"""
import json
import os

import numpy as np
import pytest
import torch

U = 2.0 ** -24  # the project's u (tests/test_gpu_eval.py)


def params(**kw):
    p = dict(Y=100.0, K=100.0, T=1.0, mu=0.08, r=0.08, sigma=0.15, rebalancing=1 / 6, N=1, P=1.0, x=0.0, l0=0.0,
             c=0.0, ita=0.0, dt=0.05, n_paths=10, payoff="call", option_type="CALL", model="gbm_log",
             mortality=False, q99=False, device="cpu", backend="torch", verbose=False, optimizer="lm",
             lm_passes_first=12, lm_passes_rest=2, early_stopping=False, batch_size=1024)
    p.update(kw)
    return p


@pytest.fixture(scope="module")
def trained():
    """(run, result) of the tiny call, trained once for the whole module."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(params()))
    assert (run.grid.n_fine, run.grid.reduction, run.grid.n_coarse) == (21, 3, 7)
    res = run.run()
    return run, res


def test_training_seed_and_window_reproduce_the_in_sample_pnl_exactly(trained):
    from rphedge.ops.paths import SEED_W1

    run, res = trained
    o = run.out_of_sample(seed=SEED_W1, offset=0, paths_log2=10)
    sf = res.self_financing_pnl
    assert o.route == "materialised" and o.n_paths == 1024
    for k in ("mean", "std", "min", "max", "mean_terminal_wealth"):
        assert getattr(o, k) == sf[k], k
        assert o.in_sample[k] == sf[k], k
    assert o.std_ratio == 1.0
    # values[0] is constant across the paths: the scalar V0 is every path's own
    v = res.induction.values[0]
    assert bool((v == v[0]).all())


def test_default_seed_gives_fresh_paths(trained):
    from rphedge import oos
    from rphedge.ops.paths import SEED_W1, SEED_W2

    run, res = trained
    assert set(oos.table_seeds(oos.OOS_SEED)).isdisjoint({SEED_W1, SEED_W2})
    assert oos.table_seeds(SEED_W1) == (SEED_W1, SEED_W2)
    o = run.out_of_sample(keep_paths=True, keep_pnl=True)
    assert o.seed == oos.OOS_SEED and o.offset == 0 and o.stress is None
    assert o.n_paths == run.n_total == 1024 and o.pnl.numel() == 1024
    assert not torch.equal(o.paths.S, run.paths.S)
    assert torch.equal(o.paths.S[0], run.paths.S[0])   # (S_0 is S_0)
    for k in ("mean", "std", "min", "max", "mean_terminal_wealth", "std_ratio"):
        assert np.isfinite(getattr(o, k)), k
    assert o.std_ratio == pytest.approx(o.std / res.self_financing_pnl["std"])
    assert o.std != res.self_financing_pnl["std"]
    assert o.quantiles["q"] == [0.01, 0.015, 0.02, 0.05]
    want = np.quantile(o.pnl.double().numpy(), o.quantiles["q"]) * run.scale
    np.testing.assert_allclose(o.quantiles["values"], want, rtol=1e-6)
    # another window of the same stream is another path set
    o2 = run.out_of_sample(offset=1024 + 7)
    assert o2.offset == 1031 and o2.std != o.std


def test_stress_changes_the_simulation_only(trained):
    run, res = trained
    before = dict(res.self_financing_pnl)
    base = run.out_of_sample(keep_pnl=True)
    same = run.out_of_sample(stress={"sigma": run.cfg.sigma}, keep_pnl=True)
    assert same.stress == {"sigma": run.cfg.sigma}
    assert torch.equal(same.pnl, base.pnl)                      # bitwise
    assert np.array_equal(same.stats, base.stats)
    hi = run.out_of_sample(stress={"sigma": 1.2 * run.cfg.sigma}, keep_paths=True)
    assert hi.std != base.std and hi.std > 0
    # only the simulation: the bond grid and the date-0 price are the run's
    assert np.array_equal(hi.paths.bond, run.paths.bond) and torch.equal(hi.paths.S[0], run.paths.S[0])
    drift = run.out_of_sample(stress={"r": 0.02})
    assert drift.mean != base.mean
    assert run.out_of_sample(stress={"mu": 0.02}).stats[2] == drift.stats[2]   # (mu / r: the one drift)
    # the in-sample record is untouched
    assert run.collect().self_financing_pnl == before
    assert run.out_of_sample().in_sample == base.in_sample
    with pytest.raises(ValueError, match="unknown out-of-sample stress key 'kappa'"):
        run.out_of_sample(stress={"kappa": 1.0})
    with pytest.raises(ValueError, match="unknown out-of-sample stress key 'vol'"):
        run.out_of_sample(stress={"vol": 0.3})


def test_chunked_run_sums_to_the_unchunked_one(trained, monkeypatch):
    from rphedge import oos
    from rphedge.ops import layout as L
    from rphedge.ops import paths as P

    run, _ = trained
    one = run.out_of_sample(keep_pnl=True, keep_paths=True)
    monkeypatch.setattr(oos, "OOS_CHUNK_LOG2", 8)
    four = run.out_of_sample(keep_pnl=True, keep_paths=True)
    assert one.chunks == 1 and four.chunks == 4 and len(four.paths) == 4
    assert four.stats[L.ES_COUNT] == one.stats[L.ES_COUNT] == 1024
    assert torch.equal(four.pnl, one.pnl)    # the same paths, the same arithmetic per path
    assert torch.equal(torch.cat([p.S for p in four.paths], dim=1), one.paths.S)
    pnl = one.pnl.double().numpy()
    payoff = P.payoff("call", one.paths, run.cfg.K / run.cfg.Y).double().numpy()
    W = pnl + payoff
    terms = {L.ES_RES: np.abs(pnl), L.ES_RES2: pnl * pnl, L.ES_ABSRES: np.abs(pnl), L.ES_V: np.abs(W),
             L.ES_V2: W * W}
    for idx, t in terms.items():
        err, tol = abs(four.stats[idx] - one.stats[idx]), 8 * U * float(t.sum())
        print(f"stat {idx}: chunked - unchunked = {err:.3e} (tol {tol:.3e})")
        assert err <= tol, idx
    assert four.stats[L.ES_RESMIN] == one.stats[L.ES_RESMIN] and four.stats[L.ES_RESMAX] == one.stats[L.ES_RESMAX]


def test_errors(trained):
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params
    from rphedge.oos import SOBOL_RANGE_MSG

    run, _ = trained
    fresh = HedgeRun(parse_params(params()))
    with pytest.raises(RuntimeError, match="needs a finished run"):
        fresh.out_of_sample()
    fresh.build()   # (simulated and built, not run)
    with pytest.raises(RuntimeError, match="needs a finished run"):
        fresh.out_of_sample()
    for kw in (dict(offset=(1 << 30) - 1023), dict(offset=1 << 30), dict(offset=-1), dict(paths_log2=31)):
        with pytest.raises(ValueError) as e:
            run.out_of_sample(**kw)
        assert SOBOL_RANGE_MSG in str(e.value), kw
    run.out_of_sample(offset=(1 << 30) - 1024)   # the last window that fits
    with pytest.raises(ValueError, match=r"fused=True.*'torch' backend"):
        run.out_of_sample(fused=True)
    assert run.out_of_sample(fused=False).route == run.out_of_sample(fused=None).route == "materialised"


def test_fused_is_refused_for_a_basket():
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    run = HedgeRun(parse_params(params(payoff="basket_call", model="basket", n_assets=2, n_paths=9, optimizer="adam",
                                       batch_size=512, epochs_first=2, epochs_rest=1, lr_schedule_first=False)))
    run.run()
    with pytest.raises(ValueError, match="fused=True.*basket liability"):
        run.out_of_sample(fused=True)
    o = run.out_of_sample()
    assert o.route == "materialised" and np.isfinite(o.std) and o.n_paths == 512


def test_config_keys_fill_the_result(capsys):
    from rphedge.__main__ import main
    from rphedge.api import european_option

    kw = {k: v for k, v in params().items() if k not in ("Y", "K", "T", "mu", "r", "sigma", "rebalancing", "dt",
                                                           "n_paths", "payoff", "option_type", "model", "N", "P",
                                                           "x", "l0", "c", "ita", "mortality", "q99")}
    off = european_option(N_paths=1024, dt=0.05, rebalancing_frequency=1 / 6, **kw)
    assert off.out_of_sample is None
    res = european_option(N_paths=1024, dt=0.05, rebalancing_frequency=1 / 6, oos_paths_log2=10, oos_seed=77,
                          oos_stress={"sigma": 0.2}, **kw)
    o = res.out_of_sample
    assert o.n_paths == 1024 and o.seed == 77 and o.stress == {"sigma": 0.2} and o.route == "materialised"
    assert o.in_sample["std"] == res.self_financing_pnl["std"] == off.self_financing_pnl["std"]
    assert res.summary["out_of_sample_pnl_std"] == o.std
    assert res.config["oos_paths_log2"] == 10
    sets = ["dt=0.05", "device=cpu", "backend=torch", "verbose=false", "optimizer=lm", "lm_passes_first=12",
            "lm_passes_rest=2", "early_stopping=false", "batch_size=1024"]
    assert main(["european", "--paths", "1024", "--rebalancing", str(1 / 6), "--oos-paths-log2", "10", "--oos-seed",
                 "77", "--oos-stress", "sigma=0.2", "--set", *sets]) == 0
    out = json.loads(capsys.readouterr().out)["out_of_sample"]
    assert out["n_paths"] == 1024 and out["seed"] == 77 and out["stress"] == {"sigma": 0.2}
    assert out["std"] == o.std and out["std_ratio"] == o.std_ratio
    # --set carries the same keys (a JSON config does too: examples/euro_call_30_oos.json)
    assert main(["european", "--paths", "1024", "--rebalancing", str(1 / 6), "--set", *sets, "oos_paths_log2=10",
                 "oos_seed=77", "oos_stress=sigma=0.2"]) == 0
    assert json.loads(capsys.readouterr().out)["out_of_sample"]["std"] == o.std
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = json.load(open(os.path.join(root, "examples", "euro_call_30_oos.json")))
    ref = json.load(open(os.path.join(root, "examples", "euro_call_30_lm.json")))
    assert {k: v for k, v in cfg.items() if not k.startswith("oos_")} == ref and cfg["oos_paths_log2"] == 22


def test_bermudan_put_reports_the_exercise_out_of_sample():
    from rphedge.api import european_option

    res = european_option(N_paths=2048, dt=0.03125, rebalancing_frequency=0.125, OPTION_TYPE="PUT",
                          exercise="bermudan", exercise_every=2, device="cpu", backend="torch", verbose=False,
                          optimizer="lm", lm_passes_first=20, lm_passes_rest=2, early_stopping=False,
                          oos_paths_log2=11)
    o = res.out_of_sample
    assert 0.0 < o.exercise_share < 1.0 and o.policy_value > 0 and 0.0 < o.mean_exercise_date <= 1.0
    assert res.exercise_share is not None and o.exercise_share != res.exercise_share   # (other paths)
    assert res.out_of_sample.as_dict()["exercise_share"] == o.exercise_share


# ---------------------------------------------------------------------------
# two gloo ranks against one process on the same window
# ---------------------------------------------------------------------------
def _dp_worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params
    from rphedge.parallel import dist as D

    di = D.init(device="cpu")
    # the networks of the one-process run: both ranks hedge with the same snapshots
    run = HedgeRun(parse_params(params()), dist_info=di)
    run.run()
    ref = torch.load(out + ".snap.pt")
    run.induction.snap.copy_(ref["snap"])
    run.induction.pnl_data.fmu.copy_(ref["fmu"])
    run.induction.pnl_data.fisd.copy_(ref["fisd"])
    run.induction.stats[0][1].copy_(ref["stats0"] / world)   # (the date-0 statistics: V0 = sum / count)
    o = run.out_of_sample(paths_log2=11, offset=333, keep_pnl=True)
    if rank == 0:
        with open(out, "w") as f:
            json.dump({"stats": o.stats.tolist(), "n": o.n_paths, "q": o.quantiles["values"]}, f)
    D.shutdown()


def test_two_ranks_match_one_process(trained, tmp_path):
    import torch.multiprocessing as mp

    from test_distributed_cpu import _free_port
    from rphedge.ops import layout as L

    run, _ = trained
    ind = run.induction
    world, port, out = 2, _free_port(), str(tmp_path / "dp.json")
    torch.save({"snap": ind.snap, "fmu": ind.pnl_data.fmu, "fisd": ind.pnl_data.fisd, "stats0": ind.stats[0][1]},
               out + ".snap.pt")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    dp = json.load(open(out))
    one = run.out_of_sample(paths_log2=11, offset=333, keep_pnl=True)
    st = np.asarray(dp["stats"])
    assert dp["n"] == one.n_paths == 2048 and st[L.ES_COUNT] == one.stats[L.ES_COUNT] == 2048
    # the same per-path values summed in another order, in fp64
    for idx in (L.ES_V, L.ES_V2, L.ES_RES, L.ES_RES2, L.ES_ABSRES):
        tol = 2048 * 2.0 ** -52 * max(abs(one.stats[L.ES_ABSRES]), abs(one.stats[idx]))
        assert abs(st[idx] - one.stats[idx]) <= tol, (idx, st[idx], one.stats[idx])
    assert st[L.ES_RESMIN] == one.stats[L.ES_RESMIN] and st[L.ES_RESMAX] == one.stats[L.ES_RESMAX]
    np.testing.assert_allclose(dp["q"], one.quantiles["values"], rtol=1e-6)


# ---------------------------------------------------------------------------
# after resume(), and the descriptor's layout check
# ---------------------------------------------------------------------------
def test_out_of_sample_after_resume(trained, tmp_path):
    """A resumed run fitted only the dates below its restart date: the later
    dates' networks come from the run directory (raw-input weights re-expressed
    for the standardisation), so the hedge is the whole run's again."""
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params
    from rphedge.utils.model_io import save_run

    run, res = trained
    save_run(str(tmp_path), run, res)
    again = HedgeRun(parse_params(params()))
    again.resume(str(tmp_path), 3)
    assert not again.induction.pnl_done
    assert float(again.induction.snap[3:].abs().sum()) == 0.0   # (not fitted in this process)
    o, ref = again.out_of_sample(), run.out_of_sample()
    assert o.in_sample is None and o.std_ratio is None and o.n_paths == 1024
    # the saved weights are fp32 of the folded networks: the hedge agrees to a few 1e-5, not bit for bit
    assert o.std == pytest.approx(ref.std, rel=2e-3) and o.mean == pytest.approx(ref.mean, abs=2e-3 * ref.std)
    assert float(again.induction.snap[3:].abs().sum()) == 0.0   # (the run's own snapshots are untouched)


def test_oos_descriptor_is_checked_by_name():
    import ctypes

    from rphedge.ops import native

    lib = native.load(required=True)   # (the layout tables need no GPU)
    fields, consts = native.native_layout(lib)
    ext = native.native_layout_ext(lib)
    assert [c.__name__ for c in native.DESCRIPTORS_EXT] == ["OosDesc"]
    assert {t for t, *_ in ext} == {"OosDesc"} and len(ext) == len(native.OosDesc._fields_)
    assert ctypes.sizeof(native.OosDesc) == ctypes.sizeof(native.SimDesc) + 104
    every = native.DESCRIPTORS + native.DESCRIPTORS_EXT
    assert native.layout_mismatches(fields + ext, consts, classes=every) == []
    # a wrong mirror is named: two fields swapped, one dropped
    f = list(native.OosDesc._fields_)
    i, j = [x[0] for x in f].index("wealth0"), [x[0] for x in f].index("strike")
    f[i], f[j] = f[j], f[i]
    swapped = type("OosDesc", (ctypes.Structure,), {"_fields_": f})
    bad = native.layout_mismatches(fields + ext, consts, classes=native.DESCRIPTORS + (swapped,))
    assert sorted(line.split(":")[0] for line in bad) == ["OosDesc.strike", "OosDesc.wealth0"]
    dropped = type("OosDesc", (ctypes.Structure,), {"_fields_": [x for x in native.OosDesc._fields_
                                                                 if x[0] != "payoff_out"]})
    bad = native.layout_mismatches(fields + ext, consts, classes=native.DESCRIPTORS + (dropped,))
    assert any(line.startswith("OosDesc.payoff_out: ") and "not in ctypes" in line for line in bad)
    # the host checks run without a device
    with pytest.raises(RuntimeError, match="null snapshot or statistics pointer"):
        native.oos_check(native.OosDesc())
