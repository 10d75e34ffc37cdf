"""Out-of-sample test of a trained hedge (:meth:`rphedge.api.HedgeRun.out_of_sample`).

Every in-sample figure of a run is measured on the paths its per-date networks
were fitted on.  This module applies the finished run - the weight snapshots
of every date, the per-date input standardisation, the strike and the bond
grid - to FRESH paths: another scramble of the Sobol stream (``seed``), a
window of it (``offset``), optionally simulated under stressed model
parameters (``stress``: the model-misspecification test).  Wealth starts at the
scalar fitted V0 on every path and follows the self-financing recursion of
the in-sample P&L scan.

Two routes compute it:

* ``materialised`` (every configuration, both backends): simulate ``Paths``
  with the run's own scans, form the payoff, call ``backend.pnl``.  Chunks of
  at most ``2^22`` paths bound the memory; their statistics rows are summed.
* ``fused`` (the MI355X backend, single-asset GBM / GBM + path statistic /
  Heston / Merton with the 8-unit nets): ``k_hedge_oos`` (Merton paths, also the
  jump stress of a ``gbm_log`` run: ``k_hedge_oos_jump``) simulates, hedges and
  scores a path in registers in one launch; nothing of size ``[dates, paths]`` exists.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import risk
from .engine import Costs, PnlData, reduce_cost_stats, reduce_stats
from .ops import layout as L
from .ops import layout_cost as LC
from .ops import paths as P
from .parallel import dist as D

# Default Sobol scramble seed of the test paths.  The training paths use
# SEED_W1 = 1235 (prices) and SEED_W2 = 1234 (second table: variance /
# mortality shocks); a test seed s scrambles the two tables with (s, s - 1), so
# s = SEED_W1 reproduces the training paths and the default shares neither.
OOS_SEED = 4321
OOS_CHUNK_LOG2 = 22          # materialised route: at most 2^22 paths are simulated at a time
SOBOL_INDEX_END = 1 << 30    # csrc/sim_step.h: the Sobol tables hold 30 direction numbers per dimension
SOBOL_RANGE_MSG = "path range leaves the 30-bit Sobol index space [0, 2^30)"   # validate_sobol_range's message
QUANTILES = (0.01, 0.015, 0.02, 0.05)   # the quantiles collect() reports for the in-sample P&L

GBM_STRESS = ("sigma", "mu", "r")
HESTON_STRESS = ("v0", "kappa", "theta", "xi", "rho")
JUMP_STRESS = ("jump_intensity", "jump_mean", "jump_std")   # the log scheme only: gbm_log, merton


def stress_keys(model: str) -> tuple:
    """The simulation parameters ``stress`` may override for ``model``."""
    if model == "heston":
        return HESTON_STRESS
    if model in ("gbm_log", "merton"):
        return GBM_STRESS + JUMP_STRESS
    return GBM_STRESS if model in ("gbm", "basket") else ()


def table_seeds(seed: int) -> tuple:
    """(price table, second table) scramble seeds of test seed ``seed``."""
    seed = int(seed)
    if seed < 1:
        raise ValueError(f"out-of-sample seed must be >= 1, got {seed}")
    return seed, seed - 1


def parse_stress(s) -> dict | None:
    """``oos_stress`` of a config: a dict, or ``"key=value,key=value"`` (``--set`` / ``--oos-stress``)."""
    if s is None or s == "" or s == {}:
        return None
    if isinstance(s, dict):
        return {str(k): float(v) for k, v in s.items()}
    out = {}
    for kv in str(s).split(","):
        if "=" not in kv:
            raise ValueError(f"oos_stress entry {kv!r} is not key=value")
        k, v = kv.split("=", 1)
        out[k.strip()] = float(v)
    return out


@dataclass
class OosResult:
    """Out-of-sample P&L of a trained hedge, in the units of ``RunResult.self_financing_pnl``."""

    mean: float
    std: float
    min: float
    max: float
    mean_terminal_wealth: float
    n_paths: int                      # global test-path count
    seed: int
    offset: int
    stress: dict | None
    route: str                        # "fused" | "materialised"
    in_sample: dict | None = None     # the run's own self-financing P&L (None: a resumed run reports none)
    std_ratio: float | None = None    # std / in_sample["std"]
    pnl: torch.Tensor | None = None   # keep_pnl: this rank's per-path P&L (unscaled, like InductionResult.pnl_paths)
    quantiles: dict | None = None     # keep_pnl: {"q": [...], "values": [...]} as collect() reports in sample
    paths: object = None              # keep_paths: the simulated Paths (a list when the window took several chunks)
    # early exercise: the stopping rule of the P&L scan on the test paths
    exercise_share: float | None = None
    mean_exercise_date: float | None = None
    policy_value: float | None = None
    stats: np.ndarray | None = None   # the summed statistics row (ES_* layout)
    # the same paths under transaction costs (the keys of RunResult.costs; "in_sample": the run's own cost scan)
    costs: dict | None = None
    seconds: float = 0.0
    chunks: int = 1
    extra: dict = field(default_factory=dict)

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k in ("mean", "std", "min", "max", "mean_terminal_wealth", "n_paths", "seed",
                                             "offset", "stress", "route", "in_sample", "std_ratio", "quantiles",
                                             "exercise_share", "mean_exercise_date", "policy_value", "costs")}
        return {k: v for k, v in d.items() if v is not None or k in ("stress", "in_sample", "std_ratio")}


def validate_window(offset: int, n: int):
    """The host check of ``validate_sobol_range`` (csrc/sim_step.h) for the window ``[offset, offset + n)``."""
    first, span = int(offset), int(n) - 1
    if first < 0 or first >= SOBOL_INDEX_END or span < 0 or span >= SOBOL_INDEX_END - first:
        raise ValueError(f"out_of_sample: {SOBOL_RANGE_MSG} (offset {offset}, {n} paths)")


def fused_unsupported(run) -> str | None:
    """Why ``k_hedge_oos`` cannot take this run (None: it can)."""
    c, spec = run.cfg, run.spec
    if run.kind != "european":
        return f"a {run.kind} liability (one simulated asset: call / put or a path-dependent payoff)"
    if c.model not in ("gbm", "gbm_log", "heston", "merton"):
        return f"model {c.model!r} (gbm | gbm_log | heston | merton)"
    if run.exercise is not None:
        return "early exercise (the stopping rule runs in the materialised scan)"
    if c.dtype != "fp32":
        return f"dtype {c.dtype!r} (the kernel simulates in fp32)"
    if run.path_stat is not None and not c.path_feature:
        return "path_feature=False (the kernel feeds the statistic to the net)"
    shape = (spec.nin, spec.hidden, spec.nout, spec.head)
    two = run.path_stat is not None or c.model == "heston"
    ok = [(2, 8, 2, L.HEAD_FREE)] if two else [(1, 8, 1, L.HEAD_COMPLEMENT), (1, 8, 2, L.HEAD_FREE)]
    if shape not in ok:
        return f"network shape {shape} (fused shapes of this model: {ok})"
    if run.backend_kind != "hip":
        return f"the {run.backend_kind!r} backend (the fused kernel runs on the GPU backend)"
    return None


def _in_sample(run, scale: float) -> dict | None:
    from .driver import DateResult

    ind = run.induction
    if not getattr(ind, "pnl_done", False):
        return None
    d = DateResult(index=-1, time=0.0, stats=reduce_stats(ind.pnl_stats, run.di.world))
    return {"mean": d.residual_mean * scale, "std": d.residual_std * scale,
            "min": float(d.stats[L.ES_RESMIN]) * scale, "max": float(d.stats[L.ES_RESMAX]) * scale,
            "mean_terminal_wealth": d.mean_value * scale}


def _in_sample_costs(run, scale: float) -> dict | None:
    """The run's own scan under its configured costs (None: it ran none)."""
    from .driver import DateResult

    ind = run.induction
    if not getattr(ind, "pnl_done", False) or getattr(ind, "costs", None) is None:
        return None
    d = DateResult(index=-1, time=0.0, stats=reduce_stats(ind.cost_pnl_stats, run.di.world))
    return run.cost_report(ind.costs, d, reduce_cost_stats(ind.cost_stats, run.di.world), None, fitted_v0(run) * scale)


def _snapshots(run) -> torch.Tensor:
    """The per-date weight snapshots the hedge runs on.  A resumed run fitted
    only the dates below its restart date in this process: the networks of the
    later dates come from its run directory (raw-input weights, re-expressed
    for this run's standardisation), into a copy of the snapshot block."""
    ind = run.induction
    resumed = getattr(run, "_resumed", None)
    if resumed is None or ind.pnl_done:
        return ind.snap
    from .models import hedge_mlp as hm
    from .utils.model_io import load_date

    out_dir, date = resumed
    snap = ind.snap.clone()
    P_ = run.spec.nparams
    for t in range(int(date), ind.n_dates):
        _, _, w, wq, _ = load_date(out_dir, t)
        if ind.norms:
            mu, isd = ind.norms[t]
            w = hm.unfold_input_norm(run.spec, w, mu, isd)
            wq = hm.unfold_input_norm(run.spec, wq, mu, isd) if wq is not None else None
        snap[t].zero_()
        snap[t, 0, :P_] = torch.from_numpy(np.asarray(w, np.float32)).to(snap.device)
        snap[t, 1, :P_] = torch.from_numpy(np.asarray(wq if wq is not None else w, np.float32)).to(snap.device)
    return snap


def fitted_v0(run) -> float:
    """The scalar fitted V0 (unscaled, fp32): the mean of the date-0 values, the
    initial wealth of every test path.  The date-0 inputs are the same on every
    path, so this is the value each training path started from."""
    ind = run.induction
    s = reduce_stats(ind.stats[0][1], run.di.world)
    return float(np.float32(s[L.ES_V] / s[L.ES_COUNT]))


def payoff_code(run) -> tuple:
    """(k_payoff kind, strike) of a single-asset run's terminal payoff, as HedgeRun._payoff forms it."""
    c = run.cfg
    if run.path_stat is not None:
        return P.PATH_PAYOFFS[c.payoff][1], c.K / c.Y
    return {"call": 1, "put": 2}[c.option_type.lower()], c.K / c.Y


def _fused_scan(run, n: int, first: int, seeds: tuple, stress, trace: bool):
    """(Paths | None, SimDesc, JumpTerms | None) of the fused kernel's scan over
    ``n`` paths from global index ``first``: with ``trace`` the descriptor the
    run's own scan would launch (deferred, so its coarse tables exist and the
    kernel fills them), else the same descriptor without any output buffer.
    The jump terms: a Merton scan's (``model="merton"``, or a jump stress)."""
    c, g = run.cfg, run.grid
    if trace:
        lst = []
        p = run._simulate_paths(n, first, None, None, defer=lst, seeds=seeds, stress=stress)
        return (p,) + (tuple(lst[0]) if isinstance(lst[0], tuple) else (lst[0], None))
    sp = run._sim_params(stress)
    if sp.jumps:
        return (None,) + P.merton_desc(g, n, c.Y, sp.r, sp.sigma, sp.jump_intensity, sp.jump_mean, sp.jump_std, c.Y,
                                       run.device, first, False, seeds[0])
    if c.model == "heston":
        scheme = P.heston_scheme(c.heston_scheme, sp.kappa, sp.xi)
        return None, P.sv_desc(g, n, c.Y, sp.r, sp.v0, "heston", 0.0, 0.0, 0.0, sp.kappa, sp.theta, sp.xi, sp.rho, c.Y,
                               run.device, first, False, False, seeds[0], seeds[1], scheme, 0.0,
                               not c.parity.paired_sobol), None
    return None, P.gbm_desc(g, n, c.Y, sp.r, sp.sigma, "arith" if c.model == "gbm" else "log", c.Y, run.device,
                            first, False, seeds[0], None, run.path_stat), None


def resolve_costs(run, costs) -> Costs | None:
    """The costs of an out-of-sample test: None = the run's, False = off, a ``Costs`` or a dict of its fields."""
    if costs is None:
        k = run.costs
    elif costs is False:
        k = None
    elif isinstance(costs, Costs):
        k = costs
    elif isinstance(costs, dict):
        unknown = set(costs) - {"rate", "band", "unwind"}
        if unknown or "rate" not in costs:
            raise ValueError(f"costs dict takes rate, band, unwind (rate required), got {sorted(costs)}")
        k = Costs(**costs)
    else:
        raise ValueError(f"costs must be None, False, an engine.Costs or a dict, got {costs!r}")
    if k is not None and not k.active:
        k = None
    if k is not None and run.exercise is not None:
        raise ValueError("out_of_sample: transaction costs with early exercise are not supported")
    return k


def out_of_sample(run, paths_log2=None, seed=None, offset=0, stress=None, fused=None, keep_pnl=False,
                  keep_paths=False, chunk_log2: int | None = None, costs=None, cost_only: bool = False) -> OosResult:
    """See :meth:`rphedge.api.HedgeRun.out_of_sample`.  ``chunk_log2``: the
    materialised route's chunk (default ``OOS_CHUNK_LOG2``).  ``cost_only``:
    only the scan under ``costs`` runs (the frontier); the result's own
    figures are then the net ones."""
    costs = resolve_costs(run, costs)
    if cost_only and costs is None:
        raise ValueError("out_of_sample(cost_only=True) needs active costs")
    ind = run.induction
    if ind is None or not getattr(ind, "ran", None):
        raise RuntimeError("out_of_sample() needs a finished run: call run(), replay() or resume() first")
    if run.device.type == "cuda":
        torch.cuda.synchronize(run.device)
    c = run.cfg
    t0 = time.perf_counter()
    paths_log2 = int(c.n_paths) if paths_log2 is None else int(paths_log2)
    if paths_log2 < 0:
        raise ValueError(f"paths_log2 must be >= 0, got {paths_log2}")
    seed = OOS_SEED if seed is None else int(seed)
    seeds = table_seeds(seed)
    offset = int(offset)
    n_total = 1 << paths_log2
    validate_window(offset, n_total)
    stress = parse_stress(stress)
    run._sim_params(stress)  # (unknown keys raise before anything is simulated)
    why = fused_unsupported(run)
    if fused and why is not None:
        raise ValueError(f"out_of_sample(fused=True) is not available with {why}")
    use_fused = why is None if fused is None else bool(fused)
    world, rank = run.di.world, run.di.rank
    off_r, n_r = D.shard(n_total, world, rank)
    first = offset + off_r
    scale = run.scale
    v0 = fitted_v0(run)
    snap = _snapshots(run)
    be, dev, nd = run.backend, run.device, ind.n_dates
    has_b, hold_c, ex = bool(ind.cfg.q99), float(ind.hold_c), ind.cfg.exercise
    pnl = torch.empty(n_r, dtype=torch.float32, device=dev) if keep_pnl else None
    kept, slabs, nslabs, cslabs = [], [], [], []
    if use_fused:
        # one launch: nothing of size [dates, paths] exists unless the paths are asked for
        # (then the kernel's trace fills the buffers of a Paths object)
        p, sim, jump = _fused_scan(run, n_r, first, seeds, stress, keep_paths)
        data = PnlData(n_dates=nd, features=None, prices=None, bond=ind.pnl_data.bond, fmu=ind.pnl_data.fmu,
                       fisd=ind.pnl_data.fisd, w0=None, wealth0=v0, payoff=None)
        slab = torch.zeros(be.oos_wgs(n_r), L.EVAL_NSTAT, dtype=torch.float64, device=dev)
        kind, strike = payoff_code(run)
        if not cost_only:
            be.oos(sim, snap, data, slab, kind, strike, has_b=has_b, hold_c=hold_c, pnl_out=pnl, jump=jump)
            slabs.append(slab)
        if costs is not None:
            nslab = torch.zeros_like(slab)
            cslab = torch.zeros(slab.shape[0], LC.COST_NSTAT, dtype=torch.float64, device=dev)
            be.oos(sim, snap, data, nslab, kind, strike, has_b=has_b, hold_c=hold_c,
                   pnl_out=pnl if cost_only else None, costs=costs, cost_stats=cslab, jump=jump)
            nslabs.append(nslab)
            cslabs.append(cslab)
        if keep_paths:
            kept.append(p)
    else:
        chunk = 1 << int(OOS_CHUNK_LOG2 if chunk_log2 is None else chunk_log2)
        for k0 in range(0, n_r, chunk):
            n_c = min(chunk, n_r - k0)
            p = run._simulate_paths(n_c, first + k0, None, None, seeds=seeds, stress=stress)
            data = PnlData(n_dates=nd, features=p.features, prices=p.prices, bond=ind.pnl_data.bond,
                           fmu=ind.pnl_data.fmu, fisd=ind.pnl_data.fisd, w0=None, wealth0=v0,
                           payoff=run._payoff(p))
            slab = torch.zeros(be.pnl_wgs(n_c) if run.backend_kind == "hip" else 1, L.EVAL_NSTAT,
                               dtype=torch.float64, device=dev)
            pout = pnl[k0:k0 + n_c] if keep_pnl else None
            if not cost_only:
                be.pnl(snap, data, slab, has_b=has_b, hold_c=hold_c, pnl_out=pout, exercise=ex, n_local=n_c)
                slabs.append(slab)
            if costs is not None:
                nslab = torch.zeros_like(slab)
                cslab = torch.zeros(slab.shape[0], LC.COST_NSTAT, dtype=torch.float64, device=dev)
                be.pnl(snap, data, nslab, has_b=has_b, hold_c=hold_c, pnl_out=pout if cost_only else None, n_local=n_c,
                       costs=costs, cost_stats=cslab)
                nslabs.append(nslab)
                cslabs.append(cslab)
            if keep_paths:
                kept.append(p)
            elif run.device.type == "cuda":
                torch.cuda.synchronize(run.device)
            del p, data  # (without keep_paths the chunk's tables are released before the next is simulated)
    # the statistics rows of every chunk (and rank), summed the way collect() sums the in-sample ones
    nst = reduce_stats(torch.cat(nslabs, dim=0), world) if costs is not None else None
    st = nst if cost_only else reduce_stats(torch.cat(slabs, dim=0), world)
    n = float(st[L.ES_COUNT])
    assert n == float(n_total), (n, n_total)
    m = st[L.ES_RES] / n
    std = float(np.sqrt(max(st[L.ES_RES2] / n - m * m, 0.0) * n / max(n - 1, 1)))
    res = OosResult(mean=float(m) * scale, std=std * scale, min=float(st[L.ES_RESMIN]) * scale,
                    max=float(st[L.ES_RESMAX]) * scale, mean_terminal_wealth=float(st[L.ES_V] / n) * scale,
                    n_paths=n_total, seed=seed, offset=offset, stress=stress,
                    route="fused" if use_fused else "materialised", stats=st, chunks=max(len(slabs), len(nslabs)))
    if costs is not None:
        from .driver import DateResult

        cst = reduce_cost_stats(torch.cat(cslabs, dim=0), world)
        assert float(cst[LC.CS_COUNT]) == float(n_total), (cst[LC.CS_COUNT], n_total)
        res.costs = run.cost_report(costs, DateResult(index=-1, time=0.0, stats=nst), cst,
                                    None if cost_only else res.std, v0 * scale)
        res.costs["in_sample"] = _in_sample_costs(run, scale)
    res.in_sample = _in_sample(run, scale)
    if res.in_sample is not None and res.in_sample["std"] > 0:
        res.std_ratio = res.std / res.in_sample["std"]
    if ex is not None:
        res.exercise_share = float(st[L.ES_EXER] / n)
        res.mean_exercise_date = float(st[L.ES_TAU] / n) * run.grid.dt_coarse
        res.policy_value = float(st[L.ES_EXVAL] / n) * scale
    if keep_pnl:
        res.pnl = pnl
        q = risk.quantile(pnl, QUANTILES, world)
        res.quantiles = {"q": list(QUANTILES), "values": [float(x) * scale for x in q]}
    if keep_paths:
        res.paths = kept[0] if len(kept) == 1 else kept
    if run.device.type == "cuda":
        torch.cuda.synchronize(run.device)
    res.seconds = time.perf_counter() - t0
    return res
