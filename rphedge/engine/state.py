"""State blocks (flat float32 tensors, layout in :mod:`rphedge.ops.layout`) and
the input helpers both backends share."""
from __future__ import annotations

import math

import numpy as np
import torch

from ..models.hedge_mlp import NetSpec
from ..ops import layout as L
from .config import DateData, FitConfig, TrainConfig


def _set_norm(d, data: DateData):
    for i, (m, s) in enumerate(zip(data.fmu, data.fisd)):
        d.fmu[i], d.fisd[i] = float(m), float(s)


def _normalise(X: torch.Tensor, data: DateData) -> torch.Tensor:
    if not data.fmu:
        return X
    mu = torch.tensor(data.fmu, dtype=X.dtype, device=X.device)
    isd = torch.tensor(data.fisd, dtype=X.dtype, device=X.device)
    return (X - mu) * isd


def with_bond(prices, bond: float, like: torch.Tensor) -> torch.Tensor:
    """[n, nhold] prices: the traded assets and the bond column (rows, dtype, device of ``like``)."""
    return torch.stack([p.to(like.dtype) for p in prices] +
                       [torch.full((like.shape[0],), float(bond), dtype=like.dtype, device=like.device)], dim=1)


def design(feats, prices, bond: float, target, norm: DateData, dt):
    """(X, prices with the bond, y) of a fit at dtype ``dt``: the features
    standardised as ``norm``'s (the reference backend's design matrices)."""
    X = _normalise(torch.stack([f.to(dt) for f in feats], dim=1), norm)
    return X, with_bond(prices, bond, X), (target.to(dt) if target is not None else None)


def _check_eval_data(spec: NetSpec, data: DateData):
    """Reject eval inputs the epilogue has no defined result for (both backends)."""
    na = spec.nhold - 1
    if len(data.prices_now) != na:
        raise ValueError(f"eval needs {na} prices_now tensor(s), got {len(data.prices_now)}")
    if len(data.prices_next) not in (0, na):
        raise ValueError(f"eval needs {na} prices_next tensor(s) or none, got {len(data.prices_next)}")
    if not data.prices_next and data.target is not None:
        raise ValueError("eval with a target needs prices_next: the residual V_{t+1} - h . p_{t+1} is undefined "
                         "without them (pass target=None for the values / holdings alone)")


def current_copy(wts: torch.Tensor, P: int) -> torch.Tensor:
    """The current weight copy as a view of ``wts`` (tensor counterpart of current_weights)."""
    cur = int(wts[L.W_CUR].item())
    return wts[cur * L.PMAX: cur * L.PMAX + P]


def store_weights(wts: torch.Tensor, P: int, w: torch.Tensor):
    """Write ``w`` (float32) into both weight copies; copy 0 becomes the current one."""
    wts[:P] = w
    wts[L.PMAX: L.PMAX + P] = w
    wts[L.W_CUR] = 0.0


def make_weights(spec: NetSpec, w0: np.ndarray, device) -> torch.Tensor:
    t = torch.zeros(L.NETW_FLOATS, dtype=torch.float32)
    store_weights(t, spec.nparams, torch.from_numpy(np.asarray(w0, np.float32)))
    return t.to(device)


def make_opt(tcfg: TrainConfig, device) -> torch.Tensor:
    t = torch.zeros(L.OPT_FLOATS, dtype=torch.float32)
    t[L.O_LR], t[L.O_B1], t[L.O_B2], t[L.O_EPS] = tcfg.lr, tcfg.beta1, tcfg.beta2, tcfg.eps
    return t.to(device)


def fit_template(fcfg: FitConfig, device) -> torch.Tensor:
    t = torch.zeros(L.FIT_FLOATS, dtype=torch.float32)
    t[L.F_BEST], t[L.F_MAXEP] = float("inf"), float(fcfg.epochs)
    t[L.F_PATIENCE] = float(fcfg.patience if fcfg.early_stopping else 1e30)
    t[L.F_RESTORE] = 1.0 if (fcfg.restore_best and fcfg.early_stopping) else 0.0
    t[L.F_RESTORE_END] = 1.0 if fcfg.restore_at_end else 0.0
    t[L.F_HIST:] = float("nan")
    return t.to(device)


def current_weights(spec: NetSpec, wts: torch.Tensor) -> np.ndarray:
    w = wts.detach().cpu().numpy()
    cur = int(w[L.W_CUR])
    return w[cur * L.PMAX: cur * L.PMAX + spec.nparams].copy()


def set_weights(spec: NetSpec, wts: torch.Tensor, w: np.ndarray):
    store_weights(wts, spec.nparams, torch.from_numpy(np.asarray(w, np.float32)).to(wts.device))


def fit_summary(fit: torch.Tensor) -> dict:
    f = fit.detach().cpu().numpy()
    ep = int(f[L.F_EPOCH])
    return {"epochs": ep, "stopped": bool(f[L.F_STOPPED]), "best_loss": float(f[L.F_BEST]),
            "last_loss": float(f[L.F_LAST_LOSS]), "mae": float(f[L.F_LAST_MAE]),
            "mape": float(f[L.F_LAST_MAPE]), "history": f[L.F_HIST:L.F_HIST + min(ep, L.MAXHIST)].tolist()}


class StateBlocks:
    """Constructors of a backend's state blocks (its spec, tcfg, device, eval_wgs and pnl_wgs())."""

    def new_weights(self, w0):
        return make_weights(self.spec, w0, self.device)

    def new_opt(self):
        return make_opt(self.tcfg, self.device)

    def new_fit(self):
        return torch.zeros(L.FIT_FLOATS, dtype=torch.float32, device=self.device)

    def new_stats(self):
        return torch.zeros(self.eval_wgs, L.EVAL_NSTAT, dtype=torch.float64, device=self.device)

    def new_pnl_stats(self):
        return torch.zeros(self.pnl_wgs(), L.EVAL_NSTAT, dtype=torch.float64, device=self.device)

    def new_cost_stats(self):
        from ..ops import layout_cost as LC

        return torch.zeros(self.pnl_wgs(), LC.COST_NSTAT, dtype=torch.float64, device=self.device)


class _Cache:
    def __init__(self):
        self.d = {}

    def get(self, key, make):
        if self.d.get(key) is None:
            self.d[key] = make()
        return self.d[key]


def _steps(n_local: int, tcfg: TrainConfig, world: int) -> tuple[int, int]:
    if tcfg.batch_size % world:
        raise ValueError(f"global batch {tcfg.batch_size} not divisible by world size {world}")
    bl = min(tcfg.batch_size // world, n_local)
    steps = max(1, math.ceil(n_local / bl))
    if n_local % bl:
        raise ValueError(f"local paths {n_local} must be a multiple of the local batch {bl}")
    return bl, steps


def reduce_stats(stats: torch.Tensor, world: int = 1) -> np.ndarray:
    """Sum per-workgroup eval partials (and across ranks) -> [EVAL_NSTAT] float64."""
    s, mn, mx = stats.sum(dim=0), stats[:, L.ES_RESMIN].min(), stats[:, L.ES_RESMAX].max()
    if world > 1:
        from ..parallel.dist import all_reduce_

        all_reduce_(s)
        all_reduce_(mn, "min")
        all_reduce_(mx, "max")
    s = s.detach().cpu().numpy().copy()
    s[L.ES_RESMIN], s[L.ES_RESMAX] = float(mn), float(mx)
    return s


def reduce_cost_stats(slab: torch.Tensor, world: int = 1) -> np.ndarray:
    """Sum the per-workgroup cost partials of a scan under transaction costs
    (and across ranks) -> [COST_NSTAT] float64 (rows ``layout_cost.CS_*``)."""
    s = slab.sum(dim=0)
    if world > 1:
        from ..parallel.dist import all_reduce_

        all_reduce_(s)
    return s.detach().cpu().numpy().copy()
