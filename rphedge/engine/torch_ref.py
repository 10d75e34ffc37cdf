"""The torch reference backend (CPU oracle; gloo data parallel)."""
from __future__ import annotations

import math

import numpy as np
import torch

from ..models.hedge_mlp import NetSpec, torch_forward
from ..ops import layout as L
from ..ops import layout_cost as LC
from . import lm_ref
from .config import Costs, DateData, Exercise, FitConfig, PnlData, TrainConfig
from .lm_geometry import _lm_bias_index
from .state import (StateBlocks, _check_eval_data, _normalise, _steps, current_copy, design, fit_template,
                    store_weights, with_bond)


def _common_stats(st, v, res):
    """The statistics ``eval`` and ``pnl`` share, from the values ``v`` and the residuals ``res`` (float64 [n])."""
    st[L.ES_V], st[L.ES_V2] = v.sum(), (v * v).sum()
    st[L.ES_RES], st[L.ES_RES2], st[L.ES_ABSRES] = res.sum(), (res * res).sum(), res.abs().sum()
    st[L.ES_COUNT] = res.numel()
    st[L.ES_RESMIN], st[L.ES_RESMAX] = res.min(), res.max()


class TorchBackend(StateBlocks):
    name = "torch"

    def __init__(self, spec: NetSpec, n_local: int, tcfg: TrainConfig, device="cpu", comm=None,
                 world: int = 1, rank: int = 0, dtype=torch.float32, stream=None):
        self.spec, self.n_local, self.tcfg = spec, int(n_local), tcfg
        self.device = torch.device(device)
        self.world, self.rank, self.dtype = world, rank, dtype
        self.batch_local, self.steps_per_epoch = _steps(self.n_local, tcfg, world)
        self.eval_wgs = 1
        self._order_cache = {}
        self._lm_lam_last = {}  # loss -> the last LM fit's final damping (FitConfig.lm_lam_carry)

    def _order(self, seed, epoch):
        from ..ops.philox import epoch_order

        key = (seed, epoch)
        o = self._order_cache.get(key)
        if o is None:
            o = torch.from_numpy(epoch_order(self.n_local, self.tcfg.chunk_log2, seed, epoch,
                                             self.tcfg.shuffle)).to(self.device)
            if len(self._order_cache) > 64:
                self._order_cache.clear()
            self._order_cache[key] = o
        return o

    def _allreduce(self, t: torch.Tensor):
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(t)
        return t

    def _lm_fit(self, wts, fit, data: DateData, fcfg: FitConfig):
        """Reference semantics of the HIP Levenberg-Marquardt fit (hedge_lm.hip) in float64: the steps of lm_ref."""
        t, loss = self.tcfg, int(fcfg.loss)
        X, pr, y = xpy = design(data.feats, data.prices_next, data.bond_next, data.target, data, lm_ref.DT)
        w0 = lm_ref.start_point(self.spec, wts, data, fcfg)
        lam0 = lam = float(t.lm_lam0 if fcfg.lm_lam0 is None else fcfg.lm_lam0)
        if float(fcfg.lm_lam_carry) > 0.0:
            lam = max(self._lm_lam_last.get(loss, 0.0) * float(np.float32(fcfg.lm_lam_carry)),
                      float(np.float32(t.lm_lam_min)))
        if int(fcfg.lm_starts) >= 1 and int(fcfg.lm_explore_passes) > 0:
            w0, lam, self.lm_explore_last = lm_ref.multi_start(self, fcfg, data, xpy, lam0)
        ev = lm_ref.make_eval(self, fcfg, xpy, self.n_local, max(self.world, 1), main=data)
        r = lm_ref.run_trials(t, ev, w0, int(fcfg.epochs), lam, float(fcfg.lm_stop_tol), max(1, int(fcfg.lm_stop_min)))
        self._lm_lam_last[loss] = r.lam
        w, best, self.lm_out_dl = lm_ref.final_step(self, fcfg, data, X, pr, r)
        lm_ref.publish(wts, fit, w, best + self.lm_out_dl, r)
        self.lm_last = {"lam": r.lam, "hist": r.hist}

    def bias_refit(self, wts, opt, fit, data: DateData, fcfg: FitConfig):
        """Reference semantics of HipBackend.bias_refit: b_psi -= mean(e) / B
        (e = fitted value - target over all paths, B = the bond price)."""
        spec, bi = self.spec, _lm_bias_index(self.spec, self.tcfg)
        if bi < 0:
            return
        X, pr, y = design(data.feats, data.prices_next, data.bond_next, data.target, data, lm_ref.DT)
        w = current_copy(wts, spec.nparams).to(lm_ref.DT)
        e = (torch_forward(spec, w, X) * pr).sum(1) - y
        es = self._allreduce(torch.stack([e.sum(), torch.tensor(float(e.numel()), dtype=lm_ref.DT)]))
        wb = float(w[bi] - es[0] / es[1] / float(data.bond_next))
        for k in range(2):
            wts[k * L.PMAX + bi] = wb
        fit[L.F_WBEST + bi] = wb

    def fit(self, wts, opt, fit, data: DateData, fcfg: FitConfig, seed: int, poll_every: int = 0):
        dt, P = self.dtype, self.spec.nparams
        if fcfg.optimizer == "lm":
            if int(fcfg.loss) not in (L.LOSS_MSE, L.LOSS_PINBALL):
                raise ValueError(f"no Levenberg-Marquardt fit for loss {fcfg.loss}")
            return self._lm_fit(wts, fit, data, fcfg)
        fit.copy_(fit_template(fcfg, self.device))
        xpy = design(data.feats, data.prices_next, data.bond_next, data.target, data, dt)
        w = current_copy(wts, P).to(dt).clone()
        m, v = (opt[i:i + P].to(dt).clone() for i in (L.O_M, L.O_V))
        t_it, lr = float(opt[L.O_T].item()), float(opt[L.O_LR].item())
        b1, b2, eps = (float(opt[i].item()) for i in (L.O_B1, L.O_B2, L.O_EPS))
        inv_b = 1.0 / float(self.batch_local * self.world)
        best, wait, has_best = float("inf"), 0, False
        w_best = w.clone()
        patience = fcfg.patience if fcfg.early_stopping else 1 << 30
        restore = fcfg.restore_best and fcfg.early_stopping
        sums = torch.zeros(4, dtype=torch.float64)
        hist, nan_steps, epoch = [], 0, 0
        for epoch in range(fcfg.epochs):
            if fcfg.lr_schedule is not None:
                l_ = fcfg.lr_schedule[epoch]
                if l_ == l_:
                    lr = float(l_)
            order = self._order(seed, epoch)
            for s in range(self.steps_per_epoch):
                pkt = self._packet(w, xpy, order[s * self.batch_local:(s + 1) * self.batch_local], fcfg, inv_b)
                g = pkt[:P].to(dt)
                if torch.isfinite(g).all():
                    t_it += 1.0
                    lr_t = lr * math.sqrt(1.0 - b2 ** t_it) / (1.0 - b1 ** t_it)
                    m = m + (g - m) * (1.0 - b1)
                    v = v + (g * g - v) * (1.0 - b2)
                    w = (w - lr_t * m / (torch.sqrt(v) + eps)).detach()
                else:
                    nan_steps += 1
                sums += pkt[P:P + 4]
            cnt = max(float(sums[3]), 1.0)
            Lval = float(sums[0]) / cnt
            hist.append(Lval)
            fit[L.F_LAST_MAE], fit[L.F_LAST_MAPE] = float(sums[1]) / cnt, 100.0 * float(sums[2]) / cnt
            sums.zero_()
            wait += 1
            if Lval < best or not has_best:
                if Lval < best:
                    best, wait = Lval, 0
                has_best = True
                w_best = w.clone()
            if wait >= patience and epoch > 0:
                if restore:
                    w = w_best.clone()
                break
        else:
            if restore and fcfg.restore_at_end:
                w = w_best.clone()
        store_weights(wts, P, w.to(torch.float32))
        opt[L.O_M:L.O_M + P] = m.to(torch.float32)
        opt[L.O_V:L.O_V + P] = v.to(torch.float32)
        opt[L.O_T], opt[L.O_LR] = t_it, lr
        opt[L.O_NAN] += nan_steps
        fit[L.F_BEST], fit[L.F_WAIT], fit[L.F_HASBEST] = best, wait, 1.0 if has_best else 0.0
        fit[L.F_STOPPED], fit[L.F_EPOCH] = 1.0, epoch + 1
        fit[L.F_LAST_LOSS] = hist[-1] if hist else float("nan")
        fit[L.F_WBEST:L.F_WBEST + P] = w_best.to(torch.float32)
        k = min(len(hist), L.MAXHIST)
        fit[L.F_HIST:L.F_HIST + k] = torch.tensor(hist[:k], dtype=torch.float32)

    def _packet(self, w, xpy, idx, fcfg: FitConfig, inv_b: float) -> torch.Tensor:
        """One minibatch's float64 packet [gradient | loss, |e|, APE sums, count], summed over the ranks."""
        spec, P, q = self.spec, self.spec.nparams, fcfg.quantile
        X, pr, y = xpy
        wv = w.detach().requires_grad_(True)
        V = (torch_forward(spec, wv, X[idx]) * pr[idx]).sum(dim=1)
        e = V - y[idx]
        if fcfg.loss == L.LOSS_PINBALL:
            ep = -e
            lvec = torch.maximum(q * ep, (q - 1.0) * ep)
        else:
            lvec = e * e
        (lvec.sum() * inv_b).backward()
        pkt = torch.zeros(P + 4, dtype=torch.float64)
        pkt[:P] = wv.grad.to(torch.float64)
        with torch.no_grad():
            pkt[P] = lvec.sum().double()
            pkt[P + 1] = e.abs().sum().double()
            pkt[P + 2] = (e.abs() / y[idx].abs().clamp_min(1e-7)).sum().double()
            pkt[P + 3] = float(len(idx))
        return self._allreduce(pkt)

    def pnl_wgs(self) -> int:
        return 1

    def pnl(self, snap, data: PnlData, stats, has_b: bool = False, hold_c: float = 0.0, pnl_out=None,
            exercise: Exercise | None = None, tau_out=None, n_local: int | None = None,
            costs: Costs | None = None, cost_stats=None, cost_out=None, turn_out=None, trades_out=None):
        """Self-financing P&L scan (reference semantics of k_hedge_pnl;
        ``n_local``: accepted like HipBackend.pnl's, the path count is the data's).

        ``costs``: under proportional transaction costs and a no-trade band
        (reference semantics of k_hedge_pnl_cost, fp32 in its operation order;
        csrc/rph_types.h CostTerms): per asset the held position follows the
        target where ``t == 0``, ``band == 0`` or ``|target - held| > band``;
        date t's cost ``rate sum_a |dh_a| S_a,t`` leaves the wealth before the
        update.  ``cost_stats`` ([1, COST_NSTAT] float64) takes the sums,
        ``cost_out`` / ``turn_out`` / ``trades_out`` the per-path cost carried
        to the horizon, turnover and trade dates (t >= 1)."""
        spec, dt, P = self.spec, torch.float32, self.spec.nparams
        bond = data.bond.detach().cpu().double().numpy()
        fmu, fisd = data.fmu.detach().cpu(), data.fisd.detach().cpu()
        if data.w0 is not None:
            wealth = data.w0.to(dt).clone()
        else:  # (PnlDesc.wealth0 with a null w0: every path starts at the scalar)
            wealth = torch.full(data.payoff.shape, float(data.wealth0), dtype=dt, device=data.payoff.device)
        nd = int(data.n_dates)
        if exercise is not None and has_b:
            raise ValueError("pnl: has_b with exercise (early exercise takes one network)")
        if exercise is None and tau_out is not None:
            raise ValueError("pnl: tau_out without exercise")
        if costs is None and any(t is not None for t in (cost_stats, cost_out, turn_out, trades_out)):
            raise ValueError("pnl: cost outputs without costs")
        if costs is not None:
            if exercise is not None:
                raise ValueError("pnl: costs with exercise (early exercise with costs is not supported)")
            if cost_stats is None:
                raise ValueError("pnl: costs without cost_stats")
            rate, band = (torch.tensor(float(v), dtype=dt) for v in (costs.rate, costs.band))
            held = None
            cost_T, turn = torch.zeros_like(wealth), torch.zeros_like(wealth)
            trades = torch.zeros(wealth.shape, dtype=torch.int32, device=wealth.device)
        tau = torch.full(wealth.shape, nd, dtype=torch.int32, device=wealth.device)
        pnl_ex = torch.zeros_like(wealth)
        paid = torch.zeros(wealth.shape, dtype=torch.float64, device=wealth.device)
        with torch.no_grad():
            for t in range(data.n_dates):
                X = torch.stack([f.to(dt) for f in data.features(t)], dim=1)
                X = (X - fmu[t, : spec.nin].to(dt)) * fisd[t, : spec.nin].to(dt)
                hold = torch_forward(spec, snap[t, 0, :P].to(dt), X)
                if has_b:
                    hb = torch_forward(spec, snap[t, 1, :P].to(dt), X)
                    hold = hold + hold_c * (hb - hold)
                grow = float(bond[t + 1] / bond[t])
                alive = tau == nd
                if exercise is not None and t % int(exercise.every) == 0:
                    # continuation value of date t's network vs the intrinsic value (the eval rule)
                    now = [s.to(dt) for s in data.prices(t)]
                    c = torch.zeros_like(wealth)
                    for a, s0 in enumerate(now):
                        c = c + hold[:, a] * s0
                    c = c + hold[:, len(now)] * float(np.float32(bond[t]))
                    x = exercise.intrinsic(now[0])
                    ex = alive & (x > 0) & (x >= c)
                    to_end = float(np.float32(bond[nd] / bond[t]))
                    pnl_ex = torch.where(ex, (wealth - x) * to_end, pnl_ex)
                    paid = torch.where(ex, x.double() * float(bond[0] / bond[t]), paid)
                    wealth = torch.where(ex, wealth * to_end, wealth)  # W_tau in the bank account to the horizon
                    tau = torch.where(ex, torch.full_like(tau, t), tau)
                    alive = tau == nd
                if costs is not None:
                    now = [s.to(dt) for s in data.prices(t)]
                    na = len(now)
                    target = hold[:, :na]
                    if held is None:
                        held = torch.zeros_like(target)
                    tr = (target - held).abs() > band
                    if t == 0 or float(band) == 0.0:
                        tr = torch.ones_like(tr)
                    new = torch.where(tr, target, held)
                    dv = torch.zeros_like(wealth)
                    for a in range(na):  # ascending a
                        dv = dv + (new[:, a] - held[:, a]).abs() * now[a]
                    c = rate * dv
                    wealth = wealth - c
                    cost_T = cost_T + c * float(np.float32(bond[nd] / bond[t]))
                    turn = turn + dv
                    if t > 0:
                        trades = trades + tr.any(dim=1).to(torch.int32)
                    held = new
                    hold = torch.cat([new, hold[:, na:]], dim=1)
                w = wealth * grow
                for a, (s0, s1) in enumerate(zip(data.prices(t), data.prices(t + 1))):
                    w = w + hold[:, a] * (s1.to(dt) - s0.to(dt) * grow)
                wealth = torch.where(alive, w, wealth) if exercise is not None else w
            if costs is not None and costs.unwind:  # the final position is sold at the horizon
                dv = torch.zeros_like(wealth)
                for a, s in enumerate(data.prices(nd)):
                    dv = dv + held[:, a].abs() * s.to(dt)
                c = rate * dv
                wealth, cost_T, turn = wealth - c, cost_T + c, turn + dv
            pnl = wealth - data.payoff.to(dt)
            if exercise is not None:
                pnl = torch.where(tau < nd, pnl_ex, pnl)
                paid = torch.where(tau < nd, paid, data.payoff.double() * float(bond[0] / bond[nd]))
                if tau_out is not None:
                    tau_out.copy_(tau)
            if pnl_out is not None:
                pnl_out.copy_(pnl)
            st = torch.zeros(L.EVAL_NSTAT, dtype=torch.float64)
            _common_stats(st, wealth.double(), pnl.double())
            if exercise is not None:
                st[L.ES_EXER], st[L.ES_EXVAL], st[L.ES_TAU] = (tau < nd).sum(), paid.sum(), tau.double().sum()
            stats[0].copy_(st)
            if costs is not None:
                for out, v in ((cost_out, cost_T), (turn_out, turn), (trades_out, trades)):
                    if out is not None:
                        out.copy_(v)
                cs = torch.zeros(LC.COST_NSTAT, dtype=torch.float64)
                cd = cost_T.double()
                cs[LC.CS_COST], cs[LC.CS_COST2], cs[LC.CS_TURN] = cd.sum(), (cd * cd).sum(), turn.double().sum()
                cs[LC.CS_TRADES], cs[LC.CS_COUNT] = trades.double().sum(), cd.numel()
                cost_stats[0].copy_(cs)

    def eval(self, wts, data: DateData, stats, wts_b=None, g_base=None, blend_c=0.0, hold_c=0.0,
             v_out=None, hold_out=None, resid_out=None, pred1_out=None, snap_a=None, snap_b=None,
             n_local: int | None = None, exercise: Exercise | None = None):
        spec, dt, P = self.spec, torch.float32, self.spec.nparams
        _check_eval_data(spec, data)
        if snap_a is not None:
            snap_a.copy_(wts)
        if snap_b is not None:
            snap_b.copy_(wts_b if wts_b is not None else wts)
        X = _normalise(torch.stack([f.to(dt) for f in data.feats], dim=1), data)
        with torch.no_grad():
            hold = torch_forward(spec, current_copy(wts, P).to(dt), X)
            holdv = hold
            if wts_b is not None:
                holdv = torch_forward(spec, current_copy(wts_b, P).to(dt), X)
                hold = hold + hold_c * (holdv - hold)
            V = (holdv * with_bond(data.prices_now, data.bond_now, X)).sum(dim=1)
            if g_base is not None:
                V = g_base + blend_c * (V - g_base)
            if exercise is not None:
                if wts_b is not None or g_base is not None:
                    raise ValueError("eval: wb / g_base with exercise (early exercise takes one network)")
                if not data.prices_now:
                    raise ValueError("eval: price_t[0] is null with exercise")
                cont = V
                xval = exercise.intrinsic(data.prices_now[0].to(dt))
                exer = (xval > 0) & (xval >= cont)
                V = torch.where(exer, xval, cont)
            if data.prices_next:
                pred1 = (hold * with_bond(data.prices_next, data.bond_next, X)).sum(dim=1)
            else:
                pred1 = torch.zeros_like(V)
            res = (data.target.to(dt) - pred1) if data.target is not None else torch.zeros_like(V)
            if v_out is not None:
                v_out.copy_(V)
            if hold_out is not None:
                for k, h in enumerate(hold_out):
                    if h is not None:
                        h.copy_(hold[:, k])
            if resid_out is not None:
                resid_out.copy_(res)
            if pred1_out is not None:
                pred1_out.copy_(pred1)
            st = torch.zeros(L.EVAL_NSTAT, dtype=torch.float64)
            rd, hd = res.double(), hold.double()
            _common_stats(st, V.double(), rd)
            if data.target is not None:
                st[L.ES_APE] = (rd.abs() / data.target.double().abs().clamp_min(1e-7)).sum()
            st[L.ES_PRED1] = pred1.double().sum()
            for k in range(spec.nhold):
                st[L.ES_HOLD + k] = hd[:, k].sum()
                st[L.ES_HOLD2 + k] = (hd[:, k] ** 2).sum()
            if exercise is not None:
                st[L.ES_EXER] = exer.sum()
                st[L.ES_EXVAL] = torch.where(exer, xval, torch.zeros_like(xval)).double().sum()
                st[L.ES_CONT] = cont.double().sum()
            stats[0].copy_(st)
