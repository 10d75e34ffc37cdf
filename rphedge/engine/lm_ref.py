"""fp64 reference of the HIP Levenberg-Marquardt fit (csrc/hedge_lm.hip), the
steps of :meth:`TorchBackend._lm_fit` (``be``).  The GPU tests compare against
it bitwise or at 1e-5: every float operation keeps its order and dtype."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from ..models.hedge_mlp import torch_forward
from ..ops import layout as L
from .lm_geometry import (_lm_bias_index, _lm_out_n, gram_subsample, lm_explore_nsub, lm_gram_geometry, lm_pass_wgs,
                          lm_shard_gram_wgs)
from .state import current_copy, design, store_weights

DT = torch.float64
_f32 = lambda v: float(np.float32(v))  # noqa: E731


def _gram_rows(t, xpy, data, pin: bool, n_loc: int, world: int):
    """(Xg, pg, yg, inv_ns, same_g): an evaluator's Gram subsample.  A main fit's (``data``) is the global one of
    gram_subsample (HipBackend._lm_gram_mode): the simulated subsample data (the same G on every rank; a pinball
    fit also needs its targets for the IRLS weights) or, on one rank, from the shard; else this rank's part
    of it from the shard."""
    side = data is not None and data.gram_feats is not None and data.gram_prices_next is not None and (
        not pin or data.gram_target is not None)
    same_g = data is not None and (side or world == 1)
    if same_g:
        ns, blk, bstride = gram_subsample(n_loc * world, t.lm_gram_paths)
        inv_ns = 1.0 / float(ns)
        if side:
            return design(data.gram_feats, data.gram_prices_next, data.bond_next, data.gram_target, data, DT) + (
                inv_ns, same_g)
    else:
        ns = lm_shard_gram_wgs(n_loc, t.lm_gram_paths, world, lm_pass_wgs(n_loc)) * L.LM_TILE
        inv_ns = 1.0 / float(ns * world)
        blk, bstride = lm_gram_geometry(n_loc, ns, world)
    sub = torch.tensor([(j // blk) * bstride + j % blk for j in range(ns)], dtype=torch.long)
    return tuple(v[sub] for v in xpy) + (inv_ns, same_g)


def make_eval(be, fcfg, xpy, n_loc: int, world: int, main=None):
    """evaluate(w) -> (G, g, stats) over the first n_loc local paths of ``xpy`` (all-reduced over the ranks when
    world > 1; ``main``: the DateData of a fit over every local path - only g and the statistics are summed
    where every rank builds the same G)."""
    from torch.func import jacrev, vmap

    spec, P = be.spec, be.spec.nparams
    pin = int(fcfg.loss) == L.LOSS_PINBALL
    q = _f32(fcfg.quantile)
    q_delta = _f32(fcfg.lm_q_delta if float(fcfg.lm_q_delta) > 0.0 else 1e-6)
    q_kappa = _f32(fcfg.lm_q_kappa)
    Xn, prn, yn = (v[:n_loc] for v in xpy)
    n_glob = float(n_loc * world)
    Xg, pg, yg, inv_ns, same_g = _gram_rows(be.tcfg, (Xn, prn, yn), main, pin, n_loc, world)

    def v_one(w, x, p):
        return (torch_forward(spec, w, x[None])[0] * p).sum()

    def evaluate(w):
        wg = w.detach().clone().requires_grad_(True)
        e = (torch_forward(spec, wg, Xn) * prn).sum(1) - yn
        if pin:
            # pinball loss of y - V (Replicating_Portfolio.py:138-145), its
            # subgradient (path_loss), the IRLS Gram weights of its
            # quadratic majoriser (k_lm_pass)
            ed = e.detach()
            pos = -q * ed >= (q - 1.0) * (-ed)
            lvec = torch.where(pos, -q * ed, (q - 1.0) * (-ed))
            lsum = lvec.sum()
            dV = torch.where(pos, torch.full_like(ed, -q), torch.full_like(ed, 1.0 - q))
            ((dV * (torch_forward(spec, wg, Xn) * prn).sum(1)).sum() / n_glob).backward()
        else:
            lsum = (e * e).sum()
            (lsum / n_glob).backward()
        J = vmap(jacrev(v_one), in_dims=(None, 0, 0))(w.detach(), Xg, pg)
        if pin:
            rg = (torch_forward(spec, w.detach(), Xg) * pg).sum(1) - yg
            ra = rg.abs()
            # per 64-path tile: delta = max(q_delta, kappa x mean |r| of the tile)
            dl = torch.clamp_min(q_kappa * ra.view(-1, L.LM_TILE).mean(1, keepdim=True), q_delta)
            J = J * (0.5 / torch.sqrt(torch.maximum(ra.view(-1, L.LM_TILE), dl).reshape(-1)))[:, None]
        G = (J.T @ J).reshape(-1) * inv_ns
        rest = torch.cat([wg.grad.detach(),
                          torch.stack([lsum.detach(), e.detach().abs().sum(),
                                       (e.detach().abs() / yn.abs().clamp_min(1e-7)).sum(),
                                       torch.tensor(float(len(yn)), dtype=DT)])])
        if world > 1:
            if same_g:
                be._allreduce(rest)  # (the gradient region only)
            else:
                red = torch.cat([G, rest])
                be._allreduce(red)
                G, rest = red[: P * P], red[P * P:]
        return G.reshape(P, P), rest[:P], rest[P:]
    return evaluate


# run_trials' result: the best point with its (G, g, stats, loss), the final damping, the loss history, the
# evaluation the best point came from and the last evaluation's (w, g, loss)
Trials = namedtuple("Trials", "w G g stats loss lam hist best_k last")


def run_trials(t, evaluate, w_best, passes: int, lam: float, tol: float = 0.0, kmin: int = 1) -> Trials:
    """The solve kernel's sequence: ``passes`` trial points after ``w_best``."""
    nielsen = str(t.lm_damping).lower() == "nielsen"
    nu = 2.0
    G, g, stb = evaluate(w_best)
    Lb = float(stb[0] / stb[3].clamp_min(1.0))
    hist = [Lb]
    best_k, last = 0, (w_best, g, Lb)
    for k in range(1, int(passes) + 1):
        Lb_old = Lb
        A = 2.0 * G
        dg = torch.diagonal(A).clone()
        dmp = torch.clamp_min(dg, float(np.float32(t.lm_diag_floor)) * float(dg.mean())) * lam + \
            float(t.lm_ridge) * float(dg.mean())
        A = A + torch.diag(dmp)
        Lc, info = torch.linalg.cholesky_ex(A)
        pred = 0.0
        if int(info) != 0:
            trial = w_best.clone()
            lam = min(lam * t.lm_lam_up * t.lm_lam_up, t.lm_lam_max)
        else:
            dlt = torch.cholesky_solve(-g[:, None], Lc)[:, 0]
            trial = w_best + dlt
            pred = float(0.5 * ((dmp * dlt * dlt).sum() - (g * dlt).sum()))
        Gt, gt, stt = evaluate(trial)
        Lt = float(stt[0] / stt[3].clamp_min(1.0))
        hist.append(Lt)
        last = (trial, gt, Lt)  # (the last trial: the final out step may start there)
        accepted = Lt == Lt and Lt < Lb
        if accepted:
            if nielsen:
                rho = (Lb - Lt) / pred if pred > 0.0 else 1.0
                lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), t.lm_lam_min)
                nu = 2.0
            else:
                lam = max(lam * t.lm_lam_down, t.lm_lam_min)
            w_best, G, g, stb, Lb = trial, Gt, gt, stt, Lt
            best_k = k
        elif nielsen:
            lam = min(lam * nu, t.lm_lam_max)
            nu *= 2.0
        else:
            lam = min(lam * t.lm_lam_up, t.lm_lam_max)
        # adaptive budget (the solve kernel's LSS_STOP rule, accepted
        # steps only; fp32 tolerance)
        if tol > 0.0 and k >= kmin and accepted and not (Lb_old - Lb > float(np.float32(tol)) * Lb):
            break
    return Trials(w_best, G, g, stb, Lb, lam, hist, best_k, last)


def start_point(spec, wts, data, fcfg) -> torch.Tensor:
    """The fit's start point: the current weights, with FitConfig.lm_renorm re-expressed for this fit's
    standardisation (the k_lm_pass start-point transform: fp64 from the fp32 weights, rounded once)."""
    w32 = current_copy(wts, spec.nparams).to(DT)
    w_best = w32.clone()
    if fcfg.lm_renorm is not None and data.fmu:
        o = spec.offsets
        mu_o, isd_o = fcfg.lm_renorm
        for j in range(spec.hidden):
            acc = float(w32[o["b1"] + j])
            for f in range(spec.nin):
                acc += float(w32[o["W1"] + f * spec.hidden + j]) * _f32(isd_o[f]) * (_f32(data.fmu[f]) - _f32(mu_o[f]))
            w_best[o["b1"] + j] = _f32(acc)
        for f in range(spec.nin):
            r = _f32(isd_o[f]) / _f32(data.fisd[f])
            for j in range(spec.hidden):
                w_best[o["W1"] + f * spec.hidden + j] = _f32(float(w32[o["W1"] + f * spec.hidden + j]) * r)
    return w_best


def multi_start(be, fcfg, data, xpy, lam0: float):
    """Multi-start exploration (k_lm_select): the same K fits on every rank, on the global path prefix
    (FitConfig.lm_explore_data); (start point, damping) of the polish fit and the lm_explore_last record."""
    t, P, K, xd = be.tcfg, be.spec.nparams, int(fcfg.lm_starts), fcfg.lm_explore_data
    nsub = lm_explore_nsub(fcfg, be.n_local)
    if xd is not None:
        xpy = design(xd.feats, xd.prices_next, xd.bond_next, xd.target, data, DT)
    elif be.world > 1:
        raise ValueError("data-parallel multi-start exploration needs lm_explore_data (the global prefix)")
    ev = make_eval(be, fcfg, xpy, nsub, 1)
    rows = np.asarray(fcfg.lm_w0s, dtype=np.float32)
    sel = torch.zeros(K, 2 + P, dtype=DT)
    for k in range(K):
        r = run_trials(t, ev, torch.from_numpy(rows[k, :P].copy()).to(DT), int(fcfg.lm_explore_passes), lam0)
        sel[k, 0], sel[k, 1], sel[k, 2:] = r.loss, r.lam, r.w
    ls = sel[:, 0].clone()
    ls[torch.isnan(ls)] = float("inf")
    pick = int(torch.argmin(ls))  # (first index of the minimum)
    return (sel[pick, 2:].to(torch.float32).to(DT), max(float(sel[pick, 1]), t.lm_lam_min),
            {"losses": sel[:, 0].tolist(), "pick": pick})


def out_step(be, X, pr, wp, gp, n_out: int):
    """lm_out_newton at point wp (gradient gp): the full-batch output-layer
    Gram G_oo = mean_p u u^T, u = dV/dtheta_o; (step, exact loss change) or None."""
    spec, t = be.spec, be.tcfg
    h, o, P = spec.hidden, spec.offsets, spec.nparams
    W1 = wp[o["W1"]:o["b1"]].view(spec.nin, h)
    a1 = torch.nn.functional.leaky_relu(X @ W1 + wp[o["b1"]:o["W2"]], spec.alpha)
    a2 = torch.nn.functional.leaky_relu(a1 @ wp[o["W2"]:o["b2"]].view(h, h) + wp[o["b2"]:o["W3"]], spec.alpha)
    c = pr if spec.head == L.HEAD_FREE else (pr[:, 0] - pr[:, 1])[:, None]
    u = torch.cat([(a2[:, :, None] * c[:, None, :]).reshape(len(c), -1), c], dim=1)
    Goo = u.T @ u
    if be.world > 1:
        be._allreduce(Goo)
    Goo = Goo / float(be.n_local * be.world)
    A = 2.0 * Goo
    dgA = torch.diagonal(A).clone()
    A = A + torch.diag(dgA * float(np.float32(t.lm_out_mu))) + \
        torch.eye(n_out, dtype=DT) * (float(np.float32(t.lm_ridge)) * float(dgA.sum()) / n_out)
    Lc, info = torch.linalg.cholesky_ex(A)
    if int(info) != 0:
        return None
    go = gp[P - n_out:]
    dlt = torch.cholesky_solve(-go[:, None], Lc)[:, 0]
    return dlt, float(go @ dlt + dlt @ Goo @ dlt)  # exact full-batch loss change


def final_step(be, fcfg, data, X, pr, r: Trials):
    """The solve kernel's final step -> (weights, loss, the out step's loss
    change): the last evaluation (k_lm_pass<BodyOG>, LM_OUTG_TAIL = 1) built
    the output Gram; out step at the best point when the last trial was
    accepted, else at the rejected last trial, published when trial + step
    beats the best point; otherwise the bias step."""
    spec, t, P = be.spec, be.tcfg, be.spec.nparams
    pin = int(fcfg.loss) == L.LOSS_PINBALL
    bi = -1 if pin else _lm_bias_index(spec, t)
    n_out, out_ok = (0 if pin else _lm_out_n(spec, t)), False
    w_best, Lb, out_dl = r.w, r.loss, 0.0
    ran_all = len(r.hist) - 1 == int(fcfg.epochs)  # (an adaptive stop skips the output-Gram pass)
    if n_out and ran_all:
        at_best = r.best_k == int(fcfg.epochs)  # (the last trial was accepted: it is the best point)
        lw, lg, lL = (w_best, r.g, Lb) if at_best else r.last
        s = out_step(be, X, pr, lw, lg, n_out) if (at_best or (lL == lL and lL < 2.0 * Lb)) else None
        if s is not None and (at_best or lL + s[1] < Lb):
            w_best = lw.clone()
            w_best[P - n_out:] += s[0]
            Lb, out_dl, out_ok = lL, s[1], True
    # (the bond holding's bias: dV/db = B on every path, so G_bb = B^2
    # exactly - as k_lm_solve, independent of the subsample Gram's rounding)
    gbb = float(np.float32(data.bond_next)) ** 2
    if not out_ok and bi >= 0 and gbb > 0.0:
        w_best = w_best.clone()
        w_best[bi] -= r.g[bi] / (2.0 * gbb)
    return w_best, Lb, out_dl


def publish(wts, fit, w_best, loss: float, r: Trials):
    """Write the fitted weights (both copies) and the fit block."""
    P = w_best.numel()
    w32 = w_best.to(torch.float32)
    store_weights(wts, P, w32)
    fit.zero_()
    fit[L.F_HIST:] = float("nan")  # (as k_lm_pass: passes never run stay NaN)
    fit[L.F_WBEST:L.F_WBEST + P] = w32
    c = max(float(r.stats[3]), 1.0)
    fit[L.F_BEST] = fit[L.F_LAST_LOSS] = loss
    fit[L.F_LAST_MAE], fit[L.F_LAST_MAPE] = float(r.stats[1]) / c, 100.0 * float(r.stats[2]) / c
    fit[L.F_EPOCH], fit[L.F_STOPPED], fit[L.F_HASBEST] = len(r.hist), 1.0, 1.0
    k = min(len(r.hist), L.MAXHIST)
    fit[L.F_HIST:L.F_HIST + k] = torch.tensor(r.hist[:k], dtype=torch.float32)
