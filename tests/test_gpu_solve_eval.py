"""The first solve of a later date's LM fit with the previous date's eval riding
in the same launch (k_lm_solve_eval, csrc/hedge_lm.hip; EvalBody::ride,
csrc/hedge_eval.h): against the two launches k_lm_solve + k_hedge_eval, the LM
state (slots, trial weights, speculative steps), v_out, the statistics slab,
the holdings, the residual, pnl_acc and the weight snapshot are equal BYTE FOR
BYTE.  The eval grid has more blocks than there are rider workgroups, so every
rider loops, with a ragged tail."""
import numpy as np
import pytest
import torch

from test_lm_cpu import _teacher_problem

pytestmark = pytest.mark.gpu

N = (1 << 11) + 37  # no multiple of 256: the last block of the eval grid is partial
# (eval blocks, riders): 9 blocks of one iteration on 4 riders (3, 2, 2, 2 blocks); 5 blocks on 2 riders - blocks
# 0..3 take two iterations, block 4 one (1024 + 5 x 256 >= N), the last iteration of block 3 holds 37 paths
GRIDS = [(9, 4), (5, 2)]


def _run(shape, eval_wgs, riders, pnl):
    """(two launches, merged launch): every output as bytes.  ``pnl``: None,
    "first" (pnl_acc written, never read) or "acc" (read and written)."""
    from rphedge.engine import DateData, FitConfig, HipBackend, TrainConfig
    from rphedge.models.hedge_mlp import NetSpec, init_weights
    from rphedge.ops import layout as L

    dev = torch.device("cuda", 0)
    spec = NetSpec(*shape)
    n = N
    feats, pr, y = _teacher_problem(spec, n, 5)
    y = y + 0.05 * torch.sin(7 * feats[0])
    feats1, pr1, _ = _teacher_problem(spec, n, 6)
    pr = [p.to(dev) for p in pr]
    fit = DateData(feats=[f.to(dev) for f in feats], prices_next=pr, bond_next=1.01, target=y.to(dev), prices_now=pr,
                   fmu=tuple([0.1] * spec.nin), fisd=tuple([1.5] * spec.nin))
    # the previous date's eval: its own features, prices at its date = the fit's prices_next, later prices and target
    ev = DateData(feats=[f.to(dev) for f in feats1], prices_next=[p.to(dev) for p in pr1], bond_next=1.02,
                  target=(1.3 * y).to(dev), prices_now=pr, bond_now=1.01, fmu=tuple([-0.2] * spec.nin),
                  fisd=tuple([0.7] * spec.nin))
    be = HipBackend(spec, n, TrainConfig(batch_size=n, lm_gram_paths=1024, lm_out_fix=True), device=dev)
    be.eval_wgs = eval_wgs
    assert (eval_wgs - 1) * 256 < n and eval_wgs > riders
    w = be.new_weights(init_weights(spec, [0.5] * spec.nout, seed=1))
    o, f = be.new_opt(), be.new_fit()
    fc = FitConfig(epochs=4, optimizer="lm", early_stopping=False)  # (4 trial points: the speculative workgroups factorise)
    d, lm = be._lm_prepare(w, o, f, fit, fc)
    b = be._lm_buffers()
    be.native.lm_eval(d, lm, b["red"], 0, None)
    torch.cuda.synchronize()
    state0, fit0 = b["state"].clone(), f.clone()
    acc0 = torch.linspace(-1.0, 1.0, n, dtype=torch.float32, device=dev)

    def outputs():
        return dict(v=torch.full((n,), float("nan"), dtype=torch.float32, device=dev),
                    hold=torch.full((spec.nhold, n), float("nan"), dtype=torch.float32, device=dev),
                    resid=torch.full((n,), float("nan"), dtype=torch.float32, device=dev),
                    stats=torch.full((eval_wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev),
                    snap=torch.zeros(L.NETW_FLOATS, dtype=torch.float32, device=dev),
                    acc=(acc0.clone() if pnl == "acc" else torch.full((n,), float("nan"), dtype=torch.float32, device=dev)))

    def desc(out):
        kw = dict(pnl_acc=out["acc"], pnl_grow=1.003, pnl_carry=0.98, pnl_first=(pnl == "first")) if pnl else {}
        return be.eval_desc(w, ev, out["stats"], v_out=out["v"], hold_out=[out["hold"][k] for k in range(spec.nhold)],
                            resid_out=out["resid"], snap_a=out["snap"], **kw)

    def collect(out):
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy().tobytes() for k, v in out.items()}
        r["state"], r["fit"] = b["state"].cpu().numpy().tobytes(), f.cpu().numpy().tobytes()
        return r

    a = outputs()
    be.native.lm_solve(d, lm, b["red"], 0, None)
    be.native.eval_(desc(a), None)
    ra = collect(a)
    assert b["state"].cpu().numpy().tobytes() != state0.cpu().numpy().tobytes()  # (the solve did write the state)
    if not pnl:
        a["acc"].fill_(0.0)
    assert all(bool(torch.isfinite(a[k]).all()) for k in ("v", "hold", "resid", "stats", "acc"))
    assert float(a["stats"][:, L.ES_COUNT].sum()) == n
    b["state"].copy_(state0)
    f.copy_(fit0)
    m = outputs()
    be.native.lm_solve_eval(d, lm, b["red"], 0, desc(m), riders, None)
    rm = collect(m)
    return ra, rm


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shape", [(1, 8, 2, 0), (2, 8, 2, 0)])
def test_merged_launch_is_bytewise_the_two_launches(shape, grid):
    ra, rm = _run(shape, grid[0], grid[1], "acc")
    for k in ra:
        assert ra[k] == rm[k], k


@pytest.mark.parametrize("pnl", ["first", None])
def test_merged_launch_pnl_first_and_without_fold(pnl):
    ra, rm = _run((1, 8, 2, 0), 5, 2, pnl)
    for k in ra:
        assert ra[k] == rm[k], k
