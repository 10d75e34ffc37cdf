"""The self-financing P&L folded into the backward induction (EvalDesc.pnl_acc,
k_pnl_finish), the parts that need no GPU: the backward form of the wealth
recursion against the forward one, the per-date factors the host hands to the
kernels, and the backends without the fold keeping the forward scan."""
import numpy as np
import pytest
import torch

from test_gpu_eval import f32, make_spec
from test_gpu_pnl import HOLD_C, make_tables, reference
from test_pnl import _np_forward


def holdings(spec, tb, t, has_b):
    """fp64 reported holdings of date t (test_gpu_pnl.reference's, per date)."""
    X = np.stack([f[t].double().numpy() for f in tb["feats"]], axis=1)
    X = (X - tb["fmu"][t, :spec.nin].double().numpy()) * tb["fisd"][t, :spec.nin].double().numpy()
    alpha = f32(spec.alpha)
    h = _np_forward(spec, tb["ws"][t, 0].astype(np.float64), X, alpha)
    if has_b:
        hb = _np_forward(spec, tb["ws"][t, 1].astype(np.float64), X, alpha)
        h = h + f32(HOLD_C) * (hb - h)
    return h


def backward_form(spec, tb, nd, has_b):
    """W_T = W_0 c_{-1} + R_0, R_t = R_{t+1} + c_t sum_a h_a,t (S_a,t+1 - S_a,t g_t), dates nd-1 .. 0;
    c_t the exact fp64 product of the fp32 g_s over s > t."""
    na = spec.nhold - 1
    bond = tb["bond"].numpy()
    g = np.array([f32(bond[t + 1] / bond[t]) for t in range(nd)], np.float64)
    R = np.zeros(tb["w0"].numel())
    c = 1.0
    for t in range(nd - 1, -1, -1):
        S0 = np.stack([p[t].double().numpy() for p in tb["prices"]], axis=1)
        S1 = np.stack([p[t + 1].double().numpy() for p in tb["prices"]], axis=1)
        R = R + c * (holdings(spec, tb, t, has_b)[:, :na] * (S1 - S0 * g[t])).sum(axis=1)
        c = c * g[t]
    return tb["w0"].double().numpy() * c + R


@pytest.mark.parametrize("nd", [1, 2, 7])
@pytest.mark.parametrize("shape,has_b", [((1, 8, 2, 0), False), ((3, 8, 2, 0), True), ((5, 8, 6, 0), False)])
def test_backward_form_equals_forward_recursion(shape, has_b, nd):
    spec = make_spec(shape)
    tb = make_tables(spec, 300, nd, has_b, seed=7 + nd)
    W, pnl = reference(spec, tb, nd, has_b)
    Wb = backward_form(spec, tb, nd, has_b)
    assert np.abs(Wb - W).max() <= 1e-12 * np.abs(W).max()
    assert np.abs((Wb - tb["payoff"].double().numpy()) - pnl).max() <= 1e-12 * max(np.abs(W).max(), np.abs(pnl).max())


@pytest.mark.parametrize("nd", [1, 2, 7, 252])
def test_fold_factors_are_fp32_roundings_of_fp64_products(nd):
    from rphedge.engine import pnl_fold_factors

    rng = np.random.default_rng(nd)
    bond = np.cumprod(np.concatenate([[1.0], 1.0 + 0.01 * rng.random(nd)]))
    grow, carry, carry_all = pnl_fold_factors(bond)
    assert grow.dtype == np.float32 and carry.dtype == np.float32 and grow.shape == carry.shape == (nd,)
    g = [np.float32(bond[t + 1] / bond[t]) for t in range(nd)]
    assert all(grow[t] == g[t] for t in range(nd))
    for t in range(-1, nd):
        prod = 1.0
        for s in range(nd - 1, t, -1):  # the order the induction visits the dates
            prod *= float(g[s])
        want = np.float32(prod)
        got = carry_all if t < 0 else carry[t]
        assert got == want, (t, got, want)
    assert carry[nd - 1] == np.float32(1.0)


def test_torch_backend_keeps_the_forward_scan(monkeypatch):
    from rphedge.api import european_option
    from rphedge.engine import TorchBackend

    calls = []
    orig = TorchBackend.pnl

    def counted(self, *a, **kw):
        calls.append(kw.get("has_b"))
        return orig(self, *a, **kw)

    monkeypatch.setattr(TorchBackend, "pnl", counted)
    assert not hasattr(TorchBackend, "pnl_finish")
    res = european_option(N_paths=1024, dt=1 / 52, rebalancing_frequency=1 / 26, epochs_first=2, epochs_rest=1,
                          batch_size=512, verbose=False, device="cpu")
    assert len(calls) == 1
    ind = res.induction
    assert ind.pnl is not None and ind.pnl.count == 1024
    assert torch.isfinite(ind.pnl_paths).all()
