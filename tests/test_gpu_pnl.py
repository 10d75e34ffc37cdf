"""k_hedge_pnl (HipBackend.pnl: the self-financing P&L scan over the per-date
network snapshots) against the fp64 numpy recursion, on synthetic
``[n_dates + 1, n]`` feature / price tables - basket shapes, path counts around
the 1024 paths of a workgroup (256 threads x 4 paths) and 1 / 2 / 7 dates.

Bounds (u = 2^-24; derivation in test_gpu_eval.py): per path ``|pnl - ref| <=
32 n_dates u max|ref|`` - about 25 sequential roundings per date for the
8-unit nets, the wealth carried through every date; the statistics ``n x`` the
per-path tolerance ``+ 8 u sum|terms|`` (the kernel accumulates them in fp64).

The 32-unit nets are held to the same bound.

Largest per-path error measured on an MI355X over every case below, in
u max|ref| per date (bound 32): 7.9 for the 8-unit nets, 5.6 for the 32-unit nets.
"""
import numpy as np
import pytest
import torch

from test_gpu_eval import GUARD, SENTINEL, U, check_guards, f32, guarded, make_spec, make_weights  # noqa: F401
from test_gpu_kernels import dev  # noqa: F401  (fixture)
from test_pnl import _np_forward

pytestmark = pytest.mark.gpu

HOLD_C = 0.1
# (shape, two networks per date)
CASES = [((1, 8, 2, 0), False), ((1, 8, 1, 1), False), ((3, 8, 2, 0), True), ((5, 8, 6, 0), False),
         # the rest of the shape table (csrc/hedge_core.h): every shape reaches rph_pnl
         ((2, 8, 2, 0), False), ((4, 8, 2, 0), False), ((6, 8, 7, 0), True),
         ((1, 32, 1, 1), False), ((1, 32, 2, 0), False), ((2, 32, 2, 0), True), ((3, 32, 2, 0), False),
         ((5, 32, 6, 0), False)]
MAX_ULPS = [0.0]


def make_tables(spec, n, nd, has_b, seed):
    from rphedge.engine import MAXIN
    from rphedge.ops import layout as L

    g = torch.Generator().manual_seed(seed)
    na = spec.nhold - 1
    feats = [(f + 1) * (0.75 + 0.5 * torch.rand(nd + 1, n, generator=g)) for f in range(spec.nin)]
    prices = [(k + 1) * (0.8 + 0.4 * torch.rand(nd + 1, n, generator=g)) for k in range(na)]
    fmu = torch.zeros(nd, MAXIN)
    fisd = torch.ones(nd, MAXIN)
    for t in range(nd):
        for f in range(spec.nin):
            fmu[t, f] = (f + 1) * (1.0 + 0.02 * t)
            fisd[t, f] = (1.0 + 0.1 * f + 0.05 * t) / ((f + 1) * 0.15)
    # snapshots: the weights of (date, net) in w[0][:P]; every other float of the
    # block is NaN, so a read past the network poisons the result
    snap = torch.full((nd, 2, L.NETW_FLOATS), float("nan"))
    ws = np.zeros((nd, 2, spec.nparams), np.float32)
    for t in range(nd):
        for k in range(2 if has_b else 1):
            ws[t, k] = make_weights(spec, 100 + 2 * t + k)
            snap[t, k, :spec.nparams] = torch.from_numpy(ws[t, k])
    bond = torch.tensor([1.03 ** (0.7 * t) for t in range(nd + 1)], dtype=torch.float64)
    w0 = 0.8 + 0.4 * torch.rand(n, generator=g)
    payoff = torch.rand(n, generator=g)
    return dict(feats=feats, prices=prices, fmu=fmu, fisd=fisd, snap=snap, ws=ws, bond=bond, w0=w0, payoff=payoff)


def reference(spec, tb, nd, has_b):
    """fp64 recursion: W <- W g + sum_a h_a (S_a,t+1 - S_a,t g), g = fp32(B_t+1 / B_t)."""
    na = spec.nhold - 1
    W = tb["w0"].double().numpy().copy()
    bond = tb["bond"].numpy()
    alpha = f32(spec.alpha)
    for t in range(nd):
        X = np.stack([f[t].double().numpy() for f in tb["feats"]], axis=1)
        X = (X - tb["fmu"][t, :spec.nin].double().numpy()) * tb["fisd"][t, :spec.nin].double().numpy()
        h = _np_forward(spec, tb["ws"][t, 0].astype(np.float64), X, alpha)
        if has_b:
            hb = _np_forward(spec, tb["ws"][t, 1].astype(np.float64), X, alpha)
            h = h + f32(HOLD_C) * (hb - h)
        grow = f32(bond[t + 1] / bond[t])
        S0 = np.stack([p[t].double().numpy() for p in tb["prices"]], axis=1)
        S1 = np.stack([p[t + 1].double().numpy() for p in tb["prices"]], axis=1)
        W = W * grow + (h[:, :na] * (S1 - S0 * grow)).sum(axis=1)
    return W, W - tb["payoff"].double().numpy()


@pytest.mark.parametrize("nd", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2500])
@pytest.mark.parametrize("shape,has_b", CASES)
def test_pnl_scan_vs_fp64_recursion(dev, shape, has_b, n, nd):  # noqa: F811
    from rphedge.engine import HipBackend, PnlData, TrainConfig, reduce_stats
    from rphedge.ops import layout as L

    spec = make_spec(shape)
    tb = make_tables(spec, n, nd, has_b, seed=1000 * nd + n)
    be = HipBackend(spec, n, TrainConfig(batch_size=n), device=dev)
    feats = [f.to(dev) for f in tb["feats"]]
    prices = [p.to(dev) for p in tb["prices"]]
    data = PnlData(n_dates=nd, features=lambda t: [f[t] for f in feats], prices=lambda t: [p[t] for p in prices],
                   bond=tb["bond"].to(dev), fmu=tb["fmu"].to(dev), fisd=tb["fisd"].to(dev), w0=tb["w0"].to(dev),
                   payoff=tb["payoff"].to(dev))
    wgs = (n + 1023) // 1024
    assert be.pnl_wgs() == wgs
    slab = torch.full((wgs, L.EVAL_NSTAT), float("nan"), dtype=torch.float64, device=dev)
    buf, out = guarded(n, dev)
    be.pnl(tb["snap"].to(dev), data, slab, has_b=has_b, hold_c=HOLD_C if has_b else 0.0, pnl_out=out)
    torch.cuda.synchronize()

    W, pnl = reference(spec, tb, nd, has_b)
    tag = f"pnl {shape} n={n} nd={nd}"
    F = 32.0 * nd
    check_guards(tag, buf)
    got = out.cpu().numpy().astype(np.float64)
    scale = float(np.abs(pnl).max())
    tol_p, tol_w = F * U * scale, F * U * float(np.abs(W).max())
    err = float(np.abs(got - pnl).max())
    MAX_ULPS[0] = max(MAX_ULPS[0], err / (U * scale * nd))
    print(f"ULPS {tag}: {err / (U * scale):.3f} u max|ref| (bound {F:.0f}); per date so far max {MAX_ULPS[0]:.3f}")
    assert err <= tol_p, f"{tag}: max err {err:.3e} = {err / (U * scale):.2f} u max|ref| > {F:.0f}"

    raw = slab.cpu().numpy()
    assert not np.isnan(raw).any(), f"{tag}: statistics rows not overwritten"
    cnt = np.bincount(np.arange(n) // 1024, minlength=wgs)
    assert np.array_equal(raw[:, L.ES_COUNT], cnt.astype(np.float64))
    st = reduce_stats(slab)
    assert st[L.ES_COUNT] == n

    def lin(x, tol):
        return float(x.sum()), n * tol + 8 * U * float(np.abs(x).sum())

    def sq(x, tol):
        return float((x * x).sum()), n * (2 * float(np.abs(x).max()) * tol + tol * tol) + 8 * U * float((x * x).sum())

    want = {L.ES_V: lin(W, tol_w), L.ES_V2: sq(W, tol_w), L.ES_RES: lin(pnl, tol_p), L.ES_RES2: sq(pnl, tol_p),
            L.ES_ABSRES: lin(np.abs(pnl), tol_p)}
    for idx, (ref, tol) in want.items():
        assert abs(st[idx] - ref) <= tol, f"{tag}: statistic {idx}: {st[idx]!r} vs {ref!r} (tol {tol:.3e})"
    assert abs(st[L.ES_RESMIN] - pnl.min()) <= tol_p and abs(st[L.ES_RESMAX] - pnl.max()) <= tol_p
    others = [c for c in range(L.EVAL_NSTAT) if c not in (*want, L.ES_COUNT, L.ES_RESMIN, L.ES_RESMAX)]
    assert np.all(raw[:, others] == 0.0)
