"""k_sim_scan_pair (native.simulate_pair): the run's scan and the LM Gram
subsample's scan in one launch against two separate launches into separate
buffers - every thread runs the scan it runs alone, so every output tensor is
bitwise equal.  One case whose descriptors select different instantiations
(ALIGNED) must come back as two launches, equal all the same."""
import pytest
import torch

from test_gpu_kernels import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SUB = dict(n=512, index_map=(64, 1024))  # the subsample: the first 64 paths of 8 global blocks of 1024


def _scan(model, grid, n, offset, index_map, dev, defer=None):  # noqa: F811
    from rphedge.ops import paths as P

    kw = dict(device=dev, offset=offset, index_map=index_map, defer=defer)
    if model == "gbm_log":
        return P.simulate_gbm(grid, n, 100.0, 0.05, 0.2, scheme="log", norm=100.0, **kw)
    return P.simulate_sv(grid, n, 100.0, 0.05, 0.04, model="heston", kappa=2.0, theta=0.04, xi=0.5, rho=-0.7,
                         norm=100.0, scheme="qe", **kw)


def _tensors(p):
    return [t for t in (p.S, p.S_final, p.vol) if t is not None]


@pytest.mark.parametrize("model,rebalancing,n_main,merged", [
    ("gbm_log", 0.25, 4096, True),    # 3 dates x 2 substeps
    ("heston", 0.375, 4096, True),    # 2 dates x 3 substeps, Andersen QE
    ("gbm_log", 0.25, 4100, False),   # main not ALIGNED, subsample ALIGNED: two launches
])
def test_pair_launch_equals_two_launches(dev, model, rebalancing, n_main, merged):  # noqa: F811
    from rphedge.ops import native
    from rphedge.ops import paths as P

    grid = P.Grid(T=0.75, dt=0.125, rebalancing=rebalancing)
    assert (grid.n_fine, grid.n_coarse) == (7, {0.25: 4, 0.375: 3}[rebalancing])
    ref_main = _scan(model, grid, n_main, 8192, None, dev)
    ref_sub = _scan(model, grid, SUB["n"], 0, SUB["index_map"], dev)
    descs = []
    main = _scan(model, grid, n_main, 8192, None, dev, defer=descs)
    sub = _scan(model, grid, SUB["n"], 0, SUB["index_map"], dev, defer=descs)
    for p in (main, sub):  # (deferred: nothing launched yet - poison what the launch must fill)
        for t in _tensors(p):
            t.fill_(float("nan"))
    assert len(descs) == 2
    assert native.simulate_pair(descs[0], descs[1]) is merged
    torch.cuda.synchronize()
    for got, ref in ((main, ref_main), (sub, ref_sub)):
        assert len(_tensors(got)) == len(_tensors(ref)) == (3 if model == "heston" else 2)
        for a, b in zip(_tensors(got), _tensors(ref)):
            assert a.data_ptr() != b.data_ptr() and torch.isfinite(b).all()
            assert torch.equal(a, b)
    assert not torch.equal(main.S[-1, :512], sub.S[-1])  # (two different path sets)
