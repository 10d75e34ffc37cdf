"""k_payoff (native.payoff), k_radix_hist (native.radix_hist) and the radix-
select quantile (risk.quantile) against numpy.

* payoff kinds 0-2 (guarantee, call, put) are one correctly rounded fp32
  operation after a comparison: bitwise equal to numpy in float32, inputs at
  the strike and one ulp beside it included;
* the basket call sums na fused multiply-adds: within ``na 2^-24 sum|w S|`` of
  the fp64 result;
* histogram counts are integers: equal exactly to the CPU branch of
  ``risk._hist_pass`` for every radix pass, with an empty prefix and with the
  prefix of a value from the data (signs mixed, +-0, denormals, +-inf, ties);
* quantiles are exact where one order statistic is selected; where two are
  interpolated (in double, like numpy, but in a different association) within
  one fp32 ulp of numpy's result.

Measured on an MI355X: basket error at most 1.7 x 2^-24 sum|w S| (na = 6,
bound 6); every interpolated quantile equal to numpy's.
"""
import numpy as np
import pytest
import torch

from test_gpu_eval import check_guards, guarded
from test_gpu_kernels import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _at_strike(x: np.ndarray, strike: np.float32):
    """Plant the strike itself and its two fp32 neighbours in the data."""
    k = np.float32(strike)
    edge = [k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))]
    for i, v in enumerate(edge):
        if i < x.size:
            x[(i * 97) % x.size] = v
    return x


@pytest.mark.parametrize("strike", [1.0, 1.1])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_payoff_single_asset_kinds_bitwise(dev, n, strike):  # noqa: F811
    from rphedge.ops import native

    rng = np.random.default_rng(n)
    k = np.float32(strike)  # (the kernel takes the strike as a float)
    if n >= 3:
        variants = [_at_strike((0.5 + rng.random(n)).astype(np.float32), k)]
    else:  # one path: the strike and each neighbour in turn
        variants = [np.full(n, v, np.float32) for v in
                    (k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf)))]
    for s in variants:
        nfrac = (0.8 + 0.2 * rng.random(n)).astype(np.float32)
        sd, nd_ = torch.from_numpy(s).to(dev), torch.from_numpy(nfrac).to(dev)
        floor = np.where(s > k, s, k).astype(np.float32)
        want = {(0, True): floor * nfrac, (0, False): floor,
                (1, False): np.maximum(s - k, np.float32(0)), (2, False): np.maximum(k - s, np.float32(0))}
        for (kind, with_n), ref in want.items():
            buf, out = guarded(n, dev)
            native.payoff(kind, sd, out, strike, nfrac=nd_ if with_n else None)
            torch.cuda.synchronize()
            check_guards(f"payoff kind {kind}", buf)
            got = out.cpu().numpy()
            assert ref.dtype == np.float32
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (kind, with_n, n, strike)


@pytest.mark.parametrize("na", [1, 5, 6])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_payoff_basket_vs_fp64(dev, n, na):  # noqa: F811
    from rphedge.ops import native

    rng = np.random.default_rng(10 * n + na)
    w = (rng.random(na) + 0.5).astype(np.float32)
    w /= w.sum()
    s = ((np.arange(na)[:, None] + 1) * (0.6 + 0.8 * rng.random((na, n)))).astype(np.float32)
    strike = np.float32(0.5 * (na + 1))  # near the basket mean: both branches
    # some paths exactly at the strike (every asset K / sum w where that is exact) and just beside it
    if n > 3:
        for j, v in enumerate([strike, np.nextafter(strike, np.float32(np.inf)),
                               np.nextafter(strike, np.float32(-np.inf))]):
            s[:, j] = v
    buf, out = guarded(n, dev)
    native.payoff(3, torch.from_numpy(s).to(dev), out, float(strike), wts=torch.from_numpy(w).to(dev), na=na)
    torch.cuda.synchronize()
    check_guards("payoff basket", buf)
    terms = w.astype(np.float64)[:, None] * s.astype(np.float64)
    ref = np.maximum(terms.sum(axis=0) - float(strike), 0.0)
    tol = na * U * np.abs(terms).sum(axis=0)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print(f"basket na={na} n={n}: max err / (2^-24 sum|wS|) = {(err / (tol / na)).max():.3f} (bound {na})")
    assert np.all(err <= tol), (err / tol).max()
    if n > 3:
        assert (ref == 0).any() and (ref > 0).any()


def _mixed_data(n: int, seed: int) -> np.ndarray:
    """Signs mixed, +-0, denormals, +-inf and long runs of ties."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) ** 3).astype(np.float32)
    if n >= 255:
        x[10:60] = np.float32(0.25)              # a run of ties ...
        x[60:90] = np.float32(-1.5)
        x[n // 2:n // 2 + n // 5] = x[5]         # ... and a long one of a value from the data
        x[100], x[101] = np.float32(0.0), np.float32(-0.0)
        x[102:106] = np.array([1e-45, -1e-45, 1e-39, -1e-39], np.float32)  # denormals
        x[106], x[107] = np.float32(np.inf), np.float32(-np.inf)
        x[108], x[109] = np.finfo(np.float32).max, np.finfo(np.float32).min
    return x


HIST_SIZES = [1, 255, 256, 257, 2048 * 256 + 5]  # (the last: the grid-stride loop wraps)


@pytest.mark.parametrize("n", HIST_SIZES)
def test_radix_hist_counts_equal_cpu(dev, n):  # noqa: F811
    from rphedge import risk
    from rphedge.ops import native

    x = _mixed_data(n, seed=n)
    xc = torch.from_numpy(x)
    xd = xc.to(dev)
    b = x.view(np.uint32)
    keys = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    pmask = 0
    for shift, nbins in risk._PASSES:
        # empty prefix, and the prefixes (the key bits above this pass) of values from the data
        picks = [n // 2, 5 % n, 100 % n, (n - 1)]
        cases = [(0, 0)] + ([(pmask, int(keys[i]) & pmask) for i in picks] if pmask else [])
        for pm, pf in dict.fromkeys(cases):
            h = torch.zeros(nbins, dtype=torch.int32, device=dev)
            native.radix_hist(xd, pm, pf, shift, nbins, h)
            torch.cuda.synchronize()
            ref = risk._hist_pass(xc, pm, pf, shift, nbins, 1)
            got = h.cpu().numpy().astype(np.int64)
            assert np.array_equal(got, ref), (n, shift, hex(pm), hex(pf))
            if pm == 0:
                assert got.sum() == n
            else:
                assert got.sum() >= 1
        pmask |= (nbins - 1) << shift


QS = (0.0, 0.5, 0.985, 0.99, 0.995, 1.0)


@pytest.mark.parametrize("n", HIST_SIZES)
def test_quantile_matches_numpy(dev, n):  # noqa: F811
    from rphedge import risk

    x = _mixed_data(n, seed=n)
    x = x[np.isfinite(x)] if n > 1 else x      # (inf - finite interpolates to nan in numpy)
    n = x.size
    got = risk.quantile(torch.from_numpy(x).to(dev), QS)
    xs = np.sort(x.astype(np.float64))
    ref = np.quantile(x.astype(np.float64), QS)
    worst = 0.0
    for q, g_, r in zip(QS, got, ref):
        h = (n - 1) * q
        lo = int(np.floor(h))
        if h == lo or lo + 1 >= n:
            assert g_ == xs[lo] == r, (n, q, g_, r)  # one order statistic: exact
        else:
            # two order statistics a, b: a + t (b - a) here, numpy's lerp switches to b - (b - a)(1 - t)
            # at t >= 0.5; both in double, so they agree far inside one fp32 ulp of the result (the
            # floor: a double rounding of the larger of the two, where the result cancels to ~0)
            tol = max(float(np.spacing(np.float32(abs(r)))), 2.0 ** -50 * max(abs(xs[lo]), abs(xs[lo + 1])))
            assert abs(g_ - r) <= tol, (n, q, g_, r, tol)
            if r != 0:
                worst = max(worst, abs(g_ - r) / abs(r))
    print(f"quantile n={n}: interpolated quantiles at most {worst:.2e} relative off numpy")


def test_quantile_extremes_with_infinities(dev):  # noqa: F811
    """With +-inf in the data only the single order statistics are defined: q = 0 and q = 1."""
    from rphedge import risk

    x = _mixed_data(1000, seed=3)
    got = risk.quantile(torch.from_numpy(x).to(dev), (0.0, 1.0))
    assert got[0] == -np.inf and got[1] == np.inf
