"""The SV / Heston, basket and mortality branches of csrc/paths.hip and the
stand-alone Sobol kernel, path by path against the fp64 numpy twins of
rphedge/ops/paths.py (``_cpu_sv``, ``_cpu_basket``, ``_cpu_mortality``,
``sobol_norm_cpu``) - on every instantiation (fp32 / fp64, ALIGNED or not,
basket widths 1..6) and at path indices up to 2^30 - 1 (gray-code bits 20..29).

Path ranges ``(n, offset, index_map)`` and the fold each selects (sim_aligned):

    R1 (1, 0)              unaligned, tail block
    R2 (257, 64)           unaligned by n
    R3 (512, 37)           unaligned by offset only
    R4 (2051, 37)          unaligned, many blocks
    R5 (512, 0, (64, 1024))  aligned with a map
    R6 (300, 0, (50, 1000))  unaligned map
    R7 (512, 2^30 - 512)   aligned, gray bits up to 29
    R8 (300, 2^30 - 300)   unaligned, gray bits up to 29
    R9 (2048, 0)           aligned baseline

Bounds.  fp64 recursions: rtol 1e-5 / atol 1e-6 (SV, Heston: the bound of
``test_sv_and_heston_vs_numpy``), survivor counts exactly, lambda rtol 1e-6.
Basket (fp32 only): rtol 2e-4 as in ``test_basket_vs_numpy``.

fp32 SV / Heston (the production precision) has no fixed bound: it is sized by
``_emu_sv_f32``, a float32 numpy emulation of the kernel's recursion (float32
state and constants, ``ndtri_u30_f32`` normals).  The emulation is never the
reference - only its distance to the fp64 twin is used.  Per parameter set and
grid, over the points of all ranges pooled (a rounding bound belongs to the
arithmetic, not to the choice of paths, and the 9 points of R1 cannot size
one): e_max and e_99.9 are the emulation's largest and 99.9th-percentile error
(relative for S, absolute for the variance).  The kernel has to stay within
4 e_max on every point and within 4 e_99.9 on 99.9 % of the points.  The 4:
two independent fp32 evaluations of one recursion may each be e away from the
exact result (2); the kernel also contracts to FMA and takes ``__logf`` in
ndtri, which numpy does not, and these differences random-walk over the up to
100 steps (another 2).

fp32 mortality: lambda rtol 1e-5; the survivor count may differ from the
twin's by one on at most 0.2 % of the (date, path) points (a float32 emulation
of the lambda recursion flips none of 2051 x 8), never by more.

Measured on an MI355X (fp32 kernel against the twin | the emulation's e_max /
e_99.9; the bounds are 4 x those), grid GA = Grid(2, 1/50, 1/4), nine ranges
pooled, and GB = Grid(1, 1/32, 1/8), R4 + R9:

    case              grid  S rel: kernel max  p99.9 | e_max    e_99.9    variance abs: max  p99.9 | e_max    e_99.9
    sv_ref            GA    5.38e-06  4.03e-06 | 5.38e-06 4.03e-06    1.71e-07  1.39e-07 | 1.71e-07 1.39e-07
    sv_ref            GB    2.95e-06  2.30e-06 | 2.87e-06 2.30e-06    1.24e-07  9.12e-08 | 1.24e-07 9.10e-08
    sv_ref tscale 252 GA    5.66e-06  3.82e-06 | 5.66e-06 3.91e-06    2.78e-07  1.40e-07 | 2.14e-07 1.40e-07
    sv_ref tscale 252 GB    3.14e-06  2.27e-06 | 2.95e-06 2.21e-06    1.39e-07  1.01e-07 | 1.41e-07 1.04e-07
    heston euler      GA    5.13e-06  3.84e-06 | 5.16e-06 3.91e-06    7.57e-08  4.31e-08 | 7.36e-08 4.11e-08
    heston euler      GB    3.15e-06  2.27e-06 | 3.15e-06 2.28e-06    4.51e-08  3.25e-08 | 5.08e-08 2.96e-08
    heston qe xi 0.3  GA    5.83e-06  4.68e-06 | 5.75e-06 4.73e-06    1.66e-07  9.11e-08 | 2.72e-07 1.38e-07
    heston qe xi 0.3  GB    2.69e-06  2.33e-06 | 2.59e-06 2.31e-06    9.45e-08  6.50e-08 | 1.34e-07 7.15e-08
    heston qe xi 0.9  GA    1.26e-04  6.34e-06 | 8.01e-05 6.55e-06    1.07e-04  4.55e-06 | 6.87e-05 4.79e-06
    heston qe xi 0.9  GB    2.30e-05  5.31e-06 | 2.30e-05 5.92e-06    2.00e-05  1.37e-06 | 1.91e-05 2.62e-06

The kernel's worst point uses 0.39 of its 4 e_max bound (xi 0.9, GA); the
smallest share of points inside 4 e_99.9 is 99.969 % (xi 0.9, GA, S; 99.9 %
required).  The twin's variance is exactly 0 on 45 - 48 % of the stored points
of the xi 0.9 case, and 47 % of the terminal values of the c = 0.5 parity run
are NaN.  fp64 mortality: lambda at most 5.1e-08 relative off the twin, every
survivor count equal; fp32: lambda 1.4e-06, no count differs (of 20510 points
at R4).  Normal branch: every count equal at n0 = 100000 and n0 = 80000
(72 - 94 % of the paths per step in the normal branch).  Basket: at most
2.8e-06 relative off the twin over NA = 1..6 (bound 2e-4).
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_eval import check_guards, guarded
from test_gpu_kernels import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F = np.float32
END = 1 << 30
RANGES = {
    "R1": (1, 0, None), "R2": (257, 64, None), "R3": (512, 37, None), "R4": (2051, 37, None),
    "R5": (512, 0, (64, 1024)), "R6": (300, 0, (50, 1000)), "R7": (512, END - 512, None),
    "R8": (300, END - 300, None), "R9": (2048, 0, None),
}
ALIGNED = {"R1": False, "R2": False, "R3": False, "R4": False, "R5": True, "R6": False, "R7": True, "R8": False,
           "R9": True}
GRIDS = {"GA": (2.0, 1 / 50, 0.25), "GB": (1.0, 1 / 32, 1 / 8), "GM": (2.0, 1 / 100, 0.25),
         "GN": (2.0, 0.25, 0.5), "GK": (1.0, 1 / 20, 1 / 10)}
S0, MU, NORM = 100.0, 0.09, 100.0
SV_CASES = {
    "sv_ref": ("sv_ref", 0.16, dict(a=0.0034, b=0.154, c=0.0158)),
    "sv_ref_tscale252": ("sv_ref", 0.16, dict(a=0.0034, b=0.154, c=0.0158, sv_tscale=252.0)),
    "heston_euler": ("heston", 0.04, dict(kappa=2.0, theta=0.04, xi=0.3, rho=-0.7, scheme="euler")),
    "heston_qe_xi03": ("heston", 0.04, dict(kappa=2.0, theta=0.04, xi=0.3, rho=-0.7, scheme="qe")),
    "heston_qe_xi09": ("heston", 0.04, dict(kappa=1.0, theta=0.04, xi=0.9, rho=-0.5, scheme="qe")),
}
LAM = (0.01, 0.075, 0.000597)   # l0, c, eta of the reference


def grid(key):
    from rphedge.ops.paths import Grid

    return Grid(*GRIDS[key])


def gidx(rk):
    from rphedge.ops.paths import path_indices

    return path_indices(*RANGES[rk]).astype(np.int64)


def frozen(*arrays):
    out = tuple(np.ascontiguousarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def test_ranges_and_grids_are_what_the_cases_assume():
    for rk, (n, off, m) in RANGES.items():
        al = n % 256 == 0 and off % 64 == 0 and (m is None or (m[0] % 64 == 0 and m[1] % 64 == 0))
        assert al == ALIGNED[rk], rk
        assert 0 <= gidx(rk).min() and gidx(rk).max() < END
    assert gidx("R7").max() == gidx("R8").max() == END - 1
    assert (gidx("R7") ^ (gidx("R7") >> 1)).max() >> 29 == 1   # gray bit 29 is set
    ga, gb = grid("GA"), grid("GB")
    assert (ga.n_fine, ga.reduction, ga.n_coarse) == (101, 12, 9) and (ga.n_coarse - 1) * ga.reduction == 96
    assert (gb.n_fine, gb.reduction, gb.n_coarse) == (33, 4, 9) and (gb.n_coarse - 1) * gb.reduction == gb.n_fine - 1
    gm, gn, gk = grid("GM"), grid("GN"), grid("GK")
    assert (gm.n_fine, gm.reduction, gm.n_coarse) == (201, 25, 9)
    assert (gn.n_fine, gn.reduction, gn.n_coarse) == (9, 2, 5)
    assert (gk.n_fine, gk.reduction, gk.n_coarse) == (21, 2, 11)


# ---------------------------------------------------------------------------
# SV / Heston
# ---------------------------------------------------------------------------
_SV_TWIN, _SV_EMU = {}, {}


def _sv_twin(case, gk, rk, parity_nan=False, **over):
    """fp64 twin, normalised: (S [n_coarse, n], variance, S_final); once per case, read-only."""
    from rphedge.ops import paths as P

    key = (case, gk, rk, parity_nan, tuple(sorted(over.items())))
    if key not in _SV_TWIN:
        model, v0, kw = SV_CASES[case]
        kw = dict(kw, **over)
        n, off, m = RANGES[rk]
        with np.errstate(invalid="ignore"):
            S, V, fin = P._cpu_sv(grid(gk), n, S0, MU, v0, model, kw.get("a", 0.0), kw.get("b", 0.0), kw.get("c", 0.0),
                                  kw.get("kappa", 0.0), kw.get("theta", 0.0), kw.get("xi", 0.0), kw.get("rho", 0.0),
                                  off, parity_nan, P.SEED_W1, P.SEED_W2, scheme=kw.get("scheme", "qe"),
                                  sv_tscale=kw.get("sv_tscale", 0.0), index_map=m)
        _SV_TWIN[key] = frozen(S / NORM, V, fin / NORM)
    return _SV_TWIN[key]


def _emu_sv_f32(g, n, off, m, model, v0, kw):
    """float32 numpy emulation of k_sim_scan<float, *, SIM_SV_REF | SIM_HESTON>
    (normalised S, variance, S_final).  Sizes the fp32 tolerance only."""
    from rphedge.ops import paths as P
    from rphedge.ops.ndtri import ndtri_u30_f32

    nf = g.n_fine
    tsc = float(kw.get("sv_tscale", 0.0))
    if model == "heston" or tsc > 0:   # one 2 n_fine-dimensional sequence (simulate_sv)
        X = P._u30(2 * nf, P.SEED_W1, n, off, 2 * nf, m)
        X1, X2 = X[:, :nf], X[:, nf:]
    else:
        X1, X2 = P._u30(nf, P.SEED_W1, n, off, nf, m), P._u30(nf, P.SEED_W2, n, off, nf, m)
    Z1, Z2 = ndtri_u30_f32(X1), ndtri_u30_f32(X2)
    assert Z1.dtype == Z2.dtype == F
    one, two, half = F(1), F(2), F(0.5)
    dt, mu = F(g.dt), F(MU)
    sdt = np.sqrt(dt)
    a, b, c = (F(kw.get(k, 0.0)) for k in ("a", "b", "c"))
    kap, th, xi, rho = (F(kw.get(k, 0.0)) for k in ("kappa", "theta", "xi", "rho"))
    rhoc = np.sqrt(one - rho * rho)
    qe = model == "heston" and kw.get("scheme", "qe") == "qe"
    if qe:
        ekd = np.exp(-kap * dt)
        qc1 = xi * xi * ekd * (one - ekd) / kap
        qc2 = th * xi * xi * (one - ekd) * (one - ekd) / (two * kap)
        qK1 = half * dt * (kap * rho / xi - half) - rho / xi
        qK2 = half * dt * (kap * rho / xi - half) + rho / xi
        qK3 = half * dt * (one - rho * rho)
        qA = qK2 + half * qK3
        qK0u = -rho * kap * th * dt / xi
    tau = F(tsc) * dt
    inv0 = F(1.0 / NORM)
    ly = np.full(n, np.log(F(S0)), F)
    v = np.full(n, F(v0), F)
    S = np.empty((g.n_coarse, n), F)
    V = np.empty((g.n_coarse, n), F)
    S[0], V[0] = F(S0) * inv0, F(v0)
    zero = F(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, nf):
            z1, z2 = Z1[:, t], Z2[:, t]
            if model == "sv_ref" and tsc > 0:
                vp = np.maximum(v, zero)
                ly = ly + ((mu - half * vp * vp) * dt + vp * sdt * z1)
                v = v + a * (b - vp) * tau + c * np.sqrt(vp * tau) * z2
            elif model == "sv_ref":
                sq = np.sqrt(np.maximum(v * dt, zero))
                v = v + a * (b - v) + c * sq * z2
                ly = ly + ((mu - half * v * v) * dt + v * sdt * z1)
            elif qe:
                mm = th + (v - th) * ekd
                psi = (v * qc1 + qc2) / (mm * mm)
                ip = two / psi
                b2 = ip - one + np.sqrt(ip) * np.sqrt(ip - one)
                qa = mm / (one + b2)
                bz = np.sqrt(b2) + z2
                vq = qa * bz * bz
                den = one - two * qA * qa
                k0q = np.where(den > zero, -qA * b2 * qa / den + half * np.log(den) - (qK1 + half * qK3) * v, qK0u)
                p = (psi - one) / (psi + one)
                beta = (one - p) / mm
                u = X2[:, t].astype(F) * F(2.0 ** -30)
                ve = np.where(u <= p, zero, np.log((one - p) / (one - u)) / beta)
                k0e = np.where(beta > qA, -np.log(p + beta * (one - p) / (beta - qA)) - (qK1 + half * qK3) * v, qK0u)
                quad = psi <= F(1.5)
                vn = np.where(quad, vq, ve).astype(F)
                k0 = np.where(quad, k0q, k0e).astype(F)
                var = qK3 * (v + vn)
                ly = ly + (mu * dt + k0 + qK1 * v + qK2 * vn + np.sqrt(np.maximum(var, zero)) * z1)
                v = vn
            else:
                vp = np.maximum(v, zero)
                sv = np.sqrt(vp * dt)
                ly = ly + ((mu - half * vp) * dt + sv * (rho * z2 + rhoc * z1))
                v = v + kap * (th - vp) * dt + xi * sv * z2
            assert ly.dtype == F and v.dtype == F
            if t % g.reduction == 0 and t // g.reduction < g.n_coarse:
                S[t // g.reduction] = np.exp(ly) * inv0
                V[t // g.reduction] = v
    return S, V, np.exp(ly) * inv0


def _errors(S, V, fin, ref):
    """(relative errors of S and S_final, absolute errors of the variance) against the twin, flattened."""
    rS, rV, rfin = ref
    S, V, fin = (np.asarray(x, np.float64) for x in (S, V, fin))
    return (np.concatenate([np.abs(S / rS - 1).ravel(), np.abs(fin / rfin - 1).ravel()]), np.abs(V - rV).ravel())


def _sv_emu_errors(case, gk, rk):
    key = (case, gk, rk)
    if key not in _SV_EMU:
        model, v0, kw = SV_CASES[case]
        _SV_EMU[key] = frozen(*_errors(*_emu_sv_f32(grid(gk), *RANGES[rk], model, v0, kw), _sv_twin(case, gk, rk)))
    return _SV_EMU[key]


def _sv_paths(P, g, rk, dev, kind):  # noqa: F811
    """A Paths whose S, variance and S_final sit between guard bands."""
    n, off, m = RANGES[rk]
    bufs = [guarded(g.n_coarse * n, dev), guarded(g.n_coarse * n, dev), guarded(n, dev)]
    p = P.Paths(kind=kind, grid=g, n_local=n, path_offset=off, S=bufs[0][1].view(g.n_coarse, n), bond=g.bond(0.0),
                S_final=bufs[2][1], vol=bufs[1][1].view(g.n_coarse, n), norm=NORM)
    return p, [b for b, _ in bufs]


def _run_sv(P, case, gk, rk, dev, fp64, parity_nan=False, **over):  # noqa: F811
    model, v0, kw = SV_CASES[case]
    n, off, m = RANGES[rk]
    g = grid(gk)
    out, bufs = _sv_paths(P, g, rk, dev, "heston" if model == "heston" else "sv")
    p = P.simulate_sv(g, n, S0, MU, v0, model=model, norm=NORM, device=dev, offset=off, fp64=fp64,
                      parity_nan=parity_nan, index_map=m, out=out, **dict(kw, **over))
    torch.cuda.synchronize()
    assert p is out
    for name, b in zip(("S", "vol", "S_final"), bufs):
        check_guards(f"{case} {rk} {name}", b)
    S, V, fin = p.S.cpu().numpy(), p.vol.cpu().numpy(), p.S_final.cpu().numpy()
    if not parity_nan:
        assert np.all(S[0] == F(S0) * F(1.0 / NORM)) and np.all(V[0] == F(v0)), (case, gk, rk)
    return S, V, fin


@pytest.mark.parametrize("case", list(SV_CASES))
def test_sv_heston_scans_vs_twin(dev, case):  # noqa: F811
    from rphedge.ops import paths as P

    for gk, rks in (("GA", list(RANGES)), ("GB", ["R4", "R9"])):
        emu_s, emu_v, got_s, got_v = [], [], [], []
        for rk in rks:
            ref = _sv_twin(case, gk, rk)
            assert all(np.all(np.isfinite(x)) for x in ref)
            if case == "heston_qe_xi09" and RANGES[rk][0] > 1:
                # the exponential branch and its point mass at 0 are exercised
                assert np.mean(ref[1] == 0.0) > 0.10, (gk, rk, np.mean(ref[1] == 0.0))
            S, V, fin = _run_sv(P, case, gk, rk, dev, fp64=True)
            tag = f"{case} {gk} {rk} fp64"
            np.testing.assert_allclose(S, ref[0], rtol=1e-5, atol=1e-6, err_msg=tag)
            np.testing.assert_allclose(V, ref[1], rtol=1e-5, atol=1e-6, err_msg=tag)
            np.testing.assert_allclose(fin, ref[2], rtol=1e-5, atol=1e-6, err_msg=tag)
            ks, kv = _errors(*_run_sv(P, case, gk, rk, dev, fp64=False), ref)
            es, ev = _sv_emu_errors(case, gk, rk)
            print(f"{case} {gk} {rk} fp32: S rel max {ks.max():.2e} (emulation {es.max():.2e}), "
                  f"variance abs max {kv.max():.2e} (emulation {ev.max():.2e})")
            emu_s.append(es), emu_v.append(ev), got_s.append(ks), got_v.append(kv)
        for name, emu, got in (("S rel", emu_s, got_s), ("variance abs", emu_v, got_v)):
            emu, got = np.concatenate(emu), np.concatenate(got)
            e_max, e_999 = float(emu.max()), float(np.quantile(emu, 0.999))
            k_max, k_999 = float(got.max()), float(np.quantile(got, 0.999))
            inside = float(np.mean(got <= 4 * e_999))
            print(f"FP32 {case} {gk} {name}: kernel max {k_max:.2e} p99.9 {k_999:.2e} | emulation e_max {e_max:.2e} "
                  f"e_99.9 {e_999:.2e} | bounds {4 * e_max:.2e} / {4 * e_999:.2e}, {100 * inside:.3f} % inside")
            assert np.isfinite(e_max) and e_max > 0
            assert k_max <= 4 * e_max, (case, gk, name, k_max, e_max)
            assert inside >= 0.999, (case, gk, name, inside, e_999)


@pytest.mark.parametrize("rk", ["R4", "R9"])
def test_sv_parity_nan_mask(dev, rk):  # noqa: F811
    """The reference recursion with c = 0.5 drives v below 0: sqrt(v dt) is NaN
    with parity_nan (as numpy's in the reference), clamped without it."""
    from rphedge.ops import paths as P

    ref = _sv_twin("sv_ref", "GA", rk, parity_nan=True, c=0.5)
    S, V, fin = _run_sv(P, "sv_ref", "GA", rk, dev, fp64=True, parity_nan=True, c=0.5)
    share = float(np.mean(np.isnan(ref[2])))
    print(f"parity NaN {rk}: {100 * share:.1f} % of the terminal values are NaN")
    assert 0.02 < share < 0.98
    for name, got, r in zip(("S", "vol", "S_final"), (S, V, fin), ref):
        assert np.array_equal(np.isnan(got), np.isnan(r)), name
        ok = ~np.isnan(r)
        assert np.all(np.isfinite(got[ok]))
        np.testing.assert_allclose(got[ok], r[ok], rtol=1e-5, atol=1e-6, err_msg=name)
    assert np.all(S[0] == F(S0) * F(1.0 / NORM))
    ref = _sv_twin("sv_ref", "GA", rk, parity_nan=False, c=0.5)
    assert (ref[1] < 0).any()
    for name, got, r in zip(("S", "vol", "S_final"), _run_sv(P, "sv_ref", "GA", rk, dev, fp64=True, c=0.5), ref):
        assert np.all(np.isfinite(got)), name
        np.testing.assert_allclose(got, r, rtol=1e-5, atol=1e-6, err_msg=name)


# ---------------------------------------------------------------------------
# mortality
# ---------------------------------------------------------------------------
_MORT_TWIN = {}


def _mort_twin(gk, rk, n0, q3):
    """(survivors [n_coarse, n] int64, lambda, survivors at the last fine point, normal-branch share per step)"""
    from rphedge.ops import paths as P

    key = (gk, rk, n0, q3)
    if key not in _MORT_TWIN:
        n, off, m = RANGES[rk]
        share = []
        nf, lm, nt = P._cpu_mortality(grid(gk), n, *LAM, n0, q3, off, P.SEED_W2, 1234, False, m, branch_share=share)
        N, NT = np.rint(nf * n0).astype(np.int64), np.rint(nt * n0).astype(np.int64)
        assert np.abs(nf * n0 - N).max() < 1e-6
        _MORT_TWIN[key] = frozen(N, lm, NT, np.asarray(share))
    return _MORT_TWIN[key]


def _run_mortality(P, gk, rk, dev, n0, q3, fp64):  # noqa: F811
    """(survivor counts, lambda, terminal counts) of the kernel; outputs between guard bands."""
    n, off, m = RANGES[rk]
    g = grid(gk)
    bufs = [guarded(g.n_coarse * n, dev), guarded(g.n_coarse * n, dev), guarded(n, dev)]
    p = P.Paths(kind="gbm", grid=g, n_local=n, path_offset=off, S=torch.empty(1, n, device=dev), bond=g.bond(0.0),
                S_final=torch.empty(n, device=dev), nfrac=bufs[0][1].view(g.n_coarse, n),
                lam=bufs[1][1].view(g.n_coarse, n))
    p.meta["index_map"], p.meta["nfrac_final_buf"] = m, bufs[2][1]
    P.simulate_mortality(p, *LAM, n0, lambda_fine_index=q3, fp64=fp64)
    torch.cuda.synchronize()
    assert p.nfrac.data_ptr() == bufs[0][1].data_ptr() and p.nfrac_final.data_ptr() == bufs[2][1].data_ptr()
    for name, (b, _) in zip(("nfrac", "lam", "nfrac_final"), bufs):
        check_guards(f"mortality {rk} {name}", b)
    out = []
    for x in (p.nfrac, p.nfrac_final):
        x = x.cpu().numpy().astype(np.float64) * n0
        assert np.abs(x - np.rint(x)).max() < 0.02 * max(1.0, n0 / 10000)   # a count times float32(1 / n0)
        out.append(np.rint(x).astype(np.int64))
    return out[0], p.lam.cpu().numpy().astype(np.float64), out[1]


@pytest.mark.parametrize("rk", ["R2", "R3", "R4", "R7", "R9"])
def test_mortality_survivors_vs_twin(dev, rk):  # noqa: F811
    from rphedge.ops import paths as P

    n0 = 10000
    g = grid("GM")
    lam_runs = {}
    for q3 in (False, True):
        N, lam, NT, share = _mort_twin("GM", rk, n0, q3)
        assert share.max() == 0.0 and N.min() > 0 and (N[-1] < n0).all()
        for fp64 in (True, False):
            gN, glam, gNT = _run_mortality(P, "GM", rk, dev, n0, q3, fp64)
            tag = f"mortality {rk} fine_index={q3} fp64={fp64}"
            assert np.all(gN[0] == n0) and np.all(glam[0] == F(LAM[0])), tag
            dN = np.abs(np.concatenate([(gN - N).ravel(), gNT - NT]))
            print(f"{tag}: lambda rel err {np.abs(glam / lam - 1).max():.2e}, |dN| max {dN.max()}, "
                  f"{int((dN > 0).sum())} of {dN.size} points differ")
            if fp64:
                np.testing.assert_allclose(glam, lam, rtol=1e-6, atol=0, err_msg=tag)
                assert dN.max() == 0, tag
            else:
                np.testing.assert_allclose(glam, lam, rtol=1e-5, atol=0, err_msg=tag)
                assert dN.max() <= 1, tag
                assert np.mean(dN > 0) <= 0.002, tag
            lam_runs[q3, fp64] = glam
    # Q3: lam[t], 1 <= t < n_coarse, is lambda at FINE point t - not the subsampled one
    for fp64 in (True, False):
        a, b = lam_runs[False, fp64], lam_runs[True, fp64]
        assert np.array_equal(a[0], b[0]) and g.n_coarse > 2
        for t in range(1, g.n_coarse):
            assert not np.array_equal(a[t], b[t]), t
    # and lambda at fine point 1 moved less than at coarse date 1 (25 fine steps later)
    assert np.abs(lam_runs[True, True][1] - LAM[0]).max() < np.abs(lam_runs[False, True][1] - LAM[0]).max()


@pytest.mark.parametrize("rk", ["R3", "R9"])
def test_mortality_normal_branch_vs_twin(dev, rk):  # noqa: F811
    """From N q >= 200 expected deaths per step the kernel draws the rounded
    normal approximation; the twin follows the same rule, so the counts agree
    exactly (the twin's un-rounded value is never within 3e-5 of an integer on
    these inputs, and the device and host ndtri agree to 1e-12)."""
    from rphedge.ops import paths as P

    # n0 = 100000: N q ~ 250, the normal branch in every step (one path of 2048 dips below 200 in the last
    # step); n0 = 80000: N q ~ 200, both branches in every step
    for n0 in (100000, 80000):
        N, lam, NT, share = _mort_twin("GN", rk, n0, False)
        print(f"normal branch {rk} n0={n0}: share of paths per step {np.round(share, 4).tolist()}")
        assert np.all(share > 0.999) if n0 == 100000 else np.all((share > 0.5) & (share < 0.99))
        gN, glam, gNT = _run_mortality(P, "GN", rk, dev, n0, False, True)
        np.testing.assert_allclose(glam, lam, rtol=1e-6, atol=0)
        assert np.array_equal(gN, N) and np.array_equal(gNT, NT), (rk, n0, np.abs(gN - N).max())
        assert np.all(np.diff(gN, axis=0) <= 0) and (gNT < n0).all()


# ---------------------------------------------------------------------------
# basket
# ---------------------------------------------------------------------------
_BASKET_TWIN = {}


def _basket_params(na):
    a = np.arange(na)
    s0 = 80.0 + 10.0 * a
    corr = np.array([[1.0 if i == j else 0.6 ** abs(i - j) * (1 - 0.05 * min(i, j)) for j in range(na)]
                     for i in range(na)])
    return dict(s0=s0, mu=0.02 + 0.01 * a, sigma=0.15 + 0.03 * a, norm=s0 * (1 + 0.1 * a), corr=corr)


def _basket_twin(na, rk):
    from rphedge.ops import paths as P

    if (na, rk) not in _BASKET_TWIN:
        bp = _basket_params(na)
        n, off, m = RANGES[rk]
        S, fin = P._cpu_basket(grid("GK"), n, bp["s0"], bp["mu"], bp["sigma"], np.linalg.cholesky(bp["corr"]), off,
                               P.SEED_W1, m)
        _BASKET_TWIN[na, rk] = frozen(S / bp["norm"][None, :, None], fin / bp["norm"][:, None])
    return _BASKET_TWIN[na, rk]


def _run_basket(P, na, rk, dev, g=None):  # noqa: F811
    bp = _basket_params(na)
    n, off, m = RANGES[rk] if isinstance(rk, str) else rk
    g = g or grid("GK")
    sb, s = guarded(g.n_coarse * na * n, dev)
    fb, f = guarded(na * n, dev)
    out = P.Paths(kind="basket", grid=g, n_local=n, path_offset=off, S=s.view(g.n_coarse, na, n), bond=g.bond(0.0),
                  S_final=f.view(na, n), na=na)
    p = P.simulate_basket(g, n, bp["s0"], bp["mu"], bp["sigma"], bp["corr"], norm=bp["norm"], device=dev, offset=off,
                          index_map=m, out=out)
    torch.cuda.synchronize()
    assert p is out
    check_guards(f"basket {na} {rk} S", sb)
    check_guards(f"basket {na} {rk} S_final", fb)
    return p.S, p.S_final


@pytest.mark.parametrize("na", [1, 2, 3, 4, 5, 6])
def test_basket_all_widths_distinct_assets(dev, na):  # noqa: F811
    """Every k_sim_basket<NA> against the twin with per-asset s0 / mu / sigma /
    norm all different and a correlation matrix without symmetry among the
    assets: a swapped asset index shows."""
    from rphedge.ops import paths as P

    bp = _basket_params(na)
    C = bp["corr"]
    assert np.allclose(C, C.T) and np.linalg.eigvalsh(C).min() > 0.05
    if na >= 3:  # no two off-diagonal entries of a row pair are alike: no asset permutation leaves C unchanged
        off_diag = C[np.triu_indices(na, 1)]
        assert len(np.unique(np.round(off_diag, 12))) == off_diag.size
    for rk in ("R2", "R4", "R6", "R9"):
        rS, rfin = _basket_twin(na, rk)
        S, fin = _run_basket(P, na, rk, dev)
        S, fin = S.cpu().numpy(), fin.cpu().numpy()
        tag = f"basket NA={na} {rk}"
        for a in range(na):
            assert np.all(S[0, a] == F(bp["s0"][a]) * F(1.0 / bp["norm"][a])), tag
        err = max(np.abs(S / rS - 1).max(), np.abs(fin / rfin - 1).max())
        print(f"{tag}: max rel err {err:.2e} (bound 2e-4)")
        np.testing.assert_allclose(S, rS, rtol=2e-4, err_msg=tag)
        np.testing.assert_allclose(fin, rfin, rtol=2e-4, err_msg=tag)


# ---------------------------------------------------------------------------
# aligned / unaligned / mapped instantiations: the same arithmetic per thread
# ---------------------------------------------------------------------------
def test_instantiations_agree_bitwise(dev):  # noqa: F811
    """[0, 5120) with the aligned kernels (it contains [0, 512) and every index
    of the R6 map), [37, 337) and the R6 map with the unaligned ones: bitwise
    equal wherever the global indices coincide, for every output tensor."""
    from rphedge.ops import paths as P
    from rphedge.ops.paths import path_indices

    full, shifted, mapped = (5120, 0, None), (300, 37, None), RANGES["R6"]
    midx = path_indices(*mapped).astype(np.int64)
    assert midx.max() < full[0] and full[0] % 256 == 0

    def sv(case, gk):
        model, v0, kw = SV_CASES[case]

        def run(r):
            p = P.simulate_sv(grid(gk), r[0], S0, MU, v0, model=model, norm=NORM, device=dev, offset=r[1],
                              index_map=r[2], **kw)
            return [p.S, p.vol, p.S_final]
        return run

    def mortality(q3):
        def run(r):
            g = grid("GM")
            p = P.Paths(kind="gbm", grid=g, n_local=r[0], path_offset=r[1], S=torch.empty(1, r[0], device=dev),
                        bond=g.bond(0.0), S_final=torch.empty(r[0], device=dev))
            p.meta["index_map"] = r[2]
            P.simulate_mortality(p, *LAM, 10000, lambda_fine_index=q3)
            return [p.nfrac, p.lam, p.nfrac_final]
        return run

    def basket(r):
        return list(_run_basket(P, 3, r, dev))

    for name, run in (("heston qe fp32", sv("heston_qe_xi09", "GB")), ("heston qe fp32 xi 0.3", sv("heston_qe_xi03", "GB")),
                      ("sv_ref fp32", sv("sv_ref", "GB")), ("mortality", mortality(False)),
                      ("mortality fine index", mortality(True)), ("basket 3", basket)):
        a, b, c = run(full), run(shifted), run(mapped)
        torch.cuda.synchronize()
        mi = torch.as_tensor(midx, device=dev)
        for k, (ta, tb, tc) in enumerate(zip(a, b, c)):
            assert torch.equal(tb, ta[..., 37:337]), (name, k, "offset 37")
            assert torch.equal(tc, ta[..., mi]), (name, k, "map")


# ---------------------------------------------------------------------------
# stand-alone Sobol kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset", [(1, 0), (255, 37), (257, 64), (300, END - 300), (512, END - 512)])
def test_sobol_normal_unaligned_and_offset(dev, n, offset):  # noqa: F811
    from rphedge.ops import native
    from rphedge.ops.sobol import device_table, sobol_norm_cpu, sobol_table

    d, seed = 7, 1235
    table = device_table(d, seed, dev)
    x = sobol_table(d, seed).points_u30(np.arange(offset, offset + n, dtype=np.uint64))
    ref = sobol_norm_cpu(0, d, seed, offset=offset, n=n)
    assert x.shape == ref.shape == (n, d)

    def run(dtype, raw):
        k = 2 if dtype == torch.float64 else 1
        buf, view = guarded(k * n * d, dev)
        out = view.view(dtype).view(n, d)
        native.sobol_normal(out, table, offset=offset, raw=raw)
        torch.cuda.synchronize()
        check_guards(f"sobol {dtype} raw={raw}", buf)
        return out.cpu().numpy()

    assert np.array_equal(run(torch.float64, True), x * 2.0 ** -30)
    assert np.array_equal(run(torch.float32, True), x.astype(F) * F(2.0 ** -30))
    got = run(torch.float64, False)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got))
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-12, atol=1e-13)
    got = run(torch.float32, False).astype(np.float64)
    core = np.abs(ref) < 5
    np.testing.assert_allclose(got[core], ref[core], rtol=2e-6, atol=2e-6)
    tail = ~core & fin
    assert np.max(np.abs(got[tail] - ref[tail]), initial=0) < 1e-3
