"""The Merton jump-diffusion kernels on the GPU: k_sim_jump path by path
against the fp64 twin ``_cpu_merton``, lam = 0 bitwise against the SIM_GBM_LOG
scan, the fused out-of-sample kernels (k_hedge_oos_jump, k_hedge_oos_jump_cost)
against the materialised route, the descriptor guards and a Merton run end to
end.

Cases: jump sets J1 = (1, -0.1, 0.15), J5 = (5, -0.05, 0.1), J8 = (8, 0.02,
0.05); grids GB = Grid(1, 1/32, 1/8) and GN = Grid(2, 0.25, 0.5); the path
ranges R1-R9 of tests/test_gpu_path_scans.py (unaligned, mapped, indices up to
2^30 - 1).  GN x J8 has lam dt = 2 and reaches the 8-jump cap.

Bounds.  fp64: rtol 1e-5 / atol 1e-6 (the SV bound of test_gpu_path_scans).
fp32: the rule of that file - ``_emu_merton_f32`` is a float32 numpy emulation
of the kernel's recursion; only its distance to the fp64 twin is used: pooled
over the nine ranges, the kernel stays within 4 x the emulation's e_max on
every point and within 4 x e_99.9 on 99.9 % of the points (relative error of
S and S_final).  The jump counts are integer comparisons against host
thresholds, the same on both sides, and no count uniform of these cases lies
within 2 of a threshold (tests/test_merton_cpu.py), so no path is left out.

Measured on an MI355X (relative error of S and S_final, fp32 kernel against
the twin | the emulation's e_max / e_99.9; the bounds are 4 x those), nine
ranges pooled:

    set  grid  kernel max  p99.9    | e_max     e_99.9    inside 4 e_99.9
    J1   GB    2.77e-06    2.23e-06 | 3.01e-06  2.27e-06  100.000 %
    J1   GN    1.46e-06    1.23e-06 | 1.46e-06  1.23e-06  100.000 %
    J5   GB    3.15e-06    2.25e-06 | 2.77e-06  2.25e-06  100.000 %
    J5   GN    1.93e-06    1.55e-06 | 1.93e-06  1.55e-06  100.000 %
    J8   GB    2.70e-06    2.40e-06 | 2.84e-06  2.44e-06  100.000 %
    J8   GN    1.86e-06    1.58e-06 | 1.86e-06  1.57e-06  100.000 %

The kernel's worst point uses 0.28 of its 4 e_max bound (J5, GB).  fp64: at
most 1.25e-07 relative off the twin (the float32 store; bound 1e-5).  lam = 0:
every stored float equals the SIM_GBM_LOG scan's, fp32 and fp64, R4 and R9.

Routes (7 dates, 2048 paths, windows 0 and 4096 + 37, with and without costs,
three runs): the per-path P&L of the fused and the materialised route is equal
bit for bit in all 12 cases, and so are the statistics rows with the
materialised route in 256-path chunks (the fused kernel's tile: both kernels
then add the same fp64 terms in the same order).  Against the materialised
route in ONE chunk (k_hedge_pnl: 1024 paths per workgroup) the sums of squares
ES_V2 / ES_RES2 differ by 1.1e-16 - 2.2e-16 relative in 11 of the 12 cases -
the order of an fp64 sum - and nothing else differs.

End to end (LM, 2^16 paths, 30 dates, J1): series price 12.7613, MC price of
the run's paths 12.7418 (-0.27 standard errors), V0 12.7681 (V0 / MC - 1 =
+2.07e-3, bound 3e-3); net P&L std 3.848 against the Merton-delta hedge's
4.266 on the same paths; two captured replays reproduce V0, the P&L std, the
per-path P&L and the paths bitwise.
"""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_eval import check_guards, guarded
from test_gpu_kernels import dev  # noqa: F401  (fixture)
from test_gpu_path_scans import ALIGNED, RANGES, frozen, grid

pytestmark = pytest.mark.gpu

F = np.float32
S0, MU, SIGMA, NORM = 100.0, 0.05, 0.2, 100.0
JUMPS = {"J1": (1.0, -0.1, 0.15), "J5": (5.0, -0.05, 0.1), "J8": (8.0, 0.02, 0.05)}
_TWIN, _EMU = {}, {}


def _twin(jk, gk, rk):
    """fp64 twin, normalised: (S [n_coarse, n], S_final); once per case, read-only."""
    from rphedge.ops import paths as P

    key = (jk, gk, rk)
    if key not in _TWIN:
        n, off, m = RANGES[rk]
        S, fin = P._cpu_merton(grid(gk), n, S0, MU, SIGMA, *JUMPS[jk], off, P.SEED_W1, m)
        _TWIN[key] = frozen(S / NORM, fin / NORM)
    return _TWIN[key]


def _emu_merton_f32(g, n, off, m, lam, mu_j, sig_j):
    """float32 numpy emulation of k_sim_jump<float, *> (normalised S, S_final).  Sizes the fp32 tolerance only."""
    from rphedge.ops import paths as P
    from rphedge.ops.ndtri import ndtri_u30_f32

    nf = g.n_fine
    X = P._u30(3 * nf, P.SEED_W1, n, off, 3 * nf, m)
    Z = ndtri_u30_f32(np.maximum(X[:, :nf], 1))
    N = P.merton_counts(X[:, nf:2 * nf], P.merton_thresholds(lam * g.dt))
    ZJ = ndtri_u30_f32(np.maximum(X[:, 2 * nf:], 1))
    assert Z.dtype == ZJ.dtype == F
    half, zero = F(0.5), F(0)
    dt, mu, sig, muj, sigj = F(g.dt), F(MU), F(SIGMA), F(mu_j), F(sig_j)
    kap = np.expm1(muj + half * sigj * sigj)
    drift = (mu - half * sig * sig - F(lam) * kap) * dt
    vol = sig * np.sqrt(dt)
    inv0 = F(1.0 / NORM)
    y = np.full(n, np.log(F(S0)), F)
    S = np.empty((g.n_coarse, n), F)
    S[0] = F(S0) * inv0
    for t in range(1, nf):
        y = y + (drift + vol * Z[:, t])
        fn = N[:, t].astype(F)
        y = y + np.where(N[:, t] > 0, fn * muj + np.sqrt(fn) * sigj * ZJ[:, t], zero)
        assert y.dtype == F
        if t % g.reduction == 0 and t // g.reduction < g.n_coarse:
            S[t // g.reduction] = np.exp(y) * inv0
    return S, np.exp(y) * inv0


def _errors(S, fin, ref):
    S, fin = np.asarray(S, np.float64), np.asarray(fin, np.float64)
    return np.concatenate([np.abs(S / ref[0] - 1).ravel(), np.abs(fin / ref[1] - 1).ravel()])


def _emu_errors(jk, gk, rk):
    key = (jk, gk, rk)
    if key not in _EMU:
        _EMU[key] = frozen(_errors(*_emu_merton_f32(grid(gk), *RANGES[rk], *JUMPS[jk]), _twin(jk, gk, rk)))[0]
    return _EMU[key]


def _run_scan(P, jk, gk, rk, dev, fp64):  # noqa: F811
    """k_sim_jump into guarded buffers through simulate_merton(out=)."""
    n, off, m = RANGES[rk]
    g = grid(gk)
    bs, bf = guarded(g.n_coarse * n, dev), guarded(n, dev)
    out = P.Paths(kind="gbm", grid=g, n_local=n, path_offset=off, S=bs[1].view(g.n_coarse, n), bond=g.bond(0.0),
                  S_final=bf[1], norm=NORM)
    p = P.simulate_merton(g, n, S0, MU, SIGMA, *JUMPS[jk], norm=NORM, device=dev, offset=off, fp64=fp64, index_map=m,
                          out=out)
    torch.cuda.synchronize()
    assert p is out
    check_guards(f"{jk} {gk} {rk} S", bs[0])
    check_guards(f"{jk} {gk} {rk} S_final", bf[0])
    S, fin = p.S.cpu().numpy(), p.S_final.cpu().numpy()
    assert np.all(S[0] == F(S0) * F(1.0 / NORM))
    return S, fin


@pytest.mark.parametrize("jk", list(JUMPS))
def test_scan_vs_twin(dev, jk):  # noqa: F811
    from rphedge.ops import paths as P

    for gk in ("GB", "GN"):
        emu, got = [], []
        for rk in RANGES:
            ref = _twin(jk, gk, rk)
            assert all(np.all(np.isfinite(x)) for x in ref)
            S, fin = _run_scan(P, jk, gk, rk, dev, fp64=True)
            tag = f"{jk} {gk} {rk} fp64"
            np.testing.assert_allclose(S, ref[0], rtol=1e-5, atol=1e-6, err_msg=tag)
            np.testing.assert_allclose(fin, ref[1], rtol=1e-5, atol=1e-6, err_msg=tag)
            k = _errors(*_run_scan(P, jk, gk, rk, dev, fp64=False), ref)
            e = _emu_errors(jk, gk, rk)
            print(f"{jk} {gk} {rk} ({'aligned' if ALIGNED[rk] else 'unaligned'}): fp64 S rel max "
                  f"{_errors(S, fin, ref).max():.2e}; fp32 S rel max {k.max():.2e} (emulation {e.max():.2e})")
            emu.append(e), got.append(k)
        emu, got = np.concatenate(emu), np.concatenate(got)
        e_max, e_999 = float(emu.max()), float(np.quantile(emu, 0.999))
        k_max, k_999 = float(got.max()), float(np.quantile(got, 0.999))
        inside = float(np.mean(got <= 4 * e_999))
        print(f"FP32 {jk} {gk} S rel: kernel max {k_max:.2e} p99.9 {k_999:.2e} | emulation e_max {e_max:.2e} "
              f"e_99.9 {e_999:.2e} | bounds {4 * e_max:.2e} / {4 * e_999:.2e}, {100 * inside:.3f} % inside")
        assert np.isfinite(e_max) and e_max > 0
        assert k_max <= 4 * e_max, (jk, gk, k_max, e_max)
        assert inside >= 0.999, (jk, gk, inside, e_999)


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("rk", ["R4", "R9"])
def test_no_jumps_is_bitwise_the_gbm_log_scan(dev, rk, fp64):  # noqa: F811
    """lam = 0 (every threshold 2^30): k_sim_jump stores what k_sim_scan<SIM_GBM_LOG> stores on the same table 1."""
    from rphedge.ops import layout as L
    from rphedge.ops import native
    from rphedge.ops import paths as P

    n, off, m = RANGES[rk]
    g = grid("GB")
    d, j = P.merton_desc(g, n, S0, MU, SIGMA, 0.0, -0.1, 0.15, NORM, dev, off, fp64, P.SEED_W1, m)
    assert all(int(t) == 1 << 30 for t in j.thr)
    q = native.SimDesc.from_buffer_copy(d)     # the SIM_GBM_LOG launch on the same table 1
    q.model, q.sv2, q.shift2, q.dims2 = L.SIM_GBM_LOG, None, None, 0
    bufs = [guarded(g.n_coarse * n, dev), guarded(n, dev), guarded(g.n_coarse * n, dev), guarded(n, dev)]
    d.out, d.final_out = bufs[0][1].data_ptr(), bufs[1][1].data_ptr()
    q.out, q.final_out = bufs[2][1].data_ptr(), bufs[3][1].data_ptr()
    native.simulate_jump(d, j)
    native.simulate(q)
    torch.cuda.synchronize()
    for b, _ in bufs:
        check_guards(f"lam0 {rk}", b)
    assert torch.equal(bufs[0][1], bufs[2][1]) and torch.equal(bufs[1][1], bufs[3][1])
    assert float(bufs[1][1].std()) > 0.1
    # ... and with an intensity the same launch differs
    d2, j2 = P.merton_desc(g, n, S0, MU, SIGMA, 1.0, -0.1, 0.15, NORM, dev, off, fp64, P.SEED_W1, m)
    d2.out, d2.final_out = d.out, d.final_out
    native.simulate_jump(d2, j2)
    torch.cuda.synchronize()
    assert not torch.equal(bufs[1][1], bufs[3][1])


# ---------------------------------------------------------------------------
# fused route against materialised route
# ---------------------------------------------------------------------------
def _api_cfg(model, complement=False, **kw):
    from rphedge.config import ParityFlags, RunConfig, TrainingParams

    tr = TrainingParams(batch_size=1 << 11, epochs_first=1, epochs_rest=1, early_stopping=False, q99=False,
                        lr_schedule_first=False, chunk_log2=6, optimizer="lm", lm_passes_first=20, lm_passes_rest=2)
    # 29 fine points, reduction 4: 8 coarse points = 7 dates (every number exact in binary)
    return RunConfig(Y=100.0, K=100.0, T=0.875, mu=0.08, r=0.08, sigma=0.15, rebalancing=0.125, dt=1 / 32, n_paths=11,
                     option_type="CALL", mortality=False, N=1, P=1.0, verbose=False, train=tr,
                     parity=ParityFlags(complement_head=complement), device="cuda:0", payoff="call", model=model, **kw)


ROUTE_CASES = {
    "gbm_log_free_J5": (dict(model="gbm_log"), JUMPS["J5"], (1, 8, 2, 0)),
    "gbm_log_complement_J5": (dict(model="gbm_log", complement=True), JUMPS["J5"], (1, 8, 1, 1)),
    "merton_free": (dict(model="merton", jump_intensity=1.0, jump_mean=-0.1, jump_std=0.15), None, (1, 8, 2, 0)),
}


@pytest.mark.parametrize("case", list(ROUTE_CASES))
def test_fused_route_is_bitwise_the_materialised_one(dev, case):  # noqa: F811
    from rphedge import oos
    from rphedge.api import HedgeRun
    from rphedge.ops import layout as L

    kw, jump, shape = ROUTE_CASES[case]
    run = HedgeRun(_api_cfg(**kw))
    run.run()
    spec = run.spec
    assert (spec.nin, spec.hidden, spec.nout, spec.head) == shape
    assert run.induction.n_dates == 7 and run.n_local == 2048 and oos.fused_unsupported(run) is None
    stress = None if jump is None else dict(zip(("jump_intensity", "jump_mean", "jump_std"), jump))
    costs = dict(rate=1e-3, band=0.02)
    for offset in (0, 4096 + 37):              # the ALIGNED kernels and the unaligned window
        for cost_only in (False, True):        # k_hedge_oos_jump / k_hedge_oos_jump_cost
            ck = dict(costs=costs, cost_only=True) if cost_only else dict(costs=False)
            o = oos.out_of_sample(run, fused=True, stress=stress, keep_pnl=True, keep_paths=True, offset=offset, **ck)
            # the materialised route in 256-path chunks: a chunk's statistics row is summed in the order of the
            # fused kernel's 256-path tile (both kernels: one fp64 term per thread, the same shuffle tree and sum4),
            # so the rows can be compared bit for bit; in one chunk k_hedge_pnl packs 1024 paths per workgroup
            # and the fp64 sums differ by their order (printed below)
            m = oos.out_of_sample(run, fused=False, stress=stress, keep_pnl=True, keep_paths=True, offset=offset,
                                  chunk_log2=8, **ck)
            m1 = oos.out_of_sample(run, fused=False, stress=stress, keep_pnl=True, offset=offset, **ck)
            assert o.route == "fused" and m.route == m1.route == "materialised" and o.n_paths == m.n_paths == 2048
            assert m.chunks == 8 and m1.chunks == 1
            tag = f"{case} offset {offset} costs {cost_only}"
            # the fused kernel's trace is the scan's output, bit for bit
            assert torch.equal(o.paths.S, torch.cat([p.S for p in m.paths], dim=1)), tag
            assert torch.equal(o.paths.S_final, torch.cat([p.S_final for p in m.paths])), tag
            a, b = o.pnl.double().cpu().numpy(), m.pnl.double().cpu().numpy()
            diff, diff1 = np.abs(o.stats - m.stats), np.abs(o.stats - m1.stats)
            print(f"ROUTES {tag}: per-path |fused - materialised| max {np.abs(a - b).max():.3e}; statistics rows "
                  f"differ in columns {np.nonzero(diff)[0].tolist()}; against the one-chunk materialised rows in "
                  f"columns {np.nonzero(diff1)[0].tolist()} by {(diff1 / np.maximum(np.abs(m1.stats), 1e-300))[np.nonzero(diff1)[0]].tolist()} (relative)")
            assert torch.equal(o.pnl, m.pnl) and torch.equal(o.pnl, m1.pnl), tag
            assert o.stats[L.ES_COUNT] == 2048
            assert np.array_equal(o.stats, m.stats), tag
            np.testing.assert_allclose(o.stats, m1.stats, rtol=1e-13, atol=0, err_msg=tag)   # (2048 fp64 terms: 11 bits of 53)
            if cost_only:
                assert o.costs["mean_cost"] > 0 and o.costs["trades_per_path"] == m.costs["trades_per_path"], tag
                assert o.costs["mean_cost"] == pytest.approx(m.costs["mean_cost"], rel=1e-12), tag
    # the paths jump: the stressed / Merton test P&L is wider than the same hedge's on jump-free paths
    calm = run.out_of_sample(fused=True, stress=None if jump is not None else {"jump_intensity": 0.0})
    wild = run.out_of_sample(fused=True, stress=stress)
    assert wild.route == calm.route == "fused" and wild.std > calm.std
    run.close()


# ---------------------------------------------------------------------------
# descriptor guards
# ---------------------------------------------------------------------------
def test_jump_terms_are_checked_by_name_at_load():
    from rphedge.ops import layout as L
    from rphedge.ops import native

    lib = native.load(required=True)
    rows = native.native_layout_jump(lib)
    assert [(t, f) for t, f, _, _ in rows] == [("JumpTerms", k) for k in ("lam", "mu_j", "sig_j", "thr")]
    assert ctypes.sizeof(native.JumpTerms) == 56 and native.DESCRIPTORS_JUMP == (native.JumpTerms,)
    assert native.layout_mismatches(rows, [], classes=native.DESCRIPTORS_JUMP, layout=SimpleNamespace()) == []
    consts = dict(native.native_layout(lib)[1])
    assert consts["SIM_MERTON"] == L.SIM_MERTON == 6 and consts["JUMP_MAX"] == L.JUMP_MAX == 8

    class JumpTerms(ctypes.Structure):   # sig_j and mu_j swapped, thr one short
        _fields_ = [("lam", ctypes.c_double), ("sig_j", ctypes.c_double), ("mu_j", ctypes.c_double),
                    ("thr", ctypes.c_uint32 * 7)]

    bad = native.layout_mismatches(rows, [], classes=(JumpTerms,), layout=SimpleNamespace())
    assert any(b.startswith("JumpTerms.mu_j:") for b in bad) and any(b.startswith("JumpTerms.sig_j:") for b in bad)
    assert any(b.startswith("JumpTerms.thr:") and "native offset 24 size 32" in b for b in bad)
    assert len(bad) == 3

    class Short(ctypes.Structure):       # a field missing: the sizes differ too
        _fields_ = [("lam", ctypes.c_double), ("mu_j", ctypes.c_double), ("sig_j", ctypes.c_double)]

    Short.__name__ = "JumpTerms"
    bad = native.layout_mismatches(rows, [], classes=(Short,), layout=SimpleNamespace())
    assert any(b.startswith("JumpTerms.thr:") and "not in ctypes" in b for b in bad)
    assert any(b.startswith("JumpTerms: native size 56, ctypes size 24") for b in bad)


def test_launchers_reject_bad_merton_descriptors(dev):  # noqa: F811
    from rphedge.ops import layout as L
    from rphedge.ops import native
    from rphedge.ops import paths as P

    g, n = grid("GB"), 512
    S = torch.full((g.n_coarse, n), float("nan"), device=dev)

    def desc(**edit):
        d, j = P.merton_desc(g, n, S0, MU, SIGMA, *JUMPS["J1"], NORM, dev)
        d.out = S.data_ptr()
        for k, v in edit.items():
            if k.startswith("thr"):
                j.thr[int(k[3:])] = v
            else:
                setattr(j if k in ("lam", "mu_j", "sig_j") else d, k, v)
        return d, j

    bad = [(dict(sv2=None), "needs Sobol table 2"), (dict(shift2=None), "needs Sobol table 2"),
           (dict(dims2=2 * g.n_fine - 1), "Sobol table 2 shorter than 2 n_fine"),
           (dict(dims2=g.n_fine), "Sobol table 2 shorter than 2 n_fine"),
           (dict(dims1=g.n_fine - 1), "Sobol table 1"), (dict(sv1=None), "Sobol table 1"),
           (dict(model=L.SIM_GBM_LOG), "model must be SIM_MERTON"), (dict(path_stat=1), "path stat"),
           (dict(lam=-1.0), "lam >= 0"), (dict(sig_j=-0.1), "sig_j >= 0"), (dict(mu_j=math.inf), "finite"),
           (dict(thr7=(1 << 30) + 1), "thresholds must be non-decreasing and at most 2\\^30"),
           (dict(thr0=(1 << 30)), "thresholds must be non-decreasing"),
           (dict(path_offset=(1 << 30) - n + 1), "path range leaves the 30-bit Sobol index space"),
           (dict(out=None), "null out buffer")]
    for edit, msg in bad:
        for fn in (native.simulate_jump_check, native.simulate_jump):
            with pytest.raises(RuntimeError, match=msg) as e:
                fn(*desc(**edit))
            assert "rph_simulate_jump failed with code -22" in str(e.value), (edit, str(e.value))
    with pytest.raises(RuntimeError, match="SIM_MERTON without JumpTerms"):
        native.simulate_jump_check(desc()[0], None)
    with pytest.raises(RuntimeError, match="rph_simulate_jump"):    # the plain launcher has no jump terms to pass
        native.simulate(desc()[0])
    torch.cuda.synchronize()
    assert torch.isnan(S).all()                       # nothing was launched
    native.simulate_jump(*desc())
    torch.cuda.synchronize()
    assert not torch.isnan(S).any()
    # the fused launch: jump terms and SIM_MERTON go together
    from rphedge.engine import HipBackend, TrainConfig
    from test_gpu_eval import make_spec

    be = HipBackend(make_spec((1, 8, 2, 0)), n, TrainConfig(batch_size=n), device=dev)
    d, j = desc()
    with pytest.raises(ValueError, match="jump terms go with a SIM_MERTON scan"):
        be.oos(d, None, None, None, 1, 1.0)
    with pytest.raises(ValueError, match="jump terms go with a SIM_MERTON scan"):
        be.oos(P.gbm_desc(g, n, S0, MU, SIGMA, "log", NORM, dev), None, None, None, 1, 1.0, jump=j)
    o = native.OosDesc()
    o.sim = d
    o.snap = o.stats = o.fmu = o.fisd = o.bond = S.data_ptr()   # (checked, never launched)
    with pytest.raises(RuntimeError, match="model must be SIM_GBM_ARITH, SIM_GBM_LOG or SIM_HESTON"):
        native.oos_check(o)                           # (rph_oos itself takes no jump model)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_merton_run_end_to_end_and_graph_replay(dev):  # noqa: F811
    """LM, 2^16 paths, 30 dates, J1: the MC price of the run's paths against the
    series, V0 against the MC price (the bound of test_heston_and_basket_runs
    for LM), and a captured replay against the eager run, bitwise."""
    from rphedge import analytic
    from rphedge.api import HedgeRun
    from rphedge.config import parse_params

    lam, mj, sj = JUMPS["J1"]
    run = HedgeRun(parse_params(dict(
        Y=100, K=100, T=1.0, mu=0.05, r=0.05, sigma=0.2, N=1, P=1, x=0, l0=0, c=0, ita=0, mortality=False, q99=False,
        dt=1 / 30, rebalancing=1 / 30, n_paths=16, payoff="call", option_type="CALL", model="merton",
        jump_intensity=lam, jump_mean=mj, jump_std=sj, chunk_log2=6, lr_schedule_first=False, early_stopping=False,
        verbose=False, optimizer="lm", batch_size=1 << 14)))
    try:
        res = run.run()
        assert run.paths.n_coarse - 1 == 30 and run.n_total == 1 << 16
        ref = analytic.merton_price(100.0, 100.0, 0.05, 0.2, 1.0, lam, mj, sj)
        assert res.summary["analytic_price"] == pytest.approx(ref)
        pay = run.v_terminal.double() * run.scale * math.exp(-0.05)
        mc, se = float(pay.mean()), float(pay.std()) / math.sqrt(pay.numel())
        sf = res.self_financing_pnl
        print(f"E2E merton J1: series {ref:.4f} MC {mc:.4f} ({(mc - ref) / se:+.2f} se) V0 {res.v0:.4f} "
              f"(V0 / MC - 1 = {res.v0 / mc - 1:+.2e}); net P&L std {sf['std']:.4f}, Merton-delta hedge "
              f"{res.summary['merton_delta_pnl_std']:.4f}")
        assert abs(mc - ref) < 4 * se
        assert abs(res.v0 / mc - 1) < 0.003
        assert math.isfinite(sf["std"]) and sf["std"] > 0 and res.summary["merton_delta_pnl_std"] > 0
        eager = (res.v0, sf["std"], res.induction.pnl_paths.clone(), run.paths.S.clone())
        run.capture(include_simulation=True)
        for _ in range(2):
            run.paths.S.zero_()               # (the replay simulates the paths again)
            run.replay()
            r = run.collect()
            assert r.v0 == eager[0] and r.self_financing_pnl["std"] == eager[1]
            assert torch.equal(r.induction.pnl_paths, eager[2]) and torch.equal(run.paths.S, eager[3])
    finally:
        run.close()
