"""What the LM kernels (csrc/hedge_lm.hip) select by the scalars of the last
solve, driven pass by pass through native.lm_eval / native.lm_solve.

One test is about code that changed with it: k_lm_reduce reads the stop flag
of an adaptive budget only in such a fit and tests it in every branch after
that branch's slab loads, before its first store.  test_stopped_launches_
write_nothing fills the slabs and (once the pass has taken its copy) the
reduced block with a sentinel before every launch after the stop: a branch
that ran on would write sums of the sentinel into the block.  The reduce's
arithmetic itself rests on the fp64 pins of tests/test_gpu_lm_geometry.py.

The other tests pin, in advance of any change to them, what the prologues of
k_lm_pass and of the solve select - code that is the same before and after
this file was added: the weight slot the pass evaluates, the best-block copy
it takes after an accept and not after a reject, the precomputed step a
rejecting solve publishes, and the block whose statistics the final solve
records.  A prologue that loads both candidates ahead and selects afterwards
(measured, not kept: BENCHMARKS.md) can go wrong in exactly these places.

The fits: 1-8-8-2 net on the teacher problem of tests/test_gpu_lm.py, 2^12
paths (16 pass workgroups, the natural grid at that size), a 1,024-path Gram
subsample.  Seed and initial damping were chosen on the torch twin
(TorchBackend, as tests/test_lm_cpu.py) for their accept / reject patterns,
which every test asserts on the device's own loss history:
  lam0 = 100, 4 passes   A R A A A   0.573 31.7 0.520 0.271 0.0387
  lam0 = 0.1, 5 passes   A R R R R R 0.573 231 699 166 9616 3139
The best-block copy spreads 17,779 doubles over the grid: 4.3 per thread on 16
workgroups (whole trips of the copy loop and a partial one); fewer than one
per thread needs more than 69 workgroups, which the natural grid has from 2^15
paths on (128), so that case runs 2^15 paths."""
import numpy as np
import pytest
import torch

from test_gpu_lm import _setup
from test_gpu_lm_geometry import G_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu

SHAPE = (1, 8, 2, 0)
ARAAA = dict(lam0=100.0, passes=4, pattern="ARAAA")
ARRRRR = dict(lam0=0.1, passes=5, pattern="ARRRRR")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _Fit:
    """One LM fit of the 1-8-8-2 net, prepared as HipBackend._lm_fit prepares
    it and launched one kernel chain at a time."""

    def __init__(self, n, lam0, passes, stop_tol=0.0, stop_min=1, seed=0, gram_paths=1024, out_fix=False, **_):
        from rphedge.engine import FitConfig, HipBackend, TrainConfig
        from rphedge.models.hedge_mlp import torch_forward

        dev = torch.device("cuda", 0)
        self.n, self.passes = n, passes
        self.spec, feats, pr, y, self.data, w0 = _setup(SHAPE, n, dev, seed=seed)
        self.be = HipBackend(self.spec, n, TrainConfig(batch_size=n, lm_gram_paths=gram_paths, lm_out_fix=out_fix),
                             device=dev)
        self.w, self.o, self.f = self.be.new_weights(w0), self.be.new_opt(), self.be.new_fit()
        fc = FitConfig(epochs=passes, optimizer="lm", early_stopping=False, lm_lam0=lam0, lm_stop_tol=stop_tol,
                       lm_stop_min=stop_min)
        self.d, self.lm = self.be._lm_prepare(self.w, self.o, self.f, self.data, fc)
        self.b = self.be._lm_buffers()
        self.P, self.R, self.nblk = self.be._lm_shape
        # fp64 evaluation of the same problem
        self._fwd = torch_forward
        self.X = (torch.stack(feats, 1).double() - 0.1) * 1.5
        self.Pm = torch.stack([p.double() for p in pr] + [torch.full((n,), 1.01, dtype=torch.float64)], 1)
        self.y = y.double()

    def eval(self, k):
        self.be.native.lm_eval(self.d, self.lm, self.b["red"], k, None)
        torch.cuda.synchronize()

    def solve(self, k):
        self.be.native.lm_solve(self.d, self.lm, self.b["red"], k, None)
        torch.cuda.synchronize()

    def get(self, name):
        return self.b[name].cpu().numpy().copy()

    def fp64(self, w):
        """(loss sum, gradient of the mean loss) at the fp32 weights ``w``, as
        fp64_reference of test_gpu_lm_geometry.py."""
        wt = torch.tensor(np.asarray(w, np.float32).astype(np.float64), requires_grad=True)
        e = (self._fwd(self.spec, wt, self.X) * self.Pm).sum(1) - self.y
        g, = torch.autograd.grad((e * e).sum() / self.n, wt)
        return float((e * e).sum().detach()), g.numpy()

    def hist(self):
        from rphedge.ops import layout as L

        return self.f.cpu().numpy()[L.F_HIST:L.F_HIST + self.passes + 1]


def _pattern(h):
    return "".join("A" if k == 0 or h[k] < h[:k].min() else "R" for k in range(len(h)))


def _weights(state, slot, P):
    from rphedge.ops import layout as L

    return state[L.LMS_W + slot * L.LM_NPMAX:L.LMS_W + slot * L.LM_NPMAX + P]


def _copied(P, nblk):
    """Index ranges of the reduced block that the best-block copy carries: the
    Gram blocks and the tile-store image, then g | stats | packed output Gram."""
    from rphedge.engine.lm_geometry import lm_out_nu, lm_tpack_len
    from rphedge.models.hedge_mlp import NetSpec
    from rphedge.ops import layout as L

    nu = lm_out_nu(NetSpec(*SHAPE))
    ng = nblk * 1024 + lm_tpack_len(P, nblk)
    ngr = L.LM_RED_OUTG - L.LM_GBLK_MAX + (nu * (nu + 1) // 2 if nu <= 64 else 1)
    return [(0, ng), (L.LM_GBLK_MAX, L.LM_GBLK_MAX + ngr)], ng + ngr


def test_pass_evaluates_the_trial_slot():
    """After each solve the next pass must evaluate slot 1 - LSS_BEST: its
    reduced loss and gradient match fp64 at that slot's weights within the
    bounds of test_gpu_lm_geometry.py and miss the other slot's by more.  The
    fit has a reject after an accept and an accept after a reject, so the trial
    slot is 1, 1, 0, 1: a pass that always read one slot, or the best one,
    fails."""
    from rphedge.ops import layout as L

    ft = _Fit(1 << 12, **ARAAA)
    P = ft.P
    trial_slots = []
    for k in range(ft.passes + 1):
        ft.eval(k)
        if k > 0:
            red = ft.get("red")
            loss = red[L.LM_GBLK_MAX + L.LM_NPMAX]
            g = red[L.LM_GBLK_MAX:L.LM_GBLK_MAX + P]
            err = {}
            for name, slot in (("trial", trial), ("other", 1 - trial)):
                l_ref, g_ref = ft.fp64(_weights(state, slot, P))
                err[name] = (abs(loss - l_ref) / l_ref, np.linalg.norm(g - g_ref) / np.linalg.norm(g_ref))
            print(f"pass {k}: trial slot {trial}: loss {err['trial'][0]:.3e} g {err['trial'][1]:.3e}; "
                  f"other slot: loss {err['other'][0]:.3e} g {err['other'][1]:.3e}")
            assert err["trial"][0] <= LOSS_TOL and err["trial"][1] < G_TOL, (k, err)
            assert err["other"][0] > LOSS_TOL and err["other"][1] > G_TOL, (k, err)
        ft.solve(k)
        state = ft.get("state")
        trial = 1 - int(state[L.lm_slot(k + 1) + L.LSS_BEST])
        assert trial == 1 - int(state[L.LMS_BEST])  # (the host mirror)
        trial_slots.append(trial)
    h = ft.hist()
    assert _pattern(h) == ARAAA["pattern"], h
    assert trial_slots[:4] == [1, 1, 0, 1], trial_slots


@pytest.mark.parametrize("n,wgs", [(1 << 12, 16), (1 << 15, 128)])
def test_best_block_copy_follows_the_accept(n, wgs):
    """A pass that follows an accept copies the trial's reduced block (as it
    stood before the pass) into the state's best block, bytewise, over the
    Gram blocks, the tile image, g, the statistics and the output-Gram region;
    one that follows a reject leaves the best block alone.  16 workgroups:
    more than 4 elements per thread (several trips of the copy loop, a last
    partial one); 128: fewer than one."""
    from rphedge.ops import layout as L

    ft = _Fit(n, gram_paths=1024 if n == 1 << 12 else 4096, **ARAAA)
    assert int(ft.lm.num_wgs) == wgs and int(ft.lm.inst) == 1
    ranges, total = _copied(ft.P, ft.nblk)
    assert (total > 4 * wgs * 256) == (wgs == 16) and (total < wgs * 256) == (wgs == 128)
    copied_after = []
    for k in range(ft.passes + 1):
        snap, before = ft.get("red"), ft.get("state")[L.LMS_RED:L.LMS_RED + L.LM_RED]
        ft.eval(k)
        best = ft.get("state")[L.LMS_RED:L.LMS_RED + L.LM_RED]
        if k > 0 and accepted:
            for a, b in ranges:
                assert _same(best[a:b], snap[a:b]), (k, a, b)
            mask = np.ones(L.LM_RED, bool)
            for a, b in ranges:
                mask[a:b] = False
            assert _same(best[mask], before[mask]), k  # nothing else
            copied_after.append(k)
        else:
            assert _same(best, before), k
        ft.solve(k)
        accepted = ft.get("state")[L.lm_slot(k + 1) + L.LSS_COPY] != 0.0
    h = ft.hist()
    assert _pattern(h) == ARAAA["pattern"], h
    assert copied_after == [1, 3, 4]


SENTINEL = -7.25


@pytest.mark.parametrize("n,out_fix", [(1 << 12, False), (1 << 12, True), (1 << 15, True)])
def test_stopped_launches_write_nothing(n, out_fix):
    """Adaptive budget (stop_tol = 0.5: the accepted pass 2 gains 10 %).  The
    slabs are filled with a sentinel before every lm_eval after the stop, and
    the reduced block too from the second one on (the first pass after the
    stop still copies the stopping pass's block into the state: that pass was
    accepted, and the final solve publishes from the best block).  A stopped
    pass writes no slab row, and a stopped reduce writes nothing: every
    sentinel survives bytewise, and the block is unchanged by the first launch.
    A reduce branch that ran on would store sums of the sentinel - Gram
    workgroups (thread-per-entry at 2^12 paths, LDS form at 2^15), packet
    workgroups (16-row form / 256-row form), the output-Gram workgroups'
    marker (out_fix off, or any pass before the last) and their sums (out_fix:
    the final evaluation, pass == passes, whose launch has no Gram
    workgroups).  The state changes only by that one copy; the history is
    NaN past the stop.  (Not entered here: the 32-row and 512-row packet
    forms and the 64-entry output-Gram form.)"""
    from rphedge.ops import layout as L

    kw = dict(ARAAA, passes=5)
    ft = _Fit(n, stop_tol=0.5, stop_min=1, out_fix=out_fix, gram_paths=1024 if n == 1 << 12 else 4096, **kw)
    assert int(ft.lm.out_gram) == int(out_fix)
    assert (int(ft.lm.num_wgs), int(ft.lm.gram_wgs)) == ((16, 16) if n == 1 << 12 else (128, 64))
    ranges, _ = _copied(ft.P, ft.nblk)
    slabs = ("slab_b", "slab_g", "slab_o")
    s = None
    for k in range(ft.passes + 1):
        if s is not None:
            for x in slabs:
                ft.b[x].fill_(SENTINEL)
            if k > s + 1:
                ft.b["red"].fill_(SENTINEL)
            torch.cuda.synchronize()
        before = {x: ft.get(x) for x in slabs + ("red", "state")}
        ft.eval(k)
        if s is not None:
            after = {x: ft.get(x) for x in slabs + ("red", "state")}
            for x in slabs:
                assert (after[x] == np.float32(SENTINEL)).all(), (k, x)
            assert _same(after["red"], before["red"]), k
            if k > s + 1:
                assert (after["red"] == SENTINEL).all(), k
            st0, st1 = before["state"], after["state"]
            if k == s + 1:  # the stopping solve accepted: its block becomes the best block
                for a, b in ranges:
                    assert _same(st1[L.LMS_RED + a:L.LMS_RED + b], before["red"][a:b]), (k, a, b)
                    st0[L.LMS_RED + a:L.LMS_RED + b] = st1[L.LMS_RED + a:L.LMS_RED + b]
            assert _same(st1, st0), k
        ft.solve(k)
        if s is None and ft.get("state")[L.lm_slot(k + 1) + L.LSS_STOP] != 0.0:
            s = k
    assert s == 2, s
    f = ft.f.cpu().numpy()
    h = f[L.F_HIST:L.F_HIST + ft.passes + 1]
    assert np.isfinite(h[:s + 1]).all() and np.isnan(h[s + 1:]).all(), h
    assert _pattern(h[:s + 1]) == "ARA" and int(f[L.F_EPOCH]) == s + 1


def test_rejection_publishes_the_precomputed_step():
    """Passes 1-3 of the A R R R R R fit are rejected with LSS_SPEC_IDX = 1, 2,
    3: the solve publishes the step the last full solve precomputed - the
    trial slot afterwards holds the bytes of LMS_SPEC_W + sidx read before the
    solve - and hands on sidx + 1."""
    from rphedge.ops import layout as L

    ft = _Fit(1 << 12, **ARRRRR)
    P = ft.P
    seen = []
    for k in range(ft.passes + 1):
        ft.eval(k)
        st0 = ft.get("state")
        ft.solve(k)
        st1 = ft.get("state")
        sidx = int(st0[L.lm_slot(k) + L.LSS_SPEC_IDX])
        if 1 <= k <= 3:
            assert sidx == k and sidx < L.LM_SPEC
            assert st0[L.LMS_SPEC_OK + sidx] != 0.0
            assert int(st1[L.LMS_BEST]) == int(st0[L.LMS_BEST]) == 0  # rejected: slot 0 stays the best point
            spec_w = st0[L.LMS_SPEC_W + sidx * L.LM_NPMAX:L.LMS_SPEC_W + sidx * L.LM_NPMAX + P]
            assert _same(_weights(st1, 1, P), spec_w), k
            for other in range(1, L.LM_SPEC):  # the steps differ, so a wrong index shows
                if other != sidx:
                    ow = st0[L.LMS_SPEC_W + other * L.LM_NPMAX:L.LMS_SPEC_W + other * L.LM_NPMAX + P]
                    assert not _same(ow, spec_w)
            assert int(st1[L.lm_slot(k + 1) + L.LSS_SPEC_IDX]) == sidx + 1  # (a full solve hands on 1)
            seen.append(sidx)
    assert seen == [1, 2, 3]
    h = ft.hist()
    assert _pattern(h) == ARRRRR["pattern"], h


@pytest.mark.parametrize("fit,last", [(ARAAA, "A"), (ARRRRR, "R")])
def test_final_solve_records_the_published_points_statistics(fit, last):
    """FitState.last_mae / last_mape after the final solve: fp32 of sb[1] / c
    and 100 sb[2] / c of the published point's block - the trial's (red) when
    the last trial was accepted, the best point's (state) when it was
    rejected.  (No output step in these fits, so the published point is the
    best point.)"""
    from rphedge.ops import layout as L

    ft = _Fit(1 << 12, **fit)
    assert int(ft.lm.out_gram) == 0
    for k in range(ft.passes + 1):
        ft.eval(k)
        if k == ft.passes:
            red, best = ft.get("red"), ft.get("state")[L.LMS_RED:L.LMS_RED + L.LM_RED]
        ft.solve(k)
    h = ft.hist()
    assert _pattern(h) == fit["pattern"] and fit["pattern"][-1] == last, h
    o = L.LM_GBLK_MAX + L.LM_NPMAX
    sb, other = (red[o:o + 4], best[o:o + 4]) if last == "A" else (best[o:o + 4], red[o:o + 4])
    c = max(sb[3], 1.0)
    f = ft.f.cpu().numpy()
    mae, mape = np.float32(sb[1] / c), np.float32(100.0 * sb[2] / c)
    assert np.float32(other[1] / max(other[3], 1.0)) != mae  # the two blocks differ
    assert f[L.F_LAST_MAE] == mae and f[L.F_LAST_MAPE] == mape, (f[L.F_LAST_MAE], mae, f[L.F_LAST_MAPE], mape)
