"""Pass 0 of a later date's LM fit evaluating its own target (k_lm_pass<BodyST>,
NarrowPairBody ST, csrc/hedge_narrow.h; SelfTargetDesc): the target net on the
raw features of date t+1 times the fit's own prices, in k_hedge_eval's
operation order.  Against the present route - k_hedge_eval writes v_out, pass 0
reads it as its target - every packet row, every Gram slab, the reduced block
and the stored target are equal BYTE FOR BYTE."""
import numpy as np
import pytest
import torch

from test_lm_cpu import _teacher_problem

pytestmark = pytest.mark.gpu

# the nets on the route (LmKernels::HAS_ST): the 1- and 2-input free-head nets
SHAPES = [(1, 8, 2, 0), (2, 8, 2, 0)]
# 2^13: 64 blocks of 128 paths; + 64: a 65th block whose second half is masked
NS = [1 << 13, (1 << 13) + 64]
# the cyclic block schedule (default) and the contiguous-leaf schedule (auto leaves)
SCHEDULES = {"cyclic": -1, "leaf": 0}
BOND = 1.01


def _problem(shape, n, dev):
    """A fit at date t and the eval inputs of date t+1 on the same paths: its
    own features and standardisation, the SAME price tensors (the fit's
    prices_next are the eval's prices_now) and bond."""
    from rphedge.engine import DateData
    from rphedge.models.hedge_mlp import NetSpec, init_weights

    spec = NetSpec(*shape)
    feats_t, pr, _ = _teacher_problem(spec, n, 3)
    feats_t1, _, _ = _teacher_problem(spec, n, 4)
    pr = [p.to(dev) for p in pr]
    ev = DateData(feats=[f.to(dev) for f in feats_t1], prices_next=[], bond_next=1.02, target=None, prices_now=pr,
                  bond_now=BOND, fmu=tuple([-0.2] * spec.nin), fisd=tuple([0.7] * spec.nin))
    target = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    fit = DateData(feats=[f.to(dev) for f in feats_t], prices_next=pr, bond_next=BOND, target=target, prices_now=pr,
                   fmu=tuple([0.1] * spec.nin), fisd=tuple([1.5] * spec.nin))
    w_star = init_weights(spec, [0.4] * spec.nout, seed=7)   # the target net (date t+1's fitted net)
    w_other = init_weights(spec, [0.5] * spec.nout, seed=1)  # a start point that is not the target net
    return spec, ev, fit, w_star, w_other


def _pass0(be, d, lm, st=None):
    b = be._lm_buffers()
    for k in ("red", "slab_b", "slab_g"):
        b[k].fill_(float("nan"))
    be.native.lm_eval(d, lm, b["red"], 0, None, st=st)
    torch.cuda.synchronize()
    return {k: b[k].cpu().numpy().copy() for k in ("red", "slab_b", "slab_g")}


def _override(lm, n, over):
    """The split block schedule at a few thousand paths: fewer path workgroups
    and a Gram of the first 64 k paths, set on a prepared LmDesc (the buffers
    are sized for the natural, larger geometry)."""
    if over is None:
        return
    num_wgs, k, skip = over
    assert num_wgs <= lm.num_wgs and k <= lm.gram_wgs and lm.leaf_blocks == 0 and lm.gram_base == 0
    lm.num_wgs, lm.gram_skip = num_wgs, skip
    lm.gram_wgs, lm.gram_blk, lm.gram_blk_stride, lm.inv_ns = k, 64 * k, n, 1.0 / (64 * k)


def _both_routes(shape, n, sched, start, over=None):
    """(present route, self-target route): slabs, reduced block and the target
    array of pass 0.  ``start``: "same" = the start point IS the target net (one
    NetWeights, the induction's case), "w0" = LmDesc.w0 names another start.
    ``over``: (num_wgs, Gram workgroups, gram_skip) set on both routes' descriptors."""
    from rphedge.engine import FitConfig, HipBackend, TrainConfig
    from rphedge.ops import layout as L

    dev = torch.device("cuda", 0)
    spec, ev, fit, w_star, w_other = _problem(shape, n, dev)
    be = HipBackend(spec, n, TrainConfig(batch_size=n, lm_gram_paths=2048, lm_out_fix=True,
                                         lm_leaf_paths=SCHEDULES[sched]), device=dev)
    assert be.eval_ride_ok(FitConfig(epochs=1, optimizer="lm", early_stopping=False))
    w, o, f = be.new_weights(w_star), be.new_opt(), be.new_fit()
    w0 = torch.zeros(L.LM_NPMAX, dtype=torch.float32, device=dev)
    w0[:spec.nparams] = torch.from_numpy(np.asarray(w_other, np.float32)).to(dev)
    fc = FitConfig(epochs=1, optimizer="lm", early_stopping=False)
    stats = be.new_stats()
    # present route: the eval writes v_out = the target, pass 0 reads it
    be.eval(w, ev, stats, v_out=fit.target)
    torch.cuda.synchronize()
    y = fit.target.cpu().numpy().copy()
    assert np.isfinite(y).all() and np.std(y) > 1e-3
    d, lm = be._lm_prepare(w, o, f, fit, fc)
    lm.w0 = w0.data_ptr() if start == "w0" else None
    _override(lm, n, over)
    old = _pass0(be, d, lm)
    # self-target route: the target array starts as NaN, pass 0 fills it
    fit.target.fill_(float("nan"))
    d, lm, st = be._lm_prepare(w, o, f, fit, fc, ride=be.eval_desc(w, ev, stats))
    lm.w0 = w0.data_ptr() if start == "w0" else None
    assert st.st_out == fit.target.data_ptr() and st.st_wts == w.data_ptr()
    _override(lm, n, over)
    new = _pass0(be, d, lm, st)
    y_st = fit.target.cpu().numpy().copy()
    lm.w0 = None
    return old, new, y, y_st, int(lm.num_wgs), int(lm.leaf_blocks)


def _same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES)
def test_self_target_pass_is_bytewise_the_present_pass(shape, n, sched):
    old, new, y, y_st, nw, leaf = _both_routes(shape, n, sched, "same")
    assert (leaf > 0) == (sched == "leaf") and nw > 1
    assert _same(y, y_st)  # the stored target IS the eval's v_out, every path written
    assert np.isfinite(old["slab_b"]).all() and np.count_nonzero(old["slab_b"]) > old["slab_b"].size // 4
    for k in ("slab_b", "slab_g", "red"):
        assert _same(old[k], new[k]), k


@pytest.mark.parametrize("shape", SHAPES)
def test_self_target_pass_is_bytewise_the_present_pass_on_the_split_schedule(shape):
    """The third block schedule (NarrowPairBody::sched with per > gram_skip,
    what a 2^20-path fit runs; tests/test_gpu_lm_geometry.py split5184): 5184
    paths on 2 path workgroups, one Gram workgroup whose waves take 2 blocks
    each, the others 9, 8, 8, 8 with the half-masked 41st block.  The same
    byte-for-byte assertions; packet rows and Gram slabs past the overridden
    grid keep their NaN fill on both routes."""
    from rphedge.engine import lm_pass_blocks

    n, over = 5184, (2, 1, 3)
    regime, blocks = lm_pass_blocks(n, *over)
    assert regime == "split" and [len(w) for w in blocks] == [2, 2, 2, 2, 9, 8, 8, 8]
    old, new, y, y_st, nw, leaf = _both_routes(shape, n, "cyclic", "same", over)
    assert leaf == 0 and nw == 2
    assert _same(y, y_st)
    live = old["slab_b"][:nw]
    assert np.isfinite(live).all() and np.count_nonzero(live) > live.size // 4
    assert np.isnan(old["slab_b"][nw:]).all() and np.isnan(old["slab_g"][1:]).all()
    assert np.isfinite(old["slab_g"][0]).all()
    for k in ("slab_b", "slab_g", "red"):
        assert _same(old[k], new[k]), k


@pytest.mark.parametrize("shape", SHAPES)
def test_start_point_and_target_net_are_independent_images(shape):
    """LmDesc.w0 names a start point that is not the target net: the body reads
    the start from one LDS image and the target net from another."""
    n = NS[1]
    old, new, y, y_st, _, _ = _both_routes(shape, n, "cyclic", "w0")
    same_start = _both_routes(shape, n, "cyclic", "same")[0]
    assert not _same(old["slab_b"], same_start["slab_b"])  # (the start point does differ)
    assert _same(y, y_st)
    for k in ("slab_b", "slab_g", "red"):
        assert _same(old[k], new[k]), k
