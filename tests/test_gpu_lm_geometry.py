"""One evaluation of the LM chain (k_lm_pass -> k_lm_reduce, csrc/hedge_lm.hip)
against fp64 torch in every launch geometry the kernels have a branch for:
the cyclic, split and contiguous-leaf path schedules (csrc/hedge_narrow.h
NarrowPairBody::sched), every packet tree and both Gram trees of k_lm_reduce
on both sides of their row-count thresholds, masked rows, ragged batches, and
Gram tiles in the path workgroups or after them.  The cases and the regime
each enters are tests/test_lm_geometry_cpu.py CASES (asserted there on the
host); the large-geometry regimes are entered at a few thousand paths by
overriding LmDesc fields after the descriptor is built (the buffers are sized
for the natural, larger geometry).

Measured on the MI355X, the largest over the 46 cases (bound):
  loss sum, relative            7.97e-08  nat256 (1, 8, 1, 1)    (1e-5)
  gradient, relative 2-norm     6.71e-08  split5184 (1, 8, 2, 0) (2e-5)
  gradient, entrywise / max|g|  8.96e-08  nat256 (5, 8, 6, 0)    (2e-5)
  Gram, relative Frobenius      1.70e-07  split5120 (1, 8, 2, 0) (2e-5)
The last half block of the ragged cases holds 1.0e-3 (65,856 paths) to 7.8e-2
(832 paths) of the fp64 loss sum and moves the fp64 gradient by as much.  No
case exposed a fault in the kernels or the launcher."""
import numpy as np
import pytest
import torch

from test_gpu_lm import _setup, decode_gram
from test_lm_geometry_cpu import CASE, CASES, WPS, case_blocks, case_geometry, wave_paths

pytestmark = pytest.mark.gpu

ST_COUNT = 3  # the statistics of a packet row / of the reduced block: [loss sum, sum |e|, sum |e| / |y|, paths]
LOSS_TOL, G_TOL, GRAM_TOL = 1e-5, 2e-5, 2e-5

_REFS, _GRAMS = {}, {}


def fp64_reference(shape, n, seed=0):
    """fp64 torch at the _setup weights: the gradient of mean((V - y)^2), the
    loss sum, and both without the last 64 paths (the half block of a ragged
    batch; still a mean over n).  Once per (shape, n), read-only."""
    from rphedge.models.hedge_mlp import NetSpec, init_weights, torch_forward
    from test_lm_cpu import _teacher_problem

    if (shape, n, seed) in _REFS:
        return _REFS[(shape, n, seed)]
    spec = NetSpec(*shape)
    feats, pr, y = _teacher_problem(spec, n, seed)
    y = y + 0.05 * torch.sin(7 * feats[0])
    X = (torch.stack(feats, 1).double() - 0.1) * 1.5
    Pm = torch.stack([p.double() for p in pr] + [torch.full((n,), 1.01, dtype=torch.float64)], 1)
    w0 = np.asarray(init_weights(spec, [0.5] * spec.nout, seed=1), np.float64)
    wt = torch.tensor(w0, requires_grad=True)
    e = (torch_forward(spec, wt, X) * Pm).sum(1) - y.double()
    head = (e[:n - 64] ** 2).sum() / n
    g_head, = torch.autograd.grad(head, wt, retain_graph=True)
    g, = torch.autograd.grad((e * e).sum() / n, wt)
    r = dict(spec=spec, X=X, Pm=Pm, w=wt.detach(), g=g.numpy().copy(), g_head=g_head.numpy().copy(),
             loss=float((e * e).sum().detach()), loss_tail=float((e[n - 64:] ** 2).sum().detach()))
    for k in ("g", "g_head"):
        r[k].setflags(write=False)
    _REFS[(shape, n, seed)] = r
    return r


def gram_reference(shape, n, seed, gw, blk, stride):
    """J^T J / ns in fp64 over the subsample of ns = 64 gw paths: the first
    ``blk`` paths of every aligned block of ``stride`` paths."""
    from rphedge.models.hedge_mlp import torch_forward
    from torch.func import jacrev, vmap

    key = (shape, n, seed, gw, blk, stride)
    if key not in _GRAMS:
        r = fp64_reference(shape, n, seed)
        ns = 64 * gw
        sub = torch.tensor([(j // blk) * stride + j % blk for j in range(ns)])
        assert int(sub.max()) < n and len(set(sub.tolist())) == ns
        J = vmap(jacrev(lambda ww, x, p: (torch_forward(r["spec"], ww, x[None])[0] * p).sum()), in_dims=(None, 0, 0))(
            r["w"], r["X"][sub], r["Pm"][sub])
        G = (J.T @ J).numpy() / ns
        G.setflags(write=False)
        _GRAMS[key] = G
    return _GRAMS[key]


def tail_is_visible(ref):
    """Whether a dropped last half block would fail the loss and the gradient
    check (from the fp64 reference alone): its share of the loss sum is at
    least 100 x the loss tolerance, and removing it moves the gradient by more
    than 10 x the gradient tolerance."""
    share = ref["loss_tail"] / ref["loss"]
    move = np.linalg.norm(ref["g"] - ref["g_head"]) / np.linalg.norm(ref["g"])
    return share, move, share >= 100 * LOSS_TOL and move > 10 * G_TOL


def _launch(case, shape):
    """Pass 0 + reduce of the case's geometry on NaN-filled buffers: (reduced
    block, packet rows, LmDesc geometry, (P, R, Gram blocks))."""
    from rphedge.engine import FitConfig, HipBackend, TrainConfig

    dev = torch.device("cuda", 0)
    n = case["n"]
    spec, feats, pr, y, data, w0 = _setup(shape, n, dev, seed=case["seed"])
    kw = dict(lm_gram_overlap=case["overlap"]) if case["leaf_paths"] >= 0 else {}
    be = HipBackend(spec, n, TrainConfig(batch_size=n, lm_gram_paths=case["gram_paths"],
                                         lm_leaf_paths=case["leaf_paths"], **kw), device=dev)
    assert be.native.lm_pass_wps(*shape) == WPS[shape]
    geo = case_geometry(case, WPS[shape])
    b = be._lm_buffers()
    w, o, f = be.new_weights(w0), be.new_opt(), be.new_fit()
    d = be._train_desc(w, o, f, data, FitConfig(), 0, None)
    d.batch, d.steps_per_epoch, d.shuffle, d.inv_batch = n, 1, 0, 1.0 / n
    lm = b["desc"]
    be._lm_gram_mode(lm, data)
    lm.passes = 1
    # the natural geometry is what the host mirror says; the overrides stay inside its buffers
    assert (int(lm.num_wgs), int(lm.gram_wgs)) == (geo["natural_wgs"], geo["natural_gram_wgs"])
    assert tuple(b["slab_b"].shape) == (geo["natural_wgs"], be._lm_shape[1])
    assert b["slab_g"].shape[0] >= geo["gram_wgs"] and geo["num_wgs"] <= geo["natural_wgs"]
    if case["leaf_paths"] >= 0:
        assert int(lm.gram_base) == (int(lm.num_wgs) if case["overlap"] else 0)
    for k, v in case["over"].items():
        setattr(lm, k, v)
    if case["gram_k"] is not None:
        lm.gram_wgs, lm.gram_blk, lm.gram_blk_stride = geo["gram_wgs"], geo["gram_blk"], geo["gram_blk_stride"]
        lm.inv_ns = geo["inv_ns"]
    lm.gram_base = geo["gram_base"]
    for k in ("num_wgs", "leaf_blocks", "gram_wgs", "gram_blk", "gram_blk_stride", "gram_skip", "gram_base"):
        assert int(getattr(lm, k)) == geo[k], k
    assert int(lm.dp_fused) == 0 and int(lm.gram_side) == 0 and int(lm.inst) == 1
    for k in ("red", "slab_b", "slab_g"):
        b[k].fill_(float("nan"))
    be.native.lm_eval(d, lm, b["red"], 0, None)
    torch.cuda.synchronize()
    return b["red"].cpu().numpy().copy(), b["slab_b"].cpu().numpy().copy(), geo, be._lm_shape


def _check(case, shape):
    from rphedge.ops import layout as L

    n = case["n"]
    red, slab_b, geo, (P, R, nblk) = _launch(case, shape)
    ref = fp64_reference(shape, n, case["seed"])
    assert P == ref["spec"].nparams
    G_ref = gram_reference(shape, n, case["seed"], geo["gram_wgs"], geo["gram_blk"], geo["gram_blk_stride"])
    nw = geo["num_wgs"]
    g = red[L.LM_GBLK_MAX:L.LM_GBLK_MAX + P]
    st = red[L.LM_GBLK_MAX + L.LM_NPMAX:L.LM_GBLK_MAX + L.LM_NPMAX + 4]
    # 1. every entry the net owns was written by this evaluation
    assert not np.isnan(red[:nblk * 1024]).any() and not np.isnan(g).any() and not np.isnan(st).any()
    # 2. every path counted once
    assert st[ST_COUNT] == n
    # 3. the schedule itself: the paths of every workgroup's four waves, exactly; no row past the grid written
    regime, blocks = case_blocks(case, WPS[shape])
    assert regime == case["expect"][0]
    want = np.array([sum(wave_paths(blocks[4 * w + k], n) for k in range(4)) for w in range(nw)], np.float32)
    assert want.sum() == n
    assert np.array_equal(slab_b[:nw, P + ST_COUNT], want), (slab_b[:nw, P + ST_COUNT], want)
    assert np.isfinite(slab_b[:nw]).all() and np.isnan(slab_b[nw:]).all()
    for w in np.flatnonzero(want == 0):  # a workgroup without paths: an all-zero row
        assert not slab_b[w].any()
    # 4. - 6. against fp64
    e_loss = abs(st[0] - ref["loss"]) / ref["loss"]
    e_g = np.linalg.norm(g - ref["g"]) / np.linalg.norm(ref["g"])
    e_gmax = np.abs(g - ref["g"]).max() / np.abs(ref["g"]).max()
    e_gram = np.linalg.norm(decode_gram(red, P) - G_ref) / np.linalg.norm(G_ref)
    print(f"lm geometry {case['name']} {shape}: loss {e_loss:.3e} g {e_g:.3e} g entrywise {e_gmax:.3e} "
          f"Gram {e_gram:.3e}")
    if n % 128:
        share, move, ok = tail_is_visible(ref)
        print(f"  tail: loss share {share:.3e} (>= {100 * LOSS_TOL:.0e}), gradient move {move:.3e} (> {10 * G_TOL:.0e})")
        assert ok, (share, move)
    assert e_loss <= LOSS_TOL
    assert e_g < G_TOL
    assert (np.abs(g - ref["g"]) <= G_TOL * np.abs(ref["g"]).max()).all()
    assert e_gram < GRAM_TOL


def _params(prefix):
    return [pytest.param(c["name"], s, id=f"{c['name']}-{'x'.join(map(str, s))}")
            for c in CASES if c["name"].startswith(prefix) for s in c["shapes"]]


@pytest.mark.parametrize("name,shape", _params("nat"))
def test_natural_geometry_matches_fp64(name, shape):
    """The geometry HipBackend builds, 1 to 257 packet rows: both sides of the
    16-, 32- and 256-row thresholds of the packet trees and of the 16-slab
    threshold of the Gram trees; masked rows; ragged batches."""
    _check(CASE[name], shape)


@pytest.mark.parametrize("name,shape", _params("split"))
def test_split_schedule_matches_fp64(name, shape):
    """The split block schedule (the production one, which the natural
    geometry enters from 2^19 paths on): the Gram workgroups' waves take per -
    gram_skip blocks, the others the rest and the remainder."""
    _check(CASE[name], shape)


@pytest.mark.parametrize("name,shape", _params("leaf"))
def test_leaf_schedule_and_gram_placement_match_fp64(name, shape):
    """Contiguous leaves with a clipped and an empty leaf, the Gram tiles in
    the first workgroups of the grid and in Gram-only workgroups after the
    path grid."""
    _check(CASE[name], shape)


def test_leaves_that_do_not_cover_the_shard_are_refused():
    """leaf_blocks x 512 x num_wgs < batch: the launcher refuses before any launch."""
    from rphedge.engine import FitConfig, HipBackend, TrainConfig

    dev = torch.device("cuda", 0)
    n = 5184
    spec, feats, pr, y, data, w0 = _setup((1, 8, 2, 0), n, dev)
    be = HipBackend(spec, n, TrainConfig(batch_size=n, lm_gram_paths=1024), device=dev)
    b = be._lm_buffers()
    d = be._train_desc(be.new_weights(w0), be.new_opt(), be.new_fit(), data, FitConfig(), 0, None)
    d.batch, d.steps_per_epoch, d.shuffle, d.inv_batch = n, 1, 0, 1.0 / n
    lm = b["desc"]
    be._lm_gram_mode(lm, data)
    lm.passes, lm.num_wgs, lm.leaf_blocks = 1, 3, 3  # 36 blocks of the 41
    b["red"].fill_(float("nan"))
    with pytest.raises(RuntimeError, match="leaf_blocks: the waves' leaves must cover the shard"):
        be.native.lm_eval(d, lm, b["red"], 0, None)
    torch.cuda.synchronize()
    assert torch.isnan(b["red"]).all()  # nothing ran
    lm.leaf_blocks = 4
    be.native.lm_eval(d, lm, b["red"], 0, None)  # the covering schedule is accepted
    torch.cuda.synchronize()
