"""One PINBALL evaluation of the LM chain (k_lm_pass -> k_lm_reduce,
csrc/hedge_lm.hip, TrainDesc.loss = LOSS_PINBALL) against fp64 torch, on both
sides of every branch the pinball path has of its own: the subgradient of
path_loss (csrc/hedge_core.h) in the packed and the scalar pass body
(csrc/hedge_narrow.h), the mask of a ragged batch on the pinball loss and
dL/dV, the IRLS row weight 0.5 rsq(max(|r|, dl)), dl = max(q_delta, q_kappa x
the tile's mean |r|), the LmDesc.gtarget read of a simulated Gram subsample,
exact ties, and the launcher's pinball rejections.  The problems and their
fp64 references are tests/test_lm_pinball_cpu.py's, which asserts on the host
that every case takes the branches it is named for; the launch geometries are
tests/test_lm_geometry_cpu.py CASES (cyclic, split and leaf schedules).

Measured on the MI355X, the largest over the 46 evaluations (bound):
  loss sum, relative            2.72e-07  nat256 (5, 8, 6, 0) q 0.99          (1e-5)
  sum |e|, relative             9.21e-08  nat256 (5, 8, 6, 0) q 0.99          (1e-5)
  sum |e| / |y|, relative       9.80e-08  split5184 (5, 8, 6, 0)              (1e-5)
  gradient, relative 2-norm     2.51e-07  tie768 (1, 8, 1, 1)                 (2e-5)
  gradient, entrywise / max|g|  2.51e-07  tie768 (1, 8, 1, 1)                 (2e-5)
  Gram, relative Frobenius      4.86e-07  nat4416 (1, 8, 2, 0) all on q_delta (2e-5)
Every maximum is below a tenth of the MSE bound of tests/test_gpu_lm_geometry.py,
so the pinball evaluation keeps those bounds: neither the hardware rsq nor the
fp32 tile mean of the row weight needed a wider one (the weight is continuous
where |r| crosses dl and where q_kappa x the tile mean crosses q_delta).  No
shifted target comes nearer to zero than 1e-3 in any case (the share of sum
|e| / |y| held by such paths is printed and is 0), so the rcp statistic is
compared whole, at the loss bound.  No case exposed a fault in the kernels or
the launcher.

Each of these deliberately wrong builds, tried once, fails the tests named and
no others: path_loss always returning -q - every evaluation of a two-sided
problem (all of test_pinball_evaluation_matches_fp64, the gtarget and the tie
tests; gradient off by 0.02 to 4.5 of its norm); `>` for `>=` in path_loss -
test_exact_ties_take_the_upper_branch alone; TrainDesc.target read in place of
LmDesc.gtarget - test_simulated_subsample_reads_its_own_targets alone; dl
without the q_delta floor - the mixed_floor and all_floor settings alone; the
pinball loss and dL/dV without the mask - the 40 evaluations of a ragged batch
alone (loss sum off by 2e-4 to 3e-2)."""
import numpy as np
import pytest
import torch

from test_gpu_lm import _setup, decode_gram
from test_lm_geometry_cpu import CASE, WPS, case_blocks, case_geometry, wave_paths
from test_lm_pinball_cpu import (APE_TOL, G_TOL, GRAM_TOL, LOSS_TOL, PIN_PARAMS, Q_DELTA, Q_KAPPA, SIDE_CASE, TIE_CASE,
                                 case_sub, gram_reference, pin_id, pinball_problem, pinball_reference, side_targets,
                                 subsample, tail_is_visible, tie_problem, weight_setting)

pytestmark = pytest.mark.gpu

ST_COUNT = 3  # [loss sum, sum |e|, sum |e| / |y|, paths]


def _prepare(case, shape, data, w0, q, q_kappa, q_delta, allow_side=False):
    """Backend, buffers and descriptors of one pinball evaluation in the
    case's geometry (the overrides stay inside the natural geometry's buffers),
    red / slab_b / slab_g NaN-filled."""
    from rphedge.engine import FitConfig, HipBackend, TrainConfig
    from rphedge.models.hedge_mlp import NetSpec
    from rphedge.ops import layout as L

    dev = torch.device("cuda", 0)
    n = case["n"]
    kw = dict(lm_gram_overlap=case["overlap"]) if case["leaf_paths"] >= 0 else {}
    be = HipBackend(NetSpec(*shape), n, TrainConfig(batch_size=n, lm_gram_paths=case["gram_paths"],
                                                     lm_leaf_paths=case["leaf_paths"], **kw), device=dev)
    assert be.native.lm_pass_wps(*shape) == WPS[shape]
    geo = case_geometry(case, WPS[shape])
    b = be._lm_buffers(L.LOSS_PINBALL)
    w, o, f = be.new_weights(w0), be.new_opt(), be.new_fit()
    d = be._train_desc(w, o, f, data, FitConfig(loss=L.LOSS_PINBALL, quantile=q), 0, None)
    d.batch, d.steps_per_epoch, d.shuffle, d.inv_batch = n, 1, 0, 1.0 / n
    d.loss, d.quantile = L.LOSS_PINBALL, q
    lm = b["desc"]
    be._lm_gram_mode(lm, data, allow_side=allow_side)
    lm.passes, lm.q_delta, lm.q_kappa = 1, q_delta, q_kappa
    assert lm.out_n == 0 and lm.out_gram == 0 and lm.bias_index == -1
    assert (int(lm.num_wgs), int(lm.gram_wgs)) == (geo["natural_wgs"], geo["natural_gram_wgs"])
    assert tuple(b["slab_b"].shape) == (geo["natural_wgs"], be._lm_shape[1])
    assert b["slab_g"].shape[0] >= geo["gram_wgs"] and geo["num_wgs"] <= geo["natural_wgs"]
    for k, v in case["over"].items():
        setattr(lm, k, v)
    if case["gram_k"] is not None:
        lm.gram_wgs, lm.gram_blk, lm.gram_blk_stride = geo["gram_wgs"], geo["gram_blk"], geo["gram_blk_stride"]
        lm.inv_ns = geo["inv_ns"]
    lm.gram_base = geo["gram_base"]
    for k in ("num_wgs", "leaf_blocks", "gram_wgs", "gram_blk", "gram_blk_stride", "gram_skip", "gram_base"):
        assert int(getattr(lm, k)) == geo[k], k
    assert int(lm.dp_fused) == 0 and int(lm.gram_side) == int(allow_side) and int(lm.inst) == 1
    for k in ("red", "slab_b", "slab_g"):
        b[k].fill_(float("nan"))
    return be, b, d, lm, geo, (w, o, f, data)  # (the last: the tensors the descriptors point into)


def _evaluate(case, shape, data, w0, q, q_kappa, q_delta, allow_side=False):
    be, b, d, lm, geo, keep = _prepare(case, shape, data, w0, q, q_kappa, q_delta, allow_side)
    be.native.lm_eval(d, lm, b["red"], 0, None)
    torch.cuda.synchronize()
    return b["red"].cpu().numpy().copy(), b["slab_b"].cpu().numpy().copy(), geo, be._lm_shape


def _check(label, case, shape, out, prob, ref, G_ref):
    """The four checks of one evaluation: everything written, every path
    counted once by the wave the schedule names, [loss | sum |e| | g | G]
    against fp64, sum |e| / |y| against fp64.  Prints the errors first."""
    from rphedge.ops import layout as L

    red, slab_b, geo, (P, R, nblk) = out
    n, nw = case["n"], geo["num_wgs"]
    assert P == prob["spec"].nparams and n == prob["n"]
    g = red[L.LM_GBLK_MAX:L.LM_GBLK_MAX + P]
    st = red[L.LM_GBLK_MAX + L.LM_NPMAX:L.LM_GBLK_MAX + L.LM_NPMAX + 4]
    e_loss = abs(st[0] - ref["loss"]) / ref["loss"]
    e_abs = abs(st[1] - ref["abs"]) / ref["abs"]
    e_ape = abs(st[2] - ref["ape"]) / ref["ape"]
    e_g = np.linalg.norm(g - ref["g"]) / np.linalg.norm(ref["g"])
    e_gmax = np.abs(g - ref["g"]).max() / np.abs(ref["g"]).max()
    e_gram = np.linalg.norm(decode_gram(red, P) - G_ref) / np.linalg.norm(G_ref)
    print(f"lm pinball {label}: loss {e_loss:.3e} abs {e_abs:.3e} ape {e_ape:.3e} g {e_g:.3e} "
          f"g entrywise {e_gmax:.3e} Gram {e_gram:.3e} (|y| < 1e-3 holds {1 - ref['ape_big'] / ref['ape']:.2e} "
          f"of sum |e| / |y|)")
    # 1. every entry the net owns was written by this evaluation
    assert not np.isnan(red[:nblk * 1024]).any() and not np.isnan(g).any() and not np.isnan(st).any()
    # 2. every path counted once; the paths of every workgroup's four waves, exactly; no row past the grid written
    assert st[ST_COUNT] == n
    regime, blocks = case_blocks(case, WPS[shape])
    assert regime == case["expect"][0]
    want = np.array([sum(wave_paths(blocks[4 * w + k], n) for k in range(4)) for w in range(nw)], np.float32)
    assert want.sum() == n
    assert np.array_equal(slab_b[:nw, P + ST_COUNT], want), (slab_b[:nw, P + ST_COUNT], want)
    assert np.isfinite(slab_b[:nw]).all() and np.isnan(slab_b[nw:]).all()
    for w in np.flatnonzero(want == 0):  # a workgroup without paths: an all-zero row
        assert not slab_b[w].any()
    # 3. against fp64
    assert e_loss <= LOSS_TOL
    assert e_abs <= LOSS_TOL
    assert e_g < G_TOL
    assert (np.abs(g - ref["g"]) <= G_TOL * np.abs(ref["g"]).max()).all()
    assert e_gram < GRAM_TOL
    # 4. the rcp statistic
    assert e_ape <= APE_TOL


@pytest.mark.parametrize("p", PIN_PARAMS, ids=pin_id)
def test_pinball_evaluation_matches_fp64(p):
    """Two-sided residuals (30 % of the paths above the hedge) in the cyclic,
    split and leaf schedules, ragged batches, q = 0.99 / 0.5 / 0.05, and the
    four row-weight settings: every tile on the q_kappa branch with and
    without paths at |r| >= dl, tiles on both sides of the q_delta floor, every
    tile on the floor."""
    name, shape, q, setting = p
    case = CASE[name]
    n = case["n"]
    prob = pinball_problem(shape, n, case["seed"])
    ref = pinball_reference(prob, q)
    geo3 = case_sub(case, shape)
    kappa, delta = weight_setting(setting, prob, geo3)
    G_ref, _, _ = gram_reference(prob, geo3, kappa, delta)
    dev = torch.device("cuda", 0)
    spec, feats, pr, y, data, w0 = _setup(shape, n, dev, seed=case["seed"])
    data.target = prob["y"].to(dev)
    if n % 128:
        assert tail_is_visible(ref)[2]
    _check(pin_id(p), case, shape, _evaluate(case, shape, data, w0, q, kappa, delta), prob, ref, G_ref)


def test_simulated_subsample_reads_its_own_targets():
    """gram_side with the pinball loss: the row weights come from
    LmDesc.gtarget (here the shard's targets plus 0.05 cos(slot)), never from
    TrainDesc.target; loss and gradient from the shard's.  16 path workgroups,
    64 Gram workgroups."""
    from rphedge.ops.paths import path_indices

    case, shape, q = SIDE_CASE, SIDE_CASE["shapes"][0], 0.99
    n = case["n"]
    prob = pinball_problem(shape, n, case["seed"])
    ref = pinball_reference(prob, q)
    geo3 = case_sub(case, shape)
    ns = 64 * geo3[0]
    assert ns == 4096 and (case_geometry(case, WPS[shape])["num_wgs"], geo3[0]) == (16, 64)
    sub = subsample(*geo3)
    assert np.array_equal(path_indices(ns, 0, geo3[1:]).astype(np.int64), sub.numpy())
    y_side = side_targets(prob, geo3)
    G_ref, _, _ = gram_reference(prob, geo3, Q_KAPPA, Q_DELTA, r_sub=y_side.double() - prob["V"][sub])
    G_shard, _, _ = gram_reference(prob, geo3, Q_KAPPA, Q_DELTA)
    # a kernel weighting the rows by the shard's targets fails the Gram check
    assert np.linalg.norm(G_shard - G_ref) / np.linalg.norm(G_ref) > 100 * GRAM_TOL
    dev = torch.device("cuda", 0)
    spec, feats, pr, y, data, w0 = _setup(shape, n, dev, seed=case["seed"])
    data.target = prob["y"].to(dev)
    data.gram_feats = [f.to(dev)[sub.to(dev)].contiguous() for f in feats]
    data.gram_prices_next = [p.to(dev)[sub.to(dev)].contiguous() for p in pr]
    data.gram_target = y_side.to(dev)
    out = _evaluate(case, shape, data, w0, q, Q_KAPPA, Q_DELTA, allow_side=True)
    _check("side4096", case, shape, out, prob, ref, G_ref)


@pytest.mark.parametrize("shape", TIE_CASE["shapes"])
def test_exact_ties_take_the_upper_branch(shape):
    """V exact and equal in fp32 and fp64; a third of the paths with y == V:
    they take dV = -q (q e >= (q - 1) e holds with equality) and loss 0, and a
    Gram row weight 0.5 / sqrt(dl).  The packed and the scalar pass body."""
    from rphedge.engine import DateData

    prob = tie_problem(shape)
    ref, other = pinball_reference(prob, 0.99), pinball_reference(prob, 0.99, strict=True)
    o = prob["spec"].offsets
    b3 = slice(o["b3"], o["P"])
    assert np.abs(ref["g"][b3] - other["g"][b3]).max() > 100 * G_TOL * np.abs(ref["g"]).max()
    geo3 = case_sub(TIE_CASE, shape)
    G_ref, _, _ = gram_reference(prob, geo3, Q_KAPPA, Q_DELTA)
    dev = torch.device("cuda", 0)
    nin = prob["spec"].nin
    data = DateData(feats=[f.to(dev) for f in prob["feats"]], prices_next=[p.to(dev) for p in prob["prices"]],
                    bond_next=1.0, target=prob["y"].to(dev), prices_now=[p.to(dev) for p in prob["prices"]],
                    fmu=tuple([0.1] * nin), fisd=tuple([1.5] * nin))
    out = _evaluate(TIE_CASE, shape, data, prob["w0"], 0.99, Q_KAPPA, Q_DELTA)
    _check(f"tie768 {shape}", TIE_CASE, shape, out, prob, ref, G_ref)


def test_pinball_descriptors_the_launcher_refuses():
    """An output Gram, an output or bias Newton step, q_delta = 0, and a
    simulated subsample without its targets: each refused before any launch
    (the reduced block stays NaN); the unmodified descriptor is accepted."""
    case, shape = SIDE_CASE, SIDE_CASE["shapes"][0]
    n = case["n"]
    prob = pinball_problem(shape, n, case["seed"])
    sub = subsample(*case_sub(case, shape))
    dev = torch.device("cuda", 0)
    spec, feats, pr, y, data, w0 = _setup(shape, n, dev, seed=case["seed"])
    data.target = prob["y"].to(dev)
    data.gram_feats = [f.to(dev)[sub.to(dev)].contiguous() for f in feats]
    data.gram_prices_next = [p.to(dev)[sub.to(dev)].contiguous() for p in pr]
    data.gram_target = prob["y"][sub].contiguous().to(dev)
    be, b, d, lm, geo, keep = _prepare(case, shape, data, w0, 0.99, Q_KAPPA, Q_DELTA, allow_side=True)
    gtarget = lm.gtarget
    assert gtarget and int(lm.gram_side) == 1
    for field, bad, good in (("out_gram", 1, 0), ("out_n", 1, 0), ("bias_index", 0, -1), ("q_delta", 0.0, Q_DELTA),
                             ("gtarget", None, gtarget)):
        setattr(lm, field, bad)
        with pytest.raises(RuntimeError, match="pinball LM fits"):
            be.native.lm_eval(d, lm, b["red"], 0, None)
        torch.cuda.synchronize()
        assert torch.isnan(b["red"]).all(), field  # nothing ran
        setattr(lm, field, good)
    be.native.lm_eval(d, lm, b["red"], 0, None)  # the valid descriptor is accepted
    torch.cuda.synchronize()
    assert not torch.isnan(b["red"][:be._lm_shape[2] * 1024]).any()
