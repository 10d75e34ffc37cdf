"""The final evaluation of an lm_out_fix fit (k_lm_pass<BodyOG>, NarrowPairBody
FINAL, csrc/hedge_narrow.h): the backward stops at the output layer, so the
reduced block holds the four statistics, the gradient of the output block
[P - NU, P), the full-batch output Gram - and exact zeros at the hidden
layers' gradient.  What remains is BITWISE what the plain body computes."""
import numpy as np
import pytest
import torch

from test_lm_cpu import _teacher_problem

pytestmark = pytest.mark.gpu

# (1, 8, 2, 0): packed-pair accumulators; (1, 8, 1, 1): complement head, scalar
# accumulators; (2, 8, 2, 0): two inputs; (5, 8, 6, 0): R = 256, NU = 54 (three
# output-Gram blocks); (6, 8, 7, 0): odd NO (scalar accumulators), NU = 63
SHAPES = [(1, 8, 2, 0), (1, 8, 1, 1), (2, 8, 2, 0), (5, 8, 6, 0), (6, 8, 7, 0)]
# 2^13 paths: 64 blocks of 128 on 32 workgroups x 4 waves - half of the waves
# get one block, the others none; + 64: a 65th block whose second half is past
# the end of the batch (the mask m of the statistics, the output gradient and
# og_accum), and wave 0 runs two blocks
NS = [1 << 13, (1 << 13) + 64]

# Relative Frobenius error of the decoded output Gram against fp64, measured
# with the PARENT build (full-backward output-Gram body) on these inputs,
# n = 2^13 | 2^13 + 64 (the final body gives the same bits, so the same
# figures); the bound of test 2 is twice the parent's value.
# (BENCHMARKS.md quotes 1.8e-5 MAX relative per entry for the bf16 hi / lo
# split; the Frobenius figure is smaller.)
OG_ERR_PARENT = {
    ((1, 8, 2, 0), 1 << 13): 8.780265e-06, ((1, 8, 2, 0), (1 << 13) + 64): 8.774548e-06,
    ((1, 8, 1, 1), 1 << 13): 2.774760e-06, ((1, 8, 1, 1), (1 << 13) + 64): 2.747489e-06,
    ((2, 8, 2, 0), 1 << 13): 8.761525e-06, ((2, 8, 2, 0), (1 << 13) + 64): 8.763407e-06,
    ((5, 8, 6, 0), 1 << 13): 4.046345e-06, ((5, 8, 6, 0), (1 << 13) + 64): 4.047794e-06,
    ((6, 8, 7, 0), 1 << 13): 3.662783e-06, ((6, 8, 7, 0), (1 << 13) + 64): 3.667415e-06,
}


def _setup(shape, n, dev, seed=0):
    """(tests/test_gpu_lm.py::_setup, which test_gpu_lm_multistart.py uses too)"""
    from rphedge.engine import DateData
    from rphedge.models.hedge_mlp import NetSpec, init_weights

    spec = NetSpec(*shape)
    feats, pr, y = _teacher_problem(spec, n, seed)
    y = y + 0.05 * torch.sin(7 * feats[0])  # not exactly representable
    data = DateData(feats=[f.to(dev) for f in feats], prices_next=[p.to(dev) for p in pr], bond_next=1.01,
                    target=y.to(dev), prices_now=[p.to(dev) for p in pr], fmu=tuple([0.1] * spec.nin),
                    fisd=tuple([1.5] * spec.nin))
    w0 = init_weights(spec, [0.5] * spec.nout, seed=1)
    return spec, feats, pr, y, data, w0


def _nu(spec):
    from rphedge.engine import lm_out_nu

    return lm_out_nu(spec)


_RUNS = {}


def lm_eval_block(shape, n, passes):
    """The reduced block of ONE evaluation (pass 0) of the _setup weights with
    ``lm.passes = passes``: 1 = the plain body (full gradient, Gram tiles),
    0 = the final-evaluation body.  The block is NaN before the launch, so
    every entry a test reads was written by it.  Computed once per case."""
    key = (shape, n, passes)
    if key in _RUNS:
        return _RUNS[key]
    from rphedge.engine import FitConfig, HipBackend, TrainConfig

    dev = torch.device("cuda", 0)
    spec, feats, pr, y, data, w0 = _setup(shape, n, dev)
    be = HipBackend(spec, n, TrainConfig(batch_size=n, lm_gram_paths=2048, lm_out_fix=True), device=dev)
    b = be._lm_buffers()
    w, o, f = be.new_weights(w0), be.new_opt(), be.new_fit()
    d = be._train_desc(w, o, f, data, FitConfig(), 0, None)
    d.batch, d.steps_per_epoch, d.shuffle, d.inv_batch = n, 1, 0, 1.0 / n
    lm = b["desc"]
    assert lm.out_gram == 1 and lm.out_n == _nu(spec)
    lm.passes = passes
    lm.gram_skip = 0  # the final and the non-final path schedules coincide
    b["red"].fill_(float("nan"))
    be.native.lm_eval(d, lm, b["red"], 0, None)
    torch.cuda.synchronize()
    red = b["red"].cpu().numpy().copy()
    red.setflags(write=False)
    _RUNS[key] = dict(red=red, spec=spec, feats=feats, pr=pr, y=y, w0=w0, num_wgs=int(lm.num_wgs))
    return _RUNS[key]


def _parts(red, spec):
    from rphedge.ops import layout as L

    P = spec.nparams
    g = red[L.LM_GBLK_MAX:L.LM_GBLK_MAX + P]
    st = red[L.LM_GBLK_MAX + L.LM_NPMAX:L.LM_GBLK_MAX + L.LM_NPMAX + 4]
    return g, st


def decode_out_gram(red, nu):
    """Dense NU x NU matrix from the packed upper triangle (i <= j, row-major) at LM_RED_OUTG."""
    from rphedge.ops import layout as L

    G = np.zeros((nu, nu))
    iu = np.triu_indices(nu)
    G[iu] = red[L.LM_RED_OUTG:L.LM_RED_OUTG + nu * (nu + 1) // 2]
    return G + np.triu(G, 1).T


_REFS = {}


def fp64_reference(r, n):
    """fp64 torch: gradient of mean((V - y)^2), the loss sum and the output
    Gram U^T U / n with the rows u = [a2_j c_k (j, k), c_k] of og_accum
    (c = the held prices; complement head: c_0 = S - B).  Once per case."""
    from rphedge.models.hedge_mlp import torch_forward
    from rphedge.ops import layout as L

    spec = r["spec"]
    key = (spec.nin, spec.hidden, spec.nout, spec.head, n)
    if key in _REFS:
        return _REFS[key]
    X = (torch.stack(r["feats"], 1).double() - 0.1) * 1.5
    Pm = torch.stack([p.double() for p in r["pr"]] + [torch.full((n,), 1.01, dtype=torch.float64)], 1)
    wt = torch.tensor(np.asarray(r["w0"], np.float64), requires_grad=True)
    e = (torch_forward(spec, wt, X) * Pm).sum(1) - r["y"].double()
    ((e * e).sum() / n).backward()
    o, h = spec.offsets, spec.hidden
    w = wt.detach()
    a1 = torch.nn.functional.leaky_relu(X @ w[o["W1"]:o["b1"]].view(spec.nin, h) + w[o["b1"]:o["W2"]], spec.alpha)
    a2 = torch.nn.functional.leaky_relu(a1 @ w[o["W2"]:o["b2"]].view(h, h) + w[o["b2"]:o["W3"]], spec.alpha)
    c = (Pm[:, :1] - Pm[:, 1:2]) if spec.head == L.HEAD_COMPLEMENT else Pm
    U = torch.cat([(a2[:, :, None] * c[:, None, :]).reshape(n, -1), c], 1)
    assert U.shape[1] == _nu(spec)
    _REFS[key] = dict(g=wt.grad.numpy().copy(), loss_sum=float((e * e).sum().detach()), G=(U.T @ U).numpy() / n)
    return _REFS[key]


def out_gram_rel_err(shape, n):
    r = lm_eval_block(shape, n, 0)
    ref = fp64_reference(r, n)
    G = decode_out_gram(r["red"], _nu(r["spec"]))
    return float(np.linalg.norm(G - ref["G"]) / np.linalg.norm(ref["G"]))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES)
def test_final_block_equals_plain_pass_bitwise(shape, n):
    """The same weights evaluated by the plain body (A: passes = 1, pass 0) and
    by the final body (B: passes = 0, pass 0), same path schedule: the output
    block's gradient and the four statistics agree bit for bit, B's hidden
    gradient is exactly 0.0 (written by this evaluation: the block was NaN
    before), A's is not.  The backend accepts a batch that is no multiple of
    128, so n = 2^13 + 64 runs too."""
    a, b = lm_eval_block(shape, n, 1), lm_eval_block(shape, n, 0)
    spec = a["spec"]
    P, nu = spec.nparams, _nu(spec)
    ga, sa = _parts(a["red"], spec)
    gb, sb = _parts(b["red"], spec)
    assert a["num_wgs"] == b["num_wgs"] == 32
    assert np.isfinite(ga).all() and np.isfinite(gb).all() and np.isfinite(sa).all()
    assert np.array_equal(ga[P - nu:].view(np.uint64), gb[P - nu:].view(np.uint64))
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
    assert sb[3] == n
    assert np.array_equal(gb[:P - nu].view(np.uint64), np.zeros(P - nu, np.uint64))  # +0.0, every entry
    assert np.count_nonzero(ga[:P - nu]) > (P - nu) // 2
    assert np.count_nonzero(gb[P - nu:]) == nu


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES)
def test_final_body_output_gram_matches_fp64(shape, n):
    """The packed output Gram of the final body (mean over every path) against
    U^T U / n in fp64: relative Frobenius error at most twice what the parent
    build's output-Gram body gives on the same inputs (OG_ERR_PARENT)."""
    err = out_gram_rel_err(shape, n)
    print(f"output Gram rel. Frobenius error {shape} n={n}: {err:.3e} (parent {OG_ERR_PARENT[(shape, n)]})")
    assert err <= 2.0 * OG_ERR_PARENT[(shape, n)]


def test_final_body_512_row_case_matches_fp64():
    """(1, 8, 2, 0) at 2^17 paths: the plain passes run 512 workgroups, the
    final evaluation is clamped to 256 (lm_pass_desc).  Its output-block
    gradient, statistics and output Gram against fp64, with the tolerances of
    test_gpu_lm.py::test_lm_pass_block_matches_fp64."""
    shape, n = (1, 8, 2, 0), 1 << 17
    r = lm_eval_block(shape, n, 0)
    spec = r["spec"]
    P, nu = spec.nparams, _nu(spec)
    assert r["num_wgs"] == 512
    ref = fp64_reference(r, n)
    g, st = _parts(r["red"], spec)
    assert np.array_equal(g[:P - nu].view(np.uint64), np.zeros(P - nu, np.uint64))
    assert np.linalg.norm(g[P - nu:] - ref["g"][P - nu:]) / np.linalg.norm(ref["g"][P - nu:]) < 2e-5
    assert st[0] == pytest.approx(ref["loss_sum"], rel=1e-5) and st[3] == n
    G = decode_out_gram(r["red"], nu)
    assert np.linalg.norm(G - ref["G"]) / np.linalg.norm(ref["G"]) < 2e-5


def test_warm_started_two_pass_fit_is_bitwise_repeatable():
    """A warm-started 2-pass lm_out_fix fit (as the later dates of an
    induction) twice in one process: the published weights and
    FitState.best_loss are bit-equal (no read of uninitialised LDS or
    registers in the final body)."""
    from rphedge.engine import FitConfig, HipBackend, TrainConfig, current_weights
    from rphedge.ops import layout as L

    dev = torch.device("cuda", 0)
    n = 1 << 13
    spec, feats, pr, y, data, w0 = _setup((1, 8, 2, 0), n, dev, seed=21)
    b0 = HipBackend(spec, n, TrainConfig(batch_size=n, lm_gram_paths=2048), device=dev)
    w = b0.new_weights(w0)
    b0.fit(w, b0.new_opt(), b0.new_fit(), data, FitConfig(epochs=12, optimizer="lm", early_stopping=False), seed=0)
    torch.cuda.synchronize()
    w1 = current_weights(spec, w).copy()
    # (the two dampings at which test_gpu_lm_multistart.py's warm-started fits
    # take the output step at the best point and at the rejected last trial)
    for lam0 in (1.2, 2.0):
        outs = []
        for _ in range(2):
            tc = TrainConfig(batch_size=n, lm_gram_paths=2048, lm_out_fix=True, lm_lam0=lam0)
            be = HipBackend(spec, n, tc, device=dev)
            w, fit = be.new_weights(w1), be.new_fit()
            be.fit(w, be.new_opt(), fit, data, FitConfig(epochs=2, optimizer="lm", early_stopping=False), seed=0)
            torch.cuda.synchronize()
            outs.append((current_weights(spec, w).copy(), fit.cpu().numpy().copy()))
        assert np.isfinite(outs[0][0]).all() and outs[0][0].tobytes() == outs[1][0].tobytes(), lam0
        b0_, b1_ = outs[0][1][L.F_BEST:L.F_BEST + 1], outs[1][1][L.F_BEST:L.F_BEST + 1]
        assert np.isfinite(b0_).all() and b0_.tobytes() == b1_.tobytes(), lam0
