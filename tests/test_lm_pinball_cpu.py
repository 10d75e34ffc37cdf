"""The inputs of tests/test_gpu_lm_pinball_geometry.py, stated and checked on
the host: a pinball (quantile) LM problem with residuals on BOTH sides of the
hedge, built from the fp64 evaluation alone, and its fp64 reference - loss
vector, subgradient with the kernel's tie rule (csrc/hedge_core.h path_loss),
gradient, statistics and the IRLS-weighted Gram (csrc/hedge_lm.hip k_lm_pass).

_setup's targets (tests/test_gpu_lm.py) sit above the start weights' hedge on
99 - 100 % of the paths of every free-head net, so a pinball evaluation on them
takes one side of the subgradient only.  pinball_problem shifts the targets to
a chosen share above the hedge and moves every path nearer to it than
``margin`` away, so that no fp32 rounding of V can change a path's side.  The
conditions the GPU tests rest on (branch mix of the subgradient and of the row
weights, a visible ragged tail) are asserted here for every GPU case, so those
tests cannot pass vacuously; engine.lm_ref.make_eval, the oracle of the
fit-level tests, is pinned to the same statement."""
import numpy as np
import pytest
import torch

from test_lm_cpu import _teacher_problem
from test_lm_geometry_cpu import CASE, S_1811, S_1820, WPS, _case, case_geometry

# The bounds of the GPU module (there: the measured maxima).  Loss, sum |e| and
# sum |e| / |y| relative; gradient relative 2-norm and entrywise over max |g|;
# Gram relative Frobenius.  The project's MSE bounds (tests/test_gpu_lm_geometry.py).
LOSS_TOL, G_TOL, GRAM_TOL, APE_TOL = 1e-5, 2e-5, 2e-5, 1e-5
TILE = 64        # LM_TILE: paths of a Gram tile
MARGIN = 1e-4    # two orders of magnitude above the fp32 forward error of these O(1) values
Q_KAPPA, Q_DELTA = 3.0, 1e-5  # the default row-weight setting (FitConfig.lm_q_kappa, the tests' lm_q_delta)

# ---------------------------------------------------------------------------
# The GPU cases: (launch geometry of tests/test_lm_geometry_cpu.py CASES, net,
# quantile, row-weight setting).
# ---------------------------------------------------------------------------
PIN_CASES = ["nat256", "nat832", "nat4416", "nat8512", "split5184", "split10304s1", "leaf5184ov", "leaf4416"]
Q_CASES, Q_EXTRA = ["nat832", "split5184"], [0.5, 0.05]
W_CASE, W_EXTRA = "nat4416", ["small_kappa", "mixed_floor", "all_floor"]
PIN_PARAMS = [(c, s, 0.99, "default") for c in PIN_CASES for s in CASE[c]["shapes"]] + \
    [(c, s, q, "default") for c in Q_CASES for q in Q_EXTRA for s in CASE[c]["shapes"]] + \
    [(W_CASE, s, 0.99, w) for w in W_EXTRA for s in CASE[W_CASE]["shapes"]]
# the geometries of the single-purpose GPU tests: a 4096-path Gram subsample on 16 path workgroups (48 Gram-only
# workgroups), and the 768 paths of the exact-tie problem
SIDE_CASE = _case("side4096", 4096, [S_1820], ("cyclic", None, "one", "lds", 16, 64), gram_paths=4096)
TIE_CASE = _case("tie768", 768, [S_1820, S_1811], ("cyclic", None, "one", "thread", 3, 4), gram_paths=256)


def pin_id(p):
    return f"{p[0]}-{'x'.join(map(str, p[1]))}-q{p[2]}-{p[3]}"


_PROBS, _REFS, _JACS = {}, {}, {}


def make_problem(key, spec, X, Pm, w, y32):
    """The fp64 statement of one evaluation: standardised inputs X, prices Pm
    (with the bond column), weights w (fp64), targets y32 (fp32, as the kernel
    reads them); V and the residuals r = y - V in fp64."""
    from rphedge.models.hedge_mlp import torch_forward

    assert y32.dtype == torch.float32 and X.dtype == Pm.dtype == w.dtype == torch.float64
    V = (torch_forward(spec, w, X) * Pm).sum(1)
    return dict(key=key, spec=spec, n=len(y32), X=X, Pm=Pm, w=w, y=y32, V=V, r=y32.double() - V)


def pinball_problem(shape, n, seed, above=0.3, margin=MARGIN):
    """_setup's problem (tests/test_gpu_lm.py: the teacher data, its start
    weights) with two-sided residuals: V in fp64 at the start weights; the
    targets shifted by the (1 - above) quantile of y - V, so that ``above`` of
    the paths end above the hedge; every path with |y - V| < margin re-pinned
    to V +- 2 margin on the side it is on.  Targets stay fp32.  Returns the
    problem (make_problem) with ``repinned``, the number of re-pinned paths.
    Once per argument tuple, read-only; the fp64 pieces that depend on the
    quantile are pinball_reference's."""
    from rphedge.models.hedge_mlp import NetSpec, init_weights

    key = (tuple(shape), n, seed, above, margin)
    if key in _PROBS:
        return _PROBS[key]
    spec = NetSpec(*shape)
    feats, pr, y = _teacher_problem(spec, n, seed)
    y = y + 0.05 * torch.sin(7 * feats[0])
    X = (torch.stack(feats, 1).double() - 0.1) * 1.5
    Pm = torch.stack([p.double() for p in pr] + [torch.full((n,), 1.01, dtype=torch.float64)], 1)
    w = torch.tensor(np.asarray(init_weights(spec, [0.5] * spec.nout, seed=1), np.float64))
    p0 = make_problem(None, spec, X, Pm, w, y)
    y1 = (y.double() - torch.quantile(p0["r"], 1.0 - above)).float()
    r1 = y1.double() - p0["V"]
    near = r1.abs() < margin
    side = torch.where(r1 >= 0, 1.0, -1.0).double()
    y1 = torch.where(near, (p0["V"] + 2.0 * margin * side).float(), y1)
    prob = make_problem(key, spec, X, Pm, w, y1)
    prob["repinned"] = int(near.sum())
    assert float(prob["r"].abs().min()) >= margin
    assert bool(((prob["r"] > 0) == (r1 >= 0)).all())  # every path kept its side
    _PROBS[key] = prob
    return prob


def pinball_reference(prob, q, strict=False):
    """fp64 pinball evaluation of ``prob`` at the quantile the descriptor
    holds (fp32): the loss vector max(q e, (q - 1) e) of e = y - V, dL/dV with
    the kernel's tie rule (q e >= (q - 1) e takes -q, so a tie does; ``strict``:
    the opposite rule), the gradient of mean(loss), the statistics sum |e| and
    sum |e| / max(|y|, 1e-7) (``ape_big``: over the paths with |y| >= 1e-3
    alone), and loss and gradient without the last 64 paths (the half block of
    a ragged batch; still a mean over n)."""
    from rphedge.models.hedge_mlp import torch_forward

    q = float(np.float32(q))
    key = (prob["key"], q, strict)
    if key in _REFS:
        return _REFS[key]
    n, e = prob["n"], prob["r"]
    pos = (q * e > (q - 1.0) * e) if strict else (q * e >= (q - 1.0) * e)
    lvec = torch.where(pos, q * e, (q - 1.0) * e)
    dV = torch.where(pos, torch.full_like(e, -q), torch.full_like(e, 1.0 - q))
    wt = prob["w"].clone().requires_grad_(True)
    V = (torch_forward(prob["spec"], wt, prob["X"]) * prob["Pm"]).sum(1)
    g_head, = torch.autograd.grad((dV[:n - 64] * V[:n - 64]).sum() / n, wt, retain_graph=True)
    g, = torch.autograd.grad((dV * V).sum() / n, wt)
    ya = prob["y"].double().abs()
    ape = e.abs() / ya.clamp_min(1e-7)
    r = dict(q=q, lvec=lvec, dV=dV, g=g.numpy().copy(), g_head=g_head.numpy().copy(), loss=float(lvec.sum()),
             loss_tail=float(lvec[n - 64:].sum()), abs=float(e.abs().sum()), ape=float(ape.sum()),
             ape_big=float(ape[ya >= 1e-3].sum()), above=float((e > 0).double().mean()))
    for k in ("g", "g_head"):
        r[k].setflags(write=False)
    _REFS[key] = r
    return r


def subsample(gw, blk, stride):
    """Path of every slot of the Gram subsample (LmDesc.gram_wgs / gram_blk / gram_blk_stride)."""
    return torch.tensor([(j // blk) * stride + j % blk for j in range(TILE * gw)])


def _jac(prob, geo3):
    from rphedge.models.hedge_mlp import torch_forward
    from torch.func import jacrev, vmap

    key = (prob["key"],) + tuple(geo3)
    if key not in _JACS:
        sub = subsample(*geo3)
        assert int(sub.max()) < prob["n"] and len(set(sub.tolist())) == len(sub)
        _JACS[key] = vmap(jacrev(lambda ww, x, p: (torch_forward(prob["spec"], ww, x[None])[0] * p).sum()),
                          in_dims=(None, 0, 0))(prob["w"], prob["X"][sub], prob["Pm"][sub])
    return _JACS[key]


def tile_scale(prob, geo3, r_sub=None):
    """Mean |r| of every 64-path Gram tile, fp64 (``r_sub``: the subsample's own residuals)."""
    ra = (prob["r"][subsample(*geo3)] if r_sub is None else r_sub).abs().view(-1, TILE)
    return ra, ra.mean(1, keepdim=True)


def gram_reference(prob, geo3, q_kappa, q_delta, r_sub=None):
    """mean_p w_p J_p J_p^T over the subsample in fp64, the row scaled by
    1 / (2 sqrt(max(|r_p|, dl))), dl = max(q_delta, q_kappa x the tile's mean
    |r|) (both as the descriptor holds them, fp32) -> (G, share of the tiles on
    the q_delta branch, share of the paths with |r| >= dl)."""
    q_kappa, q_delta = float(np.float32(q_kappa)), float(np.float32(q_delta))
    J = _jac(prob, geo3)
    ra, mean = tile_scale(prob, geo3, r_sub)
    dl = torch.clamp_min(q_kappa * mean, q_delta)
    Js = J * (0.5 / torch.sqrt(torch.maximum(ra, dl).reshape(-1)))[:, None]
    return (Js.T @ Js).numpy() / len(J), float((q_delta > q_kappa * mean).double().mean()), \
        float((ra >= dl).double().mean())


def weight_setting(name, prob, geo3):
    """(q_kappa, q_delta) of a row-weight setting, from the fp64 tile means alone."""
    _, mean = tile_scale(prob, geo3)
    if name == "default":
        return Q_KAPPA, Q_DELTA
    if name == "small_kappa":
        return 0.5, Q_DELTA
    if name == "mixed_floor":  # the median tile's delta: the tiles below it take the floor
        return Q_KAPPA, float(np.float32(float((Q_KAPPA * mean).median())))
    assert name == "all_floor"
    return Q_KAPPA, float(np.float32(4.0 * float((Q_KAPPA * mean).max())))


def case_sub(case, shape):
    g = case_geometry(case, WPS[shape])
    return g["gram_wgs"], g["gram_blk"], g["gram_blk_stride"]


def tail_is_visible(ref):
    """Whether a dropped last half block would fail the loss and the gradient
    check (from the fp64 reference alone): it holds at least 100 x the loss
    tolerance of the loss sum, and removing it moves the gradient by more than
    10 x the gradient tolerance."""
    share = ref["loss_tail"] / ref["loss"]
    move = np.linalg.norm(ref["g"] - ref["g_head"]) / np.linalg.norm(ref["g"])
    return share, move, share >= 100 * LOSS_TOL and move > 10 * G_TOL


def side_targets(prob, geo3):
    """Targets of a simulated Gram subsample that differ from the shard's: the
    shard's at the subsample's paths plus 0.05 cos(slot), fp32."""
    sub = subsample(*geo3)
    return (prob["y"][sub].double() + 0.05 * torch.cos(torch.arange(len(sub), dtype=torch.float64))).float()


def tie_problem(shape, n=768):
    """A problem whose V is exact and identical in fp32 and fp64, with exact
    ties: W3 = 0 (the holdings are the output biases 0.5, 0.25), bond 1, prices
    multiples of 2^-10 in [0.75, 1.25]; targets V, V + 0.125, V - 0.125 by path
    index mod 3 (every Gram tile holds all three)."""
    from rphedge.models.hedge_mlp import NetSpec, init_weights

    key = ("tie", tuple(shape), n)
    if key in _PROBS:
        return _PROBS[key]
    spec = NetSpec(*shape)
    feats, pr, _ = _teacher_problem(spec, n, 0)
    g = torch.Generator().manual_seed(11)
    pr = [0.75 + torch.randint(0, 513, (n,), generator=g).float() / 1024.0 for _ in pr]
    w0 = np.asarray(init_weights(spec, [0.5] * spec.nout, seed=1), np.float32)
    o = spec.offsets
    w0[o["W3"]:o["b3"]] = 0.0
    w0[o["b3"]:o["P"]] = [0.5, 0.25][:spec.nout]
    X = (torch.stack(feats, 1).double() - 0.1) * 1.5
    Pm = torch.stack([p.double() for p in pr] + [torch.ones(n, dtype=torch.float64)], 1)
    w = torch.tensor(w0.astype(np.float64))
    V = make_problem(None, spec, X, Pm, w, torch.zeros(n))["V"]
    assert torch.equal(V.float().double(), V) and torch.equal(V * 2048, (V * 2048).round())  # exact in fp32
    y = (V + 0.125 * torch.tensor([0.0, 1.0, -1.0], dtype=torch.float64)[torch.arange(n) % 3]).float()
    prob = make_problem(key, spec, X, Pm, w, y)
    prob.update(feats=feats, prices=pr, w0=w0)
    assert set(prob["r"].tolist()) == {0.0, 0.125, -0.125}
    _PROBS[key] = prob
    return prob


# ---------------------------------------------------------------------------
# The conditions on the inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", PIN_PARAMS, ids=pin_id)
def test_gpu_case_inputs_take_both_sides_of_every_branch(p):
    """For the (case, net, quantile, row-weight setting) of a GPU case: few
    re-pinned paths, 25 - 35 % of the paths above the hedge, a visible tail on
    ragged batches, and the row-weight branch mix the setting is named for."""
    name, shape, q, setting = p
    case = CASE[name]
    n = case["n"]
    prob = pinball_problem(shape, n, case["seed"])
    ref = pinball_reference(prob, q)
    assert prob["repinned"] <= 0.01 * n, prob["repinned"]
    assert 0.25 <= ref["above"] <= 0.35, ref["above"]
    assert float(prob["r"].abs().min()) >= MARGIN
    assert ref["ape_big"] == ref["ape"]  # no target within 1e-3 of zero: sum |e| / |y| is compared whole
    # both sides of the subgradient, each with a share of the gradient no kernel could lose unnoticed
    assert set(np.unique(ref["dV"].numpy())) == {-ref["q"], 1.0 - ref["q"]}
    if n % 128:
        share, move, ok = tail_is_visible(ref)
        print(f"{pin_id(p)}: tail loss share {share:.3e}, gradient move {move:.3e}")
        assert ok, (share, move)
    geo3 = case_sub(case, shape)
    kappa, delta = weight_setting(setting, prob, geo3)
    _, floor_tiles, rows_above = gram_reference(prob, geo3, kappa, delta)
    print(f"{pin_id(p)}: q_kappa {kappa} q_delta {delta:.6g}: tiles on the q_delta branch {floor_tiles:.3f}, "
          f"paths with |r| >= dl {rows_above:.3f}")
    if setting == "default":
        assert floor_tiles == 0.0
    elif setting == "small_kappa":
        assert floor_tiles == 0.0 and 0.1 <= rows_above <= 0.9
    elif setting == "mixed_floor":
        assert 0.25 <= floor_tiles <= 0.75
    else:
        assert floor_tiles == 1.0 and rows_above == 0.0
    # (not asserted) the gradient's move if the path nearest to the hedge changed side: what an evaluation
    # without the margin would risk, and why the sizes stay small
    from rphedge.models.hedge_mlp import torch_forward

    k = int(prob["r"].abs().argmin())
    wt = prob["w"].clone().requires_grad_(True)
    jk, = torch.autograd.grad((torch_forward(prob["spec"], wt, prob["X"][k:k + 1])[0] * prob["Pm"][k]).sum(), wt)
    print(f"{pin_id(p)}: min |r| {float(prob['r'].abs().min()):.3e}; that path on the other side moves the "
          f"gradient by {float(jk.norm()) / n / np.linalg.norm(ref['g']):.3e} of its norm")


def test_row_weight_settings_differ_where_the_floor_matters():
    """Without the q_delta floor (dl = q_kappa x the tile mean alone) the
    mixed-floor and all-floor Grams differ from the reference by far more than
    the Gram bound: a kernel that dropped the floor fails those settings."""
    case = CASE[W_CASE]
    for shape in case["shapes"]:
        prob = pinball_problem(shape, case["n"], case["seed"])
        geo3 = case_sub(case, shape)
        G0, _, _ = gram_reference(prob, geo3, Q_KAPPA, 1e-30)
        for setting in ("mixed_floor", "all_floor"):
            G, _, _ = gram_reference(prob, geo3, *weight_setting(setting, prob, geo3))
            assert np.linalg.norm(G - G0) / np.linalg.norm(G) > 100 * GRAM_TOL


@pytest.mark.parametrize("p", PIN_PARAMS, ids=pin_id)
def test_make_eval_is_the_same_statement(p):
    """engine.lm_ref.make_eval (the oracle of the fit-level tests) on the
    problem of a GPU case equals this module's evaluation at 1e-12 relative:
    Gram (on make_eval's own, natural subsample), gradient and statistics."""
    from rphedge.engine import DateData, FitConfig, TorchBackend, TrainConfig, gram_subsample
    from rphedge.engine import lm_ref
    from rphedge.engine.state import design
    from rphedge.ops import layout as L

    name, shape, q, setting = p
    case = CASE[name]
    n = case["n"]
    prob = pinball_problem(shape, n, case["seed"])
    ref = pinball_reference(prob, q)
    ns, blk, stride = gram_subsample(n, case["gram_paths"])
    geo3 = (ns // TILE, blk, stride)
    kappa, delta = weight_setting(setting, prob, geo3)
    feats, pr, _ = _teacher_problem(prob["spec"], n, case["seed"])
    data = DateData(feats=feats, prices_next=pr, bond_next=1.01, target=prob["y"], prices_now=pr,
                    fmu=tuple([0.1] * prob["spec"].nin), fisd=tuple([1.5] * prob["spec"].nin))
    be = TorchBackend(prob["spec"], n, TrainConfig(batch_size=n, lm_gram_paths=case["gram_paths"]))
    fc = FitConfig(optimizer="lm", loss=L.LOSS_PINBALL, quantile=q, lm_q_delta=delta, lm_q_kappa=kappa)
    xpy = design(data.feats, data.prices_next, data.bond_next, data.target, data, lm_ref.DT)
    G, g, st = lm_ref.make_eval(be, fc, xpy, n, 1, main=data)(prob["w"])
    G_ref, _, _ = gram_reference(prob, geo3, kappa, delta)
    rel = lambda a, b: np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)  # noqa: E731
    assert rel(G.numpy(), G_ref) < 1e-12
    assert rel(g.numpy(), ref["g"]) < 1e-12
    assert rel(st.numpy(), np.array([ref["loss"], ref["abs"], ref["ape"], float(n)])) < 1e-12
    for k, v in enumerate((ref["loss"], ref["abs"], ref["ape"], float(n))):
        assert abs(float(st[k]) - v) <= 1e-12 * abs(v), k


def test_side_targets_separate_gtarget_from_the_shard_target():
    """The simulated subsample's targets of the gram_side GPU test: a Gram
    weighted by the shard's own targets instead differs from the reference by
    far more than the Gram bound, so a kernel reading TrainDesc.target fails."""
    shape = SIDE_CASE["shapes"][0]
    prob = pinball_problem(shape, SIDE_CASE["n"], SIDE_CASE["seed"])
    geo3 = case_sub(SIDE_CASE, shape)
    assert geo3[0] == 64 and case_geometry(SIDE_CASE, WPS[shape])["num_wgs"] == 16
    r_sub = side_targets(prob, geo3).double() - prob["V"][subsample(*geo3)]
    G_ref, floor_tiles, _ = gram_reference(prob, geo3, Q_KAPPA, Q_DELTA, r_sub=r_sub)
    G_shard, _, _ = gram_reference(prob, geo3, Q_KAPPA, Q_DELTA)
    assert floor_tiles == 0.0
    assert np.linalg.norm(G_shard - G_ref) / np.linalg.norm(G_ref) > 100 * GRAM_TOL


@pytest.mark.parametrize("shape", TIE_CASE["shapes"])
def test_tie_problem_separates_the_tie_rules(shape):
    """A third of the paths tie exactly; the opposite tie rule moves the
    output-bias gradient by far more than the gradient bound, and tied rows
    carry the weight 0.5 / sqrt(dl) (|r| = 0 < dl on every tile)."""
    prob = tie_problem(shape)
    n, o = prob["n"], prob["spec"].offsets
    ref, other = pinball_reference(prob, 0.99), pinball_reference(prob, 0.99, strict=True)
    tied = prob["r"] == 0
    assert int(tied.sum()) == n // 3 and bool((ref["dV"][tied] == -ref["q"]).all()) and \
        bool((other["dV"][tied] == 1.0 - ref["q"]).all()) and bool((ref["lvec"][tied] == 0).all())
    b3 = slice(o["b3"], o["P"])
    assert np.abs(ref["g"][b3] - other["g"][b3]).max() > 100 * G_TOL * np.abs(ref["g"]).max()
    geo3 = case_sub(TIE_CASE, shape)
    sub = subsample(*geo3)
    assert all(set((sub.view(-1, TILE)[t] % 3).tolist()) == {0, 1, 2} for t in range(geo3[0]))
    _, floor_tiles, rows_above = gram_reference(prob, geo3, Q_KAPPA, Q_DELTA)
    assert floor_tiles == 0.0 and rows_above == 0.0  # dl = 3 x mean |r| = 0.25 > 0.125 >= |r|
