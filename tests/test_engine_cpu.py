"""The engine package without a GPU: its exported names, the LM launch
descriptors HipBackend prepares on ``device="cpu"`` (values recorded from the
single-module engine this package replaced), their independence of the order
in which the launches are first prepared, and the geometry module on its own."""
import ctypes
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from rphedge.models.hedge_mlp import NetSpec, init_weights
from rphedge.ops import layout as L

N = 1 << 12
F32 = lambda v: float(np.float32(v))  # noqa: E731

EXPORTS = """MAXIN PNL_PPT GRAM_BLOCKS PERSISTENT_MAX_WGS DateData Exercise FitConfig PnlData TrainConfig HipBackend
TorchBackend make_backend current_weights set_weights make_weights make_opt fit_template fit_seed fit_summary reduce_stats
geometric_lr_schedule keras_lr_schedule gram_subsample lm_gram_geometry lm_pass_schedule lm_pass_wgs lm_out_nu lm_out_gram
lm_og_wgs lm_tpack_len lm_tpack_image _lm_out_n _lm_bias_index _normalise""".split()

# every fit's constants of the (1, 8, 2, 0) net on 2^12 paths, lm_gram_paths 2048, lm_out_fix
CONST = dict(red_wgs=203, lam_up=4.0, lam_down=F32(1 / 3), lam_min=F32(1e-9), lam_max=1e10, ridge=F32(1e-10),
             diag_floor=0.0, damping=0, gram_skip=3, out_mu=F32(1e-5), out_tr=0.0, leaf_blocks=0, dp_fused=0, gram_base=0,
             gram_side=0, renorm=0)
MAIN = dict(CONST, num_wgs=16, gram_wgs=32, gram_blk=256, gram_blk_stride=512, inv_ns=1 / 2048, inv_n=1 / 4096, out_n=18,
            out_gram=1, bias_index=105, inst=1, explore=0, weights_only=0, lam0=F32(1e-3))
EXPLORE = dict(CONST, inst=4, explore=1, weights_only=0, passes=2, num_wgs=8, gram_wgs=8, gram_blk=64, gram_blk_stride=256,
               inv_ns=1 / 512, inv_n=1 / 2048, out_n=0, out_gram=0, bias_index=105, lam0=F32(1e-3), lam_carry=0.0,
               stop_tol=0.0)
REFIT = dict(CONST, inst=1, explore=0, weights_only=1, passes=0, num_wgs=16, gram_wgs=1, gram_blk=8, gram_blk_stride=512,
             inv_ns=1 / 64, inv_n=1 / 4096, out_n=0, out_gram=0, bias_index=105, lam0=F32(1e-3), lam_carry=0.0, stop_tol=0.0)
PINBALL = dict(CONST, inst=1, explore=0, weights_only=0, passes=2, num_wgs=16, gram_wgs=32, gram_blk=256,
               gram_blk_stride=512, inv_ns=1 / 2048, inv_n=1 / 4096, out_n=0, out_gram=0, bias_index=-1, lam0=F32(1e-3),
               lam_carry=0.0, stop_tol=0.0, stop_min=2, q_delta=F32(1e-3), q_kappa=3.0)
BUFFER_POINTERS = ("state", "slab_b", "slab_g", "slab_o", "w0")


def _backend(world=1, **kw):
    from rphedge.engine import HipBackend, TrainConfig

    return HipBackend(NetSpec(1, 8, 2, 0), N, TrainConfig(batch_size=N, lm_gram_paths=2048, lm_out_fix=True),
                      device="cpu", world=world, **kw)


def _data(n=N, side=False, norm=False):
    from rphedge.engine import DateData

    g = torch.Generator().manual_seed(3)
    x = torch.rand(n, generator=g) + 0.5
    d = DateData(feats=[x], prices_next=[x * 1.01], bond_next=1.01, target=torch.clamp(x - 1.0, min=0))
    if norm:
        d.fmu, d.fisd = (0.9,), (3.0,)
    if side:
        d.gram_feats, d.gram_prices_next, d.gram_target = [x[:2048].clone()], [x[:2048] * 1.01], d.target[:2048].clone()
    return d


def _state(be):
    return be.new_weights(init_weights(be.spec, [0.5, 0.5], seed=1)), be.new_opt(), be.new_fit()


def _explore_cfg(be, **kw):
    from rphedge.engine import FitConfig

    w0s = np.stack([init_weights(be.spec, [0.5, 0.5], seed=k) for k in range(4)])
    return FitConfig(optimizer="lm", epochs=3, lm_starts=4, lm_explore_passes=2, lm_explore_paths=1 << 11, lm_w0s=w0s, **kw)


def _check(desc, want):
    got = {k: getattr(desc, k) for k in want}
    assert got == want


def _derived(be):
    """(exploration LmDesc, refit LmDesc) of ``be``, prepared without a launch."""
    from rphedge.engine import FitConfig

    w, o, f = _state(be)
    fc = _explore_cfg(be)
    d_main = be._full_batch_desc(w, o, f, _data(), fc, L.LOSS_MSE)
    return be._lm_explore_prepare(d_main, fc)[1], be._lm_refit_prepare(w, o, f, _data(), FitConfig())[1]


def _blob(desc):
    c = type(desc).from_buffer_copy(desc)
    for name in BUFFER_POINTERS:  # (different tensors on different backends)
        setattr(c, name, None)
    return bytes(c)


def test_exports():
    import rphedge.engine as E

    missing = [n for n in EXPORTS if not hasattr(E, n)]
    assert not missing, missing
    assert E.MAXIN == 8 and E.HipBackend.__module__ == "rphedge.engine.hip"
    orig = E.TorchBackend._lm_fit
    assert isinstance(orig, types.FunctionType)
    try:
        E.TorchBackend._lm_fit = lambda self, wts, fit, data, fcfg: "replaced"
        be = E.TorchBackend(NetSpec(1, 8, 2, 0), 256, E.TrainConfig(batch_size=256))
        assert be.fit(None, None, None, None, E.FitConfig(optimizer="lm"), 0) == "replaced"
    finally:
        E.TorchBackend._lm_fit = orig


def test_main_descriptor_golden():
    from rphedge.engine import FitConfig

    be = _backend()
    b = be._lm_buffers()
    _check(b["desc"], dict(MAIN, passes=0, lam_carry=0.0))
    base0 = bytes(b["base"])
    assert bytes(b["desc"]) == base0 and b["desc"] is not b["base"]
    w, o, f = _state(be)
    fc = _explore_cfg(be, lm_stop_tol=1e-3, lm_stop_min=3)
    d, lm = be._lm_prepare(w, o, f, _data(), fc)
    assert lm is b["desc"] and be._lm_buffers()["desc"] is lm  # (the tests' handle keeps its identity)
    _check(lm, dict(MAIN, passes=3, lam_carry=1.0, stop_tol=F32(1e-3), stop_min=3))  # (polish after an exploration)
    assert (d.n_local, d.batch, d.steps_per_epoch, d.shuffle, d.loss, d.inv_batch) == (N, N, 1, 0, L.LOSS_MSE, F32(1 / N))
    d, lm = be._lm_prepare(w, o, f, _data(side=True, norm=True),
                           FitConfig(optimizer="lm", epochs=2, lm_lam0=0.5, lm_lam_carry=3.0, lm_renorm=((0.3,), (2.0,))))
    _check(lm, dict(MAIN, passes=2, lam0=0.5, lam_carry=3.0, renorm=1, gram_side=1, stop_tol=0.0, stop_min=2))
    assert (lm.ren_mu[0], lm.ren_isd[0]) == (F32(0.3), 2.0) and lm.gfeat[0] and lm.gprice[0] and lm.gtarget
    assert bytes(b["base"]) == base0  # (no fit writes to the base)


def test_derived_descriptor_goldens():
    from rphedge.engine import FitConfig

    be = _backend()
    w, o, f = _state(be)
    fc = _explore_cfg(be)
    assert be.lm_explore_paths(fc) == 1 << 11
    d_main = be._full_batch_desc(w, o, f, _data(), fc, L.LOSS_MSE)
    d, lm, x = be._lm_explore_prepare(d_main, fc)
    _check(lm, EXPLORE)
    assert (d.n_local, d.batch, d.inv_batch, d.target) == (1 << 11, 1 << 11, 1 / 2048, d_main.target)
    assert lm.state == x["state"].data_ptr() and lm.w0 == x["w0"].data_ptr() and x["state"].shape[0] == 4
    d, lm = be._lm_refit_prepare(w, o, f, _data(), FitConfig())
    _check(lm, REFIT)
    assert lm.state == be._lm_buffers()["state"].data_ptr() and d.loss == L.LOSS_MSE and d.batch == N
    d, lm = be._lm_prepare(w, o, f, _data(), FitConfig(optimizer="lm", epochs=2, loss=L.LOSS_PINBALL, lm_q_delta=1e-3))
    _check(lm, PINBALL)
    assert lm is be._lm_buffers(L.LOSS_PINBALL)["desc"] and d.loss == L.LOSS_PINBALL


def test_data_parallel_local_gram_goldens():
    """world 2 with an RCCL-style communicator and no mailbox, no simulated
    subsample: this rank's part of the Gram subsample from its shard."""
    from rphedge.engine import FitConfig

    be = _backend(world=2, comm=object())
    w, o, f = _state(be)
    local = dict(num_wgs=16, gram_wgs=16, gram_blk=256, gram_blk_stride=1024, inv_ns=1 / 2048, inv_n=1 / 8192, gram_side=0)
    _check(be._lm_buffers()["desc"], dict(MAIN, passes=0, **local))
    d, lm = be._lm_prepare(w, o, f, _data(), FitConfig(optimizer="lm", epochs=2))
    _check(lm, dict(MAIN, passes=2, stop_min=2, **local))
    assert not be._lm_same_gram and not be.lm_last_fused and d.inv_batch == F32(1 / 8192)
    d, lm = be._lm_prepare(w, o, f, _data(side=True), FitConfig(optimizer="lm", epochs=2))
    _check(lm, dict(MAIN, passes=2, num_wgs=16, inv_n=1 / 8192, gram_side=1, gram_blk_stride=1024))
    assert be._lm_same_gram and be.lm_exchange_bytes() == 8 * 200
    d, lm = be._lm_refit_prepare(w, o, f, _data(), FitConfig())
    _check(lm, dict(REFIT, gram_blk=16, gram_blk_stride=1024, inv_ns=1 / 128, inv_n=1 / 8192))


def test_derived_descriptors_do_not_depend_on_order():
    """The exploration's and the refit's descriptors are the same bytes whether
    they are first prepared before or after main fits that set every per-fit
    field (derived from the live main descriptor they used to inherit lam0,
    stop_min, ren_mu, gfeat, q_delta, q_kappa and gtarget from it)."""
    from rphedge.engine import FitConfig

    first = _derived(_backend())
    be = _backend()
    w, o, f = _state(be)
    be._lm_prepare(w, o, f, _data(side=True, norm=True),
                   FitConfig(optimizer="lm", epochs=2, lm_lam0=0.5, lm_lam_carry=3.0, lm_renorm=((0.3,), (2.0,))))
    be._lm_prepare(w, o, f, _data(side=True), FitConfig(optimizer="lm", epochs=2, loss=L.LOSS_PINBALL, lm_q_delta=1e-3))
    later = _derived(be)
    for a, b in zip(first, later):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and _blob(a) == _blob(b)


def test_lm_geometry_without_the_hip_backend():
    code = ("import sys\n"
            "import rphedge.engine.lm_geometry as g\n"
            "import rphedge.engine as E\n"
            "assert g.lm_pass_schedule(1 << 20, -1, 2) == (512, 0) and g.gram_subsample(1 << 12, 2048) == (2048, 256, 512)\n"
            "assert g.lm_gram_geometry(1 << 12, 1024, 2) == (256, 1024) and g.lm_tpack_len(106, 10) > 0\n"
            "assert g.lm_tpack_image([0.0] * 10240, 106, 10).shape == (g.lm_tpack_len(106, 10),)\n"
            "E.TorchBackend, E.make_backend, E.gram_subsample\n"
            "assert 'rphedge.engine.hip' not in sys.modules, 'hip imported'\n"
            "assert E.PNL_PPT == 4 and 'rphedge.engine.hip' in sys.modules\n")
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
