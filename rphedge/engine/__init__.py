"""Training / evaluation engine: device-resident state + two backends.

* :class:`HipBackend` — the MI355X path.  Every optimizer step runs the same
  fused body (forward + loss + backward + in-wave reduce-scatter + workgroup
  sum: ``NarrowBody`` VALU for the 8-unit nets, ``WideBody`` MFMA for the
  32-unit nets) under one of three schedules (:attr:`TrainConfig.step_mode`,
  resolved by :meth:`HipBackend.step_mode`):

  - ``lag`` — one ``k_hedge_step_lag`` launch per step; every workgroup
    applies the Keras-Adam / LR / EarlyStopping update of the PREVIOUS step
    redundantly in its prologue from float-atomic accumulators, so the kernel
    boundary is the only global synchronisation (large grids; data parallel
    with the in-kernel xGMI exchange);
  - ``persistent`` — one ``k_hedge_fit`` launch per Keras fit with an
    in-kernel barrier (small grids, e.g. the reference's batch 512);
  - ``ticket`` — ``k_hedge_train_step`` with a last-arriver update
    (deterministic slab reduction, ranks sharing a GPU, RCCL all-reduce of the
    gradient packet on the compute stream between step and update kernels).

  Whole fits are launched from the native runtime (``rph_train_*_fit``), the
  ``k_hedge_eval`` epilogue produces values / holdings / residuals / stats, and
  nothing synchronises with the host, so a whole backward-induction run is
  captured into ONE hipGraph (:mod:`rphedge.driver`).  Input standardisation
  (:attr:`DateData.fmu` / ``fisd``) is fused into the feature loads.
* :class:`TorchBackend` — CPU (or any torch device) reference with identical
  semantics: same chunk permutation (Philox), same Adam formula, same early
  stopping; multi-process via ``torch.distributed`` (gloo).  It is the oracle
  for GPU numerics tests and the "CPU plumbing" configuration of BASELINE.

State blocks are flat float32 tensors (layout in :mod:`rphedge.ops.layout`).
Reference semantics: ``Replicating_Portfolio.py:128-221`` (C17-C24).

Modules: ``config``, ``state`` (state blocks, shared helpers), ``lm_geometry`` (integer geometry of the LM
launches), ``hip`` (imported on first use), ``torch_ref`` and ``lm_ref`` (its fp64 LM oracle).
"""
from ..models.hedge_mlp import NetSpec
from ..ops.native import MAXIN  # noqa: F401
from .config import (Costs, DateData, Exercise, FitConfig, PnlData, TrainConfig, fit_seed, geometric_lr_schedule,  # noqa: F401
                     keras_lr_schedule, pnl_fold_factors)
from .lm_geometry import (GRAM_BLOCKS, _lm_bias_index, _lm_out_n, gram_subsample, lm_gram_geometry,  # noqa: F401
                          lm_gram_red_wgs, lm_og_wgs, lm_out_gram, lm_out_nu, lm_pass_blocks, lm_pass_schedule,
                          lm_pass_wgs, lm_pk_red_wgs, lm_reduce_trees, lm_tpack_image, lm_tpack_len)
from .state import (_normalise, current_weights, fit_summary, fit_template, make_opt, make_weights,  # noqa: F401
                    reduce_cost_stats, reduce_stats, set_weights)
from .torch_ref import TorchBackend


def __getattr__(name):
    if name in ("HipBackend", "PERSISTENT_MAX_WGS", "PNL_PPT"):  # (geometry and CPU oracle import without hip)
        from . import hip
        return getattr(hip, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def make_backend(kind: str, spec: NetSpec, n_local: int, tcfg: TrainConfig, **kw):
    if kind == "hip":
        from .hip import HipBackend
        return HipBackend(spec, n_local, tcfg, **kw)
    for k in ("stream", "mailbox", "lm_mailbox", "lm_comm"):
        kw.pop(k, None)
    return TorchBackend(spec, n_local, tcfg, **kw)
