"""Configuration and input records of the engine (no backend code)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from ..ops import layout as L


def keras_lr_schedule(epochs: int) -> list:
    """``scheduler`` of RP:128-136 evaluated per epoch (NaN = keep current lr)."""
    return [1e-2 if e < 100 else 1e-3 if e < 200 else 5e-4 if e < 400 else float("nan") for e in range(epochs)]


def geometric_lr_schedule(lr0: float, epochs: int, decay: float = 1.0) -> tuple:
    """Per-epoch learning rates ``lr0 * decay**(e / (epochs-1))``: decays from
    ``lr0`` to ``lr0 * decay`` over one date's fit (``decay = 1``: constant).
    Throughput-mode counterpart of the reference's step schedule for the large
    global batches; ``TrainingParams.lr_rest`` / ``lr_decay``."""
    n = max(int(epochs), 1)
    if n == 1 or decay == 1.0:
        return tuple([float(lr0)] * n)
    return tuple(float(lr0) * decay ** (e / (n - 1)) for e in range(n))


@dataclass
class FitConfig:
    epochs: int = 100
    patience: int = 7
    loss: int = L.LOSS_MSE
    quantile: float = 0.99
    lr_schedule: tuple | None = None      # per-epoch learning rates (NaN keeps current)
    restore_best: bool = True
    restore_at_end: bool = False          # Keras-3 behaviour; Keras-2 restores only on early stop
    early_stopping: bool = True
    # "adam" (the reference's Keras-Adam minibatch fit) or "lm": full-batch
    # Levenberg-Marquardt passes (MSE fits of the 8-unit nets; ``epochs`` = the
    # number of trial points after the start point; csrc/hedge_lm.hip)
    optimizer: str = "adam"
    # LM adaptive pass budget: from pass lm_stop_min on, an accepted pass that
    # lowers the best loss by less than lm_stop_tol (relative) ends the fit
    # (rejections never do; 0: off;
    # ``epochs`` stays the cap)
    lm_stop_tol: float = 0.0
    lm_stop_min: int = 2
    lm_lam0: float | None = None          # initial LM damping of this fit (None: TrainConfig.lm_lam0)
    # > 0: the fit starts at the previous LM fit's final damping x lm_lam_carry
    # (later dates: a warm start's curvature scale is the last fit's)
    lm_lam_carry: float = 0.0
    # multi-start exploration (first date; on when lm_starts >= 1 AND
    # lm_explore_passes > 0 - one start is a warm-up on the path prefix, which
    # also needs lm_w0s): lm_starts fits from the start
    # points lm_w0s[k] ([starts, P]; row 0 = the run's initial weights),
    # lm_explore_passes trial points each on the first lm_explore_paths global
    # paths (lm_explore_data; every rank runs all of them on the same data),
    # then the candidate with the lowest final loss is the start point of the
    # ``epochs`` polish passes on every path (at its damping)
    # (mu, isd) of the inputs the start weights were fitted on (the previous
    # date): the first layer is re-expressed for this fit's standardisation, so
    # a warm start is the previous hedge as a function of the raw state
    lm_renorm: tuple | None = None
    lm_starts: int = 1
    lm_explore_passes: int = 0
    lm_explore_paths: int = 0
    lm_w0s: object = None
    # the exploration's data: the first lm_explore_paths GLOBAL paths of the
    # date (DateData, simulated on every rank; None: this rank's shard prefix,
    # the global prefix on one rank) - every rank runs the same starts on the
    # same paths, so the pick is the same at every world size with no exchange
    lm_explore_data: object = None
    # pinball LM fits (loss = LOSS_PINBALL): IRLS Gram weights
    # 1 / (2 max(|r|, delta)), delta = max(lm_q_delta, lm_q_kappa x the mean |r|
    # of the path's 64-path Gram tile) (target units; lm_q_delta 0: 1e-6)
    lm_q_delta: float = 0.0
    lm_q_kappa: float = 3.0

    def key(self):
        return (self.epochs, self.patience if self.early_stopping else 1 << 30, self.restore_best,
                self.restore_at_end, tuple(self.lr_schedule) if self.lr_schedule is not None else None)


@dataclass
class TrainConfig:
    batch_size: int = 512          # GLOBAL minibatch (reference: 512)
    shuffle: bool = True           # Keras fit(shuffle=True)
    chunk_log2: int = 0            # shuffle granularity: 0 = per path (Keras), 6 = 64-path chunks
    seed: int = 1234
    lr: float = 1e-3               # Adam(learning_rate=1e-3)
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-7              # Keras epsilon
    max_wgs: int = 0               # workgroups per training step; 0 = auto: 256 (one per CU), 512 for
                                   # the 1-input 32-unit bf16 net (2 resident waves/SIMD:
                                   # the MFMA tile chain is latency-bound, profiles/r1/sweep_r1n_wide_wgs.jsonl)
    paths_per_thread: int = 1      # target work per thread per step
    deterministic: bool = False    # fixed-order slab reduction instead of float atomics
    split_update: bool = False     # force the standalone update kernel (the world_size>1 path)
    mfma_fp32: bool = False        # 32-unit nets: exact fp32 MFMA instead of bf16 operands
    # Levenberg-Marquardt fits (FitConfig.optimizer == "lm"): Gram matrix from a
    # subsample of lm_gram_paths paths (global; 64-path tiles on the matrix
    # cores), Marquardt damping lam0, x lam_up on a rejected trial, x lam_down
    # on an accepted one, clamped to [lam_min, lam_max]; ridge x mean diagonal
    lm_gram_paths: int = 4096
    lm_lam0: float = 1e-3
    lm_lam_up: float = 4.0
    lm_lam_down: float = 1.0 / 3.0
    lm_lam_min: float = 1e-9
    lm_lam_max: float = 1e10
    lm_ridge: float = 1e-10
    # damping diagonal floor (relative to the mean of diag 2G): a parameter with
    # no curvature on the Gram subsample is still damped, so lam -> inf shortens
    # its step (tests/test_lm_cpu.py: a teacher fit that stalls at lam_max
    # without it).  0 = plain Marquardt scaling (the presets: 1e-6 moved the
    # euro30 8-seed P&L 0.890 -> 0.897 in tools/lm_lab.py, 1e-9 changed nothing)
    lm_diag_floor: float = 0.0
    # damping update: "simple" (x lam_down on accept, x lam_up on reject) or
    # "nielsen" (gain ratio rho of actual / predicted reduction: accept
    # x max(1/3, 1 - (2 rho - 1)^3), reject x nu with nu doubling)
    lm_damping: str = "simple"
    # after the last pass: exact Newton step on the bond holding's output bias
    # (free heads), so the fitted values' mean over all paths equals the
    # target's and no mean error drifts down the backward induction
    lm_bias_fix: bool = True
    # pass kernel load balance (cyclic schedule only, lm_leaf_paths < 0): the
    # Gram workgroups' waves take this many 128-path blocks fewer than an even
    # split (their Gram tile follows)
    lm_gram_skip: int = 3
    # pass kernel schedule: every wave sums one contiguous "leaf" of paths
    # (LmDesc.leaf_blocks): 0 = auto (the shard over 4 x the pass workgroups),
    # > 0 = this many paths per leaf (a multiple of 128: the same leaves at
    # every world size over the same global paths - the strong-scaling
    # rehearsal reproduces the one-rank fit bit for bit), < 0 = the cyclic
    # block schedule with lm_gram_skip (default: 0.7 ms faster on the euro30
    # flagship, whose Gram workgroups then take fewer path blocks)
    lm_leaf_paths: int = -1
    # the Gram tiles in Gram-only workgroups after the path grid (LmDesc.gram_base),
    # co-resident with the path workgroups, instead of in the first path
    # workgroups; None = auto: on with contiguous leaves (no gram_skip balance
    # there: euro30 6.04 -> 5.86 ms), off on the cyclic schedule (5.69 vs 5.75)
    lm_gram_overlap: bool | None = None
    # after the last pass: exact Newton step on the whole output layer (the
    # value is linear in it; 2 G_oo d = -g_o), subsuming the bias step
    lm_out_fix: bool = False
    # its relative Marquardt damping (near-collinear hidden units: the output
    # Gram's condition number reaches 1e9+; below ~1e-5 of its scale the
    # fp32-accumulated matrix is rounding noise, tools/og_precision.py)
    lm_out_mu: float = 1e-5
    lm_out_tr: float = 0.0  # output step trust region: ||d|| <= this x max(||w_o||, 1e-3 sqrt(n_o)) (0: off)
    # run the data-parallel LM sequence (pass + reduce -> all-reduce of the
    # reduced block -> solve, one launch each) even on one rank: the test hook
    # that exercises the RCCL / mailbox exchange path at world size 1
    lm_split: bool = False
    # later dates of an eligible LM run (HipBackend.eval_ride_ok): the eval of a
    # date rides in the launch of the next fit's first solve, whose pass 0
    # evaluates its own target; False forces the sequence fit, eval, fit, ...
    # with every eval a launch of its own (same results bit for bit)
    eval_ride: bool = True
    # first date of an eligible LM run (HipBackend.sim_ride_ok): the in-place
    # re-simulation launches only the path blocks the exploration reads; the
    # others ride in the exploration's solve launches (k_lm_solve_sim)
    sim_ride: bool = True
    expose_packet: bool = False    # lagged fits: the finalize kernel writes the last step's summed (and
                                   # data-parallel exchanged) gradient packet to HipBackend.grad (tests)
    # optimizer-step schedule on the GPU:
    #   "lag"        one kernel per step, the Adam update of step k applied by every
    #                workgroup in the prologue of kernel k+1 (no in-kernel sync)
    #   "ticket"     one kernel per step, last-arriving workgroup reduces + updates
    #                (deterministic slab / split update / fused xGMI DP)
    #   "persistent" one resident kernel per fit with an in-kernel grid barrier
    #   "auto"       1 rank: persistent up to PERSISTENT_MAX_WGS workgroups, lag above;
    #                data parallel: lag (fused xGMI) where valid, else ticket
    step_mode: str = "auto"
    # narrow lag kernel: 0 = weights hoisted into registers (1 wave/SIMD);
    # 1 = 2 waves/SIMD with LDS weight re-reads; 2/3 = 0/1 with the path-data
    # prefetch 2 iterations deeper; 4 = LDS weight re-reads at 1 wave/SIMD;
    # -1 = auto (4 for nets whose gradient packet is 256 wide - no scratch
    # spills - else 0)
    variant: int = -1


@dataclass
class DateData:
    """Inputs of one backward-induction fit (RP:200-201)."""

    feats: list                    # state_t features, each [n_local]
    prices_next: list              # traded assets at t+1 (bond excluded), each [n_local]
    bond_next: float               # B_{t+1} (normalised)
    target: torch.Tensor           # V_{t+1} [n_local]
    prices_now: list = field(default_factory=list)   # assets at t (for V_t)
    bond_now: float = 1.0
    # input standardisation x' = (x - fmu) * fisd, fused into the kernels'
    # feature loads (empty: identity = the reference's raw inputs)
    fmu: tuple = ()
    fisd: tuple = ()
    # LM fits: the global Gram subsample (gram_subsample) simulated on this
    # rank, slot order: state_t features and traded assets at t+1, each [ns]
    # (None: the Gram reads the shard; data parallel it is then summed over ranks)
    gram_feats: list | None = None
    gram_prices_next: list | None = None
    # pinball LM fits: V_{t+1} on the same subsample paths ([ns]), so the IRLS
    # Gram weights need no shard data and the fit is world-invariant (None:
    # pinball fits read the subsample from the shard)
    gram_target: torch.Tensor | None = None


@dataclass
class PnlData:
    """Inputs of the self-financing P&L scan (k_hedge_pnl / TorchBackend.pnl)."""

    n_dates: int
    features: object               # t -> list of [n_local] state-feature tensors at date t (raw)
    prices: object                 # t -> list of [n_local] traded-asset tensors at date t (bond excluded)
    bond: torch.Tensor             # [n_dates + 1] float64 bank account B_t (device)
    fmu: torch.Tensor              # [n_dates, MAXIN] float32 per-date standardisation (device)
    fisd: torch.Tensor             # [n_dates, MAXIN]
    w0: torch.Tensor | None        # [n_local] initial wealth (the fitted V_0); None: the scalar ``wealth0``
    payoff: torch.Tensor           # [n_local] terminal liability
    wealth0: float = 0.0           # initial wealth of every path when ``w0`` is None (out-of-sample paths)


def pnl_fold_factors(bond) -> tuple:
    """Per-date factors of the P&L folded into the backward induction
    (``HipBackend.eval(pnl_acc=...)`` / ``pnl_finish``), from the bank account
    ``bond`` ([n_dates + 1]): ``(grow, carry, carry_all)`` with ``grow[t] = g_t
    = fp32(B_{t+1} / B_t)`` (the factor k_hedge_pnl applies), ``carry[t] = c_t``
    = the fp64 product of the fp32 ``g_s`` over ``s > t``, rounded once to
    fp32 (``c_{n-1} = 1``), and ``carry_all = c_{-1}``, the product of every
    ``g_s``: W_T = W_0 c_{-1} + sum_t c_t sum_a h_a,t (S_a,t+1 - S_a,t g_t)."""
    b = np.asarray(bond, np.float64)
    g = (b[1:] / b[:-1]).astype(np.float32)
    tail = np.concatenate([np.cumprod(g[::-1].astype(np.float64))[::-1], [1.0]])  # tail[t] = prod_{s >= t} g_s
    return g, tail[1:].astype(np.float32), np.float32(tail[0])


@dataclass(frozen=True)
class Exercise:
    """Early-exercise right of a call / put on traded asset 0 (backends' ``eval`` /
    ``pnl``): the holder takes X = max(k - S, 0) (put) or max(S - k, 0) (call)
    where ``X > 0 and X >= C``, C the continuation value of the date's network."""

    kind: str                      # "put" | "call"
    strike: float                  # k in the paths' normalised units (K / Y)
    every: int = 1                 # P&L scan: exercise dates are t % every == 0

    def __post_init__(self):
        if self.kind not in ("put", "call"):
            raise ValueError(f"exercise kind must be 'put' or 'call', got {self.kind!r}")
        if int(self.every) < 1:
            raise ValueError(f"exercise_every must be >= 1, got {self.every!r}")

    def intrinsic(self, s: torch.Tensor) -> torch.Tensor:
        """X in the dtype of ``s`` (the strike rounded to it first, as in a descriptor)."""
        k = torch.tensor(float(self.strike), dtype=s.dtype, device=s.device)
        return torch.clamp(k - s, min=0) if self.kind == "put" else torch.clamp(s - k, min=0)


@dataclass(frozen=True)
class Costs:
    """Proportional transaction costs and a no-trade band of the forward scans
    (backends' ``pnl`` / ``oos``; csrc/rph_types.h CostTerms): a trade of
    ``|dh|`` units at the price ``S`` costs ``rate |dh| S``; the position
    follows the network's target only where it differs from the held one by
    more than ``band`` (units of the holdings output; 0 always trades);
    ``unwind``: the final position is sold at the horizon, at the same rate."""

    rate: float
    band: float = 0.0
    unwind: bool = False

    def __post_init__(self):
        for name in ("rate", "band"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"cost {name} must be a number, got {v!r}")
            if not np.isfinite(v) or v < 0:
                raise ValueError(f"cost {name} must be finite and >= 0, got {v!r}")
        if self.rate > 1:
            raise ValueError(f"cost rate must be <= 1, got {self.rate!r}")

    @property
    def active(self) -> bool:
        return self.rate > 0 or self.band > 0


def fit_seed(seed: int, date: int, net: int) -> int:
    return (int(seed) * 1000003 + int(date) * 7919 + int(net) * 104729) & 0xFFFFFFFF
