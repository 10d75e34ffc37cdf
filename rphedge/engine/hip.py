"""The MI355X backend: descriptors of the native launchers (csrc/) and their launch order."""
from __future__ import annotations

import os
from dataclasses import replace

import numpy as np
import torch

from ..models.hedge_mlp import NetSpec
from ..ops import layout as L
from ..ops import layout_cost as LC
from .config import Costs, DateData, Exercise, FitConfig, PnlData, TrainConfig
from .lm_geometry import (_lm_bias_index, _lm_out_n, gram_subsample, lm_explore_nsub, lm_gram_geometry, lm_og_wgs,
                          lm_out_nu, lm_pass_schedule, lm_shard_gram_wgs, lm_tpack_len)
from .state import StateBlocks, _Cache, _check_eval_data, _set_norm, _steps, fit_template

PNL_PPT = L.PNL_PPT  # paths per thread of k_hedge_pnl (re-exported as rphedge.engine.PNL_PPT)
PERSISTENT_MAX_WGS = 64  # "auto" picks the persistent per-fit kernel up to this grid (1 rank)


def _env(name: str, default) -> int:
    """Integer tuning knob: the environment's ``RPH_<name>`` over ``default`` (A/B runs, tools/ab_env.sh)."""
    return int(os.environ.get("RPH_" + name, default))


_clone = lambda desc: type(desc).from_buffer_copy(desc)  # noqa: E731  (a descriptor's own copy)


class HipBackend(StateBlocks):
    name = "hip"

    def __init__(self, spec: NetSpec, n_local: int, tcfg: TrainConfig, device=None, comm=None,
                 world: int = 1, rank: int = 0, stream=None, mailbox=None, lm_mailbox=None, lm_comm=None):
        from ..ops import native

        self.mailbox = mailbox  # native.IpcMailbox: fused xGMI all-reduce inside the step kernel
        self.lm_mailbox = lm_mailbox  # native.IpcMailbox (LM_DP_PITCH pitch): LM block exchange
        self._lm_nccl = lm_comm       # RCCL communicator of the LM block when its xGMI probe failed
        self.native = native
        native.load(required=True)
        self.spec, self.n_local, self.tcfg = spec, int(n_local), tcfg
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.comm, self.world, self.rank, self.stream = comm, world, rank, stream
        self.shape = (spec.nin, spec.hidden, spec.nout, spec.head)  # the native launchers' shape key
        self.P, self.R = native.net_nparams(*self.shape)
        # (P, R, Gram blocks) of the LM kernels, None without an LM solver; pass workgroups per CU
        self._lm_shape, self._lm_wps = native.lm_shape(*self.shape), native.lm_pass_wps(*self.shape)
        assert self.P == spec.nparams
        self.batch_local, self.steps_per_epoch = _steps(self.n_local, tcfg, world)
        # narrow-body variant (csrc/hedge_mlp.hip launcher): 5 = W2 hoisted in
        # VGPRs + the rest from LDS, 2 waves/SIMD at 512 WGs (1-2 input nets:
        # 9.83 -> 9.64 / 10.05 -> 9.69 us per 2^18 step; the 3-input net is
        # slower that way), 4 = all weights from LDS (256-wide packets),
        # 0 = all weights hoisted (profiles/r1/stamp_r1u_hybrid.jsonl)
        # 512 workgroups only on one rank (with the in-kernel xGMI exchange every
        # workgroup polls the mailbox, so data-parallel runs keep 256) and only
        # where the hybrid body fits 2 waves/SIMD (<= 3 inputs, 128-wide packet);
        # the 256-wide-packet nets (basket 5-8-6) run it at 1 wave/SIMD, still
        # faster than all-LDS weights (16.6 -> 14.8 us, profiles/r1/stamp_r1v_masks.jsonl)
        hyb512 = spec.hidden == 8 and spec.nin <= 3 and self.R <= 128 and world == 1
        auto_v = 5 if (hyb512 or (spec.hidden == 8 and self.R > 128)) else 0
        self.variant = int(tcfg.variant) if int(tcfg.variant) >= 0 else auto_v
        work = max(1, self.batch_local // (256 * max(1, tcfg.paths_per_thread)))
        mw = int(tcfg.max_wgs)
        if mw <= 0:
            # 512 workgroups = 2 per CU only where two fit (the 1-input bf16
            # net); the wider-input nets run 1 per CU, so a 512 grid starts in
            # two waves (+15 us start spread, profiles/r1/stamp_r1s_wide_wgs.jsonl)
            mw = 512 if (spec.hidden == 32 and not tcfg.mfma_fp32 and spec.nin == 1) else 256
            if (self.variant == 5 and hyb512 and tcfg.step_mode in ("auto", "lag") and not tcfg.deterministic
                    and not tcfg.split_update):
                mw = 512  # lagged steps: 2 workgroups (2 waves/SIMD) per CU
        self.num_wgs = int(max(1, min(mw, work)))
        dev = self.device
        self.slab = torch.zeros(self.num_wgs, self.R, dtype=torch.float32, device=dev)
        self.counter = torch.zeros(4, dtype=torch.int32, device=dev)
        self.grad = torch.zeros(self.R, dtype=torch.float32, device=dev)
        self.acc = torch.zeros(8, self.R, dtype=torch.float32, device=dev)
        # persistent per-fit kernel: 3 rotating accumulator buffers + [arrivals, error] counters
        self.acc_fit = torch.zeros(3, L.LAG_SLOTS, self.R, dtype=torch.float32, device=dev)
        self.fit_ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        self.lag = torch.zeros(2, L.LAG_FLOATS, dtype=torch.float32, device=dev)
        self._acc_clean = False  # acc_fit known zero (set by a lagged fit's finalize)
        self.stamps = None  # set to an int64 [num_wgs, 8] tensor for phase diagnostics
        # eval epilogue (k_hedge_eval): weights read from LDS, up to 4 resident
        # waves per SIMD, each thread walks its paths with a 4-deep load ring;
        # 2048 workgroups (2 paths per thread at 2^20): euro30 8.42 -> 8.28 ms
        # against 512 (profiles/r4/eval_wgs_sweep.txt)
        self.eval_wgs = int(max(1, min(_env("EVAL_WGS", 2048), (self.n_local + 255) // 256)))
        self._cache = _Cache()
        self.lm_last_fused = False  # the last LM fit summed its gradient region inside k_lm_reduce
        self._lm_same_gram = True  # the last LM fit built the world-invariant Gram (exchange: gradient region only)
        # eval ride (eval_ride_ok): shapes whose LM pass 0 can evaluate its own target (k_lm_pass<BodyST>)
        self._lm_st = self._lm_shape is not None and native.lm_has_st(*self.shape)

    def _template(self, fcfg: FitConfig):
        return self._cache.get(("fit", fcfg.key()), lambda: fit_template(fcfg, self.device))

    def _lr(self, fcfg: FitConfig):
        if fcfg.lr_schedule is None:
            return None
        return self._cache.get(("lr", tuple(fcfg.lr_schedule)),
                               lambda: torch.tensor(list(fcfg.lr_schedule), dtype=torch.float32, device=self.device))

    # -- ops -----------------------------------------------------------------
    def _train_desc(self, wts, opt, fit, data: DateData, fcfg: FitConfig, seed: int, lr_t):
        n = self.native
        d = n.TrainDesc()
        n.fill_ptrs(d.feat, data.feats)
        n.fill_ptrs(d.price, data.prices_next)
        d.target = data.target.data_ptr()
        d.wts, d.opt, d.fit = wts.data_ptr(), opt.data_ptr(), fit.data_ptr()
        d.lr_sched = n.ptr(lr_t)
        d.slab, d.counter, d.grad_out = self.slab.data_ptr(), self.counter.data_ptr(), self.grad.data_ptr()
        d.bond, d.alpha, d.quantile = float(data.bond_next), float(self.spec.alpha), float(fcfg.quantile)
        d.inv_batch, d.loss = 1.0 / float(self.batch_local * self.world), int(fcfg.loss)
        d.n_local, d.batch, d.steps_per_epoch = self.n_local, self.batch_local, self.steps_per_epoch
        d.chunk_log2, d.shuffle = int(self.tcfg.chunk_log2), 1 if self.tcfg.shuffle else 0
        d.seed = int(seed) & 0xFFFFFFFF
        fused_dp = self.mailbox is not None and self.world > 1
        d.fused_update = 1 if ((self.world == 1 or fused_dp) and not self.tcfg.split_update) else 0
        if self.world > 1 and self.comm is None and not fused_dp:
            raise RuntimeError("HipBackend with world_size > 1 needs an RCCL communicator or an IPC mailbox")
        if fused_dp:
            self.mailbox.fill(d)
        else:
            d.dp_world, d.dp_rank = 1, 0
        d.acc, d.stamps = self.acc.data_ptr(), n.ptr(self.stamps)
        d.deterministic, d.mfma_fp32 = 1 if self.tcfg.deterministic else 0, 1 if self.tcfg.mfma_fp32 else 0
        d.variant, d.num_wgs = self.variant, self.num_wgs
        d.nin, d.h, d.nout, d.head = self.shape
        _set_norm(d, data)
        return d

    def _full_batch_desc(self, wts, opt, fit, data: DateData, fcfg: FitConfig, loss: int):
        """The training descriptor of a full-batch LM launch on this rank's shard."""
        d = self._train_desc(wts, opt, fit, data, fcfg, 0, None)
        d.batch, d.steps_per_epoch, d.shuffle = self.n_local, 1, 0
        d.inv_batch = 1.0 / float(self.n_local * max(self.world, 1))
        d.loss = int(loss)
        return d

    def fit(self, wts, opt, fit, data: DateData, fcfg: FitConfig, seed: int, poll_every: int = 0, ride=None,
            sim_ride=None):
        """Enqueue a full Keras ``fit`` (epochs x steps).  With ``poll_every``>0 the
        host checks the device early-stop flag every that many epochs and stops
        enqueueing; otherwise everything is asynchronous (graph-capturable) and
        surplus steps after an early stop are device-side no-ops.

        ``ride`` (an :meth:`eval_desc` of the date fitted before, t + 1, whose
        ``v_out`` is this fit's target; only where :meth:`eval_ride_ok`): that
        eval is not a launch of its own - pass 0 evaluates the target itself
        and the eval runs as extra workgroups of the first solve's launch."""
        assert len(data.feats) == self.spec.nin and len(data.prices_next) == self.spec.nhold - 1
        if fcfg.optimizer == "lm":
            return self._lm_fit(wts, opt, fit, data, fcfg, ride, sim_ride)
        if ride is not None or sim_ride is not None:
            raise ValueError("an eval or a path scan rides in Levenberg-Marquardt fits only")
        d = self._train_desc(wts, opt, fit, data, fcfg, seed, self._lr(fcfg))
        n, S = self.native, self.steps_per_epoch
        mode = self.step_mode(poll_every)
        if mode == "lag" and not self.tcfg.expose_packet:
            d.grad_out = None  # (the finalize kernel writes the packet only when asked)
        if mode == "lag" and fcfg.epochs > 0:
            # kernel 0 reads the fit-state template and publishes it as `fit`;
            # the previous lag fit's finalize left the accumulators zeroed
            d.fit_init = self._template(fcfg).data_ptr()
            if not self._acc_clean:
                n.memset_async(self.acc_fit, 0, self.stream)
        else:
            fit.copy_(self._template(fcfg), non_blocking=True)
        self._acc_clean = False
        if mode == "persistent":
            n.memset_async(self.acc_fit, 0, self.stream)
            n.memset_async(self.fit_ctl, 0, self.stream)
            d.acc, d.counter = self.acc_fit.data_ptr(), self.fit_ctl.data_ptr()
            n.train_fit(d, fcfg.epochs, self.stream)
            return
        if mode == "lag":
            d.acc, d.lag = self.acc_fit.data_ptr(), self.lag.data_ptr()
            if not poll_every:  # whole fit launched from the native runtime
                n.train_lag_fit(d, fcfg.epochs, self.stream)
                self._acc_clean = fcfg.epochs > 0
                return
            k = 0
            for e in range(fcfg.epochs):
                for s in range(S):
                    n.train_lag_step(d, k, e, self.stream)
                    k += 1
                if poll_every and (e + 1) % poll_every == 0 and e + 1 < fcfg.epochs:
                    if float(fit[L.F_STOPPED].item()) != 0.0:
                        break
            n.train_lag_finalize(d, k, self.stream)
            self._acc_clean = True  # (finalize zeroes the three accumulators)
            return
        per_step_host = (self.world > 1 and d.fused_update == 0) or self.tcfg.split_update
        if not poll_every and not per_step_host:
            n.train_ticket_fit(d, fcfg.epochs, self.stream)
            return
        for e in range(fcfg.epochs):
            for s in range(S):
                n.train_step(d, s, e, self.stream)
                if (self.world > 1 and d.fused_update == 0) or self.tcfg.split_update:
                    if self.comm is not None:
                        self.comm.allreduce_(self.grad, self.stream)
                    n.train_update(d, s, e, self.stream)
            if poll_every and (e + 1) % poll_every == 0 and e + 1 < fcfg.epochs:
                if float(fit[L.F_STOPPED].item()) != 0.0:
                    break

    # -- Levenberg-Marquardt ----------------------------------------------------
    def lm_supported(self) -> bool:
        return self._lm_shape is not None

    def _lm_buffers(self, loss: int = L.LOSS_MSE):
        """LM state, reduced block, slabs and descriptors of this backend's fits
        of one loss (MSE and pinball fits keep separate states: each carries
        its own damping across dates).  ``base`` is never written again: ``desc``
        (the main fit's), the exploration's and the bias refit's are copies of it."""
        pin = int(loss) == L.LOSS_PINBALL
        return self._cache.get(("lm",) if not pin else ("lm", L.LOSS_PINBALL), lambda: self._lm_make_buffers(pin))

    def _lm_make_buffers(self, pin: bool) -> dict:
        if self._lm_shape is None:
            raise ValueError(f"no Levenberg-Marquardt solver for net {self.spec} (8-unit nets up to 174 parameters)")
        P, R, nblk = self._lm_shape
        t, W, dev = self.tcfg, max(self.world, 1), self.device
        nw, leaf = lm_pass_schedule(self.n_local, _env("LM_LEAF", t.lm_leaf_paths), _env("LM_WPS", self._lm_wps))
        # the global Gram subsample (every rank: gw = ns / 64 Gram workgroups,
        # past the path grid where it is larger)
        ns, gblk, gstride = gram_subsample(self.n_local * W, t.lm_gram_paths)
        gw = ns // L.LM_TILE
        # fallback without simulated subsample data, data parallel: this
        # rank's part of the subsample from its shard, the Gram summed over ranks
        gw_local = lm_shard_gram_wgs(self.n_local, t.lm_gram_paths, W, nw)
        lm = self.native.LmDesc()
        bufs = dict(state=torch.zeros(L.LMS_FLOATS, dtype=torch.float64, device=dev),
                    red=torch.zeros(L.LM_RED, dtype=torch.float64, device=dev),
                    slab_b=torch.zeros(nw, R, dtype=torch.float32, device=dev),
                    slab_o=torch.zeros(nw if _lm_out_n(self.spec, t) else 1, 3 * 1024, dtype=torch.float32, device=dev),
                    slab_g=torch.zeros(max(gw, gw_local), nblk * 1024, dtype=torch.float32, device=dev))
        lm.state, lm.slab_b, lm.slab_g, lm.slab_o = (bufs[k].data_ptr() for k in ("state", "slab_b", "slab_g", "slab_o"))
        lm.num_wgs, lm.red_wgs, lm.leaf_blocks = nw, nblk * 1024 // 64 + R // 4 + lm_og_wgs(self.spec), leaf
        lm.inv_n = 1.0 / float(self.n_local * W)
        # (Gram geometry: per fit, _lm_gram_mode)
        bufs["gram"] = dict(side=(gw, gblk, gstride, 1.0 / float(ns)),
                            local=(gw_local,) + lm_gram_geometry(self.n_local, gw_local * L.LM_TILE, W) +
                            (1.0 / float(gw_local * L.LM_TILE * W),))
        # default (no subsample data): one rank reads the global subsample from its shard
        lm.gram_wgs, lm.gram_blk, lm.gram_blk_stride, lm.inv_ns = bufs["gram"]["side" if W == 1 else "local"]
        lm.lam0, lm.lam_up, lm.lam_down = t.lm_lam0, t.lm_lam_up, t.lm_lam_down  # (lam0: a fit's own, _lm_set_fit)
        lm.lam_min, lm.lam_max, lm.ridge = t.lm_lam_min, t.lm_lam_max, t.lm_ridge
        lm.diag_floor, lm.out_mu, lm.out_tr = float(t.lm_diag_floor), float(t.lm_out_mu), float(t.lm_out_tr)
        # (pinball fits: no output-layer / bias Newton step - the loss is not quadratic)
        lm.bias_index = -1 if pin else _lm_bias_index(self.spec, t)
        lm.out_n = 0 if pin else _lm_out_n(self.spec, t)
        lm.out_gram = 1 if lm.out_n > 0 else 0
        lm.damping = 1 if str(t.lm_damping).lower() == "nielsen" else 0
        lm.gram_skip = _env("LM_GRAM_SKIP", t.lm_gram_skip)
        bufs["base"], bufs["desc"] = lm, _clone(lm)
        return bufs

    def _lm_gram_mode(self, lm, data: DateData, allow_side: bool = True) -> bool:
        """Set the Gram subsample of ``lm`` for a fit on ``data``; returns True
        when every rank builds the same Gram matrix (the exchange then carries
        only the gradient region).  One rank reads the subsample from its shard
        (the shard is the whole range) unless simulated subsample data is given;
        data parallel, the simulated subsample is required for the small exchange
        (without it: this rank's part of the subsample, Gram summed over ranks)."""
        g = self._lm_buffers()["gram"]
        side = allow_side and data.gram_feats is not None and data.gram_prices_next is not None
        lm.gtarget = self.native.ptr(data.gram_target) if side else None
        gw, blk, stride, inv = g["side" if (side or self.world <= 1) else "local"]
        if side:
            if data.gram_feats[0].numel() != gw * L.LM_TILE:
                raise ValueError(f"Gram subsample data has {data.gram_feats[0].numel()} paths, expected {gw * L.LM_TILE}")
            self.native.fill_ptrs(lm.gfeat, data.gram_feats)
            self.native.fill_ptrs(lm.gprice, data.gram_prices_next)
        lm.gram_side = 1 if side else 0
        lm.gram_wgs, lm.gram_blk, lm.gram_blk_stride, lm.inv_ns = gw, blk, stride, inv
        auto = int(lm.leaf_blocks) > 0 if self.tcfg.lm_gram_overlap is None else bool(self.tcfg.lm_gram_overlap)
        lm.gram_base = lm.num_wgs if (_env("LM_GRAM_OVERLAP", auto) and int(lm.inst) == 1) else 0
        return side or self.world <= 1

    def lm_exchange_bytes(self) -> int:
        """Bytes one rank pushes to EACH peer per LM pass (the gradient region
        when the Gram is built redundantly, else the whole reduced block)."""
        if self.world <= 1:
            return 0
        P, _, nblk = self._lm_shape
        return 8 * self._lm_greg(False) if self._lm_same_gram else 8 * (nblk * 1024 + lm_tpack_len(P, nblk) + L.LM_RED - L.LM_GBLK_MAX)

    def _lm_greg(self, og: bool) -> int:
        """Doubles of the gradient region a pass exchanges (even: 16-byte
        pushes): [g (LM_NPMAX) | stats (8)], + the packed output Gram in the
        passes that build it."""
        n = L.LM_RED_OUTG - L.LM_GBLK_MAX
        if og:
            nu = lm_out_nu(self.spec)
            n += nu * (nu + 1) // 2
        return n + (n & 1)

    def lm_exchange_bytes_run(self, passes_first: int, passes_rest: int, dates: int) -> int:
        """Bytes one rank pushes to each peer over a whole induction (the
        output-Gram passes carry the packed output Gram as well)."""
        if self.world <= 1:
            return 0
        if not self._lm_same_gram:
            return self.lm_exchange_bytes() * (passes_first + 1 + (dates - 1) * (passes_rest + 1))
        og = bool(_lm_out_n(self.spec, self.tcfg))
        tot = 0
        for n in [passes_first] + [passes_rest] * (dates - 1):
            k_og = min(L.LM_OUTG_TAIL, n + 1) if og else 0
            tot += 8 * ((n + 1 - k_og) * self._lm_greg(False) + k_og * self._lm_greg(True))
        return tot

    def _lm_set_fit(self, lm, fcfg: FitConfig, data: DateData, fused: bool):
        """The fields of ``lm`` that belong to one fit (ren_mu / ren_isd / dp: only where renorm / dp_fused read them)."""
        lm.passes = int(fcfg.epochs)
        lm.stop_tol, lm.stop_min = float(fcfg.lm_stop_tol), max(1, int(fcfg.lm_stop_min))
        lm.lam0 = float(self.tcfg.lm_lam0 if fcfg.lm_lam0 is None else fcfg.lm_lam0)
        lm.lam_carry, lm.q_kappa = float(fcfg.lm_lam_carry), float(fcfg.lm_q_kappa)
        lm.q_delta = float(fcfg.lm_q_delta) if float(fcfg.lm_q_delta) > 0.0 else 1e-6
        lm.renorm = 0
        if fcfg.lm_renorm is not None and data.fmu:
            mu, isd = fcfg.lm_renorm
            for i in range(len(mu)):
                lm.ren_mu[i], lm.ren_isd[i] = float(mu[i]), float(isd[i])
            lm.renorm = 1
        lm.dp_fused = 1 if fused else 0
        if fused:
            lm.dp = self._cache.get(("lm_dp",), self.lm_mailbox.lm_desc)

    def eval_riders(self) -> int:
        """Rider workgroups of k_lm_solve_eval: every slot of the device the
        LM_SPEC solve workgroups leave free, and no more - a rider that waits
        for a slot runs after the solve instead of under it.  Every workgroup
        of that launch carries the solve's dynamic LDS and its ~236 VGPRs: two
        per CU where two of its LDS images fit the CU's 160 KB (the 1-8-8-2
        net: 70 KB), else one (2-8-8-2: 88 KB).  euro30 with 124 / 252 / 504
        riders: 5.62 / 4.85 / 4.73 ms against 4.89 without the ride
        (profiles/eval_ride/bench_ab.txt)."""
        cus = 256
        if self.device.type == "cuda":
            cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        per_cu = 2 if 2 * (self.native.lm_solve_lds(*self.shape) + 4096) <= 160 * 1024 else 1
        return max(1, _env("EVAL_RIDERS", per_cu * cus - L.LM_SPEC))

    def eval_ride_ok(self, fcfg: FitConfig) -> bool:
        """Whether a fit with ``fcfg`` can carry the previous date's eval
        (:meth:`fit` ``ride``): the switch is on, one rank, an MSE LM fit of a
        net with a self-target pass body, at least one trial point, launched
        whole, with no exploration and no start-point transform.  The caller
        adds what it alone knows: one network, no exercise date, warm starts."""
        return bool(self.tcfg.eval_ride and _env("EVAL_RIDE", 1) and self._lm_st and self.world == 1
                    and not self.tcfg.lm_split and fcfg.optimizer == "lm" and int(fcfg.loss) == L.LOSS_MSE
                    and int(fcfg.epochs) >= 1 and fcfg.lm_renorm is None
                    and not (int(fcfg.lm_starts) >= 1 and int(fcfg.lm_explore_passes) > 0))

    def sim_riders(self, K: int) -> int:
        """Rider workgroups of k_lm_solve_sim under the solves of ``K``
        exploration instances: one per CU that the ``K x LM_SPEC`` solve
        workgroups leave free.  :meth:`eval_riders` fills every slot (two per CU
        where two LDS images fit) under ONE main solve; here 21 latency-bound
        solves in a row each carry riders, and a rider that shares a CU with a
        solve workgroup slows that solve: euro30 with 448 / 384 / 320 / 256 /
        192 riders: 4.679 / 4.668 / 4.663 / 4.674 / 4.649 ms against 4.717
        without the ride (profiles/sim_ride/sweep.txt)."""
        cus = 256
        if self.device.type == "cuda":
            cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        return max(1, min(4096, _env("SIM_RIDERS", cus - int(K) * L.LM_SPEC)))

    def sim_ride_steps(self) -> int:
        """The longest scan, in Sobol points per path (fine steps x tables),
        whose blocks ride under the exploration's solves.  A rider runs at one
        wave per SIMD, where a block costs its per-step latency times its steps
        whatever else the CU does, and a solve launch ends with its slowest
        rider.  Derived from two measured times: an exploration solve takes
        22 us and a block of 30 points 20 us (0.67 us per point: the head
        launch of euro30, profiles/sim_ride/phases_commit.txt), so 22 / 0.67 =
        32 points still end with the solve.  Longer scans stretch every solve
        they ride in (600 points, heston30: 8.0 -> 18.4 ms per replay; 252
        points, euro252: 50.1 -> 52.8 ms; profiles/sim_ride/long_scans_riding.txt)
        and keep the plain scan.  ``RPH_SIM_RIDE_STEPS`` overrides (tests)."""
        return _env("SIM_RIDE_STEPS", 32)

    def sim_ride_blocks(self) -> int:
        """Blocks per rider per solve launch: one (two in a row outlast the
        solve: 4.723 against 4.679 ms, profiles/sim_ride/sweep.txt).
        ``RPH_SIM_RIDE_BLOCKS`` overrides (A/B)."""
        return max(1, _env("SIM_RIDE_BLOCKS", 1))

    def sim_ride_ok(self, fcfg: FitConfig, model: int | None = None, path_stat: int = 0) -> bool:
        """Whether a first-date fit with ``fcfg`` can carry the run's path scan
        under its exploration's solves (:meth:`fit` ``sim_ride``): the switch is
        on, one rank, an MSE LM fit launched whole with a multi-start
        exploration on this rank's own path prefix, and (``model`` given) a
        rider for that scan under this net's solve.  The caller adds what it
        alone knows: an in-place re-simulation of one network's run."""
        return bool(self.tcfg.sim_ride and _env("SIM_RIDE", 1) and self.world == 1 and not self.tcfg.lm_split
                    and fcfg.optimizer == "lm" and int(fcfg.loss) == L.LOSS_MSE and self.lm_supported()
                    and int(fcfg.lm_starts) >= 1 and int(fcfg.lm_explore_passes) > 0 and fcfg.lm_explore_data is None
                    and (model is None or self.native.lm_has_sim(*self.shape, int(model), int(path_stat))))

    def _lm_self_target(self, d, ride):
        """The SelfTargetDesc of pass 0 of a fit (TrainDesc ``d``) that carries the eval ``ride``."""
        st = self.native.SelfTargetDesc()
        nh = self.spec.nhold
        if any(ride.price_t[k] != d.price[k] for k in range(nh - 1)) or float(ride.bond_t) != float(d.bond):
            raise ValueError("ride: the eval's prices / bond at its date are not this fit's prices_next / bond_next")
        if ride.v_out not in (None, d.target) or ride.wb or ride.g_base or ride.ex_kind:
            raise ValueError("ride: one network, no exercise date, v_out the fit's target (or none)")
        for f in range(self.spec.nin):
            st.st_feat[f], st.st_fmu[f], st.st_fisd[f] = ride.feat[f], ride.fmu[f], ride.fisd[f]
        st.st_wts, st.st_out = ride.wa, d.target
        return st

    def _lm_prepare(self, wts, opt, fit, data: DateData, fcfg: FitConfig, ride=None):
        """The filled (TrainDesc, LmDesc) of a main LM fit - with ``ride``
        (TrainDesc, LmDesc, SelfTargetDesc); launches nothing and touches no GPU API."""
        pin = int(fcfg.loss) == L.LOSS_PINBALL
        if int(fcfg.loss) not in (L.LOSS_MSE, L.LOSS_PINBALL):
            raise ValueError(f"no Levenberg-Marquardt fit for loss {fcfg.loss}")
        explore = int(fcfg.lm_starts) >= 1 and int(fcfg.lm_explore_passes) > 0
        if pin and explore:
            raise ValueError("pinball LM fits have no multi-start exploration")
        lm = self._lm_buffers(fcfg.loss)["desc"]
        # (pinball: the IRLS Gram weights need the targets of the subsample
        # paths - the simulated subsample's own when the driver evaluated them
        # (DateData.gram_target), else the shard subsample)
        self._lm_same_gram = self._lm_gram_mode(lm, data, allow_side=(not pin or data.gram_target is not None))
        # data parallel on the shared Gram subsample with the xGMI mailbox: the
        # gradient region is summed inside k_lm_reduce (no extra launch per pass)
        fused = self.world > 1 and self.lm_mailbox is not None and self._lm_same_gram and not self.tcfg.lm_split
        self._lm_set_fit(lm, fcfg, data, fused)
        if explore:
            lm.lam_carry = 1.0  # the polish starts at the chosen exploration's damping
        self.lm_last_fused = fused  # (transport probe record: which exchange this fit ran)
        d = self._full_batch_desc(wts, opt, fit, data, fcfg, fcfg.loss)
        if ride is not None and not self.eval_ride_ok(fcfg):
            raise ValueError("this fit cannot carry an eval (eval_ride_ok)")
        if ride is not None:
            return d, lm, self._lm_self_target(d, ride)
        return d, lm

    def _lm_fit(self, wts, opt, fit, data: DateData, fcfg: FitConfig, ride=None, sim_ride=None):
        """Enqueue a full-batch Levenberg-Marquardt fit (MSE): ``fcfg.epochs``
        trial points after the start point, 3 launches each (pass, reduce,
        solve), graph-capturable; data parallel: the gradient region [g |
        stats | out-means] (2.1 KB) is all-reduced between reduce and solve
        (every rank builds the same Gram matrix from the simulated global
        subsample; without it the whole reduced block travels)."""
        d, lm, *st = self._lm_prepare(wts, opt, fit, data, fcfg, ride)
        if sim_ride is not None and not self.sim_ride_ok(fcfg, sim_ride.sim.model, sim_ride.sim.path_stat):
            raise ValueError("this fit cannot carry a path scan (sim_ride_ok)")
        if int(fcfg.lm_starts) >= 1 and int(fcfg.lm_explore_passes) > 0:
            self._lm_explore(d, fcfg, sim_ride)
        self._lm_launch(d, lm, self._lm_buffers(fcfg.loss)["red"],
                        (self.world <= 1 or lm.dp_fused) and not self.tcfg.lm_split, not self._lm_same_gram, ride, st[0] if st else None)

    def _lm_launch(self, d, lm, red, one_launch: bool, gram: bool, ride=None, st=None):
        """Launch a prepared LM fit: whole (``ride``: with that eval in the
        first solve's launch), else per trial point pass + reduce, all-reduce
        (``gram``: with G), solve."""
        n = self.native
        if one_launch:
            if ride is not None:
                n.lm_fit_ride(d, lm, red, st, ride, self.eval_riders(), self.stream)
            else:
                n.lm_fit(d, lm, red, self.stream)
            return
        assert ride is None
        for k in range(lm.passes + 1):
            n.lm_eval(d, lm, red, k, self.stream)
            og = bool(lm.out_gram) and k > lm.passes - L.LM_OUTG_TAIL
            self._lm_allreduce(red, gram=gram, og=og)
            n.lm_solve(d, lm, red, k, self.stream)

    def lm_explore_paths(self, fcfg: FitConfig) -> int:
        """Paths of a multi-start exploration (lm_geometry.lm_explore_nsub)."""
        return lm_explore_nsub(fcfg, self.n_local)

    def _lm_explore_buffers(self, K: int, nsub: int) -> dict:
        """State, slabs, start points and descriptor (from the base) of ``K`` exploration fits on ``nsub`` paths."""
        _, R, nblk = self._lm_shape
        t, dev = self.tcfg, self.device
        # K instances in one launch: at most 256 x wps / K pass workgroups
        # each, so the whole grid is co-resident (wps workgroups per CU) and
        # a pass costs one round of workgroups, not K
        wps = _env("LM_EXPLORE_WPS", self._lm_wps)
        nw, leaf = lm_pass_schedule(nsub, 0 if int(t.lm_leaf_paths) >= 0 else -1, wps)
        nw1 = lm_pass_schedule(nsub, 0 if int(t.lm_leaf_paths) >= 0 else -1)[0]
        if K > 1:
            nw = max(1, min(nw, 256 * wps // K))
            nw1 = max(1, min(nw1, 256 // K))
            if leaf > 0:
                leaf = -(-((nsub + 127) // 128) // (4 * nw))
        # (the Gram subsample: one 64-path tile per workgroup of a one-per-CU
        # grid - the same subsample whatever wps)
        gw = lm_shard_gram_wgs(nsub, t.lm_gram_paths, 1, nw1)
        bufs = dict(state=torch.zeros(K, L.LMS_FLOATS, dtype=torch.float64, device=dev),
                    red=torch.zeros(K, L.LM_RED, dtype=torch.float64, device=dev),
                    slab_b=torch.zeros(K, nw, R, dtype=torch.float32, device=dev),
                    slab_g=torch.zeros(K, gw, nblk * 1024, dtype=torch.float32, device=dev),
                    w0=torch.zeros(K, L.LM_NPMAX, dtype=torch.float32, device=dev), w0_rows=None,  # (_lm_explore uploads)
                    sel=torch.zeros(L.LM_RED, dtype=torch.float64, device=dev))
        lm = _clone(self._lm_buffers()["base"])
        lm.state, lm.slab_b, lm.slab_g, lm.w0 = (bufs[k].data_ptr() for k in ("state", "slab_b", "slab_g", "w0"))
        lm.inst, lm.explore, lm.out_n, lm.out_gram = K, 1, 0, 0
        lm.num_wgs, lm.gram_wgs, lm.leaf_blocks = nw, gw, leaf  # (the prefix's own Gram subsample)
        lm.gram_blk, lm.gram_blk_stride = lm_gram_geometry(nsub, gw * L.LM_TILE, 1)
        lm.inv_ns, lm.inv_n = 1.0 / float(gw * L.LM_TILE), 1.0 / float(nsub)
        bufs["desc"] = lm
        return bufs

    def _lm_explore_prepare(self, d_main, fcfg: FitConfig):
        """The filled (TrainDesc, LmDesc) of a fit's multi-start exploration and its buffers; launches nothing."""
        K, xd = int(fcfg.lm_starts), fcfg.lm_explore_data
        if self.world > 1 and xd is None:
            raise ValueError("data-parallel multi-start exploration needs lm_explore_data (the global prefix)")
        nsub = self.lm_explore_paths(fcfg)
        if K > L.LM_SEL_MAX:
            raise ValueError(f"{K} starts exceed the {L.LM_SEL_MAX} selection candidates")
        if fcfg.lm_w0s is None or len(fcfg.lm_w0s) < K:
            raise ValueError("multi-start exploration needs lm_w0s (one start point per instance)")
        x = self._cache.get(("lm_explore", K, nsub), lambda: self._lm_explore_buffers(K, nsub))
        # every exploration fit: lm_explore_passes trial points from lm_lam0, no
        # adaptive stop, damping carry or start-point transform, never fused
        self._lm_set_fit(x["desc"], replace(fcfg, epochs=int(fcfg.lm_explore_passes), lm_stop_tol=0.0, lm_lam_carry=0.0,
                                            lm_renorm=None), None, False)
        d = _clone(d_main)
        if xd is not None:
            self.native.fill_ptrs(d.feat, xd.feats)
            self.native.fill_ptrs(d.price, xd.prices_next)
            d.target = xd.target.data_ptr()
        d.n_local = d.batch = nsub
        d.inv_batch = 1.0 / float(nsub)
        return d, x["desc"], x

    def _lm_explore(self, d_main, fcfg: FitConfig, sim_ride=None):
        """Multi-start exploration of a first date (graph-capturable): K
        independent LM fits in ONE launch per kernel (grid y = instance) on the
        global path prefix (FitConfig.lm_explore_data, or this rank's shard
        prefix when it is the global one); k_lm_select writes the winner into
        the NetWeights and its damping into the main LM state (the polish fit
        carries it).  Every rank runs the same fits on the same paths: the
        pick needs no exchange and does not depend on the world size."""
        d, lm, x = self._lm_explore_prepare(d_main, fcfg)
        K, P = int(lm.inst), self.P
        # this call's start points: a cached buffer must not keep an earlier
        # fit's candidates (a new set is uploaded on the backend's stream, after
        # the work already queued there; not inside a graph capture)
        rows = np.ascontiguousarray(np.asarray(fcfg.lm_w0s, dtype=np.float32)[:K, :P])
        if rows.tobytes() != x["w0_rows"]:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("multi-start start points changed inside a graph capture")
            w0 = torch.zeros(K, L.LM_NPMAX, dtype=torch.float32)
            w0[:, :P] = torch.from_numpy(rows)
            if self.device.type == "cuda" and self.stream is not None:
                with torch.cuda.stream(self.stream):  # (the launches' stream: ordered after queued fits)
                    x["w0"].copy_(w0)
            else:
                x["w0"].copy_(w0)
            x["w0_rows"] = rows.tobytes()
        n, main_state = self.native, self._lm_buffers()["state"]
        if sim_ride is not None:
            # (the exploration reads the blocks the head launch simulated: the
            # others ride in its solve launches, all of them enqueued on return)
            if int(sim_ride.b0) * 256 < int(d.n_local):
                raise ValueError("sim ride: the head launch does not cover the exploration's paths")
            n.lm_fit_sim(d, lm, x["red"], sim_ride, self.sim_riders(K), self.stream)
        else:
            n.lm_fit(d, lm, x["red"], self.stream)
        n.lm_select(d, lm, x["sel"], main_state, 1, 0, P, 0, self.stream)
        n.lm_select(d, lm, x["sel"], main_state, 1, 0, P, 1, self.stream)
        self.lm_explore_last = x

    def _lm_allreduce(self, red: torch.Tensor, gram: bool = True, og: bool = False):
        """Sum the reduced LM block over the ranks: in-kernel exchange over the
        IPC mailboxes (xGMI transport) or one RCCL all-reduce.  ``gram=False``
        (every rank built the same Gram matrix): only the gradient region
        travels, [g | stats] = 200 doubles (1.6 KB), + the packed output Gram
        in the passes that build it (``og``)."""
        P, _, nblk = self._lm_shape
        if self.lm_mailbox is not None:
            x = self._cache.get(("lm_dp",), self.lm_mailbox.lm_desc)
            if gram:
                self.native.lm_dp_exchange(x, red, nblk * 1024 + lm_tpack_len(P, nblk), P, self.stream)
            else:
                self.native.lm_dp_exchange(x, red, 0, self._lm_greg(og), self.stream)
            return
        if gram:
            self._lm_comm().allreduce_(red, self.stream)
        else:
            self._lm_comm().allreduce_(red[L.LM_GBLK_MAX:L.LM_GBLK_MAX + self._lm_greg(og)], self.stream)

    def bias_refit(self, wts, opt, fit, data: DateData, fcfg: FitConfig):
        """Exact refit of the bond holding's output bias after an Adam fit (one
        full-batch loss + gradient pass at the fitted weights, then the 1-D
        Newton step of the LM solver, FitState untouched): the residual's mean
        over all paths becomes zero, so no mean error drifts down the induction
        (V0 then sits on the paths' price instead of scattering with the
        minibatch noise of the last fits).  No-op for complement heads."""
        bi = _lm_bias_index(self.spec, self.tcfg)
        if bi < 0:
            return
        if not self.lm_supported():
            # nets without an LM solver (32-unit MFMA family): the eval kernel's
            # residual sum (res = target - prediction) gives the same step.
            # Every buffer is preallocated and every op writes into it (nothing
            # is allocated inside a graph capture); data parallel, the two sums
            # travel like an LM block: k_lm_dp_exchange over the LM mailbox
            # (xGMI) or the RCCL communicator chosen by select_transport
            c = self._cache.get(("refit",), self._refit_buffers)
            st, red = c["stats"], c["red"]
            G, S = L.LM_GBLK_MAX, L.LM_GBLK_MAX + L.LM_NPMAX
            self.eval(wts, data, st)
            torch.sum(st[:, L.ES_RES], dim=0, out=red[G])
            torch.sum(st[:, L.ES_COUNT], dim=0, out=red[S])
            if self.world > 1:
                if self.lm_mailbox is not None:
                    x = self._cache.get(("lm_dp",), self.lm_mailbox.lm_desc)
                    self.native.lm_dp_exchange(x, red, 0, L.LM_RED_OUTG - L.LM_GBLK_MAX, self.stream)
                else:
                    self._lm_comm().allreduce_(red[G:S + 1], self.stream)
            torch.clamp_min(red[S:S + 1], 1.0, out=c["cnt"])
            torch.div(red[G:G + 1], c["cnt"], out=c["delta"])
            c["delta"].mul_(1.0 / float(data.bond_next))
            wts[bi:bi + 1].add_(c["delta"])
            fit[L.F_WBEST + bi:L.F_WBEST + bi + 1].copy_(wts[bi:bi + 1])
            return
        d, lm = self._lm_refit_prepare(wts, opt, fit, data, fcfg)
        self._lm_launch(d, lm, self._lm_buffers()["red"], self.world <= 1, True)

    def _lm_refit_prepare(self, wts, opt, fit, data: DateData, fcfg: FitConfig):
        """The filled (TrainDesc, LmDesc) of the bias refit (no trial point, weights only, one Gram tile); no launch."""
        def make():
            lm = _clone(self._lm_buffers()["base"])
            lm.weights_only, lm.gram_wgs, lm.out_n, lm.out_gram = 1, 1, 0, 0
            lm.gram_blk, lm.gram_blk_stride = lm_gram_geometry(self.n_local, L.LM_TILE, self.world)
            lm.inv_ns = 1.0 / float(L.LM_TILE * max(self.world, 1))
            return lm
        return self._full_batch_desc(wts, opt, fit, data, fcfg, L.LOSS_MSE), self._cache.get(("lm_refit",), make)

    def _refit_buffers(self) -> dict:
        dev = self.device
        return {"stats": self.new_stats(), "red": torch.zeros(L.LM_RED, dtype=torch.float64, device=dev),
                "cnt": torch.zeros(1, dtype=torch.float64, device=dev),
                "delta": torch.zeros(1, dtype=torch.float64, device=dev)}

    def _lm_comm(self):
        """RCCL communicator of the LM reduced block: the one select_transport
        created when the block's xGMI probe failed (``lm_comm``), else the
        backend's RCCL communicator.  Never created lazily here (it could be
        inside a graph capture)."""
        if self._lm_nccl is not None:
            return self._lm_nccl
        if self.comm is not None:
            return self.comm
        raise RuntimeError("LM reduced-block exchange without an xGMI mailbox or an RCCL communicator: build "
                           "data-parallel backends through rphedge.parallel.dist.select_transport (or pass lm_comm)")

    def lm_state(self) -> dict:
        """Host view of the last LM fit (accepted steps, Cholesky failures, damping)."""
        st = self._lm_buffers()["state"].cpu().numpy()
        return {"accepted": int(st[L.LMS_NACC]), "chol_failures": int(st[L.LMS_FAIL]), "lam": float(st[L.LMS_LAM]),
                "chol_failures_total": int(st[L.LMS_FAILTOT])}

    def step_mode(self, poll_every: int = 0) -> str:
        """Resolve TrainConfig.step_mode for this backend (see TrainConfig)."""
        t = self.tcfg
        atomic = not t.deterministic and not t.split_update
        dp_fused = self.mailbox is not None and self.comm is None
        if (t.step_mode == "persistent" and atomic and not poll_every and (self.world == 1 or dp_fused)
                and self.persistent_supported()):
            # (explicit only: needs every workgroup of every rank co-resident)
            return "persistent"
        shared = dp_fused and getattr(self.mailbox, "shared_device", False)
        if t.step_mode == "lag" and atomic and (self.world == 1 or dp_fused):
            return "lag"
        # small grids (the reference's batch 512 = 2 workgroups): the persistent
        # kernel's in-kernel barrier is cheaper than a kernel boundary below ~96
        # workgroups (profiles/r1/crossover_r1g.jsonl) and one launch per fit
        # removes the per-step host launch from eager runs
        if (t.step_mode == "auto" and atomic and self.world == 1 and not poll_every
                and self.spec.hidden == 8 and self.num_wgs <= PERSISTENT_MAX_WGS):
            return "persistent"
        if t.step_mode == "persistent" and atomic and (self.world == 1 or dp_fused):
            return "lag"  # shape without a persistent kernel (or host polling): lagged steps
        if t.step_mode == "auto" and atomic and (self.world == 1 or (dp_fused and not shared)):
            return "lag"
        return "ticket"

    def concurrent_with(self, other: "HipBackend") -> bool:
        """Whether a fit of this backend may run concurrently (another stream)
        with a fit of ``other`` without a co-residency deadlock: persistent
        kernels need every workgroup resident, so two of them must fit the
        device together (one workgroup per CU at one wave per SIMD)."""
        a, b = self.step_mode(), other.step_mode()
        cus = 256
        try:
            cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        except Exception:
            pass
        need = (self.num_wgs if a == "persistent" else 0) + (other.num_wgs if b == "persistent" else 0)
        if ("persistent" in (a, b)) and need > cus:
            return False
        return self.world == 1 and other.world == 1

    def persistent_supported(self) -> bool:
        """Shapes with a persistent per-fit kernel (csrc/hedge_fit.h): every
        8-unit net; the 32-unit nets up to 3 inputs (wide_has_fit,
        csrc/hedge_mlp_wide.hip)."""
        return self.spec.hidden == 8 or self.spec.nin <= 3

    def check(self):
        """Raise if a persistent fit timed out waiting for co-resident workgroups."""
        if int(self.fit_ctl[1].item()) != 0:
            raise RuntimeError("persistent fit kernel: workgroups not co-resident (wait timed out); "
                               "use TrainConfig.step_mode='lag' or 'ticket'")

    def pnl_wgs(self, n_local: int | None = None) -> int:
        return ((self.n_local if n_local is None else int(n_local)) + 256 * PNL_PPT - 1) // (256 * PNL_PPT)

    def pnl(self, snap, data: PnlData, stats, has_b: bool = False, hold_c: float = 0.0, pnl_out=None,
            exercise: Exercise | None = None, tau_out=None, n_local: int | None = None,
            costs: Costs | None = None, cost_stats=None, cost_out=None, turn_out=None, trades_out=None):
        """Enqueue the self-financing P&L scan (one k_hedge_pnl launch);
        ``exercise``: with the stopping rule, ``tau_out`` (int32) the exercise dates;
        ``n_local``: the path count of ``data`` when it is not this backend's
        shard (out-of-sample paths; ``stats`` then has ``pnl_wgs(n_local)`` rows).

        ``costs``: the scan under transaction costs and a no-trade band instead
        (one k_hedge_pnl_cost launch; None: the plain launch above): ``cost_stats``
        is its ``[pnl_wgs, COST_NSTAT]`` float64 slab, ``cost_out`` / ``turn_out``
        (float32) and ``trades_out`` (int32) the optional per-path cost carried
        to the horizon, turnover and trade dates.  Not with ``exercise``."""
        nl = self.n_local if n_local is None else int(n_local)
        if nl != int(data.payoff.numel()):
            raise ValueError(f"pnl over {data.payoff.numel()} paths with n_local {nl}")
        n = self.native
        d = n.PnlDesc()
        f0, p0, p1 = data.features(0), data.prices(0), data.prices(1)
        f1 = data.features(1) if data.n_dates >= 1 else f0
        n.fill_ptrs(d.feat, f0)
        n.fill_ptrs(d.price, p0)
        for i, (a, b) in enumerate(zip(f0, f1)):
            d.feat_ts[i] = (b.data_ptr() - a.data_ptr()) // 4
        for k, (a, b) in enumerate(zip(p0, p1)):
            d.price_ts[k] = (b.data_ptr() - a.data_ptr()) // 4
        d.snap = snap.data_ptr()
        d.fmu, d.fisd, d.bond = data.fmu.data_ptr(), data.fisd.data_ptr(), data.bond.data_ptr()
        d.w0, d.payoff = n.ptr(data.w0), data.payoff.data_ptr()
        d.pnl_out = n.ptr(pnl_out)
        d.stats = stats.data_ptr()
        wealth0 = float(data.wealth0) if data.w0 is None else 0.0
        d.alpha, d.hold_c, d.wealth0, d.has_b = float(self.spec.alpha), float(hold_c), wealth0, 1 if has_b else 0
        d.n_local, d.n_dates, d.num_wgs = nl, int(data.n_dates), self.pnl_wgs(nl)
        d.nin, d.h, d.nout, d.head = self.shape
        if exercise is not None:
            d.ex_kind, d.ex_every, d.ex_strike = L.EX_KINDS[exercise.kind], int(exercise.every), float(exercise.strike)
        if tau_out is not None:
            assert tau_out.dtype == torch.int32 and tau_out.numel() == nl
            d.tau_out = tau_out.data_ptr()
        assert stats.shape[0] == d.num_wgs and snap.shape[0] >= data.n_dates
        if costs is None:
            if any(t is not None for t in (cost_stats, cost_out, turn_out, trades_out)):
                raise ValueError("pnl: cost outputs without costs")
            n.pnl(d, self.stream)
            return
        if exercise is not None:
            raise ValueError("pnl: costs with exercise (early exercise with costs is not supported)")
        cd = n.CostPnlDesc()
        cd.p = d
        self._cost_terms(cd.c, "pnl", costs, nl, d.num_wgs, cost_stats, cost_out, turn_out, trades_out)
        n.pnl_cost(cd, self.stream)

    def _cost_terms(self, c, who, costs: Costs, nl: int, wgs: int, cost_stats, cost_out, turn_out, trades_out):
        """Fill the ``CostTerms`` of a scan over ``nl`` paths on ``wgs`` workgroups."""
        if (cost_stats is None or cost_stats.dtype != torch.float64 or cost_stats.dim() != 2
                or tuple(cost_stats.shape) != (wgs, LC.COST_NSTAT)):
            raise ValueError(f"{who}: cost_stats must be float64 [{wgs}, {LC.COST_NSTAT}]")
        for name, t, dt in (("cost_out", cost_out, torch.float32), ("turn_out", turn_out, torch.float32),
                            ("trades_out", trades_out, torch.int32)):
            if t is not None and (t.dtype != dt or t.numel() != nl):
                raise ValueError(f"{who}: {name} must be {dt} [{nl}]")
        c.cost_rate, c.band, c.unwind = float(costs.rate), float(costs.band), 1 if costs.unwind else 0
        n = self.native
        c.cost_out, c.turn_out, c.trades_out = n.ptr(cost_out), n.ptr(turn_out), n.ptr(trades_out)
        c.cstats = cost_stats.data_ptr()

    def oos_wgs(self, n_local: int) -> int:
        """Grid of a k_hedge_oos launch over ``n_local`` paths: persistent
        workgroups, at most OOS_WGS_PER_CU per CU and never more than 256-path tiles."""
        return int(max(1, min(self.native.oos_max_wgs(), (int(n_local) + 255) // 256)))

    def oos(self, sim, snap, data: PnlData, stats, payoff_kind: int, strike: float, has_b: bool = False,
            hold_c: float = 0.0, pnl_out=None, payoff_out=None, costs: Costs | None = None, cost_stats=None,
            cost_out=None, turn_out=None, trades_out=None, jump=None):
        """Enqueue the fused simulate-and-hedge of fresh paths (one k_hedge_oos
        launch).  ``sim``: the scan's ``SimDesc`` (``ops.paths.gbm_desc`` /
        ``sv_desc``; its output pointers are the optional trace); ``data``: the
        run's standardisation and bond tables and the scalar ``wealth0`` (its
        path tables are not read); ``stats``: ``[num_wgs, EVAL_NSTAT]`` float64 -
        its row count is the grid (``oos_wgs``, or fewer to make workgroups loop).
        ``costs`` and the cost outputs: as in :meth:`pnl` (one k_hedge_oos_cost
        launch; ``cost_stats`` has the rows of ``stats``).  ``jump``: the
        ``JumpTerms`` of a Merton scan (``ops.paths.merton_desc``:
        k_hedge_oos_jump / k_hedge_oos_jump_cost)."""
        n = self.native
        if (jump is not None) != (int(sim.model) == L.SIM_MERTON):
            raise ValueError("oos: jump terms go with a SIM_MERTON scan, and only with one")
        d = n.OosDesc()
        d.sim = sim
        nl = int(sim.n_local)
        d.snap = snap.data_ptr()
        d.fmu, d.fisd, d.bond = data.fmu.data_ptr(), data.fisd.data_ptr(), data.bond.data_ptr()
        for name, t in (("pnl_out", pnl_out), ("payoff_out", payoff_out)):
            if t is not None and (t.dtype != torch.float32 or t.numel() != nl):
                raise ValueError(f"oos: {name} must be float32 [{nl}]")
        d.pnl_out, d.payoff_out = n.ptr(pnl_out), n.ptr(payoff_out)
        if stats.dtype != torch.float64 or stats.dim() != 2 or stats.shape[1] != L.EVAL_NSTAT:
            raise ValueError(f"oos: stats must be float64 [num_wgs, {L.EVAL_NSTAT}]")
        d.stats = stats.data_ptr()
        d.alpha, d.hold_c, d.wealth0, d.strike = float(self.spec.alpha), float(hold_c), float(data.wealth0), float(strike)
        d.has_b, d.payoff_kind, d.n_dates, d.num_wgs = 1 if has_b else 0, int(payoff_kind), int(data.n_dates), int(stats.shape[0])
        d.nin, d.h, d.nout, d.head = self.shape
        if snap.shape[0] < data.n_dates or data.fmu.shape[0] < data.n_dates or data.bond.numel() < data.n_dates + 1:
            raise ValueError("oos: snapshot / standardisation / bond tables shorter than n_dates")
        if costs is None:
            if any(t is not None for t in (cost_stats, cost_out, turn_out, trades_out)):
                raise ValueError("oos: cost outputs without costs")
            if jump is not None:
                n.oos_jump(d, jump, self.stream)
            else:
                n.oos(d, self.stream)
            return d
        cd = n.CostOosDesc()
        cd.o = d
        self._cost_terms(cd.c, "oos", costs, nl, d.num_wgs, cost_stats, cost_out, turn_out, trades_out)
        if jump is not None:
            n.oos_jump_cost(cd, jump, self.stream)
        else:
            n.oos_cost(cd, self.stream)
        return cd

    def pnl_finish(self, acc, w0, payoff, carry: float, stats, pnl_out=None):
        """Enqueue k_pnl_finish after the eval of date 0 of a run whose evals
        accumulated ``acc`` (``eval(pnl_acc=...)``): W_T = w0 ``carry`` + acc,
        P&L = W_T - payoff, statistics in the rows :meth:`pnl` writes."""
        n = self.native
        d = n.PnlFinishDesc()
        for t in (acc, w0, payoff):
            assert t.dtype == torch.float32 and t.numel() == self.n_local
        d.acc, d.w0, d.payoff = acc.data_ptr(), w0.data_ptr(), payoff.data_ptr()
        if pnl_out is not None:
            assert pnl_out.dtype == torch.float32 and pnl_out.numel() == self.n_local
        d.pnl_out = n.ptr(pnl_out)
        d.stats = stats.data_ptr()
        d.carry = float(carry)
        d.n_local, d.num_wgs = self.n_local, self.pnl_wgs()
        d.nin, d.h, d.nout, d.head = self.shape
        assert stats.shape[0] == d.num_wgs
        n.pnl_finish(d, self.stream)

    def eval(self, wts, data: DateData, stats, wts_b=None, g_base=None, blend_c=0.0, hold_c=0.0,
             v_out=None, hold_out=None, resid_out=None, pred1_out=None, snap_a=None, snap_b=None,
             n_local: int | None = None, exercise: Exercise | None = None, pnl_acc=None, pnl_grow: float = 1.0,
             pnl_carry: float = 1.0, pnl_first: bool = False):
        """k_hedge_eval over ``data`` (``n_local``: its path count when it is
        not this backend's shard, e.g. the Gram subsample; ``exercise``: the
        date is an exercise date, ``v_out`` = max(intrinsic, continuation)).

        ``pnl_acc`` ([n] float32): fold the date's term of the self-financing
        P&L into the eval - ``pnl_acc += pnl_carry sum_a h_a (S_a,t+1 - S_a,t
        pnl_grow)`` with the reported holdings (``config.pnl_fold_factors``);
        ``pnl_first``: the first accumulated date writes ``pnl_acc`` without
        reading it.  :meth:`pnl_finish` closes the recursion after date 0."""
        self.native.eval_(self.eval_desc(wts, data, stats, wts_b=wts_b, g_base=g_base, blend_c=blend_c, hold_c=hold_c,
                                         v_out=v_out, hold_out=hold_out, resid_out=resid_out, pred1_out=pred1_out,
                                         snap_a=snap_a, snap_b=snap_b, n_local=n_local, exercise=exercise,
                                         pnl_acc=pnl_acc, pnl_grow=pnl_grow, pnl_carry=pnl_carry,
                                         pnl_first=pnl_first), self.stream)

    def eval_desc(self, wts, data: DateData, stats, wts_b=None, g_base=None, blend_c=0.0, hold_c=0.0,
                  v_out=None, hold_out=None, resid_out=None, pred1_out=None, snap_a=None, snap_b=None,
                  n_local: int | None = None, exercise: Exercise | None = None, pnl_acc=None, pnl_grow: float = 1.0,
                  pnl_carry: float = 1.0, pnl_first: bool = False):
        """The filled descriptor of :meth:`eval` (same arguments); launches nothing."""
        _check_eval_data(self.spec, data)
        n = self.native
        d = n.EvalDesc()
        d.snap_a, d.snap_b = n.ptr(snap_a), n.ptr(snap_b)
        n.fill_ptrs(d.feat, data.feats)
        n.fill_ptrs(d.price_t, data.prices_now)
        n.fill_ptrs(d.price_t1, data.prices_next)
        d.target = n.ptr(data.target)
        d.wa, d.wb, d.g_base, d.v_out = wts.data_ptr(), n.ptr(wts_b), n.ptr(g_base), n.ptr(v_out)
        if hold_out is not None:
            n.fill_ptrs(d.hold_out, hold_out)
        d.resid_out, d.pred1_out = n.ptr(resid_out), n.ptr(pred1_out)
        d.stats = stats.data_ptr()
        d.bond_t, d.bond_t1 = float(data.bond_now), float(data.bond_next)
        d.alpha = float(self.spec.alpha)
        d.blend_c, d.hold_c = float(blend_c), float(hold_c)
        d.n_local = self.n_local if n_local is None else int(n_local)
        if d.n_local != int(data.feats[0].numel()):
            raise ValueError(f"eval over {data.feats[0].numel()} paths with n_local {d.n_local}")
        d.num_wgs = self.eval_wgs
        d.nin, d.h, d.nout, d.head = self.shape
        _set_norm(d, data)
        if exercise is not None:
            d.ex_kind, d.ex_strike = L.EX_KINDS[exercise.kind], float(exercise.strike)
        if pnl_acc is not None:
            if pnl_acc.dtype != torch.float32 or pnl_acc.numel() != d.n_local:
                raise ValueError(f"eval: pnl_acc must be float32 [{d.n_local}]")
            d.pnl_acc = pnl_acc.data_ptr()
            d.pnl_grow, d.pnl_carry, d.pnl_first = float(pnl_grow), float(pnl_carry), 1 if pnl_first else 0
        return d
