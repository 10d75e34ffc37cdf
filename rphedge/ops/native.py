"""ctypes bindings to the in-tree native library ``rphedge/_lib/librphedge.so``.

The library (HIP kernels for gfx950 + C++ runtime: hipGraph capture, RCCL
communicator) exposes a plain C ABI.  ``torch`` is imported first so that the
HIP runtime (``libamdhip64.so.7``) and RCCL (``librccl.so.1``) already loaded
by torch are reused by the dynamic loader — one HIP runtime per process,
device pointers from torch tensors are valid in our kernels.

On a machine with a GPU the native library is mandatory: every op raises if it
is missing (no silent eager fallback).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch  # noqa: F401  (must be loaded before librphedge.so)

from . import layout as L
from . import layout_cost as LC
from .layout import DP_SLOTS, MAXHOLD, MAXIN  # noqa: F401  (imported from here by the engine and the tests)

# RPH_NATIVE_LIB=debug|asan selects the variant built by `python -m rphedge.build --debug|--asan`;
# a path ending in .so loads that exact library (A/B of two builds, tools/ab_presets.sh)
_LIB_ENV = os.environ.get("RPH_NATIVE_LIB", "")
_LIB_PATH = Path(_LIB_ENV).resolve() if _LIB_ENV.endswith(".so") else Path(__file__).resolve().parent.parent / "_lib" / (
    {"debug": "librphedge_debug.so", "asan": "librphedge_asan.so"}.get(_LIB_ENV, "librphedge.so"))
_lib = None
_load_error: str | None = None

VP = C.c_void_p

# The launch descriptors of csrc/rph_types.h, field by field, pads included
# (the structs have no implicit padding).  load() compares every name, offset
# and size with the native library's table (csrc/rph_layout.h).


class TrainDesc(C.Structure):
    _fields_ = [
        ("feat", VP * MAXIN), ("price", VP * MAXHOLD), ("target", VP),
        ("wts", VP), ("opt", VP), ("fit", VP), ("lr_sched", VP),
        ("slab", VP), ("counter", VP), ("grad_out", VP),
        ("bond", C.c_float), ("alpha", C.c_float), ("quantile", C.c_float), ("inv_batch", C.c_float),
        ("loss", C.c_int), ("n_local", C.c_int), ("batch", C.c_int), ("steps_per_epoch", C.c_int),
        ("chunk_log2", C.c_int), ("shuffle", C.c_int), ("seed", C.c_uint32), ("fused_update", C.c_int),
        ("num_wgs", C.c_int), ("nin", C.c_int), ("h", C.c_int), ("nout", C.c_int), ("head", C.c_int),
        ("pad_acc", C.c_int), ("acc", VP), ("deterministic", C.c_int), ("pad_stamps", C.c_int), ("stamps", VP),
        ("dp_world", C.c_int), ("dp_rank", C.c_int), ("dp_mbox", VP * 8), ("dp_flags", VP * 8),
        ("dp_counter", VP), ("dp_error", VP), ("mfma_fp32", C.c_int), ("pad_lag", C.c_int), ("lag", VP),
        ("variant", C.c_int), ("pad_fit_init", C.c_int), ("fit_init", VP),
        ("fmu", C.c_float * MAXIN), ("fisd", C.c_float * MAXIN),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        for f in range(MAXIN):  # identity standardisation unless the backend sets one
            self.fisd[f] = 1.0


class EvalDesc(C.Structure):
    _fields_ = [
        ("feat", VP * MAXIN), ("price_t", VP * MAXHOLD), ("price_t1", VP * MAXHOLD), ("target", VP),
        ("wa", VP), ("wb", VP), ("g_base", VP), ("v_out", VP), ("hold_out", VP * MAXHOLD),
        ("resid_out", VP), ("pred1_out", VP), ("stats", VP),
        ("bond_t", C.c_float), ("bond_t1", C.c_float), ("alpha", C.c_float), ("blend_c", C.c_float),
        ("hold_c", C.c_float),
        ("n_local", C.c_int), ("num_wgs", C.c_int), ("nin", C.c_int), ("h", C.c_int), ("nout", C.c_int),
        ("head", C.c_int), ("fmu", C.c_float * MAXIN), ("fisd", C.c_float * MAXIN),
        ("pad_snap", C.c_int), ("snap_a", VP), ("snap_b", VP), ("ex_kind", C.c_int), ("ex_strike", C.c_float),
        ("pnl_acc", VP), ("pnl_grow", C.c_float), ("pnl_carry", C.c_float), ("pnl_first", C.c_int),
        ("pad_pnl", C.c_int),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        for f in range(MAXIN):
            self.fisd[f] = 1.0


class PnlFinishDesc(C.Structure):
    _fields_ = [
        ("acc", VP), ("w0", VP), ("payoff", VP), ("pnl_out", VP), ("stats", VP),
        ("carry", C.c_float), ("n_local", C.c_int), ("num_wgs", C.c_int),
        ("nin", C.c_int), ("h", C.c_int), ("nout", C.c_int), ("head", C.c_int), ("pad0", C.c_int),
    ]


class PnlDesc(C.Structure):
    _fields_ = [
        ("feat", VP * MAXIN), ("feat_ts", C.c_longlong * MAXIN), ("price", VP * MAXHOLD),
        ("price_ts", C.c_longlong * MAXHOLD), ("snap", VP), ("fmu", VP), ("fisd", VP), ("bond", VP),
        ("w0", VP), ("payoff", VP), ("pnl_out", VP), ("stats", VP),
        ("alpha", C.c_float), ("hold_c", C.c_float), ("wealth0", C.c_float), ("has_b", C.c_int),
        ("n_local", C.c_int), ("n_dates", C.c_int), ("num_wgs", C.c_int),
        ("nin", C.c_int), ("h", C.c_int), ("nout", C.c_int), ("head", C.c_int),
        ("ex_kind", C.c_int), ("ex_every", C.c_int), ("ex_strike", C.c_float), ("tau_out", VP),
    ]


class LmDpDesc(C.Structure):
    _fields_ = [
        ("mbox", VP * 8), ("counter", VP), ("error", VP),
        ("world", C.c_int), ("rank", C.c_int), ("pitch", C.c_int), ("fault", C.c_int),
    ]


class LmDesc(C.Structure):
    _fields_ = [
        ("state", VP), ("slab_b", VP), ("slab_g", VP),
        ("num_wgs", C.c_int), ("gram_wgs", C.c_int), ("red_wgs", C.c_int), ("passes", C.c_int),
        ("gram_blk", C.c_int), ("gram_blk_stride", C.c_int), ("inv_ns", C.c_float), ("inv_n", C.c_float),
        ("lam0", C.c_float), ("lam_up", C.c_float), ("lam_down", C.c_float), ("lam_min", C.c_float),
        ("lam_max", C.c_float), ("ridge", C.c_float), ("bias_index", C.c_int), ("weights_only", C.c_int),
        ("damping", C.c_int), ("stop_min", C.c_int), ("stop_tol", C.c_float), ("gram_skip", C.c_int),
        ("inst", C.c_int), ("explore", C.c_int), ("lam_carry", C.c_float), ("diag_floor", C.c_float), ("w0", VP),
        ("renorm", C.c_int), ("pad1", C.c_int), ("ren_mu", C.c_float * MAXIN), ("ren_isd", C.c_float * MAXIN),
        ("out_n", C.c_int), ("out_mu", C.c_float), ("out_gram", C.c_int), ("out_tr", C.c_float),
        ("slab_o", VP),
        ("gfeat", VP * MAXIN), ("gprice", VP * MAXIN), ("gram_side", C.c_int), ("q_delta", C.c_float), ("q_kappa", C.c_float),
        ("pad_dp", C.c_int), ("dp", LmDpDesc), ("dp_fused", C.c_int), ("leaf_blocks", C.c_int), ("gtarget", VP),
        ("gram_base", C.c_int), ("pad4", C.c_int),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.inst = 1  # one fit per launch unless a multi-start exploration sets more


class SelfTargetDesc(C.Structure):
    """Pass 0 of an LM fit evaluating its own target (csrc/rph_types.h; ``st_out`` null: off)."""

    _fields_ = [
        ("st_feat", VP * MAXIN), ("st_wts", VP), ("st_out", VP), ("st_fmu", C.c_float * MAXIN),
        ("st_fisd", C.c_float * MAXIN),
    ]


class SimDesc(C.Structure):
    _fields_ = [
        ("model", C.c_int), ("n_local", C.c_int), ("path_offset", C.c_longlong),
        ("n_fine", C.c_int), ("reduction", C.c_int), ("n_coarse", C.c_int), ("na", C.c_int),
        ("fp64", C.c_int), ("parity", C.c_int),
        ("sv1", VP), ("shift1", VP), ("dims1", C.c_int), ("pad_sv2", C.c_int),
        ("sv2", VP), ("shift2", VP), ("dims2", C.c_int), ("pad_s0", C.c_int),
        ("s0", C.c_double * MAXIN), ("mu", C.c_double * MAXIN), ("sigma", C.c_double * MAXIN),
        ("chol", C.c_double * (MAXIN * MAXIN)), ("dt", C.c_double), ("inv_norm", C.c_double * MAXIN),
        ("v0", C.c_double), ("a", C.c_double), ("b", C.c_double), ("c", C.c_double),
        ("kappa", C.c_double), ("theta", C.c_double), ("xi", C.c_double), ("rho", C.c_double),
        ("l0", C.c_double), ("lc", C.c_double), ("eta", C.c_double), ("n0", C.c_int), ("seed", C.c_uint32),
        ("out", VP), ("out2", VP), ("out3", VP), ("final_out", VP), ("final2_out", VP),
        ("sv_tscale", C.c_double), ("scheme", C.c_int), ("path_stat", C.c_int),
        ("map_blk", C.c_longlong), ("map_stride", C.c_longlong),
    ]


class OosDesc(C.Structure):
    """k_hedge_oos (csrc/hedge_oos.hip): ``sim`` is the scan of the fresh paths;
    its output pointers are the optional trace (null in production)."""

    _fields_ = [
        ("sim", SimDesc), ("snap", VP), ("fmu", VP), ("fisd", VP), ("bond", VP), ("pnl_out", VP),
        ("payoff_out", VP), ("stats", VP),
        ("alpha", C.c_float), ("hold_c", C.c_float), ("wealth0", C.c_float), ("strike", C.c_float),
        ("has_b", C.c_int), ("payoff_kind", C.c_int), ("n_dates", C.c_int), ("num_wgs", C.c_int),
        ("nin", C.c_int), ("h", C.c_int), ("nout", C.c_int), ("head", C.c_int),
    ]


class SimRideDesc(C.Structure):
    """The run's scan split over the solve launches of a first date's
    exploration (csrc/rph_types.h): ``sim`` is the run's scan, blocks
    ``[b0, b1)`` of 256 paths are still to simulate after the head launch."""

    _fields_ = [
        ("sim", SimDesc), ("pay_out", VP), ("pay_out2", VP), ("strike", C.c_float), ("pay_kind", C.c_int),
        ("b0", C.c_int), ("b1", C.c_int), ("per_rider", C.c_int), ("pad_ride", C.c_int),
    ]


class CostTerms(C.Structure):
    """Proportional transaction costs and the no-trade band of a forward scan
    (csrc/rph_types.h); ``cstats``: ``[num_wgs, COST_NSTAT]`` float64."""

    _fields_ = [
        ("cost_rate", C.c_float), ("band", C.c_float), ("unwind", C.c_int), ("pad", C.c_int),
        ("cost_out", VP), ("turn_out", VP), ("trades_out", VP), ("cstats", VP),
    ]


class CostPnlDesc(C.Structure):
    """k_hedge_pnl_cost (csrc/hedge_cost.hip): the P&L scan ``p`` under the costs ``c``."""

    _fields_ = [("p", PnlDesc), ("c", CostTerms)]


class CostOosDesc(C.Structure):
    """k_hedge_oos_cost (csrc/hedge_oos.hip): the fused simulate-and-hedge ``o`` under the costs ``c``."""

    _fields_ = [("o", OosDesc), ("c", CostTerms)]


class JumpTerms(C.Structure):
    """The jump terms of a Merton scan (csrc/rph_types.h), a second kernel
    argument beside ``SimDesc``; ``thr``: ``ops.paths.merton_thresholds(lam * dt)``."""

    _fields_ = [("lam", C.c_double), ("mu_j", C.c_double), ("sig_j", C.c_double), ("thr", C.c_uint32 * L.JUMP_MAX)]


DESCRIPTORS = (TrainDesc, EvalDesc, PnlFinishDesc, PnlDesc, LmDpDesc, LmDesc, SimDesc)
# descriptors of the native library's second field table (csrc/rph_layout.h
# RPH_DESCRIPTORS_EXT, rph_layout_fields_ext): checked by name at load like the first
DESCRIPTORS_EXT = (OosDesc,)
# ... and of its third (RPH_DESCRIPTORS_RIDE, rph_layout_fields_ride): the eval ride
DESCRIPTORS_RIDE = (SelfTargetDesc,)
# ... and its fourth (RPH_DESCRIPTORS_SIM, rph_layout_fields_sim): the sim ride
DESCRIPTORS_SIM = (SimRideDesc,)

# ... and its fifth (RPH_DESCRIPTORS_COST, rph_layout_fields_cost): the scans under
# transaction costs; the table also holds the rows of the embedded CostTerms,
# and has constants of its own (rph_layout_consts_cost, ops/layout_cost.py)
DESCRIPTORS_COST = (CostPnlDesc, CostOosDesc)

# ... and its sixth (RPH_DESCRIPTORS_JUMP, rph_layout_fields_jump): the Merton jump scans
DESCRIPTORS_JUMP = (JumpTerms,)

# upper-case ints of layout.py that the native table does not hold (Python only)
PYTHON_ONLY: tuple[str, ...] = ()


class _FieldRow(C.Structure):  # csrc/rph_layout.h FieldRow
    _fields_ = [("strct", C.c_char_p), ("field", C.c_char_p), ("offset", C.c_uint), ("size", C.c_uint)]


class _ConstRow(C.Structure):  # csrc/rph_layout.h ConstRow
    _fields_ = [("name", C.c_char_p), ("value", C.c_longlong)]


def native_layout(lib) -> tuple[list[tuple[str, str, int, int]], list[tuple[str, int]]]:
    """The library's tables: (struct, field, offset, size) of every descriptor
    field in declaration order, and (name, value) of every constant."""
    fr, cr = C.POINTER(_FieldRow)(), C.POINTER(_ConstRow)()
    nf, nc = lib.rph_layout_fields(C.byref(fr)), lib.rph_layout_consts(C.byref(cr))
    return ([(r.strct.decode(), r.field.decode(), r.offset, r.size) for r in fr[:nf]],
            [(r.name.decode(), r.value) for r in cr[:nc]])


def native_layout_ext(lib) -> list[tuple[str, str, int, int]]:
    """The library's second field table: the rows of :data:`DESCRIPTORS_EXT`."""
    fr = C.POINTER(_FieldRow)()
    nf = lib.rph_layout_fields_ext(C.byref(fr))
    return [(r.strct.decode(), r.field.decode(), r.offset, r.size) for r in fr[:nf]]


def native_layout_ride(lib) -> list[tuple[str, str, int, int]]:
    """The library's third field table: the rows of :data:`DESCRIPTORS_RIDE`."""
    fr = C.POINTER(_FieldRow)()
    nf = lib.rph_layout_fields_ride(C.byref(fr))
    return [(r.strct.decode(), r.field.decode(), r.offset, r.size) for r in fr[:nf]]


def native_layout_sim(lib) -> list[tuple[str, str, int, int]]:
    """The library's fourth field table: the rows of :data:`DESCRIPTORS_SIM`."""
    fr = C.POINTER(_FieldRow)()
    nf = lib.rph_layout_fields_sim(C.byref(fr))
    return [(r.strct.decode(), r.field.decode(), r.offset, r.size) for r in fr[:nf]]


def native_layout_jump(lib) -> list[tuple[str, str, int, int]]:
    """The library's sixth field table: the rows of :data:`DESCRIPTORS_JUMP`."""
    fr = C.POINTER(_FieldRow)()
    nf = lib.rph_layout_fields_jump(C.byref(fr))
    return [(r.strct.decode(), r.field.decode(), r.offset, r.size) for r in fr[:nf]]


def native_layout_cost(lib) -> tuple[list[tuple[str, str, int, int]], list[tuple[str, int]]]:
    """The library's fifth field table, the rows of :data:`DESCRIPTORS_COST` and
    of ``CostTerms``, and the constants of ``ops/layout_cost.py``."""
    fr, cr = C.POINTER(_FieldRow)(), C.POINTER(_ConstRow)()
    nf, nc = lib.rph_layout_fields_cost(C.byref(fr)), lib.rph_layout_consts_cost(C.byref(cr))
    return ([(r.strct.decode(), r.field.decode(), r.offset, r.size) for r in fr[:nf]],
            [(r.name.decode(), r.value) for r in cr[:nc]])


def layout_mismatches(fields, consts, classes=DESCRIPTORS, layout=L) -> list[str]:
    """Every difference between the native tables (:func:`native_layout`) and
    the Python mirrors: the ctypes ``classes`` field by field (offset and size
    by name, which fixes the order too) and their sizes, and the constants of
    ``layout``, both ways."""
    bad = []
    for cls in classes:
        s = cls.__name__
        nat = {f: (o, z) for t, f, o, z in fields if t == s}
        py = {f[0]: (getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_}
        say = lambda v, side: f"{side} offset {v[0]} size {v[1]}" if v else f"not in {side}"  # noqa: E731
        bad += [f"{s}.{f}: {say(nat.get(f), 'native')}, {say(py.get(f), 'ctypes')}"
                for f in dict(nat, **py) if nat.get(f) != py.get(f)]
        size = max((o + z for o, z in nat.values()), default=0)  # (the native list is gapless: static_assert)
        if size != C.sizeof(cls):
            bad.append(f"{s}: native size {size}, ctypes size {C.sizeof(cls)}")
    nat = dict(consts)
    py = {k: v for k, v in vars(layout).items() if k.isupper() and type(v) is int}
    bad += [f"layout.{k}: native {v}, python {py.get(k, 'has none')}" for k, v in nat.items() if py.get(k) != v]
    bad += [f"layout.{k}: python {v}, not in the native table" for k, v in py.items()
            if k not in nat and k not in PYTHON_ONLY]
    return bad


def _bind(lib):
    sig = {
        "rph_last_error": (C.c_char_p, []),
        "rph_layout_fields": (C.c_int, [C.POINTER(C.POINTER(_FieldRow))]),
        "rph_layout_consts": (C.c_int, [C.POINTER(C.POINTER(_ConstRow))]),
        "rph_layout_fields_ext": (C.c_int, [C.POINTER(C.POINTER(_FieldRow))]),
        "rph_layout_fields_ride": (C.c_int, [C.POINTER(C.POINTER(_FieldRow))]),
        "rph_layout_fields_sim": (C.c_int, [C.POINTER(C.POINTER(_FieldRow))]),
        "rph_layout_fields_cost": (C.c_int, [C.POINTER(C.POINTER(_FieldRow))]),
        "rph_layout_consts_cost": (C.c_int, [C.POINTER(C.POINTER(_ConstRow))]),
        "rph_layout_fields_jump": (C.c_int, [C.POINTER(C.POINTER(_FieldRow))]),
        "rph_simulate_jump": (C.c_int, [C.POINTER(SimDesc), C.POINTER(JumpTerms), VP]),
        "rph_simulate_jump_check": (C.c_int, [C.POINTER(SimDesc), C.POINTER(JumpTerms)]),
        "rph_oos_jump": (C.c_int, [C.POINTER(OosDesc), C.POINTER(JumpTerms), VP]),
        "rph_oos_jump_check": (C.c_int, [C.POINTER(OosDesc), C.POINTER(JumpTerms)]),
        "rph_oos_jump_cost": (C.c_int, [C.POINTER(CostOosDesc), C.POINTER(JumpTerms), VP]),
        "rph_oos_jump_cost_check": (C.c_int, [C.POINTER(CostOosDesc), C.POINTER(JumpTerms)]),
        "rph_pnl_cost": (C.c_int, [C.POINTER(CostPnlDesc), VP]),
        "rph_pnl_cost_check": (C.c_int, [C.POINTER(CostPnlDesc)]),
        "rph_oos_cost": (C.c_int, [C.POINTER(CostOosDesc), VP]),
        "rph_oos_cost_check": (C.c_int, [C.POINTER(CostOosDesc)]),
        "rph_sim_ride_slice": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2),
        "rph_sim_ride_head": (C.c_int, [C.POINTER(SimRideDesc), C.POINTER(SimDesc), VP]),
        "rph_sim_ride_rest": (C.c_int, [C.POINTER(SimRideDesc), C.c_int, VP]),
        "rph_lm_has_sim": (C.c_int, [C.c_int] * 6),
        "rph_lm_solve_sim": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, C.c_int, C.POINTER(SimRideDesc),
                                       C.c_int, C.c_int, VP]),
        "rph_lm_fit_sim": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, C.POINTER(SimRideDesc), C.c_int, VP]),
        "rph_oos": (C.c_int, [C.POINTER(OosDesc), VP]),
        "rph_oos_check": (C.c_int, [C.POINTER(OosDesc)]),
        "rph_oos_max_wgs": (C.c_int, [C.POINTER(C.c_int)]),
        "rph_device_info": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong),
                                      C.c_char_p, C.c_int]),
        "rph_memset_async": (C.c_int, [VP, C.c_int, C.c_longlong, VP]),
        "rph_stream_sync": (C.c_int, [VP]),
        "rph_graph_begin": (C.c_int, [VP]),
        "rph_graph_end": (C.c_int, [VP, C.POINTER(VP), C.POINTER(C.c_longlong)]),
        "rph_graph_launch": (C.c_int, [VP, VP]),
        "rph_graph_destroy": (C.c_int, [VP]),
        "rph_nccl_unique_id": (C.c_int, [C.c_char_p]),
        "rph_nccl_init": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(VP)]),
        "rph_nccl_allreduce_f32": (C.c_int, [VP, VP, C.c_longlong, VP]),
        "rph_nccl_allreduce_f64": (C.c_int, [VP, VP, C.c_longlong, VP]),
        "rph_nccl_allreduce_u32": (C.c_int, [VP, VP, C.c_longlong, VP]),
        "rph_nccl_destroy": (C.c_int, [VP]),
        "rph_net_nparams": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "rph_train_step": (C.c_int, [C.POINTER(TrainDesc), C.c_int, C.c_int, VP]),
        "rph_train_update": (C.c_int, [C.POINTER(TrainDesc), C.c_int, C.c_int, VP]),
        "rph_train_fit": (C.c_int, [C.POINTER(TrainDesc), C.c_int, VP]),
        "rph_train_lag_step": (C.c_int, [C.POINTER(TrainDesc), C.c_int, C.c_int, VP]),
        "rph_train_lag_finalize": (C.c_int, [C.POINTER(TrainDesc), C.c_int, VP]),
        "rph_train_lag_fit": (C.c_int, [C.POINTER(TrainDesc), C.c_int, VP]),
        "rph_train_ticket_fit": (C.c_int, [C.POINTER(TrainDesc), C.c_int, VP]),
        "rph_eval": (C.c_int, [C.POINTER(EvalDesc), VP]),
        "rph_pnl": (C.c_int, [C.POINTER(PnlDesc), VP]),
        "rph_pnl_finish": (C.c_int, [C.POINTER(PnlFinishDesc), VP]),
        "rph_lm_shape": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)] * 3),
        "rph_lm_pass_wps": (C.c_int, [C.c_int] * 4),
        "rph_lm_eval": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, C.c_int, VP]),
        "rph_lm_solve": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, C.c_int, VP]),
        "rph_lm_fit": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, VP]),
        "rph_lm_fit_ride": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, C.POINTER(SelfTargetDesc),
                                      C.POINTER(EvalDesc), C.c_int, VP]),
        "rph_lm_eval_st": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), C.POINTER(SelfTargetDesc), VP, C.c_int,
                                     VP]),
        "rph_lm_solve_eval": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, C.c_int, C.POINTER(EvalDesc),
                                        C.c_int, VP]),
        "rph_lm_has_st": (C.c_int, [C.c_int] * 4),
        "rph_lm_solve_lds": (C.c_int, [C.c_int] * 4),
        "rph_lm_dp_exchange": (C.c_int, [C.POINTER(LmDpDesc), VP, C.c_int, C.c_int, VP]),
        "rph_lm_select": (C.c_int, [C.POINTER(TrainDesc), C.POINTER(LmDesc), VP, VP, C.c_int, C.c_int, C.c_int,
                                    C.c_int, VP]),
        "rph_sobol_normal": (C.c_int, [VP, C.c_int, C.c_int, VP, VP, C.c_longlong, C.c_int, C.c_int, VP]),
        "rph_sobol_normal_check": (C.c_int, [C.c_int, C.c_longlong]),
        "rph_simulate": (C.c_int, [C.POINTER(SimDesc), VP]),
        "rph_simulate_check": (C.c_int, [C.POINTER(SimDesc)]),
        "rph_simulate_pair": (C.c_int, [C.POINTER(SimDesc), C.POINTER(SimDesc), C.POINTER(C.c_int), VP]),
        "rph_payoff": (C.c_int, [C.c_int, C.c_int, C.c_int, VP, VP, C.c_float, VP, VP, VP, VP]),
        "rph_radix_hist": (C.c_int, [VP, C.c_longlong, C.c_uint32, C.c_uint32, C.c_int, C.c_int, VP, VP]),
        "rph_ipc_alloc": (C.c_int, [C.c_longlong, C.POINTER(VP), C.c_char_p]),
        "rph_ipc_open": (C.c_int, [C.c_char_p, C.POINTER(VP)]),
        "rph_ipc_close": (C.c_int, [VP]),
        "rph_free": (C.c_int, [VP]),
        "rph_ipc_handle_size": (C.c_int, []),
        "rph_ipc_is_finegrained": (C.c_int, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def load(required: bool | None = None):
    """Load (building if needed) the native library.  ``required`` defaults to
    True whenever a GPU is visible."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if required is None:
        required = torch.cuda.is_available()
    try:
        if _LIB_ENV.endswith(".so") and not _LIB_PATH.exists():
            raise FileNotFoundError(f"RPH_NATIVE_LIB={_LIB_ENV} does not exist (it is never built implicitly)")
        if not _LIB_PATH.exists() or os.environ.get("RPH_REBUILD"):
            from .. import build as _build

            v = os.environ.get("RPH_NATIVE_LIB", "")
            _build.build(debug=v == "debug", asan=v == "asan")
        lib = C.CDLL(str(_LIB_PATH), mode=C.RTLD_GLOBAL)
        _bind(lib)
        fields, consts = native_layout(lib)
        bad = layout_mismatches(fields + native_layout_ext(lib) + native_layout_ride(lib) + native_layout_sim(lib)
                                + native_layout_jump(lib), consts,
                                classes=DESCRIPTORS + DESCRIPTORS_EXT + DESCRIPTORS_RIDE + DESCRIPTORS_SIM + DESCRIPTORS_JUMP)
        cfields, cconsts = native_layout_cost(lib)
        bad += layout_mismatches(cfields, cconsts, classes=(CostTerms,) + DESCRIPTORS_COST, layout=LC)
        if bad:
            raise RuntimeError("native/Python layout mismatch:\n  " + "\n  ".join(bad))
        _lib = lib
        return lib
    except Exception as e:  # pragma: no cover - exercised on broken installs only
        _load_error = f"{type(e).__name__}: {e}"
        if required:
            raise RuntimeError(f"rphedge native library unavailable on a GPU machine: {_load_error}") from e
        return None


def available() -> bool:
    return load(required=False) is not None


def _check(rc: int, what: str):
    if rc != 0:
        msg = _lib.rph_last_error().decode() if _lib is not None else ""
        raise RuntimeError(f"{what} failed with code {rc}: {msg}")


def ptr(t) -> int | None:
    if t is None:
        return None
    return t.data_ptr()


def fill_ptrs(arr, tensors):
    """Fill a ``VP * N`` descriptor array from a sequence of tensors (None: a null pointer)."""
    for i, t in enumerate(tensors):
        arr[i] = ptr(t)


def stream_handle(stream=None) -> int:
    """HIP stream handle of a torch stream (None: the current stream; an int is
    taken as a raw handle, 0 = the null stream)."""
    if isinstance(stream, int):
        return stream
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


# ---------------------------------------------------------------------------
# thin wrappers
# ---------------------------------------------------------------------------
def net_nparams(nin: int, h: int, nout: int, head: int) -> tuple[int, int]:
    lib = load(required=True)
    p, r = C.c_int(), C.c_int()
    if lib.rph_net_nparams(nin, h, nout, head, C.byref(p), C.byref(r)) != 0:
        raise ValueError(f"unsupported hedge network shape nin={nin} h={h} nout={nout} head={head}")
    return p.value, r.value


def sobol_normal(out: torch.Tensor, table, offset: int = 0, raw: bool = False, stream=None):
    lib = load(required=True)
    sv, sh, dims = table
    n, d = out.shape
    assert d <= dims
    fp64 = 1 if out.dtype == torch.float64 else 0
    _check(lib.rph_sobol_normal(ptr(out), n, d, ptr(sv), ptr(sh), int(offset), fp64, int(raw),
                                stream_handle(stream)), "rph_sobol_normal")


def simulate(desc: SimDesc, stream=None):
    lib = load(required=True)
    _check(lib.rph_simulate(C.byref(desc), stream_handle(stream)), "rph_simulate")


def simulate_check(desc: SimDesc):
    """The descriptor checks of :func:`simulate` alone: raises as it would, launches nothing."""
    lib = load(required=True)
    _check(lib.rph_simulate_check(C.byref(desc)), "rph_simulate")


def simulate_jump(desc: SimDesc, jump: JumpTerms, stream=None):
    """The Merton jump-diffusion scan (k_sim_jump): ``desc.model`` SIM_MERTON, ``jump`` its jump terms."""
    lib = load(required=True)
    _check(lib.rph_simulate_jump(C.byref(desc), C.byref(jump) if jump is not None else None, stream_handle(stream)),
           "rph_simulate_jump")


def simulate_jump_check(desc: SimDesc, jump: JumpTerms):
    """The descriptor checks of :func:`simulate_jump` alone: raises as it would, launches nothing."""
    lib = load(required=True)
    _check(lib.rph_simulate_jump_check(C.byref(desc), C.byref(jump) if jump is not None else None),
           "rph_simulate_jump")


def sobol_normal_check(n: int, offset: int = 0):
    """The range check of :func:`sobol_normal` alone: raises as it would, launches nothing."""
    lib = load(required=True)
    _check(lib.rph_sobol_normal_check(int(n), int(offset)), "rph_sobol_normal")


def simulate_pair(a: SimDesc, b: SimDesc, stream=None) -> bool:
    """Scans ``a`` and ``b`` in one launch (k_sim_scan_pair) when both select
    the same scan instantiation, else in two; returns whether it was one."""
    lib = load(required=True)
    merged = C.c_int(0)
    _check(lib.rph_simulate_pair(C.byref(a), C.byref(b), C.byref(merged), stream_handle(stream)), "rph_simulate_pair")
    return bool(merged.value)


def sim_ride_slice(b0: int, b1: int, riders: int, per_rider: int, k: int) -> tuple[int, int]:
    """Slice ``k`` of a sim ride's schedule (csrc/sim_scan.h sim_ride_slice): the
    ``(start, count)`` of the blocks of ``[b0, b1)`` that solve launch ``k``
    carries; rider ``r`` scans ``start + r + j * riders``, ``j < per_rider``."""
    lib = load(required=True)
    start, count = C.c_int(0), C.c_int(0)
    lib.rph_sim_ride_slice(int(b0), int(b1), int(riders), int(per_rider), int(k), C.byref(start), C.byref(count))
    return start.value, count.value


def sim_ride_head(r: SimRideDesc, g: SimDesc | None, stream=None):
    """Blocks ``[0, b0)`` of the ride's scan with their payoff and the whole scan ``g`` beside them: one launch."""
    lib = load(required=True)
    _check(lib.rph_sim_ride_head(C.byref(r), C.byref(g) if g is not None else None, stream_handle(stream)),
           "rph_sim_ride_head")


def sim_ride_rest(r: SimRideDesc, start: int | None = None, stream=None):
    """Blocks ``[start, b1)`` (default: from ``b0``) of the ride's scan with their payoff, one plain launch."""
    lib = load(required=True)
    _check(lib.rph_sim_ride_rest(C.byref(r), int(r.b0 if start is None else start), stream_handle(stream)),
           "rph_sim_ride_rest")


def lm_has_sim(nin: int, h: int, nout: int, head: int, model: int, path_stat: int) -> bool:
    """Whether the shape's solve launch has a rider for the scan (csrc/hedge_lm.hip sim_rider_for)."""
    return bool(load(required=True).rph_lm_has_sim(nin, h, nout, head, int(model), int(path_stat)))


def lm_solve_sim(desc: TrainDesc, lm: LmDesc, red_new: torch.Tensor, pass_: int, r: SimRideDesc, riders: int, k: int,
                 stream=None):
    """The solve of ``pass_`` of an exploration with slice ``k`` of the sim ride on ``riders`` riders (k_lm_solve_sim)."""
    _check(_lib.rph_lm_solve_sim(C.byref(desc), C.byref(lm), ptr(red_new), int(pass_), C.byref(r), int(riders), int(k),
                                 stream_handle(stream)), "rph_lm_solve_sim")


def lm_fit_sim(desc: TrainDesc, lm: LmDesc, red_new: torch.Tensor, r: SimRideDesc, riders: int, stream=None):
    """:func:`lm_fit` of an exploration whose solves carry the sim ride ``r``;
    every block of the ride has been enqueued when it returns."""
    load(required=True)
    _check(_lib.rph_lm_fit_sim(C.byref(desc), C.byref(lm), ptr(red_new), C.byref(r), int(riders),
                               stream_handle(stream)), "rph_lm_fit_sim")


def train_step(desc: TrainDesc, step: int, epoch: int, stream=None):
    _check(_lib.rph_train_step(C.byref(desc), int(step), int(epoch), stream_handle(stream)), "rph_train_step")


def train_fit(desc: TrainDesc, epochs: int, stream=None):
    """One persistent launch for a whole fit (csrc/hedge_fit.h); desc.counter
    (>= 2 u32) and desc.acc (3 x 8 x R floats) must be zeroed before it."""
    _check(_lib.rph_train_fit(C.byref(desc), int(epochs), stream_handle(stream)), "rph_train_fit")


def train_lag_step(desc: TrainDesc, k: int, epoch: int, stream=None):
    """Lagged-update step kernel k of a fit (csrc/hedge_lag.h)."""
    _check(_lib.rph_train_lag_step(C.byref(desc), int(k), int(epoch), stream_handle(stream)), "rph_train_lag_step")


def train_lag_fit(desc: TrainDesc, epochs: int, stream=None):
    """All steps + finalize of a lagged-schedule fit, launched from C++."""
    load(required=True)
    _check(_lib.rph_train_lag_fit(C.byref(desc), int(epochs), stream_handle(stream)), "rph_train_lag_fit")


def train_ticket_fit(desc: TrainDesc, epochs: int, stream=None):
    """All steps of a ticketed fit (fused update), launched from C++."""
    load(required=True)
    _check(_lib.rph_train_ticket_fit(C.byref(desc), int(epochs), stream_handle(stream)), "rph_train_ticket_fit")


def train_lag_finalize(desc: TrainDesc, K: int, stream=None):
    _check(_lib.rph_train_lag_finalize(C.byref(desc), int(K), stream_handle(stream)), "rph_train_lag_finalize")


def train_update(desc: TrainDesc, step: int, epoch: int, stream=None):
    _check(_lib.rph_train_update(C.byref(desc), int(step), int(epoch), stream_handle(stream)), "rph_train_update")


def eval_(desc: EvalDesc, stream=None):
    _check(_lib.rph_eval(C.byref(desc), stream_handle(stream)), "rph_eval")


def lm_shape(nin: int, h: int, nout: int, head: int):
    """(P, R, Gram blocks) of the LM kernels, or None."""
    lib = load(required=True)
    v = [C.c_int() for _ in range(3)]
    if lib.rph_lm_shape(nin, h, nout, head, *[C.byref(x) for x in v]) != 0:
        return None
    return tuple(int(x.value) for x in v)


def lm_pass_wps(nin: int, h: int, nout: int, head: int) -> int:
    """Pass workgroups per CU of the shape's plain LM pass body (1 or 2;
    csrc/hedge_narrow.h NarrowPairBody::WAVES_PER_SIMD)."""
    return int(load(required=True).rph_lm_pass_wps(nin, h, nout, head))


def lm_eval(desc: TrainDesc, lm: LmDesc, red_new: torch.Tensor, pass_: int, stream=None, st=None):
    """One pass + reduce; ``st`` (:class:`SelfTargetDesc`): pass 0 evaluates its own target."""
    if st is not None:
        _check(_lib.rph_lm_eval_st(C.byref(desc), C.byref(lm), C.byref(st), ptr(red_new), int(pass_),
                                   stream_handle(stream)), "rph_lm_eval_st")
        return
    _check(_lib.rph_lm_eval(C.byref(desc), C.byref(lm), ptr(red_new), int(pass_), stream_handle(stream)),
           "rph_lm_eval")


def lm_solve(desc: TrainDesc, lm: LmDesc, red_new: torch.Tensor, pass_: int, stream=None):
    _check(_lib.rph_lm_solve(C.byref(desc), C.byref(lm), ptr(red_new), int(pass_), stream_handle(stream)),
           "rph_lm_solve")


def lm_fit(desc: TrainDesc, lm: LmDesc, red_new: torch.Tensor, stream=None):
    """Whole single-rank Levenberg-Marquardt fit (csrc/hedge_lm.hip), launched from C++."""
    load(required=True)
    _check(_lib.rph_lm_fit(C.byref(desc), C.byref(lm), ptr(red_new), stream_handle(stream)), "rph_lm_fit")


def lm_has_st(nin: int, h: int, nout: int, head: int) -> bool:
    """Whether the shape has a self-target pass body (``SelfTargetDesc``; csrc/hedge_lm.hip LmKernels::HAS_ST)."""
    return bool(load(required=True).rph_lm_has_st(nin, h, nout, head))


def lm_solve_lds(nin: int, h: int, nout: int, head: int) -> int:
    """Dynamic LDS bytes of the shape's LM solve launch (0: no LM solver)."""
    return int(load(required=True).rph_lm_solve_lds(nin, h, nout, head))


def lm_solve_eval(desc: TrainDesc, lm: LmDesc, red_new: torch.Tensor, pass_: int, ev: EvalDesc, riders: int,
                  stream=None):
    """The solve of ``pass_`` with the eval ``ev`` riding on ``riders`` extra workgroups (k_lm_solve_eval)."""
    _check(_lib.rph_lm_solve_eval(C.byref(desc), C.byref(lm), ptr(red_new), int(pass_), C.byref(ev), int(riders),
                                  stream_handle(stream)), "rph_lm_solve_eval")


def lm_fit_ride(desc: TrainDesc, lm: LmDesc, red_new: torch.Tensor, st: SelfTargetDesc, ev: EvalDesc, riders: int,
                stream=None):
    """:func:`lm_fit` with pass 0 evaluating its own target (``st``) and the
    eval ``ev`` riding in the launch of the first solve."""
    load(required=True)
    _check(_lib.rph_lm_fit_ride(C.byref(desc), C.byref(lm), ptr(red_new), C.byref(st), C.byref(ev), int(riders),
                                stream_handle(stream)), "rph_lm_fit_ride")


def lm_select(desc: TrainDesc, lm: LmDesc, sel: torch.Tensor, main_state: torch.Tensor, world: int, rank: int,
              p: int, phase: int, stream=None):
    """Multi-start selection (k_lm_select): phase 0 packs this rank's exploration
    results into ``sel``, phase 1 picks the best candidate into the NetWeights
    and ``main_state``'s damping."""
    _check(_lib.rph_lm_select(C.byref(desc), C.byref(lm), ptr(sel), ptr(main_state), int(world), int(rank), int(p),
                              int(phase), stream_handle(stream)), "rph_lm_select")


def lm_dp_exchange(x: LmDpDesc, red: torch.Tensor, ng: int, p: int, stream=None):
    """All-reduce of the LM reduced block over the IPC mailboxes (k_lm_dp_exchange)."""
    load(required=True)
    _check(_lib.rph_lm_dp_exchange(C.byref(x), ptr(red), int(ng), int(p), stream_handle(stream)),
           "rph_lm_dp_exchange")


def pnl(desc: PnlDesc, stream=None):
    """Self-financing hedge P&L scan over the rebalancing dates (k_hedge_pnl)."""
    load(required=True)
    _check(_lib.rph_pnl(C.byref(desc), stream_handle(stream)), "rph_pnl")


def pnl_cost(desc: CostPnlDesc, stream=None):
    """The P&L scan under transaction costs and a no-trade band (k_hedge_pnl_cost)."""
    load(required=True)
    _check(_lib.rph_pnl_cost(C.byref(desc), stream_handle(stream)), "rph_pnl_cost")


def pnl_cost_check(desc: CostPnlDesc):
    """The descriptor checks of :func:`pnl_cost` alone: raises as it would, launches nothing."""
    lib = load(required=True)
    _check(lib.rph_pnl_cost_check(C.byref(desc)), "rph_pnl_cost")


def oos_cost(desc: CostOosDesc, stream=None):
    """Fused simulate-and-hedge of fresh paths under transaction costs (k_hedge_oos_cost)."""
    load(required=True)
    _check(_lib.rph_oos_cost(C.byref(desc), stream_handle(stream)), "rph_oos_cost")


def oos_cost_check(desc: CostOosDesc):
    """The descriptor checks of :func:`oos_cost` alone: raises as it would, launches nothing."""
    lib = load(required=True)
    _check(lib.rph_oos_cost_check(C.byref(desc)), "rph_oos_cost")


def oos(desc: OosDesc, stream=None):
    """Fused simulate-and-hedge of fresh paths (k_hedge_oos)."""
    load(required=True)
    _check(_lib.rph_oos(C.byref(desc), stream_handle(stream)), "rph_oos")


def oos_check(desc: OosDesc):
    """The descriptor checks of :func:`oos` alone: raises as it would, launches nothing."""
    lib = load(required=True)
    _check(lib.rph_oos_check(C.byref(desc)), "rph_oos")


def oos_jump(desc: OosDesc, jump: JumpTerms, stream=None):
    """Fused simulate-and-hedge on Merton jump-diffusion paths (k_hedge_oos_jump)."""
    load(required=True)
    _check(_lib.rph_oos_jump(C.byref(desc), C.byref(jump), stream_handle(stream)), "rph_oos_jump")


def oos_jump_check(desc: OosDesc, jump: JumpTerms):
    """The descriptor checks of :func:`oos_jump` alone: raises as it would, launches nothing."""
    lib = load(required=True)
    _check(lib.rph_oos_jump_check(C.byref(desc), C.byref(jump)), "rph_oos_jump")


def oos_jump_cost(desc: CostOosDesc, jump: JumpTerms, stream=None):
    """... under transaction costs (k_hedge_oos_jump_cost)."""
    load(required=True)
    _check(_lib.rph_oos_jump_cost(C.byref(desc), C.byref(jump), stream_handle(stream)), "rph_oos_jump_cost")


def oos_max_wgs() -> int:
    """Workgroups a k_hedge_oos launch may use on the current device (OOS_WGS_PER_CU per CU)."""
    lib = load(required=True)
    v = C.c_int()
    _check(lib.rph_oos_max_wgs(C.byref(v)), "rph_oos_max_wgs")
    return int(v.value)


def pnl_finish(desc: PnlFinishDesc, stream=None):
    """Finish of the P&L folded into the evals (k_pnl_finish)."""
    load(required=True)
    _check(_lib.rph_pnl_finish(C.byref(desc), stream_handle(stream)), "rph_pnl_finish")


def payoff(kind: int, s: torch.Tensor, out: torch.Tensor, strike: float, nfrac=None, wts=None, na: int = 1,
           stream=None, x=None):
    """K7; ``x``: the per-path floating strike of kinds 4 / 5 (max(s - x, 0) / max(x - s, 0))."""
    lib = load(required=True)
    n = out.numel()
    _check(lib.rph_payoff(kind, n, na, ptr(s), ptr(nfrac), float(strike), ptr(wts), ptr(x), ptr(out),
                          stream_handle(stream)), "rph_payoff")


def radix_hist(x: torch.Tensor, pmask: int, prefix: int, shift: int, nbins: int, hist: torch.Tensor, stream=None):
    lib = load(required=True)
    _check(lib.rph_radix_hist(ptr(x), x.numel(), pmask & 0xFFFFFFFF, prefix & 0xFFFFFFFF, shift, nbins, ptr(hist),
                              stream_handle(stream)), "rph_radix_hist")


def memset_async(t: torch.Tensor, value: int = 0, stream=None):
    lib = load(required=True)
    _check(lib.rph_memset_async(ptr(t), value, t.numel() * t.element_size(), stream_handle(stream)),
           "rph_memset_async")


def device_info(dev: int = 0) -> dict:
    lib = load(required=True)
    cus, lds = C.c_int(), C.c_int()
    hbm = C.c_longlong()
    name = C.create_string_buffer(128)
    _check(lib.rph_device_info(dev, C.byref(cus), C.byref(lds), C.byref(hbm), name, 128), "rph_device_info")
    return {"cus": cus.value, "lds_per_cu": lds.value, "hbm_bytes": hbm.value, "arch": name.value.decode()}


class Graph:
    """hipGraph captured from a stream with the native runtime."""

    def __init__(self):
        self.exec = None
        self.num_nodes = 0

    def capture_begin(self, stream=None):
        lib = load(required=True)
        self._stream = stream_handle(stream)
        _check(lib.rph_graph_begin(self._stream), "rph_graph_begin")

    def capture_end(self):
        ex = VP()
        nn = C.c_longlong()
        _check(_lib.rph_graph_end(self._stream, C.byref(ex), C.byref(nn)), "rph_graph_end")
        self.exec = ex.value
        self.num_nodes = nn.value

    def replay(self, stream=None):
        _check(_lib.rph_graph_launch(self.exec, stream_handle(stream)), "rph_graph_launch")

    def __del__(self):
        if self.exec is not None and _lib is not None:
            try:
                _lib.rph_graph_destroy(self.exec)
            except Exception:
                pass
            self.exec = None


class NcclComm:
    """RCCL communicator owned by the native runtime (one per process/GPU).

    The 128-byte unique id is created on rank 0 and broadcast via the
    torch.distributed store, then every rank calls ``ncclCommInitRank``.
    """

    def __init__(self, rank: int, world: int, store, tag: str = "rph_nccl"):
        lib = load(required=True)
        key = f"{tag}_uid"
        if rank == 0:
            buf = C.create_string_buffer(128)
            n = lib.rph_nccl_unique_id(buf)
            if n <= 0:
                _check(-1, "rph_nccl_unique_id")
            store.set(key, bytes(buf.raw[:128]))
        uid = store.get(key)
        comm = VP()
        _check(lib.rph_nccl_init(uid, world, rank, C.byref(comm)), "rph_nccl_init")
        self.comm = comm.value
        self.rank, self.world = rank, world

    def allreduce_(self, t: torch.Tensor, stream=None):
        fn = {torch.float32: _lib.rph_nccl_allreduce_f32, torch.float64: _lib.rph_nccl_allreduce_f64,
              torch.int32: _lib.rph_nccl_allreduce_u32}[t.dtype]
        _check(fn(self.comm, ptr(t), t.numel(), stream_handle(stream)), "rph_nccl_allreduce")

    def close(self):
        if self.comm is not None:
            _lib.rph_nccl_destroy(self.comm)
            self.comm = None


class IpcMailbox:
    """Peer-mapped mailboxes for the fused xGMI gradient all-reduce.

    Every rank allocates ``[DP_SLOTS][W][R]`` 8-byte entries (a float + flag
    pair per entry for the ticket path; a data-tagged {value, seq} granule for
    the lagged path) + ``[DP_SLOTS][W]`` flags,
    exports an IPC handle through the torch.distributed store and opens every
    peer's handle.  The step kernel's last-arriving workgroup then writes its
    packet straight into each peer's HBM over xGMI (no RCCL launch, no extra
    kernel per step)."""

    def __init__(self, rank: int, world: int, R: int, store, device, tag: str = "rph_mbox"):
        lib = load(required=True)
        if world > 8:
            raise ValueError("fused xGMI all-reduce supports up to 8 ranks (one node)")
        self.rank, self.world, self.R = rank, world, R
        data_bytes = DP_SLOTS * world * R * 8
        self.flag_off = (data_bytes + 255) // 256 * 256
        nbytes = self.flag_off + DP_SLOTS * world * 4 + 256
        hs = lib.rph_ipc_handle_size()
        buf = C.create_string_buffer(hs)
        p = VP()
        _check(lib.rph_ipc_alloc(nbytes, C.byref(p), buf), "rph_ipc_alloc")
        self.own = p.value
        self.finegrained = lib.rph_ipc_is_finegrained() == 1  # coherent-by-memory-type mailbox
        store.set(f"{tag}_{rank}", bytes(buf.raw[:hs]))
        self.ptrs, self.opened = [], []
        for q in range(world):
            if q == rank:
                self.ptrs.append(self.own)
                continue
            h = store.get(f"{tag}_{q}")
            pq = VP()
            _check(lib.rph_ipc_open(h, C.byref(pq)), "rph_ipc_open")
            self.ptrs.append(pq.value)
            self.opened.append(pq.value)
        self.counter = torch.zeros(4, dtype=torch.int32, device=device)
        self.error = torch.zeros(4, dtype=torch.int32, device=device)

    def fill(self, d: TrainDesc):
        d.dp_world, d.dp_rank = self.world, self.rank
        for q in range(self.world):
            d.dp_mbox[q] = self.ptrs[q]
            d.dp_flags[q] = self.ptrs[q] + self.flag_off
        d.dp_counter = self.counter.data_ptr()
        d.dp_error = self.error.data_ptr()

    def lm_desc(self) -> "LmDpDesc":
        """Descriptor of this mailbox for the LM block exchange (k_lm_dp_exchange,
        and the exchange fused into k_lm_reduce; allocated with R >= LM_DP_PITCH
        entries per row)."""
        x = LmDpDesc()
        for q in range(self.world):
            x.mbox[q] = self.ptrs[q]
        x.counter, x.error = self.counter.data_ptr(), self.error.data_ptr()
        x.world, x.rank, x.pitch = self.world, self.rank, self.R
        return x

    def check(self):
        if int(self.error[0].item()) != 0:
            raise RuntimeError("fused xGMI all-reduce: a peer rank did not arrive (timeout)")

    def close(self):
        for p in self.opened:
            _lib.rph_ipc_close(p)
        self.opened = []
        if self.own is not None:
            _lib.rph_free(self.own)
            self.own = None
