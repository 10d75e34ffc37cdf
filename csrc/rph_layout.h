// rphedge — the labelled layout tables the Python mirrors are compared with at
// load time (rphedge/ops/native.py layout_mismatches): every field of every
// launch descriptor, and every constant of rph_types.h that rphedge/ops/layout.py
// repeats.  Host only (runtime.cpp).
//
// Adding a descriptor field: the struct (rph_types.h), its list here, the
// ctypes mirror (native.py).  A field missing here does not compile, one
// missing or different in the mirror does not load.
#pragma once
#include <stddef.h>

#include "rph_types.h"

namespace rph {

// Field names in declaration order; offsets and sizes are taken from the struct.
#define RPH_FIELDS_TrainDesc(X, T)                                                                                  \
  X(T, feat) X(T, price) X(T, target) X(T, wts) X(T, opt) X(T, fit) X(T, lr_sched) X(T, slab) X(T, counter)          \
  X(T, grad_out) X(T, bond) X(T, alpha) X(T, quantile) X(T, inv_batch) X(T, loss) X(T, n_local) X(T, batch)         \
  X(T, steps_per_epoch) X(T, chunk_log2) X(T, shuffle) X(T, seed) X(T, fused_update) X(T, num_wgs) X(T, nin)        \
  X(T, h) X(T, nout) X(T, head) X(T, pad_acc) X(T, acc) X(T, deterministic) X(T, pad_stamps) X(T, stamps)           \
  X(T, dp_world) X(T, dp_rank) X(T, dp_mbox) X(T, dp_flags) X(T, dp_counter) X(T, dp_error) X(T, mfma_fp32)         \
  X(T, pad_lag) X(T, lag) X(T, variant) X(T, pad_fit_init) X(T, fit_init) X(T, fmu) X(T, fisd)
#define RPH_FIELDS_EvalDesc(X, T)                                                                                   \
  X(T, feat) X(T, price_t) X(T, price_t1) X(T, target) X(T, wa) X(T, wb) X(T, g_base) X(T, v_out) X(T, hold_out)    \
  X(T, resid_out) X(T, pred1_out) X(T, stats) X(T, bond_t) X(T, bond_t1) X(T, alpha) X(T, blend_c) X(T, hold_c)     \
  X(T, n_local) X(T, num_wgs) X(T, nin) X(T, h) X(T, nout) X(T, head) X(T, fmu) X(T, fisd) X(T, pad_snap)           \
  X(T, snap_a) X(T, snap_b) X(T, ex_kind) X(T, ex_strike) X(T, pnl_acc) X(T, pnl_grow) X(T, pnl_carry)              \
  X(T, pnl_first) X(T, pad_pnl)
#define RPH_FIELDS_PnlFinishDesc(X, T)                                                                              \
  X(T, acc) X(T, w0) X(T, payoff) X(T, pnl_out) X(T, stats) X(T, carry) X(T, n_local) X(T, num_wgs) X(T, nin)       \
  X(T, h) X(T, nout) X(T, head) X(T, pad0)
#define RPH_FIELDS_PnlDesc(X, T)                                                                                    \
  X(T, feat) X(T, feat_ts) X(T, price) X(T, price_ts) X(T, snap) X(T, fmu) X(T, fisd) X(T, bond) X(T, w0)           \
  X(T, payoff) X(T, pnl_out) X(T, stats) X(T, alpha) X(T, hold_c) X(T, wealth0) X(T, has_b) X(T, n_local)           \
  X(T, n_dates) X(T, num_wgs) X(T, nin) X(T, h) X(T, nout) X(T, head) X(T, ex_kind) X(T, ex_every) X(T, ex_strike)  \
  X(T, tau_out)
#define RPH_FIELDS_LmDpDesc(X, T) \
  X(T, mbox) X(T, counter) X(T, error) X(T, world) X(T, rank) X(T, pitch) X(T, fault)
#define RPH_FIELDS_LmDesc(X, T)                                                                                     \
  X(T, state) X(T, slab_b) X(T, slab_g) X(T, num_wgs) X(T, gram_wgs) X(T, red_wgs) X(T, passes) X(T, gram_blk)      \
  X(T, gram_blk_stride) X(T, inv_ns) X(T, inv_n) X(T, lam0) X(T, lam_up) X(T, lam_down) X(T, lam_min) X(T, lam_max) \
  X(T, ridge) X(T, bias_index) X(T, weights_only) X(T, damping) X(T, stop_min) X(T, stop_tol) X(T, gram_skip)       \
  X(T, inst) X(T, explore) X(T, lam_carry) X(T, diag_floor) X(T, w0) X(T, renorm) X(T, pad1) X(T, ren_mu)           \
  X(T, ren_isd) X(T, out_n) X(T, out_mu) X(T, out_gram) X(T, out_tr) X(T, slab_o) X(T, gfeat) X(T, gprice)          \
  X(T, gram_side) X(T, q_delta) X(T, q_kappa) X(T, pad_dp) X(T, dp) X(T, dp_fused) X(T, leaf_blocks) X(T, gtarget)  \
  X(T, gram_base) X(T, pad4)
#define RPH_FIELDS_SimDesc(X, T)                                                                                    \
  X(T, model) X(T, n_local) X(T, path_offset) X(T, n_fine) X(T, reduction) X(T, n_coarse) X(T, na) X(T, fp64)       \
  X(T, parity) X(T, sv1) X(T, shift1) X(T, dims1) X(T, pad_sv2) X(T, sv2) X(T, shift2) X(T, dims2) X(T, pad_s0)     \
  X(T, s0) X(T, mu) X(T, sigma) X(T, chol) X(T, dt) X(T, inv_norm) X(T, v0) X(T, a) X(T, b) X(T, c) X(T, kappa)     \
  X(T, theta) X(T, xi) X(T, rho) X(T, l0) X(T, lc) X(T, eta) X(T, n0) X(T, seed) X(T, out) X(T, out2) X(T, out3)    \
  X(T, final_out) X(T, final2_out) X(T, sv_tscale) X(T, scheme) X(T, path_stat) X(T, map_blk) X(T, map_stride)

#define RPH_FIELDS_OosDesc(X, T)                                                                                    \
  X(T, sim) X(T, snap) X(T, fmu) X(T, fisd) X(T, bond) X(T, pnl_out) X(T, payoff_out) X(T, stats) X(T, alpha)       \
  X(T, hold_c) X(T, wealth0) X(T, strike) X(T, has_b) X(T, payoff_kind) X(T, n_dates) X(T, num_wgs) X(T, nin)       \
  X(T, h) X(T, nout) X(T, head)

#define RPH_FIELDS_SelfTargetDesc(X, T) X(T, st_feat) X(T, st_wts) X(T, st_out) X(T, st_fmu) X(T, st_fisd)

#define RPH_FIELDS_SimRideDesc(X, T) \
  X(T, sim) X(T, pay_out) X(T, pay_out2) X(T, strike) X(T, pay_kind) X(T, b0) X(T, b1) X(T, per_rider) X(T, pad_ride)

#define RPH_FIELDS_CostTerms(X, T) \
  X(T, cost_rate) X(T, band) X(T, unwind) X(T, pad) X(T, cost_out) X(T, turn_out) X(T, trades_out) X(T, cstats)
#define RPH_FIELDS_JumpTerms(X, T) X(T, lam) X(T, mu_j) X(T, sig_j) X(T, thr)
#define RPH_FIELDS_CostPnlDesc(X, T) X(T, p) X(T, c)
#define RPH_FIELDS_CostOosDesc(X, T) X(T, o) X(T, c)

#define RPH_DESCRIPTORS(X) \
  X(TrainDesc) X(EvalDesc) X(PnlFinishDesc) X(PnlDesc) X(LmDpDesc) X(LmDesc) X(SimDesc)
// Descriptors of later kernels, in a table of their own (rph_layout_fields_ext;
// native.py DESCRIPTORS_EXT): checked by name at load exactly like the first.
#define RPH_DESCRIPTORS_EXT(X) X(OosDesc)
// ... and of the eval ride (rph_layout_fields_ride; native.py DESCRIPTORS_RIDE)
#define RPH_DESCRIPTORS_RIDE(X) X(SelfTargetDesc)
// ... and of the sim ride (rph_layout_fields_sim; native.py DESCRIPTORS_SIM)
#define RPH_DESCRIPTORS_SIM(X) X(SimRideDesc)
// ... and of the scans under transaction costs (rph_layout_fields_cost; native.py DESCRIPTORS_COST)
#define RPH_DESCRIPTORS_COST(X) X(CostTerms) X(CostPnlDesc) X(CostOosDesc)
// ... and of the Merton jump scans (rph_layout_fields_jump; native.py DESCRIPTORS_JUMP)
#define RPH_DESCRIPTORS_JUMP(X) X(JumpTerms)

struct FieldRow {
  const char* strct;
  const char* field;
  unsigned offset, size;
};

#define RPH_FIELD_ROW(T, f) {#T, #f, (unsigned)offsetof(T, f), (unsigned)sizeof(T::f)},
#define RPH_STRUCT_ROWS(T) RPH_FIELDS_##T(RPH_FIELD_ROW, T)
constexpr FieldRow kFieldRows[] = {RPH_DESCRIPTORS(RPH_STRUCT_ROWS)};
constexpr FieldRow kFieldRowsExt[] = {RPH_DESCRIPTORS_EXT(RPH_STRUCT_ROWS)};
constexpr FieldRow kFieldRowsRide[] = {RPH_DESCRIPTORS_RIDE(RPH_STRUCT_ROWS)};
constexpr FieldRow kFieldRowsSim[] = {RPH_DESCRIPTORS_SIM(RPH_STRUCT_ROWS)};
constexpr FieldRow kFieldRowsCost[] = {RPH_DESCRIPTORS_COST(RPH_STRUCT_ROWS)};
constexpr FieldRow kFieldRowsJump[] = {RPH_DESCRIPTORS_JUMP(RPH_STRUCT_ROWS)};

// The listed fields of `strct` start at 0, follow each other with no gap and
// end at `size`: with no implicit padding in the struct, none is left out.
constexpr bool layout_same(const char* a, const char* b) {
  for (; *a && *a == *b; ++a, ++b) {}
  return *a == *b;
}
template <size_t N>
constexpr bool layout_covers(const FieldRow (&rows)[N], const char* strct, size_t size) {
  size_t end = 0;
  for (const FieldRow& r : rows)
    if (layout_same(r.strct, strct)) {
      if (r.offset != end) return false;
      end += r.size;
    }
  return end == size;
}
#define RPH_STRUCT_COVERED_IN(rows, T)                                                         \
  static_assert(layout_covers(rows, #T, sizeof(T)), "RPH_FIELDS_" #T " does not cover " #T     \
                                                    ": a field is missing or out of order, or " \
                                                    "the struct has implicit padding");
#define RPH_STRUCT_COVERED(T) RPH_STRUCT_COVERED_IN(kFieldRows, T)
#define RPH_STRUCT_COVERED_EXT(T) RPH_STRUCT_COVERED_IN(kFieldRowsExt, T)
#define RPH_STRUCT_COVERED_RIDE(T) RPH_STRUCT_COVERED_IN(kFieldRowsRide, T)
#define RPH_STRUCT_COVERED_SIM(T) RPH_STRUCT_COVERED_IN(kFieldRowsSim, T)
#define RPH_STRUCT_COVERED_COST(T) RPH_STRUCT_COVERED_IN(kFieldRowsCost, T)
#define RPH_STRUCT_COVERED_JUMP(T) RPH_STRUCT_COVERED_IN(kFieldRowsJump, T)
RPH_DESCRIPTORS(RPH_STRUCT_COVERED)
RPH_DESCRIPTORS_EXT(RPH_STRUCT_COVERED_EXT)
RPH_DESCRIPTORS_RIDE(RPH_STRUCT_COVERED_RIDE)
RPH_DESCRIPTORS_SIM(RPH_STRUCT_COVERED_SIM)
RPH_DESCRIPTORS_COST(RPH_STRUCT_COVERED_COST)
RPH_DESCRIPTORS_JUMP(RPH_STRUCT_COVERED_JUMP)

// Constants, by their names in rphedge/ops/layout.py.
struct ConstRow {
  const char* name;
  long long value;
};

#define RPH_CONST(n) {#n, (long long)(n)},
#define RPH_FLOAT_INDEX(n, T, f) {#n, (long long)(offsetof(T, f) / 4)},
constexpr ConstRow kConstRows[] = {
    // constexpr ints
    RPH_CONST(PMAX) RPH_CONST(MAXIN) RPH_CONST(MAXHOLD) RPH_CONST(MAXHIST) RPH_CONST(EVAL_NSTAT) RPH_CONST(LAG_SLOTS)
    RPH_CONST(LAG_FLOATS) RPH_CONST(PNL_PPT) RPH_CONST(OOS_WGS_PER_CU) RPH_CONST(NETW_FLOATS) RPH_CONST(OPT_FLOATS) RPH_CONST(FIT_FLOATS)
    RPH_CONST(DP_SLOTS) RPH_CONST(LM_NPMAX) RPH_CONST(LM_TILE) RPH_CONST(LM_GBLK_MAX) RPH_CONST(LM_OUTG)
    RPH_CONST(LM_OUTG_TAIL) RPH_CONST(LM_RED_OUTG) RPH_CONST(LM_RED) RPH_CONST(LM_PASS_WGS_MAX) RPH_CONST(LM_OG_MAX)
    RPH_CONST(LM_SPEC) RPH_CONST(LM_SLOT) RPH_CONST(LM_DP_WGS) RPH_CONST(LM_DP_FLAGS) RPH_CONST(LM_DP_PITCH)
    RPH_CONST(LM_SEL_W) RPH_CONST(LM_SEL_MAX)
    // Head, Loss, ExKind, HestonScheme, PathStat, SimModel
    RPH_CONST(HEAD_FREE) RPH_CONST(HEAD_COMPLEMENT) RPH_CONST(LOSS_MSE) RPH_CONST(LOSS_PINBALL)
    RPH_CONST(EX_NONE) RPH_CONST(EX_PUT) RPH_CONST(EX_CALL) RPH_CONST(HESTON_EULER) RPH_CONST(HESTON_QE)
    RPH_CONST(STAT_NONE) RPH_CONST(STAT_MEAN) RPH_CONST(STAT_GEOMEAN) RPH_CONST(STAT_MAX) RPH_CONST(STAT_MIN)
    RPH_CONST(SIM_GBM_ARITH) RPH_CONST(SIM_GBM_LOG) RPH_CONST(SIM_SV_REF) RPH_CONST(SIM_HESTON) RPH_CONST(SIM_BASKET)
    RPH_CONST(SIM_MORTALITY) RPH_CONST(SIM_MERTON) RPH_CONST(JUMP_MAX)
    // EvalStat
    RPH_CONST(ES_V) RPH_CONST(ES_V2) RPH_CONST(ES_RES) RPH_CONST(ES_RES2) RPH_CONST(ES_ABSRES) RPH_CONST(ES_APE)
    RPH_CONST(ES_PRED1) RPH_CONST(ES_COUNT) RPH_CONST(ES_HOLD) RPH_CONST(ES_HOLD2) RPH_CONST(ES_RESMIN)
    RPH_CONST(ES_RESMAX) RPH_CONST(ES_EXER) RPH_CONST(ES_EXVAL) RPH_CONST(ES_CONT) RPH_CONST(ES_TAU)
    // LmState, LmSlot
    RPH_CONST(LMS_W) RPH_CONST(LMS_RED) RPH_CONST(LMS_BEST) RPH_CONST(LMS_LAM) RPH_CONST(LMS_NACC) RPH_CONST(LMS_FAIL)
    RPH_CONST(LMS_LFIN) RPH_CONST(LMS_FAILTOT) RPH_CONST(LMS_SPEC_LAM) RPH_CONST(LMS_SPEC_PRED) RPH_CONST(LMS_SPEC_OK)
    RPH_CONST(LMS_SPEC_W) RPH_CONST(LMS_SLOTS) RPH_CONST(LMS_FLOATS)
    RPH_CONST(LSS_BEST) RPH_CONST(LSS_LAM) RPH_CONST(LSS_NU) RPH_CONST(LSS_PRED) RPH_CONST(LSS_COPY)
    RPH_CONST(LSS_SPEC_IDX) RPH_CONST(LSS_LBEST) RPH_CONST(LSS_STOP)
    // float indices of NetWeights, OptState and FitState
    RPH_FLOAT_INDEX(W_CUR, NetWeights, cur)
    RPH_FLOAT_INDEX(O_M, OptState, m) RPH_FLOAT_INDEX(O_V, OptState, v) RPH_FLOAT_INDEX(O_T, OptState, t)
    RPH_FLOAT_INDEX(O_LR, OptState, lr) RPH_FLOAT_INDEX(O_B1, OptState, beta1) RPH_FLOAT_INDEX(O_B2, OptState, beta2)
    RPH_FLOAT_INDEX(O_EPS, OptState, eps) RPH_FLOAT_INDEX(O_NAN, OptState, nan_steps)
    RPH_FLOAT_INDEX(F_WBEST, FitState, w_best) RPH_FLOAT_INDEX(F_BEST, FitState, best_loss)
    RPH_FLOAT_INDEX(F_WAIT, FitState, wait) RPH_FLOAT_INDEX(F_STOPPED, FitState, stopped)
    RPH_FLOAT_INDEX(F_EPOCH, FitState, epoch) RPH_FLOAT_INDEX(F_PATIENCE, FitState, patience)
    RPH_FLOAT_INDEX(F_MAXEP, FitState, max_epochs) RPH_FLOAT_INDEX(F_RESTORE, FitState, restore_best)
    RPH_FLOAT_INDEX(F_HASBEST, FitState, has_best) RPH_FLOAT_INDEX(F_LOSS_SUM, FitState, loss_sum)
    RPH_FLOAT_INDEX(F_LOSS_CNT, FitState, loss_cnt) RPH_FLOAT_INDEX(F_ABS_SUM, FitState, abs_sum)
    RPH_FLOAT_INDEX(F_APE_SUM, FitState, ape_sum) RPH_FLOAT_INDEX(F_LAST_LOSS, FitState, last_loss)
    RPH_FLOAT_INDEX(F_LAST_MAE, FitState, last_mae) RPH_FLOAT_INDEX(F_LAST_MAPE, FitState, last_mape)
    RPH_FLOAT_INDEX(F_RESTORE_END, FitState, restore_at_end) RPH_FLOAT_INDEX(F_HIST, FitState, hist)
};

// ... and the constants of the cost scans, by their names in rphedge/ops/layout_cost.py
// (a table of its own: rph_layout_consts_cost).
constexpr ConstRow kConstRowsCost[] = {
    RPH_CONST(COST_NSTAT) RPH_CONST(CS_COST) RPH_CONST(CS_COST2) RPH_CONST(CS_TURN) RPH_CONST(CS_TRADES)
    RPH_CONST(CS_COUNT)
};

}  // namespace rph
