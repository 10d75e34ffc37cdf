// rphedge — EvalBody: the value / holdings / residual epilogue of a
// backward-induction date (K12) in pieces, shared by k_hedge_eval
// (hedge_mlp.hip: one workgroup per block of the path grid) and by the rider
// workgroups of k_lm_solve_eval (hedge_lm.hip: the next fit's first solve
// launch, every rider looping over its share of the same blocks).
//   V_t       = h(state_t) . p_t           (Keras predict(X0), RP:212)
//   blend     = g + c (h - g)              (RP:221)
//   residual  = V_{t+1} - h . p_{t+1}       ("VaR", RP:120; Q24)
// Per-block fp64 statistics go to a [num_wgs][EVAL_NSTAT] slab.  A BLOCK vb of
// the grid of nvb is the paths vb 256 + tid + i nvb 256 (i = 0, 1, ...): the
// per-thread fp32 partials, the reduce-scatter, the four-wave fp64 combine and
// the slab row of a block are the same operations whoever runs it.
#pragma once
#include "hedge_core.h"

namespace rph {

// PA: the traded-asset prices at t ARE the leading features (GBM / basket:
// same tensors, detected by pointer on the host) - loaded once per path.
// EX: the date is an exercise date (EvalDesc.ex_kind / ex_strike): the stored
// value is max(intrinsic, continuation) by the rule X > 0 && X >= C, and the
// slab gains ES_EXER / ES_EXVAL / ES_CONT.  Holdings, pred1 and the residual
// are the fitted hedge's either way (it is held over [t, t+1) by the paths
// that go on).  The plain instantiations (EX = false) keep their code path.
template <int NIN, int H, int NO, int HEAD, bool PA, bool EX = false>
struct EvalBody {
  using S = NetShape<NIN, H, NO, HEAD>;
  static constexpr int NHOLD = S::NHOLD;
  static_assert(!PA || NIN >= NHOLD - 1, "price alias needs a feature per traded asset");
  static constexpr int WBOFF = (S::P + 3) / 4 * 4;  // net B's weights 16-byte aligned (ds_read_b128)
  static constexpr int WL_FLOATS = WBOFF + S::P + 4;
  // per-thread fp32 partials (a thread sees only a handful of paths), one
  // in-wave reduce-scatter, fp64 only across waves / workgroups
  static constexpr int NS = 64;
  // Inputs of one path; a ring of EPF of them is kept in flight so every
  // iteration's loads were issued EPF-1 iterations earlier (a thread walks
  // n_local / (256 * num_wgs) paths, typically 16: one resident wave per SIMD
  // would otherwise wait a full memory round trip per path).
  static constexpr int EPF = 4;
  struct In {
    float x[NIN], pt[NHOLD], pt1[NHOLD], tgt, gb;
    int p;
    bool valid;
  };
  // what the descriptor switches on, the same for every path
  struct Mode {
    bool has_b, has1, pnl_on, pnl_read;
    RPH_INLINE explicit Mode(const EvalDesc& d)
        : has_b(d.wb != nullptr),
          has1(d.price_t1[0] != nullptr),
          // folded P&L (EvalDesc.pnl_acc): a path's R is read and written by its own thread only
          pnl_on(!EX && d.pnl_acc != nullptr),
          pnl_read(!EX && d.pnl_acc != nullptr && !d.pnl_first) {}
  };

  // the weights of net A (and B) into wl; `snap`: this workgroup also writes
  // the per-date weight snapshots (saved-model format, P&L scan)
  RPH_INLINE static void stage(const EvalDesc& d, const Mode& md, float* wl, const bool snap) {
    for (int i = threadIdx.x; i < S::P; i += 256) {
      wl[i] = d.wa->w[0][i];
      if (md.has_b) wl[WBOFF + i] = d.wb->w[0][i];
    }
    __syncthreads();
    if (snap) {
      for (int i = threadIdx.x; i < S::P; i += 256) {
        if (d.snap_a) d.snap_a->w[0][i] = wl[i];
        if (d.snap_b) d.snap_b->w[0][i] = md.has_b ? wl[WBOFF + i] : wl[i];
      }
    }
  }

  RPH_INLINE static void load_in(const EvalDesc& d, const Mode& md, int p, In& in) {
    in.p = p;
    in.valid = p < d.n_local;
    const int pp = in.valid ? p : 0;
#pragma unroll
    for (int f = 0; f < NIN; ++f) in.x[f] = d.feat[f][pp];  // raw (ring): standardised where consumed
#pragma unroll
    for (int k = 0; k < NHOLD - 1; ++k) {
      if constexpr (PA) in.pt[k] = in.x[PA ? k : 0];  // (raw feature = raw price)
      else in.pt[k] = d.price_t[k][pp];
      in.pt1[k] = md.has1 ? d.price_t1[k][pp] : 0.f;
    }
    in.tgt = (md.has1 && d.target) ? d.target[pp] : 0.f;
    in.gb = d.g_base ? d.g_base[pp] : 0.f;
  }

  RPH_INLINE static void reset(float (&st)[NS], float& rmin, float& rmax) {
#pragma unroll
    for (int i = 0; i < NS; ++i) st[i] = 0.f;
    rmin = INFINITY;
    rmax = -INFINITY;
  }

  // one path: the network(s), V_t, the residual, the per-path outputs and the
  // thread's partial statistics.  WA / WB: the staged weights in LDS
  RPH_INLINE static void path(const EvalDesc& d, const Mode& md, const In& cur, const float* __restrict__ WA,
                              const float* __restrict__ WB, float (&st)[NS], float& rmin, float& rmax) {
    const int p = cur.p;
    const bool valid = cur.valid;
    // R of the path: issued here, consumed after the network (one register; a
    // slot in the load ring cost four and a wave per SIMD of occupancy)
    const float racc = md.pnl_read ? d.pnl_acc[valid ? p : 0] : 0.f;
    // opaque zero offset: the weights stay in LDS and are read as broadcasts
    // every iteration instead of being hoisted into (and spilling out of) VGPRs
    uint32_t zo = 0;
    asm volatile("" : "+v"(zo));
    const float* __restrict__ WAi = (const float*)__builtin_assume_aligned(WA + (zo & ~3u), 16);
    const float* __restrict__ WBi = (const float*)__builtin_assume_aligned(WB + (zo & ~3u), 16);
    float z1[H], a1[H], z2[H], a2[H], hold[NHOLD], holdv[NHOLD], xn[NIN];
#pragma unroll
    for (int f = 0; f < NIN; ++f) xn[f] = (cur.x[f] - d.fmu[f]) * d.fisd[f];
    net_forward<NIN, H, NO, HEAD>(WAi, xn, d.alpha, z1, a1, z2, a2, hold);
#pragma unroll
    for (int k = 0; k < NHOLD; ++k) holdv[k] = hold[k];
    if (md.has_b) {
      // V_t comes from net B (model2.predict, RP:218); reported holdings are
      // the blend hA + hold_c (hB - hA) (get_phi_psi_VaR, RP:114-115).
      net_forward<NIN, H, NO, HEAD>(WBi, xn, d.alpha, z1, a1, z2, a2, holdv);
#pragma unroll
      for (int k = 0; k < NHOLD; ++k) hold[k] = hold[k] + d.hold_c * (holdv[k] - hold[k]);
    }
    float V = 0.f;
#pragma unroll
    for (int k = 0; k < NHOLD - 1; ++k) V = fmaf(holdv[k], cur.pt[k], V);
    V = fmaf(holdv[NHOLD - 1], d.bond_t, V);
    if (d.g_base) V = cur.gb + d.blend_c * (V - cur.gb);
    [[maybe_unused]] float cont = V, xval = 0.f;
    [[maybe_unused]] bool exer = false;
    if constexpr (EX) {
      xval = d.ex_kind == EX_PUT ? fmaxf(d.ex_strike - cur.pt[0], 0.f) : fmaxf(cur.pt[0] - d.ex_strike, 0.f);
      exer = xval > 0.f && xval >= cont;
      V = exer ? xval : cont;
    }
    float res = 0.f, pred1 = 0.f;
    const float tgt = cur.tgt;
    if (md.has1) {
#pragma unroll
      for (int k = 0; k < NHOLD - 1; ++k) pred1 = fmaf(hold[k], cur.pt1[k], pred1);
      pred1 = fmaf(hold[NHOLD - 1], d.bond_t1, pred1);
      if (d.target) res = tgt - pred1;
    }
    if (valid) {
      if (d.v_out) d.v_out[p] = V;
#pragma unroll
      for (int k = 0; k < NHOLD; ++k)
        if (d.hold_out[k]) d.hold_out[k][p] = hold[k];
      if (d.resid_out) d.resid_out[p] = res;
      if (d.pred1_out) d.pred1_out[p] = pred1;
      if constexpr (!EX) {
        if (md.pnl_on) {  // R_t = R_{t+1} + c_t sum_a h_a (S_a,t+1 - S_a,t g_t), the reported holdings
          float gain = 0.f;
#pragma unroll
          for (int k = 0; k < NHOLD - 1; ++k) gain = fmaf(hold[k], cur.pt1[k] - cur.pt[k] * d.pnl_grow, gain);
          d.pnl_acc[p] = fmaf(d.pnl_carry, gain, racc);
        }
      }
      st[ES_V] += V;
      st[ES_V2] += V * V;
      st[ES_RES] += res;
      st[ES_RES2] += res * res;
      st[ES_ABSRES] += fabsf(res);
      st[ES_APE] += d.target ? fabsf(res) * __frcp_rn(fmaxf(fabsf(tgt), 1e-7f)) : 0.f;
      st[ES_PRED1] += pred1;
      st[ES_COUNT] += 1.f;
      if constexpr (EX) {
        st[ES_EXER] += exer ? 1.f : 0.f;
        st[ES_EXVAL] += exer ? xval : 0.f;
        st[ES_CONT] += cont;
      }
#pragma unroll
      for (int k = 0; k < NHOLD; ++k) {
        st[ES_HOLD + k] += hold[k];
        st[ES_HOLD2 + k] += hold[k] * hold[k];
      }
      rmin = fminf(rmin, res);
      rmax = fmaxf(rmax, res);
    }
  }

  // the block's statistics: in-wave reduce-scatter, fp64 across the four
  // waves (sst: [4][EVAL_NSTAT] doubles of LDS), row vb of the slab.  One
  // workgroup barrier inside; a caller that goes on to another block adds one
  // before it writes sst again.
  RPH_INLINE static void finish(const EvalDesc& d, float (&st)[NS], float rmin, float rmax,
                                double (*sst)[EVAL_NSTAT], const int vb) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    wave_reduce_scatter<NS>(st, lane);  // lane L now holds the wave total of stat L
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      rmin = fminf(rmin, __shfl_xor(rmin, o, 64));
      rmax = fmaxf(rmax, __shfl_xor(rmax, o, 64));
    }
    if (lane < EVAL_NSTAT) sst[wid][lane] = (double)st[0];
    if (lane == 0) {
      sst[wid][ES_RESMIN] = rmin;
      sst[wid][ES_RESMAX] = rmax;
    }
    __syncthreads();
    if (threadIdx.x < EVAL_NSTAT) {
      const int i = threadIdx.x;
      double v;
      if (i == ES_RESMIN) v = fmin(fmin(sst[0][i], sst[1][i]), fmin(sst[2][i], sst[3][i]));
      else if (i == ES_RESMAX) v = fmax(fmax(sst[0][i], sst[1][i]), fmax(sst[2][i], sst[3][i]));
      else v = sst[0][i] + sst[1][i] + sst[2][i] + sst[3][i];
      d.stats[(size_t)vb * EVAL_NSTAT + i] = v;
    }
  }

  // A rider workgroup (rider r of nr) of another kernel's launch: blocks r,
  // r + nr, ... < d.num_wgs of the eval grid, one after the other.  The
  // weights are staged once; the load ring runs on across the block
  // boundaries, so a block's epilogue has the next block's loads in flight.
  RPH_INLINE static void ride(const EvalDesc& d, const int r, const int nr, float* wl, double (*sst)[EVAL_NSTAT]) {
    const Mode md(d);
    stage(d, md, wl, r == 0);
    const float* __restrict__ WA = wl;
    const float* __restrict__ WB = md.has_b ? wl + WBOFF : wl;
    const int nvb = d.num_wgs, stride = nvb * 256, n = d.n_local;
    const int tid = threadIdx.x;
    int lvb = r, lp0 = r * 256;  // the load cursor: (block, its iteration's first path)
    auto load_next = [&](In& in) {
      load_in(d, md, lvb < nvb ? lp0 + tid : n, in);
      lp0 += stride;
      if (lp0 >= n) {
        lvb += nr;
        lp0 = lvb * 256;
      }
    };
    In q[EPF];
#pragma unroll
    for (int i = 0; i < EPF; ++i) load_next(q[i]);
    float st[NS], rmin, rmax;
    reset(st, rmin, rmax);
    int cvb = r, cp0 = r * 256;  // the block being consumed
    while (cvb < nvb) {
      const In cur = q[0];
#pragma unroll
      for (int i = 0; i + 1 < EPF; ++i) q[i] = q[i + 1];
      if (lvb < nvb) load_next(q[EPF - 1]);
      path(d, md, cur, WA, WB, st, rmin, rmax);
      cp0 += stride;
      if (cp0 >= n) {  // the block's last iteration
        finish(d, st, rmin, rmax, sst, cvb);
        reset(st, rmin, rmax);
        cvb += nr;
        cp0 = cvb * 256;
        __syncthreads();  // sst is free again
      }
    }
  }
};

}  // namespace rph
