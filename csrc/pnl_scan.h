// rphedge — body of the self-financing hedge P&L scan (PnlDesc, rph_types.h),
// shared by k_hedge_pnl (hedge_mlp.hip: COST = false, `ct` unused) and
// k_hedge_pnl_cost (hedge_cost.hip: COST = true, proportional transaction
// costs and a no-trade band, CostTerms).  Every cost term sits behind
// `if constexpr (COST)`, so the COST = false instantiation is the plain scan.
//
// One thread per path (PNL_PPT paths per thread), dates in lockstep per
// workgroup so each date's network(s) are staged once in LDS; the path inputs
// run one date ahead.  Wealth starts at V_0, holds the traded-asset holdings of
// date t's network and keeps the remainder in the bank account; P&L_T = W_T -
// liability.  Per-workgroup fp64 statistics in the eval-stats layout (ES_V =
// W_T, ES_RES = P&L).  Not a hot path (one pass per run, a few hundred VALU
// flops per path and date); the corrected counterpart of the reference's
// one-step "P&L" (Q24, Replicating_Portfolio.py:120).
//
// EX: the stopping rule of an early-exercise run (PnlDesc.ex_kind): a path is
// frozen at its first exercise date; the workgroup still walks every date in
// lockstep (the weights of a date are staged once for all its paths).
//
// COST: the held position h (registers, PNL_PPT x NA) follows the network's
// target only where it leaves the band; the date's cost leaves the wealth
// before the update; the cost carried to the horizon, the turnover and the
// trade dates are kept per path and summed per workgroup into ct->cstats in
// the shuffle and sum4 order of the P&L rows.
#pragma once
#include "hedge_core.h"

namespace rph {

template <int NIN, int H, int NO, int HEAD, bool EX, bool COST>
__device__ __forceinline__ void pnl_scan(const PnlDesc& d, [[maybe_unused]] const CostTerms* ct) {
  static_assert(!(EX && COST), "no early exercise with transaction costs");
  using S = NetShape<NIN, H, NO, HEAD>;
  constexpr int NHOLD = S::NHOLD;
  constexpr int NA = NHOLD - 1;  // traded assets (the last holding is the bank account)
  constexpr int WBOFF = (S::P + 3) / 4 * 4;
  RPH_DASSERT(d.n_local > 0 && d.num_wgs == (int)gridDim.x && d.snap != nullptr && d.stats != nullptr);
  __shared__ __attribute__((aligned(16))) float wl[WBOFF + S::P + 4];
  __shared__ double sred[4][EX ? 12 : 8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long base = (long long)blockIdx.x * 256 * PNL_PPT + tid;
  const bool has_b = d.has_b != 0;
  // per path: wealth, the traded prices at the current date (carried to the
  // next date: each price row is loaded once) and the next date's inputs,
  // all loads of a date issued together before any compute
  float wealth[PNL_PPT], s_cur[PNL_PPT][NA > 0 ? NA : 1];
  long long pidx[PNL_PPT];
#pragma unroll
  for (int j = 0; j < PNL_PPT; ++j) {
    const long long p = base + (long long)j * 256;
    const bool ok = p < d.n_local;
    pidx[j] = ok ? p : 0;  // invalid paths compute on path 0 and are never stored
    wealth[j] = ok ? (d.w0 ? d.w0[p] : d.wealth0) : 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) s_cur[j][a] = d.price[a][pidx[j]];
  }
  // date t's inputs are loaded one date ahead (software pipeline): their
  // latency hides under date t-1's network evaluation
  float xr[PNL_PPT][NIN], s_nxt[PNL_PPT][NA > 0 ? NA : 1];
  auto load_date = [&](int t) {
#pragma unroll
    for (int j = 0; j < PNL_PPT; ++j) {
#pragma unroll
      for (int f = 0; f < NIN; ++f) xr[j][f] = d.feat[f][(long long)t * d.feat_ts[f] + pidx[j]];
#pragma unroll
      for (int a = 0; a < NA; ++a) s_nxt[j][a] = d.price[a][(long long)(t + 1) * d.price_ts[a] + pidx[j]];
    }
  };
  // early exercise: a path's exercise date (n_dates: alive), its P&L and the
  // amount it was paid, discounted to date 0
  [[maybe_unused]] int tau[PNL_PPT];
  [[maybe_unused]] float pnl_ex[PNL_PPT];
  [[maybe_unused]] double paid[PNL_PPT];
  if constexpr (EX) {
#pragma unroll
    for (int j = 0; j < PNL_PPT; ++j) {
      tau[j] = d.n_dates;
      pnl_ex[j] = 0.f;
      paid[j] = 0.0;
    }
  }
  // costs: the held position, the cost carried to the horizon, the turnover
  // and the trade dates of every path
  [[maybe_unused]] float h_prev[PNL_PPT][NA > 0 ? NA : 1], cost_T[PNL_PPT], turn[PNL_PPT];
  [[maybe_unused]] int trades[PNL_PPT];
  [[maybe_unused]] float rate = 0.f, band = 0.f;
  if constexpr (COST) {
    rate = ct->cost_rate;
    band = ct->band;
#pragma unroll
    for (int j = 0; j < PNL_PPT; ++j) {
      cost_T[j] = 0.f;
      turn[j] = 0.f;
      trades[j] = 0;
#pragma unroll
      for (int a = 0; a < NA; ++a) h_prev[j][a] = 0.f;
    }
  }
  if (d.n_dates > 0) load_date(0);
  for (int t = 0; t < d.n_dates; ++t) {
    float xc[PNL_PPT][NIN], sc_nxt[PNL_PPT][NA > 0 ? NA : 1];
#pragma unroll
    for (int j = 0; j < PNL_PPT; ++j) {
#pragma unroll
      for (int f = 0; f < NIN; ++f) xc[j][f] = xr[j][f];
#pragma unroll
      for (int a = 0; a < NA; ++a) sc_nxt[j][a] = s_nxt[j][a];
    }
    if (t + 1 < d.n_dates) load_date(t + 1);
    __syncthreads();  // every thread is done with date t-1's weights
    const NetWeights* wt = d.snap + (size_t)t * 2;
    for (int i = tid; i < S::P; i += 256) {
      wl[i] = wt[0].w[0][i];
      if (has_b) wl[WBOFF + i] = wt[1].w[0][i];
    }
    float mu[NIN], isd[NIN];
#pragma unroll
    for (int f = 0; f < NIN; ++f) {
      mu[f] = d.fmu[t * MAXIN + f];
      isd[f] = d.fisd[t * MAXIN + f];
    }
    const float grow = (float)(d.bond[t + 1] / d.bond[t]);
    [[maybe_unused]] bool ex_date = false;
    [[maybe_unused]] float bond_t = 0.f, to_end = 0.f;
    [[maybe_unused]] double disc = 0.0;
    if constexpr (EX) {
      ex_date = t % d.ex_every == 0;
      bond_t = (float)d.bond[t];
      to_end = (float)(d.bond[d.n_dates] / d.bond[t]);
      disc = d.bond[0] / d.bond[t];
    }
    [[maybe_unused]] bool always = false;  // the first purchase, and band = 0, always trade
    if constexpr (COST) {
      to_end = (float)(d.bond[d.n_dates] / d.bond[t]);
      always = t == 0 || band == 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PNL_PPT; ++j) {
      uint32_t zo = 0;  // opaque zero: weights stay in LDS (broadcast reads), not hoisted into VGPRs
      asm volatile("" : "+v"(zo));
      const float* __restrict__ WA = (const float*)__builtin_assume_aligned(wl + (zo & ~3u), 16);
      const float* __restrict__ WB = (const float*)__builtin_assume_aligned(wl + WBOFF + (zo & ~3u), 16);
      float x[NIN];
#pragma unroll
      for (int f = 0; f < NIN; ++f) x[f] = (xc[j][f] - mu[f]) * isd[f];
      float z1[H], a1[H], z2[H], a2[H], hold[NHOLD], hb[NHOLD];
      net_forward<NIN, H, NO, HEAD>(WA, x, d.alpha, z1, a1, z2, a2, hold);
      if (has_b) {
        net_forward<NIN, H, NO, HEAD>(WB, x, d.alpha, z1, a1, z2, a2, hb);
#pragma unroll
        for (int k = 0; k < NHOLD; ++k) hold[k] = hold[k] + d.hold_c * (hb[k] - hold[k]);
      }
      if constexpr (EX) {
        if (ex_date && tau[j] == d.n_dates) {
          // continuation value of date t's network in the eval kernel's operation order
          float c = 0.f;
#pragma unroll
          for (int a = 0; a < NA; ++a) c = fmaf(hold[a], s_cur[j][a], c);
          c = fmaf(hold[NHOLD - 1], bond_t, c);
          const float s0 = s_cur[j][0];
          const float xv = d.ex_kind == EX_PUT ? fmaxf(d.ex_strike - s0, 0.f) : fmaxf(s0 - d.ex_strike, 0.f);
          if (xv > 0.f && xv >= c) {
            tau[j] = t;
            pnl_ex[j] = (wealth[j] - xv) * to_end;
            paid[j] = (double)xv * disc;
            wealth[j] = wealth[j] * to_end;  // W_tau carried in the bank account to the horizon
          }
        }
      }
      if constexpr (COST) {
        // the held position: the target where it leaves the band, else yesterday's;
        // its cost leaves the wealth before the update (rounded products, no contraction)
#pragma clang fp contract(off)
        float dv = 0.f;  // sum_a |dh_a| S_a,t
        bool traded = false;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const bool tr = always || fabsf(hold[a] - h_prev[j][a]) > band;
          const float hn = tr ? hold[a] : h_prev[j][a];
          dv = fmaf(fabsf(hn - h_prev[j][a]), s_cur[j][a], dv);
          traded = traded || tr;
          h_prev[j][a] = hn;
          hold[a] = hn;
        }
        const float c = rate * dv;
        wealth[j] = wealth[j] - c;
        cost_T[j] = fmaf(c, to_end, cost_T[j]);
        turn[j] = turn[j] + dv;
        trades[j] += (t > 0 && traded) ? 1 : 0;
      }
      float w = wealth[j] * grow;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        w = fmaf(hold[a], sc_nxt[j][a] - s_cur[j][a] * grow, w);
        s_cur[j][a] = sc_nxt[j][a];
      }
      if constexpr (EX) wealth[j] = tau[j] == d.n_dates ? w : wealth[j];  // an exercised path is frozen
      else wealth[j] = w;
    }
  }
  if constexpr (COST) {
    if (ct->unwind) {  // the final position is sold at the horizon (s_cur holds S_n)
#pragma clang fp contract(off)
#pragma unroll
      for (int j = 0; j < PNL_PPT; ++j) {
        float dv = 0.f;
#pragma unroll
        for (int a = 0; a < NA; ++a) dv = fmaf(fabsf(h_prev[j][a]), s_cur[j][a], dv);
        const float c = rate * dv;
        wealth[j] = wealth[j] - c;
        cost_T[j] = cost_T[j] + c;
        turn[j] = turn[j] + dv;
      }
    }
  }
  // P&L and per-workgroup fp64 statistics
  double sv = 0, sv2 = 0, sp = 0, sp2 = 0, sa = 0, cnt = 0;
  float pmin = INFINITY, pmax = -INFINITY;
  [[maybe_unused]] double sx = 0, sxv = 0, stau = 0;
  [[maybe_unused]] double sc = 0, sc2 = 0, stn = 0, str = 0;
#pragma unroll
  for (int j = 0; j < PNL_PPT; ++j) {
    const long long p = base + (long long)j * 256;
    if (p >= d.n_local) continue;
    float pnl = wealth[j] - d.payoff[p];
    if constexpr (EX) {
      const bool exd = tau[j] < d.n_dates;
      if (exd) pnl = pnl_ex[j];
      if (d.tau_out) d.tau_out[p] = tau[j];
      sx += exd ? 1.0 : 0.0;
      sxv += exd ? paid[j] : (double)d.payoff[p] * (d.bond[0] / d.bond[d.n_dates]);
      stau += (double)tau[j];
    }
    if constexpr (COST) {
      if (ct->cost_out) ct->cost_out[p] = cost_T[j];
      if (ct->turn_out) ct->turn_out[p] = turn[j];
      if (ct->trades_out) ct->trades_out[p] = trades[j];
      sc += cost_T[j];
      sc2 += (double)cost_T[j] * cost_T[j];
      stn += turn[j];
      str += (double)trades[j];
    }
    if (d.pnl_out) d.pnl_out[p] = pnl;
    sv += wealth[j];
    sv2 += (double)wealth[j] * wealth[j];
    sp += pnl;
    sp2 += (double)pnl * pnl;
    sa += fabsf(pnl);
    cnt += 1.0;
    pmin = fminf(pmin, pnl);
    pmax = fmaxf(pmax, pnl);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    sv += __shfl_xor(sv, o, 64);
    sv2 += __shfl_xor(sv2, o, 64);
    sp += __shfl_xor(sp, o, 64);
    sp2 += __shfl_xor(sp2, o, 64);
    sa += __shfl_xor(sa, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
    pmin = fminf(pmin, __shfl_xor(pmin, o, 64));
    pmax = fmaxf(pmax, __shfl_xor(pmax, o, 64));
    if constexpr (EX) {
      sx += __shfl_xor(sx, o, 64);
      sxv += __shfl_xor(sxv, o, 64);
      stau += __shfl_xor(stau, o, 64);
    }
    if constexpr (COST) {
      sc += __shfl_xor(sc, o, 64);
      sc2 += __shfl_xor(sc2, o, 64);
      stn += __shfl_xor(stn, o, 64);
      str += __shfl_xor(str, o, 64);
    }
  }
  if constexpr (EX) {
    if (lane == 0) {
      sred[wid][8] = sx; sred[wid][9] = sxv; sred[wid][10] = stau;
    }
  }
  if (lane == 0) {
    sred[wid][0] = sv; sred[wid][1] = sv2; sred[wid][2] = sp; sred[wid][3] = sp2;
    sred[wid][4] = sa; sred[wid][5] = cnt; sred[wid][6] = pmin; sred[wid][7] = pmax;
  }
  __syncthreads();
  auto sum4 = [&](int k) { return (sred[0][k] + sred[1][k]) + (sred[2][k] + sred[3][k]); };
  if (tid < EVAL_NSTAT) {
    double v = 0.0;
    if (tid == ES_V) v = sum4(0);
    else if (tid == ES_V2) v = sum4(1);
    else if (tid == ES_RES) v = sum4(2);
    else if (tid == ES_RES2) v = sum4(3);
    else if (tid == ES_ABSRES) v = sum4(4);
    else if (tid == ES_COUNT) v = sum4(5);
    else if (tid == ES_RESMIN) v = fmin(fmin(sred[0][6], sred[1][6]), fmin(sred[2][6], sred[3][6]));
    else if (tid == ES_RESMAX) v = fmax(fmax(sred[0][7], sred[1][7]), fmax(sred[2][7], sred[3][7]));
    if constexpr (EX) {
      if (tid == ES_EXER) v = sum4(8);
      else if (tid == ES_EXVAL) v = sum4(9);
      else if (tid == ES_TAU) v = sum4(10);
    }
    d.stats[(size_t)blockIdx.x * EVAL_NSTAT + tid] = v;
  }
  if constexpr (COST) {  // the cost rows, through the same LDS block once the P&L rows are read
    __syncthreads();
    if (lane == 0) {
      sred[wid][0] = sc; sred[wid][1] = sc2; sred[wid][2] = stn; sred[wid][3] = str; sred[wid][4] = cnt;
    }
    __syncthreads();
    if (tid < COST_NSTAT) {
      static_assert(CS_COST == 0 && CS_COST2 == 1 && CS_TURN == 2 && CS_TRADES == 3 && CS_COUNT == 4, "cstats rows");
      ct->cstats[(size_t)blockIdx.x * COST_NSTAT + tid] = tid <= CS_COUNT ? sum4(tid) : 0.0;
    }
  }
}

}  // namespace rph
