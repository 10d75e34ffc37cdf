// rphedge — body of the fused simulate-and-hedge of fresh paths (OosDesc,
// rph_types.h), shared by k_hedge_oos (COST = false, `ct` unused) and
// k_hedge_oos_cost (COST = true: proportional transaction costs and a no-trade
// band, CostTerms), both in hedge_oos.hip.  Every cost term sits behind
// `if constexpr (COST)`, so the COST = false instantiation is the plain kernel.
//
// One thread owns one path of a 256-path tile.  It walks the fine grid with
// the step code of the path scans (sim_step.h: the same recursion, Sobol
// index, Gray code, sobol_point fold and ndtri_u30 as k_sim_scan), and at every
// coarse date t
//   - forms the features the scan would have STORED at t, as rounded fp32
//     values ((float)S * inv_norm, the statistic, (float)v), standardises them
//     with the date's (fmu, fisd) - contraction is off around both, so a trace
//     holds exactly what the net consumed;
//   - evaluates date t's network(s) from LDS (k_hedge_pnl's design: the dates
//     run in lockstep per workgroup, the snapshots of a date are staged once,
//     an opaque zero offset keeps the weights in LDS);
//   - COST: moves the held position to the target where it leaves the band and
//     takes the trade's cost off the wealth (pnl_scan.h's operations);
//   - after the fine steps to date t + 1, advances the wealth in k_hedge_pnl's
//     operation order, W <- W g + h (S_{t+1} - S_t g), g = (float)(B_{t+1} / B_t).
// After the last fine point it forms the payoff (k_payoff kinds 1, 2, 4, 5)
// from the fine-grid terminal state and accumulates the P&L statistics.
//
// Workgroups are persistent: workgroup w takes the tiles w, w + gridDim.x, ...
// and keeps its statistics in fp64 registers across them; the held position
// and the cost by-products are per path and start afresh with every tile.  The
// date loop holds __syncthreads(), so NO thread leaves early: every thread of
// a workgroup runs the same tiles and dates; the threads past n_local in the
// last tile simulate a valid path index and are never stored or counted.
#pragma once
#include "hedge_core.h"
#include "sim_step.h"

namespace rph {

// MODEL = SIM_MERTON (k_hedge_oos_jump / k_hedge_oos_jump_cost): the Merton
// step of k_sim_jump (JumpScan) with the jump terms `jt`; every jump term sits
// behind `if constexpr (JUMP)`, and `jt` is unused otherwise.
template <int NIN, int H, int NO, int HEAD, int MODEL, int STAT, bool ALIGNED, bool COST>
__device__ __forceinline__ void oos_scan(const OosDesc& d, [[maybe_unused]] const CostTerms* ct,
                                         [[maybe_unused]] const JumpTerms* jt = nullptr) {
  using S = NetShape<NIN, H, NO, HEAD>;
  constexpr int NHOLD = S::NHOLD;
  static_assert(NHOLD == 2, "one traded asset and the bank account");
  static_assert(NIN == ((STAT != STAT_NONE || MODEL == SIM_HESTON) ? 2 : 1), "features: S, or S and statistic / variance");
  constexpr bool SV = MODEL == SIM_HESTON;
  constexpr bool JUMP = MODEL == SIM_MERTON;
  static_assert(!JUMP || STAT == STAT_NONE, "the Merton scan has no path statistic");
  constexpr int WBOFF = (S::P + 3) / 4 * 4;
  RPH_DASSERT(d.sim.n_local > 0 && d.num_wgs == (int)gridDim.x && d.snap != nullptr && d.stats != nullptr);
  __shared__ __attribute__((aligned(16))) float wl[WBOFF + S::P + 4];
  __shared__ double sred[4][8];
  const SimDesc& sd = d.sim;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool has_b = d.has_b != 0;
  const int n = sd.n_local, red = sd.reduction, n_fine = sd.n_fine, n_dates = d.n_dates;
  const size_t nn = (size_t)n;
  const float inv0 = (float)sd.inv_norm[0];
  const int ntiles = (n + 255) / 256;
  // fp64 statistics of this thread's paths over every tile of the workgroup
  double sv = 0, sv2 = 0, sp = 0, sp2 = 0, sa = 0, cnt = 0;
  float pmin = INFINITY, pmax = -INFINITY;
  [[maybe_unused]] double sc = 0, sc2 = 0, stn = 0, str = 0;
  [[maybe_unused]] float rate = 0.f, band = 0.f;
  if constexpr (COST) {
    rate = ct->cost_rate;
    band = ct->band;
  }

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * 256 + tid;
    const bool ok = p < n;
    const int pp = ok ? p : n - 1;  // past the end: a valid path, never stored or counted
    const uint32_t g = gray_code((uint64_t)sim_gidx(sd, pp));
    GbmScan<float, (SV || JUMP) ? SIM_GBM_LOG : MODEL, STAT> gs;
    SvScan<float, SIM_HESTON> ss;
    [[maybe_unused]] JumpScan<float> js;
    if constexpr (SV) ss.init(sd);
    else if constexpr (JUMP) js.init(sd, *jt);
    else gs.init(sd);
    // one fine step, as the scan takes it
    auto fine = [&](const int t) {
      if constexpr (SV) {
        const float z1 = ndtri_u30<float>(sobol_point<ALIGNED>(sd.sv1 + (size_t)t * 32, sd.shift1[t], g));
        const uint32_t x2 = sobol_point<ALIGNED>(sd.sv2 + (size_t)t * 32, sd.shift2[t], g);
        ss.step(sd, z1, x2);
      } else if constexpr (JUMP) {
        const size_t nf = (size_t)n_fine;
        const float z = ndtri_u30<float>(sobol_point<ALIGNED>(sd.sv1 + (size_t)t * 32, sd.shift1[t], g));
        const int nj = JumpScan<float>::count(*jt, sobol_point<ALIGNED>(sd.sv2 + (size_t)t * 32, sd.shift2[t], g));
        float zeta = 0.f;
        if (JumpScan<float>::jumps_in_wave(nj))
          zeta = ndtri_u30<float>(sobol_point<ALIGNED>(sd.sv2 + (nf + (size_t)t) * 32, sd.shift2[nf + (size_t)t], g));
        js.step(z, nj, zeta);
      } else {
        const float z = ndtri_u30<float>(sobol_point<ALIGNED>(sd.sv1 + (size_t)t * 32, sd.shift1[t], g));
        gs.step(z);
        if (t % red == 0 || (STAT != STAT_NONE && t == n_fine - 1)) gs.refresh(t);
      }
    };
    // the values the scan stores at the current point: rounded fp32 products
    // (no contraction into their consumers)
    auto stored = [&](float& s, float& x) {
#pragma clang fp contract(off)
      if constexpr (SV) {
        s = (float)ss.price() * inv0;
        x = (float)ss.v;
      } else if constexpr (JUMP) {
        s = (float)js.price() * inv0;
        x = s;
      } else {
        s = (float)gs.price() * inv0;
        x = (float)gs.stat * inv0;
      }
    };
    float s_cur, x_cur;
    {
#pragma clang fp contract(off)
      s_cur = (float)sd.s0[0] * inv0;
      x_cur = SV ? (float)ss.v : s_cur;
    }
    if (ok && sd.out) sd.out[p] = s_cur;
    if (ok && sd.out2) sd.out2[p] = x_cur;
    float wealth = d.wealth0;
    // costs: this path's held position, cost carried to the horizon, turnover, trade dates
    [[maybe_unused]] float h_prev = 0.f, cost_T = 0.f, turn = 0.f;
    [[maybe_unused]] int trades = 0;
    int t = 0;
    for (int c = 0; c < n_dates; ++c) {
      __syncthreads();  // every thread is done with the previous date's (or tile's) weights
      const NetWeights* wt = d.snap + (size_t)c * 2;
      for (int i = tid; i < S::P; i += 256) {
        wl[i] = wt[0].w[0][i];
        if (has_b) wl[WBOFF + i] = wt[1].w[0][i];
      }
      float mu[NIN], isd[NIN];
#pragma unroll
      for (int f = 0; f < NIN; ++f) {
        mu[f] = d.fmu[c * MAXIN + f];
        isd[f] = d.fisd[c * MAXIN + f];
      }
      const float grow = (float)(d.bond[c + 1] / d.bond[c]);
      [[maybe_unused]] float to_end = 0.f;
      if constexpr (COST) to_end = (float)(d.bond[n_dates] / d.bond[c]);
      __syncthreads();
      uint32_t zo = 0;  // opaque zero: weights stay in LDS (broadcast reads), not hoisted into VGPRs
      asm volatile("" : "+v"(zo));
      const float* __restrict__ WA = (const float*)__builtin_assume_aligned(wl + (zo & ~3u), 16);
      const float* __restrict__ WB = (const float*)__builtin_assume_aligned(wl + WBOFF + (zo & ~3u), 16);
      float x[NIN];
      {
#pragma clang fp contract(off)
        x[0] = (s_cur - mu[0]) * isd[0];
        if constexpr (NIN == 2) x[1] = (x_cur - mu[1]) * isd[1];
      }
      float z1[H], a1[H], z2[H], a2[H], hold[NHOLD], hb[NHOLD];
      net_forward<NIN, H, NO, HEAD>(WA, x, d.alpha, z1, a1, z2, a2, hold);
      if (has_b) {
        net_forward<NIN, H, NO, HEAD>(WB, x, d.alpha, z1, a1, z2, a2, hb);
#pragma unroll
        for (int k = 0; k < NHOLD; ++k) hold[k] = hold[k] + d.hold_c * (hb[k] - hold[k]);
      }
      if constexpr (COST) {
        // the held position and the trade's cost, in pnl_scan.h's operations
#pragma clang fp contract(off)
        const bool tr = c == 0 || band == 0.f || fabsf(hold[0] - h_prev) > band;
        const float hn = tr ? hold[0] : h_prev;
        const float dv = fmaf(fabsf(hn - h_prev), s_cur, 0.f);
        h_prev = hn;
        hold[0] = hn;
        const float cc = rate * dv;
        wealth = wealth - cc;
        cost_T = fmaf(cc, to_end, cost_T);
        turn = turn + dv;
        trades += (c > 0 && tr) ? 1 : 0;
      }
      for (int k = 0; k < red; ++k) fine(++t);
      float s_nxt, x_nxt;
      stored(s_nxt, x_nxt);
      if (ok && sd.out) sd.out[(size_t)(c + 1) * nn + p] = s_nxt;
      if (ok && sd.out2) sd.out2[(size_t)(c + 1) * nn + p] = x_nxt;
      float w = wealth * grow;
      w = fmaf(hold[0], s_nxt - s_cur * grow, w);
      wealth = w;
      s_cur = s_nxt;
      x_cur = x_nxt;
    }
    if constexpr (COST) {
      if (ct->unwind) {  // the final position is sold at the last coarse date (s_cur)
#pragma clang fp contract(off)
        const float dv = fmaf(fabsf(h_prev), s_cur, 0.f);
        const float cc = rate * dv;
        wealth = wealth - cc;
        cost_T = cost_T + cc;
        turn = turn + dv;
      }
    }
    while (t < n_fine - 1) fine(++t);  // fine steps after the last coarse date
    float s_fin, x_fin;
    stored(s_fin, x_fin);
    // k_payoff kinds 1 / 2 on the price (path statistic: on the statistic), 4 / 5 floating strike
    const float u = (STAT != STAT_NONE && d.payoff_kind <= 2) ? x_fin : s_fin;
    float pay;
    if (d.payoff_kind == 1) pay = fmaxf(u - d.strike, 0.f);
    else if (d.payoff_kind == 2) pay = fmaxf(d.strike - u, 0.f);
    else if (d.payoff_kind == 4) pay = fmaxf(s_fin - x_fin, 0.f);
    else pay = fmaxf(x_fin - s_fin, 0.f);
    const float pnl = wealth - pay;
    if (ok) {
      if (sd.final_out) sd.final_out[p] = s_fin;
      if (sd.final2_out) sd.final2_out[p] = x_fin;
      if (d.payoff_out) d.payoff_out[p] = pay;
      if (d.pnl_out) d.pnl_out[p] = pnl;
      sv += wealth;
      sv2 += (double)wealth * wealth;
      sp += pnl;
      sp2 += (double)pnl * pnl;
      sa += fabsf(pnl);
      cnt += 1.0;
      pmin = fminf(pmin, pnl);
      pmax = fmaxf(pmax, pnl);
      if constexpr (COST) {
        if (ct->cost_out) ct->cost_out[p] = cost_T;
        if (ct->turn_out) ct->turn_out[p] = turn;
        if (ct->trades_out) ct->trades_out[p] = trades;
        sc += cost_T;
        sc2 += (double)cost_T * cost_T;
        stn += turn;
        str += (double)trades;
      }
    }
  }
  // per-workgroup statistics in the eval-stats layout (k_hedge_pnl's rows)
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
    if constexpr (COST) {
      sc += __shfl_xor(sc, o, 64);
      sc2 += __shfl_xor(sc2, o, 64);
      stn += __shfl_xor(stn, o, 64);
      str += __shfl_xor(str, o, 64);
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
