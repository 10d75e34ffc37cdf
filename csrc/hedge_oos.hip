// rphedge — fused simulate-and-hedge of fresh paths for gfx950 (OosDesc,
// rph_types.h): the out-of-sample test of a trained hedge in one launch.
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
//   - after the fine steps to date t + 1, advances the wealth in k_hedge_pnl's
//     operation order, W <- W g + h (S_{t+1} - S_t g), g = (float)(B_{t+1} / B_t).
// After the last fine point it forms the payoff (k_payoff kinds 1, 2, 4, 5)
// from the fine-grid terminal state and accumulates the P&L statistics.
//
// Workgroups are persistent: workgroup w takes the tiles w, w + gridDim.x, ...
// and keeps its statistics in fp64 registers across them.  The date loop holds
// __syncthreads(), so NO thread leaves early: every thread of a workgroup runs
// the same tiles and dates; the threads past n_local in the last tile simulate
// a valid path index and are never stored or counted.
#include "hedge_core.h"
#include "sim_step.h"

namespace rph {

template <int NIN, int H, int NO, int HEAD, int MODEL, int STAT, bool ALIGNED>
__global__ __launch_bounds__(256) void k_hedge_oos(const OosDesc d) {
  using S = NetShape<NIN, H, NO, HEAD>;
  constexpr int NHOLD = S::NHOLD;
  static_assert(NHOLD == 2, "one traded asset and the bank account");
  static_assert(NIN == ((STAT != STAT_NONE || MODEL == SIM_HESTON) ? 2 : 1), "features: S, or S and statistic / variance");
  constexpr bool SV = MODEL == SIM_HESTON;
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

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * 256 + tid;
    const bool ok = p < n;
    const int pp = ok ? p : n - 1;  // past the end: a valid path, never stored or counted
    const uint32_t g = gray_code((uint64_t)sim_gidx(sd, pp));
    GbmScan<float, SV ? SIM_GBM_LOG : MODEL, STAT> gs;
    SvScan<float, SIM_HESTON> ss;
    if constexpr (SV) ss.init(sd);
    else gs.init(sd);
    // one fine step, as the scan takes it
    auto fine = [&](const int t) {
      if constexpr (SV) {
        const float z1 = ndtri_u30<float>(sobol_point<ALIGNED>(sd.sv1 + (size_t)t * 32, sd.shift1[t], g));
        const uint32_t x2 = sobol_point<ALIGNED>(sd.sv2 + (size_t)t * 32, sd.shift2[t], g);
        ss.step(sd, z1, x2);
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
  }
  if (lane == 0) {
    sred[wid][0] = sv; sred[wid][1] = sv2; sred[wid][2] = sp; sred[wid][3] = sp2;
    sred[wid][4] = sa; sred[wid][5] = cnt; sred[wid][6] = pmin; sred[wid][7] = pmax;
  }
  __syncthreads();
  if (tid < EVAL_NSTAT) {
    double v = 0.0;
    auto sum4 = [&](int k) { return (sred[0][k] + sred[1][k]) + (sred[2][k] + sred[3][k]); };
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
}

}  // namespace rph

using namespace rph;

static bool oos_two_inputs(const SimDesc& s) { return s.path_stat != STAT_NONE || s.model == SIM_HESTON; }

// Host-side check of an OosDesc (run before every launch: a bad descriptor
// must not reach the GPU).
static int validate_oos(const OosDesc* d, const char* who) {
  const SimDesc& s = d->sim;
  if (!d->snap || !d->stats) return rph_report(who, "null snapshot or statistics pointer");
  if (!d->fmu || !d->fisd || !d->bond) return rph_report(who, "null standardisation or bond table");
  if (s.n_local < 1) return rph_report(who, "n_local must be >= 1");
  if (s.model != SIM_GBM_ARITH && s.model != SIM_GBM_LOG && s.model != SIM_HESTON)
    return rph_report(who, "model must be SIM_GBM_ARITH, SIM_GBM_LOG or SIM_HESTON");
  if (s.fp64 || s.na != 1 || s.map_blk != 0) return rph_report(who, "fp32, one asset, contiguous path indices only");
  if (s.path_stat < STAT_NONE || s.path_stat > STAT_MIN) return rph_report(who, "path_stat outside 0..4");
  if (s.path_stat != STAT_NONE && s.model == SIM_HESTON) return rph_report(who, "path statistics need a GBM model");
  if (s.path_stat == STAT_GEOMEAN && s.model != SIM_GBM_LOG)
    return rph_report(who, "geomean needs the log scheme (SIM_GBM_LOG)");
  if (s.model == SIM_HESTON && s.scheme != HESTON_EULER && s.scheme != HESTON_QE)
    return rph_report(who, "scheme must be HESTON_EULER or HESTON_QE");
  // the network: (1, 8, 1, COMPLEMENT) | (1, 8, 2, FREE), with a second input (2, 8, 2, FREE)
  const bool two = oos_two_inputs(s);
  const bool shape_ok = d->h == 8 && (two ? (d->nin == 2 && d->nout == 2 && d->head == HEAD_FREE)
                                          : (d->nin == 1 && ((d->nout == 1 && d->head == HEAD_COMPLEMENT) ||
                                                             (d->nout == 2 && d->head == HEAD_FREE))));
  if (!shape_ok) return rph_report_shape(who, d->nin, d->h, d->nout, d->head);
  if (s.reduction < 1 || s.n_fine < 2 || s.n_coarse != (s.n_fine + s.reduction - 1) / s.reduction ||
      d->n_dates != s.n_coarse - 1 || d->n_dates < 1)
    return rph_report(who, "n_coarse / n_dates inconsistent with n_fine and reduction");
  if (!s.sv1 || !s.shift1 || s.dims1 < s.n_fine) return rph_report(who, "Sobol table 1 missing or shorter than n_fine");
  if (s.model == SIM_HESTON && (!s.sv2 || !s.shift2 || s.dims2 < s.n_fine))
    return rph_report(who, "Sobol table 2 missing or shorter than n_fine");
  if (int rc = validate_sobol_range(who, s.path_offset, (long long)s.n_local - 1)) return rc;
  if (!(d->alpha >= 0.f && d->alpha <= 1.f)) return rph_report(who, "LeakyReLU slope must be in [0, 1]");
  if (d->payoff_kind != 1 && d->payoff_kind != 2 && d->payoff_kind != 4 && d->payoff_kind != 5)
    return rph_report(who, "payoff_kind must be 1, 2, 4 or 5");
  if (d->payoff_kind >= 4 && s.path_stat == STAT_NONE)
    return rph_report(who, "floating-strike payoff without a path statistic");
  if (!(fabsf(d->strike) <= 3.0e38f) || !(fabsf(d->wealth0) <= 3.0e38f) || !(fabsf(d->hold_c) <= 3.0e38f))
    return rph_report(who, "strike, wealth0 and hold_c must be finite");
  const int ntiles = (s.n_local + 255) / 256;
  if (d->num_wgs < 1 || d->num_wgs > ntiles) return rph_report(who, "num_wgs must be in [1, tiles of 256 paths]");
  return 0;
}

// The checks of rph_oos without the launch (and without a device).
extern "C" int rph_oos_check(const OosDesc* d) { return validate_oos(d, "rph_oos"); }

// (aligned: every wave's 64 paths are one aligned range of global indices and no tile is partial)
static bool oos_aligned(const OosDesc* d) { return (d->sim.n_local % 256 == 0) && (d->sim.path_offset % 64 == 0); }

template <class T, int MODEL, int STAT>
static int launch_oos(const OosDesc* d, hipStream_t s) {
  if (oos_aligned(d))
    hipLaunchKernelGGL((k_hedge_oos<T::NIN, T::H, T::NO, T::HEAD, MODEL, STAT, true>), dim3(d->num_wgs), dim3(256), 0, s, *d);
  else
    hipLaunchKernelGGL((k_hedge_oos<T::NIN, T::H, T::NO, T::HEAD, MODEL, STAT, false>), dim3(d->num_wgs), dim3(256), 0, s, *d);
  return (int)hipGetLastError();
}

template <class T, int MODEL>
static int launch_oos_stat(const OosDesc* d, hipStream_t s) {
  switch (d->sim.path_stat) {
    case STAT_MEAN: return launch_oos<T, MODEL, STAT_MEAN>(d, s);
    case STAT_GEOMEAN: return launch_oos<T, SIM_GBM_LOG, STAT_GEOMEAN>(d, s);
    case STAT_MAX: return launch_oos<T, MODEL, STAT_MAX>(d, s);
    case STAT_MIN: return launch_oos<T, MODEL, STAT_MIN>(d, s);
    default: return -1;
  }
}

// Workgroups the launch may use on the current device (OOS_WGS_PER_CU per CU).
extern "C" int rph_oos_max_wgs(int* out) {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        v <= 0)
      return rph_report("rph_oos_max_wgs", "cannot read the device's CU count");
    cus = v;
  }
  *out = OOS_WGS_PER_CU * cus;
  return 0;
}

extern "C" int rph_oos(const OosDesc* d, void* stream) {
  if (int rc = validate_oos(d, "rph_oos")) return rc;
  int max_wgs = 0;
  if (int rc = rph_oos_max_wgs(&max_wgs)) return rc;
  if (d->num_wgs > max_wgs) return rph_report("rph_oos", "num_wgs above 8 workgroups per CU");
  hipStream_t s = (hipStream_t)stream;
  // the instantiations come from the narrow shape table (hedge_core.h): its one- and two-input, two-holding shapes
  return with_shape(NarrowShapes{}, d->nin, d->h, d->nout, d->head, "rph_oos", [&](auto t) {
    using T = decltype(t);
    if constexpr (T::NIN == 1 && T::S::NHOLD == 2) {
      return d->sim.model == SIM_GBM_LOG ? launch_oos<T, SIM_GBM_LOG, STAT_NONE>(d, s)
                                         : launch_oos<T, SIM_GBM_ARITH, STAT_NONE>(d, s);
    } else if constexpr (T::NIN == 2 && T::S::NHOLD == 2) {
      if (d->sim.model == SIM_HESTON) return launch_oos<T, SIM_HESTON, STAT_NONE>(d, s);
      return d->sim.model == SIM_GBM_LOG ? launch_oos_stat<T, SIM_GBM_LOG>(d, s)
                                         : launch_oos_stat<T, SIM_GBM_ARITH>(d, s);
    } else {
      return rph_report_shape("rph_oos", d->nin, d->h, d->nout, d->head);
    }
  });
}
