// rphedge — the scan of one 256-path workgroup of the single-asset path scans
// (GBM, SV / Heston, mortality), shared by the scan kernels (paths.hip:
// k_sim_scan / k_sim_scan_pair) and the rider workgroups of the first date's
// exploration solves (hedge_lm.hip: k_lm_solve_sim), so a path is simulated by
// the same operations in the same order wherever its block runs; and the
// payoff a block may write behind its scan (SimPay).
#pragma once
#include "rph_common.h"
#include "rph_types.h"

#include "sim_step.h"  // the per-step scan code, ndtri_u30, sim_gidx

namespace rph {

// Payoff epilogue of a scan block (kind 0: none): the k_payoff kinds 1 (call)
// and 2 (put) of the path's own terminal price - the float the scan stores as
// final_out - written to out and out2 (may be null).  Scans without a path
// statistic only (the split scans, SimRideDesc).
struct SimPay {
  float* out;
  float* out2;
  float strike;
  int kind;
};

RPH_INLINE void sim_pay_store(const SimPay& pay, const int p, const float s) {
  if (pay.kind == 0) return;
  const float v = pay.kind == 1 ? fmaxf(s - pay.strike, 0.f) : fmaxf(pay.strike - s, 0.f);
  pay.out[p] = v;
  if (pay.out2) pay.out2[p] = v;
}

int validate_sim_ride(const SimRideDesc* r, const char* who);  // paths.hip

// Slice k of a sim ride's schedule (SimRideDesc; host and device): the blocks
// [start, start + count) of [b0, b1) that solve launch k carries on `riders`
// riders of per_rider blocks each; count 0 once none are left.
struct SimRideSlice {
  int start, count;
};
__host__ __device__ inline SimRideSlice sim_ride_slice(int b0, int b1, int riders, int per_rider, int k) {
  const long long cap = (long long)(riders > 0 ? riders : 0) * (per_rider > 0 ? per_rider : 0);
  long long start = (long long)b0 + (long long)(k > 0 ? k : 0) * cap;
  if (start > b1) start = b1;
  long long count = (long long)b1 - start;
  if (count > cap) count = cap;
  return SimRideSlice{(int)start, (int)count};
}

// The Sobol points of one path in the dimensions t = 1, 2, ... of one table,
// asked for in that order.  WIDE (aligned scans only): sobol_point_wide, one
// step ahead - the loads and the fold of dimension t + 1 are issued before the
// caller's work on the point of t, so the inverse CDF hides them.
template <bool ALIGNED, bool WIDE>
struct SobolWalk {
  const uint32_t* sv;
  const uint32_t* sh;
  uint32_t g, hu, xn;
  int last;
  RPH_INLINE void init(const uint32_t* sv_, const uint32_t* sh_, uint32_t g_, int n_fine) {
    sv = sv_, sh = sh_, g = g_, last = n_fine - 1;
    if (WIDE) {
      hu = __builtin_amdgcn_readfirstlane(g >> 6);
      xn = last >= 1 ? sobol_point_wide(sv + 32, sh[1], g, hu) : 0u;
    }
  }
  RPH_INLINE uint32_t at(int t) {
    if (!WIDE) return sobol_point<ALIGNED>(sv + (size_t)t * 32, sh[t], g);
    const uint32_t x = xn;
    const int tn = t < last ? t + 1 : last;
    xn = sobol_point_wide(sv + (size_t)tn * 32, sh[tn], g, hu);
    return x;
  }
};

// The coarse dates of a scan: whether fine point t = 1, 2, ... (asked for in
// that order) is stored, and its coarse index.  WIDE: a counter in place of the
// division by the run-time `reduction` at every step.
template <bool WIDE>
struct CoarseClock {
  int red, left, c;
  RPH_INLINE void init(int reduction) { red = reduction, left = reduction, c = 0; }
  RPH_INLINE bool tick(int t) {
    if (!WIDE) {
      c = t / red;
      return t % red == 0;
    }
    if (--left != 0) return false;
    left = red;
    ++c;
    return true;
  }
};

// STAT (GBM models only; PathStat in rph_types.h): a running statistic of the
// FINE-grid path, monitored at the fine points j = 1..t (max / min also at
// j = 0), kept in a register beside the state and stored to out2 / final2_out
// exactly like the price.  STAT = 0 is the plain scan.
// The scan of workgroup `blk` of descriptor d (k_sim_scan: the whole grid one
// descriptor; k_sim_scan_pair: two descriptors side by side; k_lm_solve_sim: a
// rider's blocks), followed by its paths' payoff where `pay` asks for one (the
// products are formed unfused, so they are the floats k_payoff would read back).
// WIDE (aligned scans): the low-occupancy step code (SobolWalk, CoarseClock) -
// the same points and the same stores.
template <typename Real, bool ALIGNED, int MODEL, int STAT, bool WIDE = false>
RPH_INLINE void sim_scan_block(const SimDesc& d, const int blk, const SimPay& pay = SimPay{}) {
  static_assert(!WIDE || ALIGNED, "the wide Sobol fold is the aligned one");
  const int p = blk * 256 + threadIdx.x;
  if (!ALIGNED && p >= d.n_local) return;
  const long long gp = sim_gidx(d, p);
  const uint32_t g = gray_code((uint64_t)gp);
  const Real dt = (Real)d.dt;
  const Real sdt = sqrt(dt);
  const float inv0 = (float)d.inv_norm[0];
  const size_t n = (size_t)d.n_local;

  if (MODEL == SIM_GBM_ARITH || MODEL == SIM_GBM_LOG) {
    GbmScan<Real, MODEL, STAT> gs;  // (sim_step.h)
    gs.init(d);
    d.out[p] = (float)d.s0[0] * inv0;
    if (STAT != STAT_NONE) d.out2[p] = (float)d.s0[0] * inv0;
    SobolWalk<ALIGNED, WIDE> w1;
    w1.init(d.sv1, d.shift1, g, d.n_fine);
    CoarseClock<WIDE> clk;
    clk.init(d.reduction);
    for (int t = 1; t < d.n_fine; ++t) {
      const Real z = ndtri_u30<Real>(w1.at(t));
      gs.step(z);
      const bool coarse = clk.tick(t);
      if (coarse || (STAT != STAT_NONE && t == d.n_fine - 1)) gs.refresh(t);
      if (coarse) {
        const int c = clk.c;
        const Real s = gs.price();
        if (c < d.n_coarse) {
          d.out[(size_t)c * n + p] = (float)s * inv0;
          if (STAT != STAT_NONE) d.out2[(size_t)c * n + p] = (float)gs.stat * inv0;
        }
      }
    }
    const Real s = gs.price();
    if (d.final_out) d.final_out[p] = (float)s * inv0;
    if (STAT != STAT_NONE && d.final2_out) d.final2_out[p] = (float)gs.stat * inv0;
    if (STAT == STAT_NONE) sim_pay_store(pay, p, __fmul_rn((float)s, inv0));
  } else if (MODEL == SIM_SV_REF || MODEL == SIM_HESTON) {
    // table 1 -> price shocks (W1, seed 1235), table 2 -> variance shocks (W_SV)
    SvScan<Real, MODEL> ss;  // (sim_step.h)
    ss.init(d);
    d.out[p] = (float)d.s0[0] * inv0;
    if (d.out2) d.out2[p] = (float)ss.v;
    SobolWalk<ALIGNED, WIDE> w1, w2;
    w1.init(d.sv1, d.shift1, g, d.n_fine);
    w2.init(d.sv2, d.shift2, g, d.n_fine);
    CoarseClock<WIDE> clk;
    clk.init(d.reduction);
    for (int t = 1; t < d.n_fine; ++t) {
      const Real z1 = ndtri_u30<Real>(w1.at(t));
      const uint32_t x2 = w2.at(t);
      ss.step(d, z1, x2);
      if (clk.tick(t)) {
        const int c = clk.c;
        if (c < d.n_coarse) {
          d.out[(size_t)c * n + p] = (float)ss.price() * inv0;
          if (d.out2) d.out2[(size_t)c * n + p] = (float)ss.v;
        }
      }
    }
    const float sT = __fmul_rn((float)ss.price(), inv0);
    if (d.final_out) d.final_out[p] = sT;
    sim_pay_store(pay, p, sT);
  } else if (MODEL == SIM_MORTALITY) {
    // RP:73-76 lambda Euler (Sobol seed 1234); RP:78-84 N_t ~ Binom(N_{t-1}, exp(-lambda_t dt)).
    Real lam = (Real)d.l0;
    int N = d.n0;
    const float invn = 1.0f / (float)d.n0;
    d.out2[p] = 1.0f;
    if (d.out3) d.out3[p] = (float)lam;
    const Real lc = (Real)d.lc, eta_sdt = (Real)d.eta * sdt;
    for (int t = 1; t < d.n_fine; ++t) {
      const Real z = ndtri_u30<Real>(sobol_point<ALIGNED>(d.sv2 + (size_t)t * 32, d.shift2[t], g));
      lam = lam + (lc * lam * dt + eta_sdt * z);
      // binomial deaths by inversion (mean N q << 1 per fine step)
      double q = 1.0 - exp(-(double)lam * (double)dt);
      q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
      if (N > 0 && q > 0.0) {
        const u32x4 r = philox4x32_10({(uint32_t)gp, (uint32_t)(gp >> 32),
                                       (uint32_t)t, 0xB1A0u},
                                      d.seed, 0x1234u);
        const double u = u01d(r.x, r.y);
        const double mean = (double)N * q;
        int D;
        if (mean < 200.0 && q < 1.0) {
          double f = exp((double)N * log1p(-q));  // P(D = 0)
          double F = f;
          const double ratio = q / (1.0 - q);
          D = 0;
          while (u > F && D < N) {
            f *= (double)(N - D) / (double)(D + 1) * ratio;
            ++D;
            F += f;
            if (f < 1e-300 && F < u) { break; }
          }
        } else {
          // N q >= 200 expected deaths in the step (or q = 1): the CDF walk
          // would take that many iterations per thread, so D is the rounded
          // normal approximation N q + sqrt(N q (1 - q)) z clipped to [0, N],
          // z from the top 30 bits of the same uniform (made odd: never 0).
          // Reached from about 10^5 members at quarterly steps, 10^6 at
          // dt = 0.01; _cpu_mortality follows the same rule.
          const double z2n = ndtri_u30<double>((uint32_t)(u * 1073741824.0) | 1u);
          double dd = mean + sqrt(mean * (1.0 - q)) * z2n + 0.5;
          dd = dd < 0.0 ? 0.0 : (dd > (double)N ? (double)N : dd);
          D = (int)dd;
        }
        N -= D;
      }
      if (d.parity) {  // Q3: lambda is NOT subsampled in the reference (RP:200 uses fine index t_i)
        if (t < d.n_coarse && d.out3) d.out3[(size_t)t * n + p] = (float)lam;
      }
      if (t % d.reduction == 0) {
        const int c = t / d.reduction;
        if (c < d.n_coarse) {
          d.out2[(size_t)c * n + p] = (float)N * invn;
          if (!d.parity && d.out3) d.out3[(size_t)c * n + p] = (float)lam;
        }
      }
    }
    if (d.final2_out) d.final2_out[p] = (float)N * invn;
  }
}

}  // namespace rph
