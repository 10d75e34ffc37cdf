// rphedge — the per-step code of the single-asset path scans, shared by the
// scans that store paths (paths.hip: k_sim_scan / k_sim_scan_pair / k_sim_jump)
// and the fused simulate-and-hedge kernels (hedge_oos.hip), so both walk a
// path through the same operations in the same order:
//   GbmScan  arithmetic Euler (RP:64-65) / log-Euler (EO:161-165) GBM with the
//            optional running statistic of the fine path
//   SvScan   reference CIR-on-sigma SV (RP:282-289), full-truncation Euler
//            Heston and Andersen QE Heston
//   JumpScan Merton jump-diffusion: the log scheme plus compound-Poisson
//            log-normal jumps (k_sim_jump, k_hedge_oos_jump)
// plus the global path index of a local path and the host checks of a Sobol
// index range and of a jump scan's terms and tables.
#pragma once
#include "rph_common.h"
#include "rph_types.h"

namespace rph {

int rph_report(const char* what, const char* msg);  // runtime.cpp

template <typename Real>
RPH_INLINE Real ndtri_u30(uint32_t x);
template <>
RPH_INLINE float ndtri_u30<float>(uint32_t x) {
  x = x == 0u ? 1u : x;  // fp32 path: keep samples finite (x==0 has probability 2^-30)
  return ndtri_u30_f32(x);
}
template <>
RPH_INLINE double ndtri_u30<double>(uint32_t x) {
  return ndtri_u30_f64(x);
}

// global (Sobol / Philox) index of local path p (SimDesc.map_blk: the LM Gram
// subsample, a few aligned blocks of the global range, simulated on every rank)
RPH_INLINE long long sim_gidx(const SimDesc& d, int p) {
  return d.map_blk > 0 ? d.path_offset + ((long long)p / d.map_blk) * d.map_stride + (long long)p % d.map_blk
                       : d.path_offset + p;
}

// ---------------------------------------------------------------------------
// GBM state of one path.  STAT (PathStat in rph_types.h): a running statistic
// of the FINE-grid path, monitored at the fine points j = 1..t (max / min also
// at j = 0), kept in a register beside the state.  STAT = 0 is the plain scan.
// A scan calls step() at every fine point t >= 1, refresh(t) at the points
// whose statistic is stored (the coarse dates and the last fine point) and
// price() where the price is stored.
// ---------------------------------------------------------------------------
template <typename Real, int MODEL, int STAT>
struct GbmScan {
  Real y;      // log S (log scheme) or S
  Real drift, vol;
  Real acc;    // running sum of S (mean) / of log S (geomean), or running extreme from S_0
  Real stat;   // the statistic at the last refreshed fine point (S_0 at j = 0)
  Real sf;     // S at the current fine point (STAT: mean / max / min)

  RPH_INLINE void init(const SimDesc& d) {
    const Real dt = (Real)d.dt;
    const Real sdt = sqrt(dt);
    const Real mu = (Real)d.mu[0], sig = (Real)d.sigma[0];
    y = (MODEL == SIM_GBM_LOG) ? log((Real)d.s0[0]) : (Real)d.s0[0];
    drift = (MODEL == SIM_GBM_LOG) ? (mu - (Real)0.5 * sig * sig) * dt : mu * dt;
    vol = sig * sdt;
    acc = (STAT == STAT_MEAN || STAT == STAT_GEOMEAN) ? (Real)0 : (Real)d.s0[0];
    stat = (Real)d.s0[0];
    sf = (Real)d.s0[0];
  }

  RPH_INLINE void step(Real z) {
    if (MODEL == SIM_GBM_LOG) y += drift + vol * z;
    else y = y + y * (drift + vol * z);
    if (STAT == STAT_GEOMEAN) {
      acc += y;  // (log scheme only: the sum of log S, no exp per step)
    } else if (STAT != STAT_NONE) {
      sf = (MODEL == SIM_GBM_LOG) ? exp(y) : y;
      if (STAT == STAT_MEAN) acc += sf;
      else if (STAT == STAT_MAX) acc = sf > acc ? sf : acc;
      else acc = sf < acc ? sf : acc;
    }
  }

  RPH_INLINE void refresh(int t) {
    if (STAT == STAT_MEAN) stat = acc / (Real)t;
    else if (STAT == STAT_GEOMEAN) stat = exp(acc / (Real)t);
    else if (STAT != STAT_NONE) stat = acc;
  }

  RPH_INLINE Real price() const {
    return (STAT != STAT_NONE && STAT != STAT_GEOMEAN) ? sf : ((MODEL == SIM_GBM_LOG) ? exp(y) : y);
  }
};

// ---------------------------------------------------------------------------
// SV / Heston state of one path: table 1 -> price shocks (z1), table 2 ->
// variance shocks (the raw Sobol integer x2: the QE exponential branch inverts
// the uniform itself).
// ---------------------------------------------------------------------------
template <typename Real, int MODEL>
struct SvScan {
  Real ly, v;
  Real dt, sdt, mu, rho, rhoc;
  // Andersen (2008) QE constants (uniform over the launch): variance moments
  // m = theta + (v - theta) e^{-kappa dt}, s^2 = v*qc1 + qc2; log-price
  // central discretisation gamma1 = gamma2 = 1/2 (K1..K4) with the
  // martingale-corrected K0* (E[S_{t+dt}] = S_t e^{mu dt} exactly)
  Real kap, th, xi, ekd, qc1, qc2, qK1, qK2, qK3, qA, qK0u;
  Real tau;  // SV_REF corrected: calibration-day time step
  bool qe;

  RPH_INLINE void init(const SimDesc& d) {
    dt = (Real)d.dt;
    sdt = sqrt(dt);
    mu = (Real)d.mu[0];
    ly = log((Real)d.s0[0]);
    v = (Real)d.v0;
    rho = (Real)d.rho;
    rhoc = sqrt((Real)1 - rho * rho);
    kap = (Real)d.kappa, th = (Real)d.theta, xi = (Real)d.xi;
    ekd = exp(-kap * dt);
    qc1 = xi * xi * ekd * ((Real)1 - ekd) / kap;
    qc2 = th * xi * xi * ((Real)1 - ekd) * ((Real)1 - ekd) / ((Real)2 * kap);
    qK1 = (Real)0.5 * dt * (kap * rho / xi - (Real)0.5) - rho / xi;
    qK2 = (Real)0.5 * dt * (kap * rho / xi - (Real)0.5) + rho / xi;
    qK3 = (Real)0.5 * dt * ((Real)1 - rho * rho);
    qA = qK2 + (Real)0.5 * qK3;
    qK0u = -rho * kap * th * dt / xi;  // uncorrected K0 (when the correction does not exist)
    qe = MODEL == SIM_HESTON && d.scheme == HESTON_QE;
    tau = (Real)d.sv_tscale * dt;
  }

  RPH_INLINE void step(const SimDesc& d, Real z1, uint32_t x2) {
    if (MODEL == SIM_SV_REF) {
      const Real z2 = ndtri_u30<Real>(x2);
      if (d.sv_tscale > 0.0) {
        // corrected CIR-on-sigma: rates in calibration-day units, full
        // truncation, price shock with the start-of-step volatility
        const Real vp = v > (Real)0 ? v : (Real)0;
        ly += (mu - (Real)0.5 * vp * vp) * dt + vp * sdt * z1;
        v = v + (Real)d.a * ((Real)d.b - vp) * tau + (Real)d.c * sqrt(vp * tau) * z2;
      } else {
        // RP:285  vt = vt + a(b - vt) + c sqrt(vt dt) W_SV   (no dt on the drift: Q5)
        const Real arg = v * dt;
        const Real sq = d.parity ? sqrt(arg) : sqrt(arg > (Real)0 ? arg : (Real)0);  // parity: NaN like numpy
        v = v + (Real)d.a * ((Real)d.b - v) + (Real)d.c * sq * z2;
        // RP:287  logY += (mu - vt^2/2) dt + vt sqrt(dt) W1   (vt used as a volatility)
        ly += (mu - (Real)0.5 * v * v) * dt + v * sdt * z1;
      }
    } else if (qe) {
      const Real m = th + (v - th) * ekd;
      const Real s2 = v * qc1 + qc2;
      const Real psi = s2 / (m * m);
      Real vn, k0;
      if (psi <= (Real)1.5) {  // quadratic branch: v' = a (b + Z)^2
        const Real z2 = ndtri_u30<Real>(x2);
        const Real ip = (Real)2 / psi;
        const Real b2 = ip - (Real)1 + sqrt(ip) * sqrt(ip - (Real)1);
        const Real qa = m / ((Real)1 + b2);
        const Real bz = sqrt(b2) + z2;
        vn = qa * bz * bz;
        const Real den = (Real)1 - (Real)2 * qA * qa;
        k0 = den > (Real)0 ? -qA * b2 * qa / den + (Real)0.5 * log(den) - (qK1 + (Real)0.5 * qK3) * v : qK0u;
      } else {  // exponential branch: point mass p at 0, exponential tail (inverse CDF of the uniform)
        const Real p = (psi - (Real)1) / (psi + (Real)1);
        const Real beta = ((Real)1 - p) / m;
        const Real u = (Real)x2 * (Real)9.313225746154785e-10;
        vn = u <= p ? (Real)0 : log(((Real)1 - p) / ((Real)1 - u)) / beta;
        k0 = beta > qA ? -log(p + beta * ((Real)1 - p) / (beta - qA)) - (qK1 + (Real)0.5 * qK3) * v : qK0u;
      }
      const Real var = qK3 * (v + vn);
      ly += mu * dt + k0 + qK1 * v + qK2 * vn + sqrt(var > (Real)0 ? var : (Real)0) * z1;
      v = vn;
    } else {
      const Real z2 = ndtri_u30<Real>(x2);
      const Real vp = v > (Real)0 ? v : (Real)0;
      const Real sv = sqrt(vp * dt);
      ly += (mu - (Real)0.5 * vp) * dt + sv * (rho * z2 + rhoc * z1);
      v = v + (Real)d.kappa * ((Real)d.theta - vp) * dt + (Real)d.xi * sv * z2;
    }
  }

  RPH_INLINE Real price() const { return exp(ly); }
};

// ---------------------------------------------------------------------------
// Merton jump-diffusion state of one path (SIM_MERTON, JumpTerms): the log
// scheme of GbmScan with the compensated drift, then the step's jumps.
// A scan calls count(u) on the step's raw count uniform, draws the jump-size
// normal zeta only where some lane of the wave jumps (jumps_in_wave: the
// condition is wave-uniform, and a lane that does not jump never reads zeta)
// and then step(z, nj, zeta).  The thresholds are kernel arguments, the same
// for every lane: they stay in scalar registers.
// ---------------------------------------------------------------------------
template <typename Real>
struct JumpScan {
  Real y;  // log S
  Real drift, vol, mu_j, sig_j;

  RPH_INLINE void init(const SimDesc& d, const JumpTerms& j) {
    const Real dt = (Real)d.dt;
    const Real sdt = sqrt(dt);
    const Real mu = (Real)d.mu[0], sig = (Real)d.sigma[0];
    mu_j = (Real)j.mu_j, sig_j = (Real)j.sig_j;
    const Real kap = expm1(mu_j + (Real)0.5 * sig_j * sig_j);
    y = log((Real)d.s0[0]);
    drift = (mu - (Real)0.5 * sig * sig - (Real)j.lam * kap) * dt;  // lam = 0: GbmScan's drift, bit for bit
    vol = sig * sdt;
  }

  static RPH_INLINE int count(const JumpTerms& j, uint32_t u) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < JUMP_MAX; ++k) n += u >= j.thr[k] ? 1 : 0;
    return n;
  }

  static RPH_INLINE bool jumps_in_wave(int nj) { return __any(nj > 0) != 0; }

  RPH_INLINE void step(Real z, int nj, Real zeta) {
    y += drift + vol * z;  // (GbmScan<SIM_GBM_LOG>::step's statement)
    if (nj > 0) {
      const Real fn = (Real)nj;
      y += fn * mu_j + sqrt(fn) * sig_j * zeta;
    }
  }

  RPH_INLINE Real price() const { return exp(y); }
};

// The Sobol tables hold 30 direction numbers per dimension: point indices are
// 30-bit.  Past 2^30 the two folds of sobol_point disagree (the aligned one
// folds gray bits 30 / 31 through the zero columns, the general one stops at
// bit 29), so a range is rejected unless [first, first + span] lies in
// [0, 2^30).
static constexpr long long SOBOL_INDEX_END = 1LL << 30;

inline int validate_sobol_range(const char* who, long long first, long long span) {
  if (first < 0 || first >= SOBOL_INDEX_END || span < 0 || span >= SOBOL_INDEX_END - first)
    return rph_report(who, "path range leaves the 30-bit Sobol index space [0, 2^30)");
  return 0;
}

// Host check of a SIM_MERTON scan's jump terms and Sobol tables (the scan
// kernels and the fused out-of-sample kernel).
inline int validate_jump(const char* who, const SimDesc& s, const JumpTerms* j) {
  if (!j) return rph_report(who, "SIM_MERTON without JumpTerms");
  if (s.path_stat != STAT_NONE) return rph_report(who, "SIM_MERTON has no path statistic");
  if (s.n_fine < 2 || s.reduction < 1) return rph_report(who, "n_fine must be >= 2 and reduction >= 1");
  if (!s.sv1 || !s.shift1 || s.dims1 < s.n_fine) return rph_report(who, "Sobol table 1 missing or shorter than n_fine");
  if (!s.sv2 || !s.shift2) return rph_report(who, "SIM_MERTON needs Sobol table 2 (count uniforms, jump-size normals)");
  if ((long long)s.dims2 < 2LL * s.n_fine) return rph_report(who, "SIM_MERTON: Sobol table 2 shorter than 2 n_fine");
  if (!(j->lam >= 0.0 && j->lam <= 1e300) || !(j->sig_j >= 0.0 && j->sig_j <= 1e300) || !(fabs(j->mu_j) <= 1e300))
    return rph_report(who, "JumpTerms: lam >= 0, sig_j >= 0 and mu_j must be finite");
  for (int k = 0; k < JUMP_MAX; ++k)
    if (j->thr[k] > (uint32_t)SOBOL_INDEX_END || (k > 0 && j->thr[k] < j->thr[k - 1]))
      return rph_report(who, "JumpTerms: thresholds must be non-decreasing and at most 2^30");
  return 0;
}

}  // namespace rph
