// rphedge — fused simulate-and-hedge of fresh paths for gfx950 (OosDesc,
// rph_types.h): the out-of-sample test of a trained hedge in one launch, plain
// (k_hedge_oos) and under proportional transaction costs with a no-trade band
// (k_hedge_oos_cost, CostOosDesc), and both again on Merton jump-diffusion
// paths (k_hedge_oos_jump, k_hedge_oos_jump_cost: a second argument JumpTerms).
// All run the body oos_scan (oos_scan.h).
#include "oos_scan.h"

#include <type_traits>

namespace rph {

template <int NIN, int H, int NO, int HEAD, int MODEL, int STAT, bool ALIGNED>
__global__ __launch_bounds__(256) void k_hedge_oos(const OosDesc d) {
  oos_scan<NIN, H, NO, HEAD, MODEL, STAT, ALIGNED, false>(d, nullptr);
}

template <int NIN, int H, int NO, int HEAD, int MODEL, int STAT, bool ALIGNED>
__global__ __launch_bounds__(256) void k_hedge_oos_cost(const CostOosDesc d) {
  oos_scan<NIN, H, NO, HEAD, MODEL, STAT, ALIGNED, true>(d.o, &d.c);
}

// ... and on Merton jump-diffusion paths (SIM_MERTON): the jump terms are a
// second by-value argument, as in k_sim_jump.
template <int NIN, int H, int NO, int HEAD, bool ALIGNED>
__global__ __launch_bounds__(256) void k_hedge_oos_jump(const OosDesc d, const JumpTerms j) {
  oos_scan<NIN, H, NO, HEAD, SIM_MERTON, STAT_NONE, ALIGNED, false>(d, nullptr, &j);
}

template <int NIN, int H, int NO, int HEAD, bool ALIGNED>
__global__ __launch_bounds__(256) void k_hedge_oos_jump_cost(const CostOosDesc d, const JumpTerms j) {
  oos_scan<NIN, H, NO, HEAD, SIM_MERTON, STAT_NONE, ALIGNED, true>(d.o, &d.c, &j);
}

}  // namespace rph

using namespace rph;

static bool oos_two_inputs(const SimDesc& s) { return s.path_stat != STAT_NONE || s.model == SIM_HESTON; }

// Host-side check of an OosDesc (run before every launch: a bad descriptor
// must not reach the GPU).
// `j`: the jump terms of a SIM_MERTON scan (rph_oos_jump / rph_oos_jump_cost; null: the other models).
static int validate_oos(const OosDesc* d, const char* who, const JumpTerms* j = nullptr) {
  const SimDesc& s = d->sim;
  if (!d->snap || !d->stats) return rph_report(who, "null snapshot or statistics pointer");
  if (!d->fmu || !d->fisd || !d->bond) return rph_report(who, "null standardisation or bond table");
  if (s.n_local < 1) return rph_report(who, "n_local must be >= 1");
  if (j) {
    if (s.model != SIM_MERTON) return rph_report(who, "model must be SIM_MERTON");
  } else if (s.model != SIM_GBM_ARITH && s.model != SIM_GBM_LOG && s.model != SIM_HESTON) {
    return rph_report(who, "model must be SIM_GBM_ARITH, SIM_GBM_LOG or SIM_HESTON");
  }
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
  if (j)
    if (int rc = validate_jump(who, s, j)) return rc;
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

// `c` null: the plain kernel; else k_hedge_oos_cost on (*d, *c)
template <class T, int MODEL, int STAT>
static int launch_oos(const OosDesc* d, const CostTerms* c, hipStream_t s) {
  auto go = [&](auto aligned) {
    constexpr bool A = decltype(aligned)::value;
    if (c) {
      const CostOosDesc cd{*d, *c};
      hipLaunchKernelGGL((k_hedge_oos_cost<T::NIN, T::H, T::NO, T::HEAD, MODEL, STAT, A>), dim3(d->num_wgs), dim3(256), 0, s, cd);
    } else {
      hipLaunchKernelGGL((k_hedge_oos<T::NIN, T::H, T::NO, T::HEAD, MODEL, STAT, A>), dim3(d->num_wgs), dim3(256), 0, s, *d);
    }
  };
  if (oos_aligned(d)) go(std::true_type{});
  else go(std::false_type{});
  return (int)hipGetLastError();
}

template <class T, int MODEL>
static int launch_oos_stat(const OosDesc* d, const CostTerms* c, hipStream_t s) {
  switch (d->sim.path_stat) {
    case STAT_MEAN: return launch_oos<T, MODEL, STAT_MEAN>(d, c, s);
    case STAT_GEOMEAN: return launch_oos<T, SIM_GBM_LOG, STAT_GEOMEAN>(d, c, s);
    case STAT_MAX: return launch_oos<T, MODEL, STAT_MAX>(d, c, s);
    case STAT_MIN: return launch_oos<T, MODEL, STAT_MIN>(d, c, s);
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

// The launch behind rph_oos (`c` null) and rph_oos_cost, the descriptor(s) already checked.
static int oos_dispatch(const OosDesc* d, const CostTerms* c, const char* who, void* stream) {
  int max_wgs = 0;
  if (int rc = rph_oos_max_wgs(&max_wgs)) return rc;
  if (d->num_wgs > max_wgs) return rph_report(who, "num_wgs above 8 workgroups per CU");
  hipStream_t s = (hipStream_t)stream;
  // the instantiations come from the narrow shape table (hedge_core.h): its one- and two-input, two-holding shapes
  return with_shape(NarrowShapes{}, d->nin, d->h, d->nout, d->head, who, [&](auto t) {
    using T = decltype(t);
    if constexpr (T::NIN == 1 && T::S::NHOLD == 2) {
      return d->sim.model == SIM_GBM_LOG ? launch_oos<T, SIM_GBM_LOG, STAT_NONE>(d, c, s)
                                         : launch_oos<T, SIM_GBM_ARITH, STAT_NONE>(d, c, s);
    } else if constexpr (T::NIN == 2 && T::S::NHOLD == 2) {
      if (d->sim.model == SIM_HESTON) return launch_oos<T, SIM_HESTON, STAT_NONE>(d, c, s);
      return d->sim.model == SIM_GBM_LOG ? launch_oos_stat<T, SIM_GBM_LOG>(d, c, s)
                                         : launch_oos_stat<T, SIM_GBM_ARITH>(d, c, s);
    } else {
      return rph_report_shape(who, d->nin, d->h, d->nout, d->head);
    }
  });
}

// The Merton launch behind rph_oos_jump (`c` null) and rph_oos_jump_cost: the one-input, two-holding shapes.
static int oos_jump_dispatch(const OosDesc* d, const CostTerms* c, const JumpTerms* j, const char* who, void* stream) {
  int max_wgs = 0;
  if (int rc = rph_oos_max_wgs(&max_wgs)) return rc;
  if (d->num_wgs > max_wgs) return rph_report(who, "num_wgs above 8 workgroups per CU");
  hipStream_t s = (hipStream_t)stream;
  return with_shape(NarrowShapes{}, d->nin, d->h, d->nout, d->head, who, [&](auto t) {
    using T = decltype(t);
    if constexpr (T::NIN == 1 && T::S::NHOLD == 2) {
      auto go = [&](auto aligned) {
        constexpr bool A = decltype(aligned)::value;
        if (c) {
          const CostOosDesc cd{*d, *c};
          hipLaunchKernelGGL((k_hedge_oos_jump_cost<T::NIN, T::H, T::NO, T::HEAD, A>), dim3(d->num_wgs), dim3(256), 0, s, cd, *j);
        } else {
          hipLaunchKernelGGL((k_hedge_oos_jump<T::NIN, T::H, T::NO, T::HEAD, A>), dim3(d->num_wgs), dim3(256), 0, s, *d, *j);
        }
      };
      if (oos_aligned(d)) go(std::true_type{});
      else go(std::false_type{});
      return (int)hipGetLastError();
    } else {
      return rph_report_shape(who, d->nin, d->h, d->nout, d->head);
    }
  });
}

extern "C" int rph_oos_jump_check(const OosDesc* d, const JumpTerms* j) {
  if (!j) return rph_report("rph_oos_jump", "SIM_MERTON without JumpTerms");
  return validate_oos(d, "rph_oos_jump", j);
}

// Fused simulate-and-hedge on Merton jump-diffusion paths (k_hedge_oos_jump).
extern "C" int rph_oos_jump(const OosDesc* d, const JumpTerms* j, void* stream) {
  if (int rc = rph_oos_jump_check(d, j)) return rc;
  return oos_jump_dispatch(d, nullptr, j, "rph_oos_jump", stream);
}

extern "C" int rph_oos(const OosDesc* d, void* stream) {
  if (int rc = validate_oos(d, "rph_oos")) return rc;
  return oos_dispatch(d, nullptr, "rph_oos", stream);
}

// Fused simulate-and-hedge under transaction costs (CostOosDesc): rph_oos's
// checks on the embedded descriptor, then the cost terms'.
static int validate_oos_cost(const CostOosDesc* d, const char* who) {
  if (int rc = validate_oos(&d->o, who)) return rc;
  return validate_cost(&d->c, who);
}

extern "C" int rph_oos_cost_check(const CostOosDesc* d) { return validate_oos_cost(d, "rph_oos_cost"); }

extern "C" int rph_oos_cost(const CostOosDesc* d, void* stream) {
  if (int rc = validate_oos_cost(d, "rph_oos_cost")) return rc;
  return oos_dispatch(&d->o, &d->c, "rph_oos_cost", stream);
}

extern "C" int rph_oos_jump_cost_check(const CostOosDesc* d, const JumpTerms* j) {
  if (!j) return rph_report("rph_oos_jump_cost", "SIM_MERTON without JumpTerms");
  if (int rc = validate_oos(&d->o, "rph_oos_jump_cost", j)) return rc;
  return validate_cost(&d->c, "rph_oos_jump_cost");
}

// ... under transaction costs (k_hedge_oos_jump_cost).
extern "C" int rph_oos_jump_cost(const CostOosDesc* d, const JumpTerms* j, void* stream) {
  if (int rc = rph_oos_jump_cost_check(d, j)) return rc;
  return oos_jump_dispatch(&d->o, &d->c, j, "rph_oos_jump_cost", stream);
}
