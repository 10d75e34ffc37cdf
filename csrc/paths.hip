// rphedge — Monte-Carlo path generation for gfx950:
//   K1  scrambled Sobol (index-addressable, bit-exact with scipy.stats.qmc.Sobol)
//   K2  inverse normal CDF fused into K1 (fp32 Giles / fp64 Acklam+Halley)
//   K3  GBM scans (arithmetic Euler RP:64-65, log-Euler EO:161-165), basket;
//       optional running statistic of the fine GBM path (mean / geometric
//       mean / max / min: Asian and lookback options)
//   K4  SV scans (reference CIR-on-sigma RP:282-289; full-truncation Heston)
//   K3b Merton jump-diffusion scan (k_sim_jump: log-Euler GBM + compound-Poisson jumps)
//   K5+K6 mortality intensity Euler + binomial survivors (RP:71-84)
//   K7  payoffs (guarantee RP:88/:184, call/put EO:328-329, basket call,
//       floating strike)
//
// One thread per path; the time recursion lives in registers; Sobol normals
// are regenerated on the fly (W is never stored); only the coarse rebalancing
// grid (every `reduction` fine steps, RP:92-96) is written, time-major
// [n_coarse][n_local] so each date is one coalesced row per wave.
#include <type_traits>

#include "rph_common.h"
#include "rph_types.h"

#include "sim_scan.h"  // sim_scan_block (shared with hedge_lm.hip); sim_step.h: the per-step code, ndtri_u30, sim_gidx

namespace rph {

// Standalone K1+K2: out[i*d + j] (path-major like scipy) of N(0,1) draws.
template <typename Real, bool ALIGNED>
__global__ __launch_bounds__(256) void k_sobol_normal(Real* __restrict__ out, int n, int d,
                                                      const uint32_t* __restrict__ sv,
                                                      const uint32_t* __restrict__ shift,
                                                      long long offset, int raw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (ALIGNED == false && i >= n) return;
  const uint32_t g = gray_code((uint64_t)(offset + i));
  for (int j = 0; j < d; ++j) {
    const uint32_t x = sobol_point<ALIGNED>(sv + (size_t)j * 32, shift[j], g);
    Real v;
    if (raw) v = (Real)x * (Real)9.313225746154785e-10;
    else v = ndtri_u30<Real>(x);
    if (i < n) out[(size_t)i * d + j] = v;
  }
}

// ---------------------------------------------------------------------------
// Single-asset / SV / Heston / mortality scans.
// ---------------------------------------------------------------------------
// Workgroup b scans block blk0 + b of d (blk0 > 0: the blocks a split scan has
// left, rph_sim_ride_rest) and writes the payoff `pay` asks for.
// WIDE: the low-occupancy step code of sim_scan_block (the parts of a split scan).
template <typename Real, bool ALIGNED, int MODEL, int STAT = 0, bool WIDE = false>
__global__ __launch_bounds__(256) void k_sim_scan(const SimDesc d, const int blk0, const SimPay pay) {
  sim_scan_block<Real, ALIGNED, MODEL, STAT, WIDE>(d, blk0 + (int)blockIdx.x, pay);
}

// Two scans of the same instantiation in one launch: workgroups [0, split) run
// descriptor a, the rest descriptor b (the run's paths and the LM Gram
// subsample: the second is a few workgroups of pure Sobol / ndtri latency,
// which hide beside the first instead of following it on an empty GPU).  Every
// thread runs sim_scan_block exactly as in a launch of its own.  `pay`: the
// payoff of a's paths (split below a's grid: the head of a split scan,
// rph_sim_ride_head).
template <typename Real, bool ALIGNED, int MODEL, int STAT = 0, bool WIDE = false>
__global__ __launch_bounds__(256) void k_sim_scan_pair(const SimDesc a, const SimDesc b, const int split,
                                                       const SimPay pay) {
  if ((int)blockIdx.x < split) sim_scan_block<Real, ALIGNED, MODEL, STAT, WIDE>(a, (int)blockIdx.x, pay);
  else sim_scan_block<Real, ALIGNED, MODEL, STAT, WIDE>(b, (int)blockIdx.x - split);
}

// ---------------------------------------------------------------------------
// Merton jump-diffusion scan (SIM_MERTON; JumpScan in sim_step.h): the stores,
// the index map and the final value of the plain GBM scan.  Table 1 -> the
// diffusion normals, table 2 -> the count uniform of step t at dimension t and
// the jump-size normal at dimension n_fine + t.
// ---------------------------------------------------------------------------
template <typename Real, bool ALIGNED>
__global__ __launch_bounds__(256) void k_sim_jump(const SimDesc d, const JumpTerms j) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (!ALIGNED && p >= d.n_local) return;
  const uint32_t g = gray_code((uint64_t)sim_gidx(d, p));
  const float inv0 = (float)d.inv_norm[0];
  const size_t n = (size_t)d.n_local;
  const size_t nf = (size_t)d.n_fine;
  JumpScan<Real> js;
  js.init(d, j);
  d.out[p] = (float)d.s0[0] * inv0;
  for (int t = 1; t < d.n_fine; ++t) {
    const Real z = ndtri_u30<Real>(sobol_point<ALIGNED>(d.sv1 + (size_t)t * 32, d.shift1[t], g));
    const int nj = JumpScan<Real>::count(j, sobol_point<ALIGNED>(d.sv2 + (size_t)t * 32, d.shift2[t], g));
    Real zeta = (Real)0;
    if (JumpScan<Real>::jumps_in_wave(nj))
      zeta = ndtri_u30<Real>(sobol_point<ALIGNED>(d.sv2 + (nf + (size_t)t) * 32, d.shift2[nf + (size_t)t], g));
    js.step(z, nj, zeta);
    if (t % d.reduction == 0) {
      const int c = t / d.reduction;
      if (c < d.n_coarse) d.out[(size_t)c * n + p] = (float)js.price() * inv0;
    }
  }
  if (d.final_out) d.final_out[p] = (float)js.price() * inv0;
}

// ---------------------------------------------------------------------------
// Correlated basket (log-Euler), Cholesky factor in kernel args (uniform).
// Sobol dimension of (step t, asset a) = a * n_fine + t  (column 0 unused, Q8).
// ---------------------------------------------------------------------------
template <int NA, bool ALIGNED>
__global__ __launch_bounds__(256) void k_sim_basket(const SimDesc d) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (!ALIGNED && p >= d.n_local) return;
  const uint32_t g = gray_code((uint64_t)sim_gidx(d, p));
  const float dt = (float)d.dt, sdt = sqrtf(dt);
  float ly[NA], drift[NA], vol[NA], inv[NA], ch[NA * (NA + 1) / 2];
  const size_t n = (size_t)d.n_local;
#pragma unroll
  for (int a = 0, i = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b, ++i) ch[i] = (float)d.chol[a * MAXIN + b];  // hoisted fp64 -> fp32
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    ly[a] = logf((float)d.s0[a]);
    drift[a] = (float)((d.mu[a] - 0.5 * d.sigma[a] * d.sigma[a]) * d.dt);
    vol[a] = (float)d.sigma[a] * sdt;
    inv[a] = (float)d.inv_norm[a];
    d.out[(size_t)a * n + p] = (float)d.s0[a] * inv[a];
  }
  for (int t = 1; t < d.n_fine; ++t) {
    float w[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int dim = a * d.n_fine + t;
      w[a] = ndtri_u30<float>(sobol_point<ALIGNED>(d.sv1 + (size_t)dim * 32, d.shift1[dim], g));
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      float z = 0.f;
#pragma unroll
      for (int b = 0; b <= a; ++b) z = fmaf(ch[a * (a + 1) / 2 + b], w[b], z);
      ly[a] += drift[a] + vol[a] * z;
    }
    if (t % d.reduction == 0) {
      const int c = t / d.reduction;
      if (c < d.n_coarse) {
#pragma unroll
        for (int a = 0; a < NA; ++a) d.out[((size_t)c * NA + a) * n + p] = __expf(ly[a]) * inv[a];
      }
    }
  }
  if (d.final_out) {
#pragma unroll
    for (int a = 0; a < NA; ++a) d.final_out[(size_t)a * n + p] = __expf(ly[a]) * inv[a];
  }
}

// ---------------------------------------------------------------------------
// K7 payoffs (normalised units).
//   0 guarantee: max(Y_T, K) * N_T/N      (RP:88, :184)
//   1 call: max(S_T - K, 0)   2 put: max(K - S_T, 0)   (EO cell 8)
//   3 basket call: max(sum_a w_a S_a,T - K, 0)
//   4 floating-strike call: max(s - x, 0)   5 floating-strike put: max(x - s, 0)
//     (x: a second per-path array, e.g. the path's running mean / extreme)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_payoff(int kind, int n, int na, const float* __restrict__ s,
                                                const float* __restrict__ nfrac, float strike,
                                                const float* __restrict__ wts, const float* __restrict__ x,
                                                float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  float v;
  if (kind == 0) {
    const float y = s[p];
    v = (y > strike ? y : strike) * (nfrac ? nfrac[p] : 1.f);
  } else if (kind == 1) {
    v = fmaxf(s[p] - strike, 0.f);
  } else if (kind == 2) {
    v = fmaxf(strike - s[p], 0.f);
  } else if (kind == 4) {
    v = fmaxf(s[p] - x[p], 0.f);
  } else if (kind == 5) {
    v = fmaxf(x[p] - s[p], 0.f);
  } else {
    float b = 0.f;
    for (int a = 0; a < na; ++a) b = fmaf(wts[a], s[(size_t)a * n + p], b);
    v = fmaxf(b - strike, 0.f);
  }
  out[p] = v;
}

// ---------------------------------------------------------------------------
// K13 building block: radix-select histogram of monotone float keys.
// key(x) = x>=0 ? bits|0x80000000 : ~bits.  Counts keys whose (key & pmask) ==
// prefix, binned by (key >> shift) & (nbins-1).  LDS histogram per workgroup,
// one global atomic per non-empty bin.
// ---------------------------------------------------------------------------
RPH_INLINE uint32_t fkey(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_radix_hist(const float* __restrict__ x, long long n, uint32_t pmask,
                                                    uint32_t prefix, int shift, int nbins,
                                                    unsigned int* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned int h[];
  for (int i = threadIdx.x; i < nbins; i += 256) h[i] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const uint32_t k = fkey(x[i]);
    if ((k & pmask) == prefix) atomicAdd(&h[(k >> shift) & (uint32_t)(nbins - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

}  // namespace rph

using namespace rph;

static inline int grid_for(int n) { return (n + 255) / 256; }

// The checks of rph_sobol_normal without the launch.
extern "C" int rph_sobol_normal_check(int n, long long offset) {
  return n > 0 ? validate_sobol_range("rph_sobol_normal", offset, (long long)n - 1) : 0;
}

extern "C" int rph_sobol_normal(void* out, int n, int d, const uint32_t* sv, const uint32_t* shift,
                                long long offset, int fp64, int raw, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = rph_sobol_normal_check(n, offset)) return rc;
  const bool aligned = (n % 256 == 0) && (offset % 64 == 0);
  if (fp64) {
    if (aligned) hipLaunchKernelGGL((k_sobol_normal<double, true>), dim3(grid_for(n)), dim3(256), 0, s, (double*)out, n, d, sv, shift, offset, raw);
    else hipLaunchKernelGGL((k_sobol_normal<double, false>), dim3(grid_for(n)), dim3(256), 0, s, (double*)out, n, d, sv, shift, offset, raw);
  } else {
    if (aligned) hipLaunchKernelGGL((k_sobol_normal<float, true>), dim3(grid_for(n)), dim3(256), 0, s, (float*)out, n, d, sv, shift, offset, raw);
    else hipLaunchKernelGGL((k_sobol_normal<float, false>), dim3(grid_for(n)), dim3(256), 0, s, (float*)out, n, d, sv, shift, offset, raw);
  }
  return (int)hipGetLastError();
}

// One scan instantiation: descriptor d alone, or d and d2 side by side in one
// grid (d2 non-null: k_sim_scan_pair; the mortality scan is never paired).
// cut (may be null: d's whole grid, no payoff) = {first block, blocks, payoff}
// of d: a part of a split scan (SimRideDesc).
struct ScanCut {
  int blk0, nblk;
  SimPay pay;
};

template <typename Real, bool AL, int MODEL, int STAT = 0>
static void launch_scan_kernel(const SimDesc* d, const SimDesc* d2, hipStream_t s, const ScanCut* cut = nullptr) {
  const int split = cut ? cut->nblk : grid_for(d->n_local);
  const SimPay pay = cut ? cut->pay : SimPay{};
  if constexpr ((MODEL == SIM_GBM_ARITH || MODEL == SIM_GBM_LOG || MODEL == SIM_HESTON) && STAT == STAT_NONE && AL &&
                std::is_same<Real, float>::value) {
    // the parts of a split scan (validate_sim_ride: these scans only) are small grids: the low-occupancy step code
    if (cut) {
      if (d2)
        hipLaunchKernelGGL((k_sim_scan_pair<Real, AL, MODEL, STAT, true>), dim3(split + grid_for(d2->n_local)), dim3(256),
                           0, s, *d, *d2, split, pay);
      else
        hipLaunchKernelGGL((k_sim_scan<Real, AL, MODEL, STAT, true>), dim3(split), dim3(256), 0, s, *d, cut->blk0, pay);
      return;
    }
  }
  if constexpr (MODEL != SIM_MORTALITY) {
    if (d2) {
      hipLaunchKernelGGL((k_sim_scan_pair<Real, AL, MODEL, STAT>), dim3(split + grid_for(d2->n_local)), dim3(256), 0, s,
                         *d, *d2, split, pay);
      return;
    }
  }
  hipLaunchKernelGGL((k_sim_scan<Real, AL, MODEL, STAT>), dim3(split), dim3(256), 0, s, *d, cut ? cut->blk0 : 0, pay);
}

// GBM scans with a running path statistic (SimDesc.path_stat, validated by rph_simulate)
template <typename Real, bool AL, int MODEL>
static int launch_scan_stat(const SimDesc* d, const SimDesc* d2, hipStream_t s, const ScanCut* cut) {
  switch (d->path_stat) {
    case STAT_MEAN: launch_scan_kernel<Real, AL, MODEL, STAT_MEAN>(d, d2, s, cut); break;
    case STAT_GEOMEAN: launch_scan_kernel<Real, AL, SIM_GBM_LOG, STAT_GEOMEAN>(d, d2, s, cut); break;
    case STAT_MAX: launch_scan_kernel<Real, AL, MODEL, STAT_MAX>(d, d2, s, cut); break;
    case STAT_MIN: launch_scan_kernel<Real, AL, MODEL, STAT_MIN>(d, d2, s, cut); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

template <typename Real, bool AL>
static int launch_scan(const SimDesc* d, hipStream_t s, const SimDesc* d2 = nullptr, const ScanCut* cut = nullptr) {
  if (d->path_stat != STAT_NONE)
    return d->model == SIM_GBM_LOG ? launch_scan_stat<Real, AL, SIM_GBM_LOG>(d, d2, s, cut)
                                   : launch_scan_stat<Real, AL, SIM_GBM_ARITH>(d, d2, s, cut);
  switch (d->model) {
    case SIM_GBM_ARITH: launch_scan_kernel<Real, AL, SIM_GBM_ARITH>(d, d2, s, cut); break;
    case SIM_GBM_LOG: launch_scan_kernel<Real, AL, SIM_GBM_LOG>(d, d2, s, cut); break;
    case SIM_SV_REF: launch_scan_kernel<Real, AL, SIM_SV_REF>(d, d2, s, cut); break;
    case SIM_HESTON: launch_scan_kernel<Real, AL, SIM_HESTON>(d, d2, s, cut); break;
    case SIM_MORTALITY: launch_scan_kernel<Real, AL, SIM_MORTALITY>(d, nullptr, s); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

template <bool AL>
static int launch_basket(const SimDesc* d, hipStream_t s) {
  const dim3 grid(grid_for(d->n_local)), block(256);
  switch (d->na) {
    case 1: hipLaunchKernelGGL((k_sim_basket<1, AL>), grid, block, 0, s, *d); break;
    case 2: hipLaunchKernelGGL((k_sim_basket<2, AL>), grid, block, 0, s, *d); break;
    case 3: hipLaunchKernelGGL((k_sim_basket<3, AL>), grid, block, 0, s, *d); break;
    case 4: hipLaunchKernelGGL((k_sim_basket<4, AL>), grid, block, 0, s, *d); break;
    case 5: hipLaunchKernelGGL((k_sim_basket<5, AL>), grid, block, 0, s, *d); break;
    case 6: hipLaunchKernelGGL((k_sim_basket<6, AL>), grid, block, 0, s, *d); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

static int validate_sim(const SimDesc* d, const char* who) {
  if (d->map_blk < 0 || (d->map_blk > 0 && d->map_stride < d->map_blk)) return rph_report(who, "bad path-index map");
  if (d->path_stat < STAT_NONE || d->path_stat > STAT_MIN) return rph_report(who, "path_stat outside 0..4");
  if (d->path_stat != STAT_NONE) {
    if (d->model != SIM_GBM_ARITH && d->model != SIM_GBM_LOG) return rph_report(who, "path statistics need a GBM model");
    if (!d->out2) return rph_report(who, "path statistic without an out2 buffer");
    if (d->path_stat == STAT_GEOMEAN && d->model != SIM_GBM_LOG)
      return rph_report(who, "geomean needs the log scheme (SIM_GBM_LOG)");
  }
  if (d->n_local > 0) {
    // the largest global index (sim_gidx of the last local path; the map is monotone), in 64 bits
    const long long lp = (long long)d->n_local - 1;
    long long span = lp;
    if (d->map_blk > 0) {
      const long long q = lp / d->map_blk;
      if (q > 0 && d->map_stride > SOBOL_INDEX_END / q) return validate_sobol_range(who, d->path_offset, -1);
      span = q * d->map_stride + lp % d->map_blk;
    }
    if (int rc = validate_sobol_range(who, d->path_offset, span)) return rc;
  }
  return 0;
}

// The checks of rph_simulate without the launch.
extern "C" int rph_simulate_check(const SimDesc* d) { return validate_sim(d, "rph_simulate"); }

// (aligned: every wave's 64 paths are one aligned range of global indices)
static bool sim_aligned(const SimDesc* d) {
  return (d->n_local % 256 == 0) && (d->path_offset % 64 == 0) &&
         (d->map_blk == 0 || (d->map_blk % 64 == 0 && d->map_stride % 64 == 0));
}

extern "C" int rph_simulate(const SimDesc* d, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = validate_sim(d, "rph_simulate")) return rc;
  if (d->model == SIM_MERTON) return rph_report("rph_simulate", "SIM_MERTON scans take their JumpTerms through rph_simulate_jump");
  const bool aligned = sim_aligned(d);
  if (d->model == SIM_BASKET) return aligned ? launch_basket<true>(d, s) : launch_basket<false>(d, s);
  if (d->fp64) return aligned ? launch_scan<double, true>(d, s) : launch_scan<double, false>(d, s);
  return aligned ? launch_scan<float, true>(d, s) : launch_scan<float, false>(d, s);
}

// The Merton jump-diffusion scan (k_sim_jump): rph_simulate's checks, then the jump terms' and the tables'.
static int validate_sim_jump(const SimDesc* d, const JumpTerms* j, const char* who) {
  if (d->model != SIM_MERTON) return rph_report(who, "model must be SIM_MERTON");
  if (int rc = validate_sim(d, who)) return rc;
  if (d->na != 1) return rph_report(who, "SIM_MERTON simulates one asset");
  if (int rc = validate_jump(who, *d, j)) return rc;
  if (d->n_local > 0 && !d->out) return rph_report(who, "null out buffer");
  return 0;
}

// The checks of rph_simulate_jump without the launch.
extern "C" int rph_simulate_jump_check(const SimDesc* d, const JumpTerms* j) {
  return validate_sim_jump(d, j, "rph_simulate_jump");
}

extern "C" int rph_simulate_jump(const SimDesc* d, const JumpTerms* j, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = validate_sim_jump(d, j, "rph_simulate_jump")) return rc;
  if (d->n_local <= 0) return 0;
  const dim3 grid(grid_for(d->n_local)), block(256);
  const bool aligned = sim_aligned(d);
  if (d->fp64) {
    if (aligned) hipLaunchKernelGGL((k_sim_jump<double, true>), grid, block, 0, s, *d, *j);
    else hipLaunchKernelGGL((k_sim_jump<double, false>), grid, block, 0, s, *d, *j);
  } else {
    if (aligned) hipLaunchKernelGGL((k_sim_jump<float, true>), grid, block, 0, s, *d, *j);
    else hipLaunchKernelGGL((k_sim_jump<float, false>), grid, block, 0, s, *d, *j);
  }
  return (int)hipGetLastError();
}

// Scans a and b (independent outputs) in ONE launch when both select the same
// k_sim_scan instantiation (Real, ALIGNED, MODEL, STAT), a's workgroups first;
// otherwise - and for the basket and mortality kernels - two launches, as two
// rph_simulate calls.  *merged (may be null) tells which it was.
extern "C" int rph_simulate_pair(const SimDesc* a, const SimDesc* b, int* merged, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (merged) *merged = 0;
  if (int rc = validate_sim(a, "rph_simulate_pair")) return rc;
  if (int rc = validate_sim(b, "rph_simulate_pair")) return rc;
  const bool aligned = sim_aligned(a);
  const bool same = a->model == b->model && (a->fp64 != 0) == (b->fp64 != 0) && a->path_stat == b->path_stat &&
                    aligned == sim_aligned(b) && a->model != SIM_BASKET && a->model != SIM_MORTALITY &&
                    (long long)grid_for(a->n_local) + grid_for(b->n_local) <= 0x7fffffffLL;
  if (!same) {
    if (int rc = rph_simulate(a, stream)) return rc;
    return rph_simulate(b, stream);
  }
  if (merged) *merged = 1;
  if (a->fp64) return aligned ? launch_scan<double, true>(a, s, b) : launch_scan<double, false>(a, s, b);
  return aligned ? launch_scan<float, true>(a, s, b) : launch_scan<float, false>(a, s, b);
}

// ---------------------------------------------------------------------------
// The sim ride (SimRideDesc): the head launch, the slice schedule of the
// riders, and the plain launch of the blocks nobody has simulated yet.
// ---------------------------------------------------------------------------
namespace rph {
int validate_sim_ride(const SimRideDesc* r, const char* who) {
  if (!r) return rph_report(who, "null SimRideDesc");
  const SimDesc* d = &r->sim;
  if (int rc = validate_sim(d, who)) return rc;
  if ((d->model != SIM_GBM_ARITH && d->model != SIM_GBM_LOG && d->model != SIM_HESTON) || d->path_stat != STAT_NONE)
    return rph_report(who, "sim ride: GBM or Heston scans without a path statistic");
  if (d->fp64 || d->map_blk != 0 || !sim_aligned(d)) return rph_report(who, "sim ride: fp32, contiguous aligned paths");
  if (!d->out || !d->final_out || !r->pay_out) return rph_report(who, "sim ride: null out / final_out / pay_out");
  if (r->pay_kind != 1 && r->pay_kind != 2) return rph_report(who, "sim ride: payoff kinds 1 (call) / 2 (put)");
  if (r->b0 < 0 || r->b1 != grid_for(d->n_local) || r->b0 > r->b1 || r->per_rider < 1)
    return rph_report(who, "sim ride: bad block range / blocks per rider");
  return 0;
}
}  // namespace rph

// Slice k of the riders' schedule: blocks [*start, *start + *count) of [b0, b1)
// go to solve launch k (count 0: none left); rider r of `riders` scans the
// blocks *start + r + j * riders below *start + *count, j < per_rider.
// Returns the first block no slice up to k covers.
extern "C" int rph_sim_ride_slice(int b0, int b1, int riders, int per_rider, int k, int* start, int* count) {
  const SimRideSlice sl = sim_ride_slice(b0, b1, riders, per_rider, k);
  if (start) *start = sl.start;
  if (count) *count = sl.count;
  return sl.start + sl.count;
}

static SimPay ride_pay(const SimRideDesc* r) { return SimPay{r->pay_out, r->pay_out2, r->strike, r->pay_kind}; }

// Blocks [0, b0) of the ride's scan with their payoff, and the whole scan g
// (the LM Gram subsample; may be null) beside them: one launch.
extern "C" int rph_sim_ride_head(const SimRideDesc* r, const SimDesc* g, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = validate_sim_ride(r, "rph_sim_ride_head")) return rc;
  const SimDesc* a = &r->sim;
  if (g) {
    if (int rc = validate_sim(g, "rph_sim_ride_head")) return rc;
    if (g->model != a->model || g->fp64 || g->path_stat != a->path_stat || !sim_aligned(g))
      return rph_report("rph_sim_ride_head", "the second scan must select the same kernel");
  }
  if (r->b0 == 0 && !g) return 0;
  const ScanCut cut{0, r->b0, ride_pay(r)};
  if (r->b0 == 0) return launch_scan<float, true>(g, s);
  return launch_scan<float, true>(a, s, g, &cut);
}

// Blocks [from, b1) of the ride's scan with their payoff in one plain launch
// (from >= b1: nothing).
extern "C" int rph_sim_ride_rest(const SimRideDesc* r, int from, void* stream) {
  if (int rc = validate_sim_ride(r, "rph_sim_ride_rest")) return rc;
  if (from < r->b0) return rph_report("rph_sim_ride_rest", "block below the ride's range");
  if (from >= r->b1) return 0;
  const ScanCut cut{from, r->b1 - from, ride_pay(r)};
  return launch_scan<float, true>(&r->sim, (hipStream_t)stream, nullptr, &cut);
}

extern "C" int rph_payoff(int kind, int n, int na, const float* s, const float* nfrac, float strike,
                          const float* wts, const float* x, float* out, void* stream) {
  if ((kind == 4 || kind == 5) && !x) return rph_report("rph_payoff", "floating-strike payoff without the x array");
  hipLaunchKernelGGL(k_payoff, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, kind, n, na, s, nfrac,
                     strike, wts, x, out);
  return (int)hipGetLastError();
}

extern "C" int rph_radix_hist(const float* x, long long n, uint32_t pmask, uint32_t prefix, int shift,
                              int nbins, unsigned int* hist, void* stream) {
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_radix_hist, dim3((unsigned)blocks), dim3(256), nbins * sizeof(unsigned int),
                     (hipStream_t)stream, x, n, pmask, prefix, shift, nbins, hist);
  return (int)hipGetLastError();
}
