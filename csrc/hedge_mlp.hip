// rphedge — thread-per-path hedge-MLP training body for the reference's 8-unit
// nets (K8/K9), the ticketed step kernel with the fused Adam/early-stop update
// (K10), the minibatch chunk permutation (K11), the value/holdings/residual
// epilogue (K12) and the C ABI launchers of every training schedule, for gfx950.
//
// Reference semantics (one backward-induction date):
//   model(X1=[state_t, prices_{t+1}]) -> V = holdings(state_t) . prices_{t+1}
//   fit MSE / 99% pinball, Adam(1e-3), batch 512, EarlyStopping(loss)
//   (/root/reference/Replicating_Portfolio.py:149-221).
//
// Design (MI355X-first):
//   * NarrowBody: thread-per-path fp32 forward+backward (the compiler packs the
//     FMAs into v_pk_fma_f32); weights are wave-uniform, staged once in LDS and
//     either hoisted into registers or re-read as ds_read_b128 broadcasts
//     (variants); per-thread register accumulation of the full gradient
//     (R = next pow2 of P+4 floats), one in-wave recursive-halving
//     reduce-scatter (permlane32_swap / ds_swizzle / DPP), one LDS cross-wave sum;
//   * the same body runs under three schedules: k_hedge_step_lag (hedge_lag.h,
//     default above 64 workgroups: the update of step k-1 applied redundantly in
//     every workgroup's prologue, no in-kernel sync), k_hedge_fit (hedge_fit.h,
//     persistent per fit, default for small grids) and k_hedge_train_step below
//     (ticketed: the last-arriving workgroup sums the float-atomic replicas or
//     the deterministic slab, optionally exchanges the packet with the other
//     ranks over xGMI, and applies Keras-Adam + EarlyStopping in the same
//     launch; with an RCCL all-reduce instead, k_hedge_update applies it).
#include "hedge_core.h"
#include "hedge_eval.h"
#include "hedge_fit.h"
#include "hedge_lag.h"
#include "hedge_narrow.h"
#include "pnl_scan.h"

#include <type_traits>

namespace rph {

// ---------------------------------------------------------------------------
// K9: one optimizer step.  Grid = num_wgs workgroups of 256 threads.
// ---------------------------------------------------------------------------
template <int NIN, int H, int NO, int HEAD>
__global__ __launch_bounds__(256) void k_hedge_train_step(const TrainDesc d, const int step, const int epoch,
                                                          const Perm perm) {
  using B = NarrowBody<NIN, H, NO, HEAD>;
  constexpr int R = B::R;
  constexpr int P = B::P;
  prefetch_kernarg<sizeof(TrainDesc) + 2 * sizeof(int) + sizeof(Perm)>();
  __shared__ __attribute__((aligned(16))) float lds[B::SCRATCH_FLOATS];
  __shared__ __attribute__((aligned(16))) float wl[P + 4];
  __shared__ int s_last;

  // prologue: every independent load is issued up front — early-stop flag,
  // weights, the optimizer state for a possible last-arriver update, and the
  // first path's data (epoch is a launch argument, so the permutation needs no
  // device read).
  RPH_DASSERT(d.batch > 0 && d.n_local >= d.batch && d.num_wgs == (int)gridDim.x);
  RPH_STAMP(0);
  const float stopped = d.fit->stopped;
  const float wv = threadIdx.x < P ? d.wts->w[0][threadIdx.x] : 0.f;
  UpdPre<P> up;
  if (d.fused_update) prefetch_update<P>(up, d.wts, d.opt, d.fit, d.lr_sched, epoch, step);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  typename B::Pre pre;
  pre.valid = false;
  if (B::first(wid) < d.batch) B::load(d, step, perm, B::first(wid), lane, pre);

  if (stopped != 0.f) return;  // early-stopped fit: remaining steps are no-ops
  // Weights are wave-uniform: stage them once in LDS and read them as
  // broadcast ds_read_b128 (keeps the 100+ weights out of the SGPR file).
  if (threadIdx.x < P) wl[threadIdx.x] = wv;
  if (d.fused_update) {  // keep the prefetch here (the compiler would sink it into the last-arriver branch)
    asm volatile("" ::"v"(up.m[0]), "v"(up.v[0]), "v"(up.w[0]), "v"(up.wbest[0]), "s"(up.t), "s"(up.lr), "s"(up.loss_sum),
                 "s"(up.wait), "s"(up.best_loss), "s"(up.lr_sched_e));
  }
  __syncthreads();
  RPH_STAMP(1);
  float vv[1];
  B::partial(d, step, perm, wl, typename B::Frags{}, lds, pre, vv);
  float val = vv[0];
  float* red = lds;  // reuse: red[t] for t < R after the hand-off below
  RPH_STAMP(3);

  if (gridDim.x > 1) {
    // ---- publish the partial write-through (sc1) / float-atomically, then draw
    // the arrival ticket.  No release/acquire fences: every handed-off byte is
    // stored sc1 (or added at the memory side) and every load of it by the last
    // arriver is an sc1 load (MI355X_MICROARCH visibility table, row 1).
    const int G = gridDim.x;
    if (threadIdx.x < R) {
      if (d.deterministic) st_agent(d.slab + (size_t)blockIdx.x * R + threadIdx.x, val);
      else __hip_atomic_fetch_add(d.acc + (blockIdx.x % ACC_REPLICAS) * R + threadIdx.x, val, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY storing wave drains
    __syncthreads();
    RPH_STAMP(4);
    if (threadIdx.x == 0) {
      const uint32_t ticket = __hip_atomic_fetch_add(d.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = (ticket == (uint32_t)G - 1u) ? 1 : 0;
    }
    __syncthreads();
    RPH_STAMP(5);
    if (!s_last) return;
    if (d.deterministic) {
      // fixed row partition + fixed combine order => bitwise reproducible
      constexpr int GROUPS = 256 / R;
      const int col = threadIdx.x % R;
      const int grp = threadIdx.x / R;
      float a = 0.f;
#pragma unroll 8
      for (int r = grp; r < G; r += GROUPS) a += ld_agent(d.slab + (size_t)r * R + col);
      lds[grp * R + col] = a;
      __syncthreads();
      if (threadIdx.x < R) {
        float s2 = 0.f;
        for (int gi = 0; gi < GROUPS; ++gi) s2 += lds[gi * R + threadIdx.x];
        val = s2;
      }
      __syncthreads();
    } else {
      if (threadIdx.x < R) {
        // all 8 replica loads in ONE asm statement with one wait (sc1: every load
        // of the handed-off bytes bypasses the non-coherent L1), then re-arm.
        float* a = d.acc + threadIdx.x;
        float r0, r1, r2, r3, r4, r5, r6, r7;
        if (R == 128) {
          asm volatile(
              "global_load_dword %0, %8, off sc1\n\t"
              "global_load_dword %1, %8, off offset:512 sc1\n\t"
              "global_load_dword %2, %8, off offset:1024 sc1\n\t"
              "global_load_dword %3, %8, off offset:1536 sc1\n\t"
              "global_load_dword %4, %8, off offset:2048 sc1\n\t"
              "global_load_dword %5, %8, off offset:2560 sc1\n\t"
              "global_load_dword %6, %8, off offset:3072 sc1\n\t"
              "global_load_dword %7, %8, off offset:3584 sc1\n\t"
              "s_waitcnt vmcnt(0)"
              : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
              : "v"(a)
              : "memory");
        } else {
          float* b = a + 4 * R;
          asm volatile(
              "global_load_dword %0, %8, off sc1\n\t"
              "global_load_dword %1, %8, off offset:1024 sc1\n\t"
              "global_load_dword %2, %8, off offset:2048 sc1\n\t"
              "global_load_dword %3, %8, off offset:3072 sc1\n\t"
              "global_load_dword %4, %9, off sc1\n\t"
              "global_load_dword %5, %9, off offset:1024 sc1\n\t"
              "global_load_dword %6, %9, off offset:2048 sc1\n\t"
              "global_load_dword %7, %9, off offset:3072 sc1\n\t"
              "s_waitcnt vmcnt(0)"
              : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
              : "v"(a), "v"(b)
              : "memory");
        }
        val = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
#pragma unroll
        for (int rp = 0; rp < ACC_REPLICAS; ++rp) st_agent(a + rp * R, 0.f);  // re-arm (completes by kernel end)
      }
    }
    if (threadIdx.x == 0) __hip_atomic_store(d.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x < R) red[threadIdx.x] = val;
  __syncthreads();
  RPH_STAMP(6);

  if (d.dp_world > 1) {
    dp_allreduce<R>(d, red);
    RPH_STAMP(7);
  }
  if (d.fused_update) {
    apply_update<P>(red, up, d.wts, d.opt, d.fit, epoch, step, d.steps_per_epoch);
  } else if (threadIdx.x < R) {
    d.grad_out[threadIdx.x] = red[threadIdx.x];
  }
  if (d.dp_world <= 1) RPH_STAMP(7);
}

// ---------------------------------------------------------------------------
// K12: value / holdings / residual epilogue of a backward-induction date.
//   V_t       = h(state_t) . p_t           (Keras predict(X0), RP:212)
//   blend     = g + c (h - g)              (RP:221)
//   residual  = V_{t+1} - h . p_{t+1}       ("VaR", RP:120; Q24)
// Per-workgroup fp64 statistics go to a [num_wgs][EVAL_NSTAT] slab.
// ---------------------------------------------------------------------------
// The body is EvalBody (hedge_eval.h); this kernel runs one block of the path
// grid per workgroup.
template <int NIN, int H, int NO, int HEAD, bool PA, bool EX = false>
__global__ __launch_bounds__(256) void k_hedge_eval(const EvalDesc d) {
  using E = EvalBody<NIN, H, NO, HEAD, PA, EX>;
  using In = typename E::In;
  constexpr int EPF = E::EPF;
  prefetch_kernarg<sizeof(EvalDesc)>();
  RPH_DASSERT(d.n_local > 0 && d.num_wgs == (int)gridDim.x && d.wa != nullptr && d.stats != nullptr);
  __shared__ double sst[4][EVAL_NSTAT];
  __shared__ __attribute__((aligned(16))) float wl[E::WL_FLOATS];
  const typename E::Mode md(d);
  E::stage(d, md, wl, blockIdx.x == 0);
  const float* __restrict__ WA = wl;
  const float* __restrict__ WB = md.has_b ? wl + E::WBOFF : wl;
  float st[E::NS], rmin, rmax;
  E::reset(st, rmin, rmax);
  const int stride = (int)gridDim.x * 256;
  In q[EPF];
  const int p_first = blockIdx.x * 256 + threadIdx.x;
#pragma unroll
  for (int i = 0; i < EPF; ++i) E::load_in(d, md, p_first + i * stride, q[i]);
  for (int p0 = blockIdx.x * 256; p0 < d.n_local; p0 += stride) {
    const In cur = q[0];
#pragma unroll
    for (int i = 0; i + 1 < EPF; ++i) q[i] = q[i + 1];
    if (p0 + EPF * stride < d.n_local) E::load_in(d, md, cur.p + EPF * stride, q[EPF - 1]);
    E::path(d, md, cur, WA, WB, st, rmin, rmax);
  }
  E::finish(d, st, rmin, rmax, sst, blockIdx.x);
}

// ---------------------------------------------------------------------------
// Self-financing hedge P&L scan (PnlDesc, rph_types.h): the body is pnl_scan
// (pnl_scan.h), shared with the scan under transaction costs (hedge_cost.hip).
// EX: the stopping rule of an early-exercise run (PnlDesc.ex_kind).
// ---------------------------------------------------------------------------
template <int NIN, int H, int NO, int HEAD, bool EX = false>
__global__ __launch_bounds__(256) void k_hedge_pnl(const PnlDesc d) {
  prefetch_kernarg<sizeof(PnlDesc)>();
  pnl_scan<NIN, H, NO, HEAD, EX, false>(d, nullptr);
}

// ---------------------------------------------------------------------------
// Finish of the P&L folded into the backward induction (PnlFinishDesc,
// EvalDesc.pnl_acc): the evals of dates n-1 .. 0 left R_0 per path; one thread
// per path closes W_T = W_0 c + R_0, P&L = W_T - liability.  Workgroup w owns
// the paths [w, w + 1) x 256 PNL_PPT and writes the statistics row k_hedge_pnl
// writes for them (collect() / reduce_stats read either).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pnl_finish(const PnlFinishDesc d) {
  RPH_DASSERT(d.n_local > 0 && d.num_wgs == (int)gridDim.x && d.acc != nullptr && d.stats != nullptr);
  __shared__ double sred[4][8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long base = (long long)blockIdx.x * 256 * PNL_PPT + tid;
  double sv = 0, sv2 = 0, sp = 0, sp2 = 0, sa = 0, cnt = 0;
  float pmin = INFINITY, pmax = -INFINITY;
#pragma unroll
  for (int j = 0; j < PNL_PPT; ++j) {
    const long long p = base + (long long)j * 256;
    if (p >= d.n_local) continue;
    const float w = fmaf(d.w0[p], d.carry, d.acc[p]);
    const float pnl = w - d.payoff[p];
    if (d.pnl_out) d.pnl_out[p] = pnl;
    sv += w;
    sv2 += (double)w * w;
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

// ---------------------------------------------------------------------------
// Host dispatch over the supported network shapes.
// ---------------------------------------------------------------------------
using namespace rph;

extern "C" int rph_net_nparams(int nin, int h, int nout, int head, int* p_out, int* r_out) {
  int rc = -1;
  match_shape(AllShapes{}, nin, h, nout, head, &rc, [&](auto t) {
    using S = typename decltype(t)::S;
    *p_out = S::P;
    *r_out = S::R;
    return 0;
  });
  return rc;
}

// The epoch's chunk permutation of a (ticketed or lagged) minibatch step.
static Perm step_perm(const TrainDesc* d, int epoch) {
  const uint32_t n_chunks = (uint32_t)((d->n_local + (1 << d->chunk_log2) - 1) >> d->chunk_log2);
  return make_perm(n_chunks, d->seed, (uint32_t)epoch, d->shuffle != 0);
}

extern "C" int rph_train_step(const TrainDesc* d, int step, int epoch, void* stream) {
  if (int rc = validate_train(d, 0, "rph_train_step")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Perm perm = step_perm(d, epoch);
  int rc = 0;
  if (match_shape(NarrowShapes{}, d->nin, d->h, d->nout, d->head, &rc, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_hedge_train_step<T::NIN, T::H, T::NO, T::HEAD>), dim3(d->num_wgs), dim3(256), 0, s, *d,
                           step, epoch, perm);
        return (int)hipGetLastError();
      }))
    return rc;
  return launch_wide_step(d, step, epoch, perm, s);
}

// One launch per Keras fit() (persistent kernel, hedge_fit.h); world_size 1.
extern "C" int rph_train_fit(const TrainDesc* d, int epochs, void* stream) {
  if (int rc = validate_train(d, 2, "rph_train_fit")) return rc;
  hipStream_t s = (hipStream_t)stream;
  int rc = 0;
  if (match_shape(NarrowShapes{}, d->nin, d->h, d->nout, d->head, &rc, [&](auto t) {
        using T = decltype(t);
        return launch_fit<NarrowBody<T::NIN, T::H, T::NO, T::HEAD>>(d, epochs, s);
      }))
    return rc;
  return launch_wide_fit(d, epochs, s);
}

// Lagged-update step kernel k of a fit (hedge_lag.h) and its finalize.
extern "C" int rph_train_lag_step(const TrainDesc* d, int k, int epoch, void* stream) {
  if (int rc = validate_train(d, 1, "rph_train_lag_step")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Perm perm = step_perm(d, epoch);
  int rc = 0;
  if (match_shape(NarrowShapes{}, d->nin, d->h, d->nout, d->head, &rc, [&](auto t) {
        constexpr int A = decltype(t)::NIN, B = decltype(t)::H, C = decltype(t)::NO, E = decltype(t)::HEAD;
        switch (d->variant) {  // NarrowBody<..., WPE, PFD, LDSW, HYB>
          case 1: return launch_step_lag<NarrowBody<A, B, C, E, 2>>(d, k, epoch, perm, s);
          case 2: return launch_step_lag<NarrowBody<A, B, C, E, 1, 3>>(d, k, epoch, perm, s);
          case 3: return launch_step_lag<NarrowBody<A, B, C, E, 2, 3>>(d, k, epoch, perm, s);
          case 4: return launch_step_lag<NarrowBody<A, B, C, E, 1, 1, true>>(d, k, epoch, perm, s);
          case 5: return launch_step_lag<NarrowBody<A, B, C, E, 1, 1, false, true>>(d, k, epoch, perm, s);
          default: return launch_step_lag<NarrowBody<A, B, C, E>>(d, k, epoch, perm, s);
        }
      }))
    return rc;
  return launch_wide_lag_step(d, k, epoch, perm, s);
}

extern "C" int rph_train_lag_finalize(const TrainDesc* d, int K, void* stream) {
  if (int rc = validate_train(d, 1, "rph_train_lag_finalize")) return rc;
  hipStream_t s = (hipStream_t)stream;
  return with_shape(AllShapes{}, d->nin, d->h, d->nout, d->head, "rph_train_lag_finalize", [&](auto t) {
    using T = decltype(t);
    constexpr int NREP = T::H == 8 ? NARROW_NREP : WIDE_NREP;
    hipLaunchKernelGGL((k_hedge_lag_finalize<T::S::P, T::S::R, NREP>), dim3(1), dim3(256), 0, s, *d, K);
    return (int)hipGetLastError();
  });
}

// Whole fit on the host side of the native runtime: the epochs x steps launch
// loop (lagged schedule, or ticketed steps with fused update) runs in C++ so an
// eager (non-graph) fit pays one hipLaunchKernel per step instead of a Python
// + ctypes round trip per step.  Graph capture records the same launches.
extern "C" int rph_train_lag_fit(const TrainDesc* d, int epochs, void* stream) {
  if (int rc = validate_train(d, 1, "rph_train_lag_fit")) return rc;
  int k = 0;
  for (int e = 0; e < epochs; ++e)
    for (int s = 0; s < d->steps_per_epoch; ++s, ++k)
      if (int rc = rph_train_lag_step(d, k, e, stream)) return rc;
  return rph_train_lag_finalize(d, k, stream);
}

extern "C" int rph_train_ticket_fit(const TrainDesc* d, int epochs, void* stream) {
  if (int rc = validate_train(d, 0, "rph_train_ticket_fit")) return rc;
  if (!d->fused_update) return rph_report("rph_train_ticket_fit", "needs the fused (in-kernel) update");
  for (int e = 0; e < epochs; ++e)
    for (int s = 0; s < d->steps_per_epoch; ++s)
      if (int rc = rph_train_step(d, s, e, stream)) return rc;
  return 0;
}


extern "C" int rph_train_update(const TrainDesc* d, int step, int epoch, void* stream) {
  if (!d->grad_out || !d->wts || !d->opt || !d->fit) return rph_report("rph_train_update", "null pointer");
  hipStream_t s = (hipStream_t)stream;
  return with_shape(AllShapes{}, d->nin, d->h, d->nout, d->head, "rph_train_update", [&](auto t) {
    using S = typename decltype(t)::S;
    hipLaunchKernelGGL((k_hedge_update<S::P, S::R>), dim3(1), dim3(256), 0, s, *d, step, epoch);
    return (int)hipGetLastError();
  });
}

extern "C" int rph_eval(const EvalDesc* d, void* stream) {
  if (!d->wa || !d->stats || d->n_local < 1 || d->num_wgs < 1 || d->nin < 1 || d->nin > MAXIN)
    return rph_report("rph_eval", "bad eval descriptor");
  if (!(d->alpha >= 0.f && d->alpha <= 1.f)) return rph_report("rph_eval", "LeakyReLU slope must be in [0, 1]");
  for (int f = 0; f < d->nin; ++f)
    if (!(d->fisd[f] > 0.f && d->fisd[f] < 3.0e38f && d->fmu[f] == d->fmu[f]))
      return rph_report("rph_eval", "feature standardisation must be finite with fisd > 0");
  for (int f = 0; f < d->nin; ++f)
    if (!d->feat[f]) return rph_report("rph_eval", "null feature pointer");
  hipStream_t s = (hipStream_t)stream;
  const int nhold = d->head == HEAD_COMPLEMENT ? 2 : d->nout;
  bool alias = d->nin >= nhold - 1;
  for (int k = 0; alias && k < nhold - 1; ++k) alias = d->price_t[k] == d->feat[k];
  const bool ex = d->ex_kind != EX_NONE;
  if (ex) {  // exercise date: one network, intrinsic value from price_t[0]
    if (d->ex_kind != EX_PUT && d->ex_kind != EX_CALL) return rph_report("rph_eval", "ex_kind must be 0, 1 (put) or 2 (call)");
    if (d->wb) return rph_report("rph_eval", "wb with ex_kind (early exercise takes one network)");
    if (d->g_base) return rph_report("rph_eval", "g_base with ex_kind (early exercise takes one network)");
    if (nhold < 2 || !d->price_t[0]) return rph_report("rph_eval", "price_t[0] is null with ex_kind");
    if (!(d->ex_strike == d->ex_strike) || d->ex_strike < 0.f || d->ex_strike > 3.0e38f)
      return rph_report("rph_eval", "ex_strike must be finite and >= 0");
  }
  if (d->pnl_acc) {  // folded P&L: the term needs both price rows; the stopping rule of an exercise run does not fold
    if (ex) return rph_report("rph_eval", "pnl_acc with ex_kind (the early-exercise P&L is the forward scan)");
    for (int k = 0; k < nhold - 1; ++k)
      if (!d->price_t[k] || !d->price_t1[k]) return rph_report("rph_eval", "pnl_acc needs price_t and price_t1");
    if (!(fabsf(d->pnl_grow) <= 3.0e38f) || !(fabsf(d->pnl_carry) <= 3.0e38f))
      return rph_report("rph_eval", "pnl_grow / pnl_carry must be finite");
  }
  return with_shape(AllShapes{}, d->nin, d->h, d->nout, d->head, "rph_eval", [&](auto t) {
    using T = decltype(t);
    auto launch = [&](auto pa, auto exv) {
      hipLaunchKernelGGL((k_hedge_eval<T::NIN, T::H, T::NO, T::HEAD, decltype(pa)::value, decltype(exv)::value>),
                         dim3(d->num_wgs), dim3(256), 0, s, *d);
      return (int)hipGetLastError();
    };
    if constexpr (T::NIN >= T::S::NHOLD - 1) {
      if (alias) return ex ? launch(std::true_type{}, std::true_type{}) : launch(std::true_type{}, std::false_type{});
    }
    return ex ? launch(std::false_type{}, std::true_type{}) : launch(std::false_type{}, std::false_type{});
  });
}

extern "C" int rph_pnl(const PnlDesc* d, void* stream) {
  if (int rc = validate_pnl(d, "rph_pnl")) return rc;
  const bool ex = d->ex_kind != EX_NONE;
  hipStream_t s = (hipStream_t)stream;
  return with_shape(AllShapes{}, d->nin, d->h, d->nout, d->head, "rph_pnl", [&](auto t) {
    using T = decltype(t);
    if (ex) hipLaunchKernelGGL((k_hedge_pnl<T::NIN, T::H, T::NO, T::HEAD, true>), dim3(d->num_wgs), dim3(256), 0, s, *d);
    else hipLaunchKernelGGL((k_hedge_pnl<T::NIN, T::H, T::NO, T::HEAD, false>), dim3(d->num_wgs), dim3(256), 0, s, *d);
    return (int)hipGetLastError();
  });
}

// Finish of the folded P&L (the evals accumulated PnlFinishDesc.acc): the grid
// and statistics rows of rph_pnl, so either fills the same slab.
extern "C" int rph_pnl_finish(const PnlFinishDesc* d, void* stream) {
  if (!d->acc || !d->w0 || !d->payoff || !d->stats || d->n_local < 1)
    return rph_report("rph_pnl_finish", "bad P&L finish descriptor");
  if (!(fabsf(d->carry) <= 3.0e38f)) return rph_report("rph_pnl_finish", "carry must be finite");
  const long long per_wg = 256LL * PNL_PPT;
  if ((long long)d->num_wgs * per_wg < d->n_local || (long long)(d->num_wgs - 1) * per_wg >= d->n_local)
    return rph_report("rph_pnl_finish", "num_wgs does not match n_local / (256 * PNL_PPT)");
  hipStream_t s = (hipStream_t)stream;
  return with_shape(AllShapes{}, d->nin, d->h, d->nout, d->head, "rph_pnl_finish", [&](auto) {
    hipLaunchKernelGGL(k_pnl_finish, dim3(d->num_wgs), dim3(256), 0, s, *d);
    return (int)hipGetLastError();
  });
}
