// rphedge — the self-financing hedge P&L scan under proportional transaction
// costs with a no-trade band, for gfx950 (CostPnlDesc, rph_types.h):
// k_hedge_pnl_cost is the COST instantiation of pnl_scan (pnl_scan.h), the body
// of k_hedge_pnl, over the same shape table.  Its P&L and wealth rows go to
// p.stats exactly as k_hedge_pnl writes them, the cost rows to c.cstats.
#include "pnl_scan.h"

namespace rph {

template <int NIN, int H, int NO, int HEAD>
__global__ __launch_bounds__(256) void k_hedge_pnl_cost(const CostPnlDesc d) {
  prefetch_kernarg<sizeof(CostPnlDesc)>();
  pnl_scan<NIN, H, NO, HEAD, false, true>(d.p, &d.c);
}

}  // namespace rph

using namespace rph;

// rph_pnl's checks on the embedded descriptor, then the cost terms'; the band
// makes the position path-dependent, which the stopping rule's scan is not built for.
static int validate_pnl_cost(const CostPnlDesc* d, const char* who) {
  if (int rc = validate_pnl(&d->p, who)) return rc;
  if (int rc = validate_cost(&d->c, who)) return rc;
  if (d->p.ex_kind != EX_NONE) return rph_report(who, "ex_kind with costs (early exercise with costs is not supported)");
  return 0;
}

// The checks of rph_pnl_cost without the launch (and without a device).
extern "C" int rph_pnl_cost_check(const CostPnlDesc* d) { return validate_pnl_cost(d, "rph_pnl_cost"); }

extern "C" int rph_pnl_cost(const CostPnlDesc* d, void* stream) {
  if (int rc = validate_pnl_cost(d, "rph_pnl_cost")) return rc;
  hipStream_t s = (hipStream_t)stream;
  return with_shape(AllShapes{}, d->p.nin, d->p.h, d->p.nout, d->p.head, "rph_pnl_cost", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_hedge_pnl_cost<T::NIN, T::H, T::NO, T::HEAD>), dim3(d->p.num_wgs), dim3(256), 0, s, *d);
    return (int)hipGetLastError();
  });
}
