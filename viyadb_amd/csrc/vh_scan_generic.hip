// Generic scan kernel instantiations (any element type, any number of predicate columns).
#include "vh_kernels.h"
#include "vh_launch.h"

template <int MODE, int BLOCK>
static void launch(const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private) {
  vh_with_scope(xcd_private, [&](auto scope) {
    constexpr int SCOPE = decltype(scope)::value;
    L.named("scan_agg_kernel<%d, %d, %d>", MODE, BLOCK, SCOPE);
    vh_launch_or_ask(L, scan_agg_kernel<MODE, BLOCK, SCOPE>, BLOCK, false, P);      // (the occupancy is not asked: the host's default of blocks per CU)
  });
}

void vh_launch_scan_generic(int mode, const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private) {
  if (mode == VH_MODE_DENSE_LDS) launch<VH_MODE_DENSE_LDS, 1024>(P, L, xcd_private);
  else if (mode == VH_MODE_DENSE_GLOBAL) launch<VH_MODE_DENSE_GLOBAL, 256>(P, L, xcd_private);
  else launch<VH_MODE_HASH, 256>(P, L, false);
}
