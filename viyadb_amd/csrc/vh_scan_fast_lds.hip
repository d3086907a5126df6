// Fast scan kernel instantiations: dense table in LDS (1024-thread blocks).
#include "vh_kernels.h"
#include "vh_launch.h"

void vh_launch_scan_fast_lds(const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private) {
  vh_with_scope(xcd_private, [&](auto scope) { vh_with_np(P.npred, [&](auto np) {
    constexpr int SCOPE = decltype(scope)::value, NP = decltype(np)::value;
    L.named("scan_agg_fast_kernel<%d, %d, %d, %d>", VH_MODE_DENSE_LDS, 1024, SCOPE, NP);
    vh_launch_or_ask(L, scan_agg_fast_kernel<VH_MODE_DENSE_LDS, 1024, SCOPE, NP>, 1024, false, P);      // (one block per CU: the occupancy is not asked)
  }); });
}
