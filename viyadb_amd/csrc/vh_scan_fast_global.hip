// Fast scan kernel instantiations: dense per-XCD tables in HBM/L2.
#include "vh_kernels.h"
#include "vh_launch.h"

void vh_launch_scan_fast_global(const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private) {
  vh_with_scope(xcd_private, [&](auto scope) { vh_with_np(P.npred, [&](auto np) {
    constexpr int SCOPE = decltype(scope)::value, NP = decltype(np)::value;
    L.named("scan_agg_fast_kernel<%d, %d, %d, %d>", VH_MODE_DENSE_GLOBAL, 256, SCOPE, NP);
    vh_launch_or_ask(L, scan_agg_fast_kernel<VH_MODE_DENSE_GLOBAL, 256, SCOPE, NP>, 256, true, P);
  }); });
}
