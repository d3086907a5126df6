// "Lanes" scan kernel instantiations (no compaction): dense table in LDS, the hash path's LDS front table, and
// phase 1 of the radix-partitioned aggregation.
#include "vh_kernels.h"
#include "vh_launch.h"

template <int MODE, int BLOCK, int SCOPE>
static void launch_np(const VhPlanDev& P, const VhScanLaunch& L) {
  vh_with_np(P.npred, [&](auto np) {
    constexpr int NP = decltype(np)::value;
    L.named("scan_agg_lanes_kernel<%d, %d, %d, %d>", MODE, BLOCK, SCOPE, NP);
    vh_launch_or_ask(L, scan_agg_lanes_kernel<MODE, BLOCK, SCOPE, NP>, BLOCK, true, P);
  });
}
template <int BLOCK>
static void launch_lds(const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private) {
  vh_with_scope(xcd_private, [&](auto scope) { launch_np<VH_MODE_DENSE_LDS, BLOCK, decltype(scope)::value>(P, L); });
}

void vh_launch_scan_lanes_lds(const VhPlanDev& P, int block, const VhScanLaunch& L, bool xcd_private) {
  if (block == 256) launch_lds<256>(P, L, xcd_private);
  else if (block == 512) launch_lds<512>(P, L, xcd_private);
  else launch_lds<1024>(P, L, xcd_private);
}
void vh_launch_scan_lanes_hash(const VhPlanDev& P, const VhScanLaunch& L) { launch_np<VH_MODE_HASH, 256, __HIP_MEMORY_SCOPE_AGENT>(P, L); }
void vh_launch_scan_lanes_part(const VhPlanDev& P, const VhScanLaunch& L) { launch_np<VH_MODE_DENSE_PART, 256, __HIP_MEMORY_SCOPE_AGENT>(P, L); }
