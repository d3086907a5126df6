// Fast scan kernel instantiations: open-addressing hash table in HBM.
#include "vh_kernels.h"
#include "vh_launch.h"

void vh_launch_scan_fast_hash(const VhPlanDev& P, const VhScanLaunch& L) {
  vh_with_np(P.npred, [&](auto np) {
    constexpr int NP = decltype(np)::value;
    L.named("scan_agg_fast_kernel<%d, %d, %d, %d>", VH_MODE_HASH, 256, __HIP_MEMORY_SCOPE_AGENT, NP);
    vh_launch_or_ask(L, scan_agg_fast_kernel<VH_MODE_HASH, 256, __HIP_MEMORY_SCOPE_AGENT, NP>, 256, true, P);
  });
}
