// Fast scan kernel instantiations: radix-partitioned tuples (phase 1) + LDS aggregation (phase 2).
#include "vh_kernels.h"
#include "vh_launch.h"

template <int SHAPE>
static void launch_np(const VhPlanDev& P, const VhScanLaunch& L) {
  vh_with_np(P.npred, [&](auto np) {
    constexpr int NP = decltype(np)::value, MODE = VH_MODE_DENSE_PART, SCOPE = __HIP_MEMORY_SCOPE_AGENT;
    if constexpr (SHAPE != 0) {      // the drain specialised for the plan's shape (VhPlanDev::shape)
      L.named("scan_agg_shape_kernel<%d, %d, %d, %d, %d>", MODE, 256, SCOPE, NP, SHAPE);
      vh_launch_or_ask(L, scan_agg_shape_kernel<MODE, 256, SCOPE, NP, SHAPE>, 256, true, P);
    } else {
      L.named("scan_agg_fast_kernel<%d, %d, %d, %d>", MODE, 256, SCOPE, NP);
      vh_launch_or_ask(L, scan_agg_fast_kernel<MODE, 256, SCOPE, NP>, 256, true, P);
    }
  });
}

void vh_launch_scan_fast_part(const VhPlanDev& P, const VhScanLaunch& L) {
  if (P.shape == 1) launch_np<1>(P, L);
  else if (P.shape == 2) launch_np<2>(P, L);
  else launch_np<0>(P, L);
}

void vh_launch_part_agg(const VhPlanDev& P, int blocks_per_part, size_t lds, hipStream_t s) {
  if (lds > 64 * 1024)   // a workgroup may own up to 160 KB of LDS on gfx950, but dynamic LDS above 64 KB has to be asked for
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&part_agg_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((part_agg_kernel<1024>), dim3(P.nfine * blocks_per_part), dim3(1024), lds, s, P, blocks_per_part);
}
const char* vh_part_agg_name() { return "part_agg_kernel<1024>"; }

// part_split_ring_kernel's second template argument: the bytes of a tuple — four-byte and one-word tuples (VhPlanDev::gid_bits), or two words
static int split_tuple_bytes(const VhPlanDev& P) { return P.tw == 1 && P.tuple4 ? 4 : P.tw == 1 ? 8 : 16; }

// Two levels: size the partitions' slices of pool 2 from what phase 1 wrote, then split every partition 64 ways.
void vh_launch_part_split(const VhPlanDev& P, int blocks_per_part, bool ring, hipStream_t s) {
  if (ring && vh_part_split_rings(P) && P.ext_tuples2 == VH_SPLIT_TILE_TUPLES) {      // extents by position, no barriers (part_split_ring_kernel)
    hipLaunchKernelGGL((part_l2_count_kernel<256>), dim3(256), dim3(256), 0, s, P);
    hipLaunchKernelGGL((part_l2_plan_kernel<64>), dim3(1), dim3(64), 0, s, P, blocks_per_part, blocks_per_part);
    const int bytes = split_tuple_bytes(P);
    if (bytes == 4) hipLaunchKernelGGL((part_split_ring_kernel<256, 4>), dim3(P.npart * blocks_per_part), dim3(256), VH_SPLIT_RING_LDS(256), s, P, blocks_per_part);
    else if (bytes == 8) hipLaunchKernelGGL((part_split_ring_kernel<256, 8>), dim3(P.npart * blocks_per_part), dim3(256), VH_SPLIT_RING_LDS(256), s, P, blocks_per_part);
    else hipLaunchKernelGGL((part_split_ring_kernel<256, 16>), dim3(P.npart * blocks_per_part), dim3(256), VH_SPLIT_RING_LDS(256), s, P, blocks_per_part);
    return;
  }
  hipLaunchKernelGGL((part_l2_count_kernel<256>), dim3(256), dim3(256), 0, s, P);
  hipLaunchKernelGGL((part_l2_plan_kernel<64>), dim3(1), dim3(64), 0, s, P, blocks_per_part * 4, 0);
  hipLaunchKernelGGL((part_split_kernel<256>), dim3(P.npart * blocks_per_part), dim3(256), 0, s, P, blocks_per_part);
}
std::string vh_part_split_name(const VhPlanDev& P) {
  return vh_part_split_rings(P) ? "part_split_ring_kernel<256, " + std::to_string(split_tuple_bytes(P)) + ">" : std::string("part_split_kernel<256>");
}
