// vh_batch.h — which members of a batch of aggregates (vh_query_agg_batch, include/viya_hip.h) share ONE fused launch of
// scan_agg_planes_batch_kernel (vh_scan_planes_batch.hip). Plain C++ without a dependency, like vh_sliced_walk.h: the host includes it
// (vhh_finalize.h), and a host-compiled check runs it over hand-made and random lists (tests/batch_fuse_host.cc).
//
// A member is a CANDIDATE when QueryBuild::choose_plane_agg made its plan `plane_agg` (vhh_launch.h: that rule is the single query's, unchanged).
// Candidates with the same FUSE KEY can share a walk and a load of the value planes: the projection V (its serial), the memory scope of the
// table updates (a private copy per XCD or not), the segments of the snapshot and the chunks per segment. Members are taken in plan order; a
// group holds at most VH_BATCH_MAX members and VH_BATCH_LDS_CAP bytes of LDS tables, and the candidate that would pass either opens the
// next group of its key. A group that ends up with one member is no group: that member runs as the single query it is.
#pragma once
#include <stdint.h>

#ifndef VH_BATCH_MAX
#define VH_BATCH_MAX 8                        // (include/viya_hip.h says the same)
#endif
#define VH_BATCH_LDS_CAP (48u * 1024u)        // dynamic LDS of one fused launch: the members' tables, each rounded up to 16 bytes by the host

struct VhFuseDesc {
  uint32_t candidate;          // 0: never grouped
  uint32_t scope;              // 1: the table has a private copy per XCD (workgroup-scope updates)
  uint64_t v_serial;           // VhLayout::serial of the projection V
  uint32_t nseg, chunks_per_seg;
  uint32_t lds_bytes;          // the member's LDS table
};
static inline bool vh_fuse_same_key(const VhFuseDesc& a, const VhFuseDesc& b) {
  return a.v_serial == b.v_serial && a.scope == b.scope && a.nseg == b.nseg && a.chunks_per_seg == b.chunks_per_seg;
}
// group_of[i]: the group of member i, numbered from 0 in the order of the groups' first members, or -1 — the member is answered singly.
// Returns the number of groups.
static inline uint32_t vh_batch_group(const VhFuseDesc* d, uint32_t n, int32_t* group_of) {
  for (uint32_t i = 0; i < n; ++i) group_of[i] = -1;
  uint32_t ngroups = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!d[i].candidate || group_of[i] >= 0) continue;
    // member i opens a group; the later candidates of its key join while the caps hold, the first that does not fit opens the next one
    uint32_t members = 1, lds = d[i].lds_bytes;
    for (uint32_t k = i + 1; k < n; ++k) {
      if (!d[k].candidate || group_of[k] >= 0 || !vh_fuse_same_key(d[i], d[k])) continue;
      if (members == VH_BATCH_MAX || (uint64_t)lds + d[k].lds_bytes > VH_BATCH_LDS_CAP) break;
      group_of[k] = (int32_t)ngroups; ++members; lds += d[k].lds_bytes;
    }
    if (members > 1) group_of[i] = (int32_t)ngroups++;      // (else a lone candidate: it stays -1, and no later opener looks back at it)
  }
  return ngroups;
}
