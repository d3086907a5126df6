// vh_batch.h — which members of a batch of aggregates (vh_query_agg_batch, include/viya_hip.h) share ONE fused launch of
// scan_agg_planes_batch_kernel (vh_scan_planes_batch.hip). Plain C++ without a dependency, like vh_sliced_walk.h: the host includes it
// (vhh_finalize.h), and a host-compiled check runs it over hand-made and random lists (tests/batch_fuse_host.cc).
//
// A member is a CANDIDATE when QueryBuild::choose_plane_agg made its plan `plane_agg` (vhh_launch.h: that rule is the single query's, unchanged).
// Candidates with the same FUSE KEY can share a walk and a load of the value planes: the projection V (its serial), the memory scope of the
// table updates (a private copy per XCD or not), the segments of the snapshot and the chunks per segment. Members are taken in plan order; a
// group holds at most VH_BATCH_MAX members and VH_BATCH_LDS_CAP bytes of LDS tables, and the candidate that would pass either opens the
// next group of its key. A group that ends up with one member is no group: that member runs as the single query it is.
// A COMPILED candidate — a member that asked for the compiled plane aggregate and has its own kernel at hand (VH_PLAN2_PLANE_JIT: vhh_launch.h,
// compile_plane_agg) — groups with compiled candidates only, and a pre-built one with pre-built ones: `compiled` is part of the key. A
// compiled group is answered by ONE kernel compiled for its BATCH SHAPE, the ordered list of its members' shapes (vh_jit_planes_batch.h).
//
// Within ONE group, members whose pass masks are equal by construction share ONE evaluation of the mask per plane word (vh_batch_share below:
// the MASK KEY): the dashboard's shape, K breakdowns under one filter.
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
  uint32_t compiled;           // 1: a compiled candidate (its own compiled kernel is at hand)
};
static inline bool vh_fuse_same_key(const VhFuseDesc& a, const VhFuseDesc& b) {
  return a.v_serial == b.v_serial && a.scope == b.scope && a.nseg == b.nseg && a.chunks_per_seg == b.chunks_per_seg && (a.compiled != 0) == (b.compiled != 0);
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

// ---- which members of ONE fused group share a pass mask
// The kernel evaluates a member's mask of a plane word from its filter program over its projection F, cut at its snapshot. Two members get
// the same word whenever all of that is the same, and then the later one takes the earlier one's word instead of running the interpreter
// again. The MASK KEY, compared part by part (only what the kernel reads: the staging need not zero-fill the rest):
//   - both have a filter, or both have none;
//   - with a filter: the same projection F (its layout serial, and where its planes lie: address, stride, pitch); the same program as staged
//     (nprog, flat, the nprog ops, and every literal an op refers to — a REL leaf one, an IN leaf `count` of them); no set leaf in either: a
//     set leaf's truth table lies behind a pointer into the member's own plan block, so such a program is always a class of its own;
//   - the same effective rows in every segment (the snapshot, 0 for a skipped segment: what the planner uploads as VhPlanDev::seg_rows). One
//     row fewer in one segment is another class: the kernel takes the leader's word as it is, the cut at the snapshot included;
//   - in a COMPILED group, the same filter member-shape (filter_shape: a number the host gives equal filter texts — the program, the fields'
//     places in F and the leaves' types as the generator sees them): the leader's evaluation is then the text this member would have had.
// The op's words are those of VhBitsOp (vh_bits_eval.h), restated here because this file includes nothing: kind = w0 & 0xFF, count = w0 >> 24,
// first literal = w1 & 0xFFFF; the kinds are enum vh_fkind's (include/viya_hip.h). vhh_finalize.h asserts that both still agree.
#define VH_SHARE_KIND_REL 1u
#define VH_SHARE_KIND_IN 2u
#define VH_SHARE_KIND_INSET 5u
struct VhShareDesc {
  uint32_t has_filter;         // VhPlaneAggDesc::has_filter; 0: everything up to `lits` is ignored
  uint64_t f_serial;           // VhLayout::serial of the projection F
  uint64_t f_planes, f_stride, f_pitch;      // VhSlicedPlanes of F (the address as a number)
  int32_t nprog, flat;         // VhBitsProg::nprog, ::flat
  const uint32_t* ops;         // nprog ops of two words each (w0, w1)
  const uint64_t* lits;        // the program's literals
  uint32_t nlits;              // ... and how many there are room for (an op that points beyond them never shares)
  uint32_t nseg;
  const uint32_t* seg_rows;    // nseg words: the effective rows per segment
  uint32_t filter_shape;       // compiled groups: equal numbers for equal filter member-shapes (0 throughout a pre-built group)
};
static inline uint32_t vh_share_op_lits(uint32_t w0) {      // literals the op refers to, from `w1 & 0xFFFF` on
  const uint32_t kind = w0 & 0xFFu;
  return kind == VH_SHARE_KIND_REL ? 1u : kind == VH_SHARE_KIND_IN ? w0 >> 24 : 0u;
}
// false: a set leaf, or an op whose literals do not lie within `lits` — a program nobody shares with
static inline bool vh_share_prog_plain(const VhShareDesc& a) {
  if (a.nprog < 0) return false;
  for (int32_t k = 0; k < a.nprog; ++k) {
    const uint32_t w0 = a.ops[2 * k], w1 = a.ops[2 * k + 1];
    if ((w0 & 0xFFu) == VH_SHARE_KIND_INSET) return false;
    if ((uint64_t)(w1 & 0xFFFFu) + vh_share_op_lits(w0) > a.nlits) return false;
  }
  return true;
}
static inline bool vh_share_same_key(const VhShareDesc& a, const VhShareDesc& b) {
  if ((a.has_filter != 0) != (b.has_filter != 0)) return false;
  if (a.filter_shape != b.filter_shape) return false;
  if (a.nseg != b.nseg) return false;
  for (uint32_t s = 0; s < a.nseg; ++s) if (a.seg_rows[s] != b.seg_rows[s]) return false;
  if (!a.has_filter) return true;
  if (a.f_serial != b.f_serial || a.f_planes != b.f_planes || a.f_stride != b.f_stride || a.f_pitch != b.f_pitch) return false;
  if (a.nprog != b.nprog || a.flat != b.flat) return false;
  if (!vh_share_prog_plain(a) || !vh_share_prog_plain(b)) return false;
  for (int32_t k = 0; k < a.nprog; ++k) {
    if (a.ops[2 * k] != b.ops[2 * k] || a.ops[2 * k + 1] != b.ops[2 * k + 1]) return false;
    const uint32_t first = a.ops[2 * k + 1] & 0xFFFFu, cnt = vh_share_op_lits(a.ops[2 * k]);
    for (uint32_t i = 0; i < cnt; ++i) if (a.lits[first + i] != b.lits[first + i]) return false;
  }
  return true;
}
// members[0 .. cnt): the group's members in launch order, as indices into d. mask_of[k]: the position in the launch of the first member whose
// pass mask member k may use; == k: it evaluates its own. Always mask_of[k] <= k and mask_of[mask_of[k]] == mask_of[k]. Returns the number of
// classes (the masks the launch evaluates per plane word).
static inline uint32_t vh_batch_share(const VhShareDesc* d, const uint32_t* members, uint32_t cnt, uint32_t* mask_of) {
  uint32_t classes = 0;
  for (uint32_t k = 0; k < cnt; ++k) {
    mask_of[k] = k;
    for (uint32_t j = 0; j < k; ++j)
      if (mask_of[j] == j && vh_share_same_key(d[members[j]], d[members[k]])) { mask_of[k] = j; break; }
    if (mask_of[k] == k) ++classes;
  }
  return classes;
}
