// nabo_tree.h -- the libnabo kd-tree of nn_mode = SMHIP_NN_NABO as the host sees it: the arrays a handle owns and the
// constants the launch plan restates.  Built and walked by nabo_kernels.hip; held in smhip_context (smhip_context.h).
#pragma once
#include "kd_median_tree.h"

namespace smhip {

constexpr int kKdBucket = 8;              // libnabo's default bucketSize
constexpr int kKdStack = 18;              // pending siblings per query: at most one per tree level (18 levels: > 1 M target points; node < 2^23)
constexpr int kNaboListedBlocks = 96;     // workgroups per pair striding over the lists of queries to walk again (32: -2 %, 64: -1 %, 128: equal)
constexpr int kKdTopNodes = 511;          // tree levels 0..8 staged in LDS by the search kernel (4 KiB)

struct KdDev {
  uint2* nodes;        // [slots][kd_node_cap]  inner: {cut value bits, (left child << 2) | dim}; leaf: {first, (count << 2) | 3}
  KdSeg* segs;         // [slots][2][kd_seg_cap]
  float4* alt;         // [slots][nt_cap]       second working order (ping-pong with tq)
  uint32_t* cnt;       // [slots][2 * seg_cap]  left / right fill counters of a level with more segments than LDS holds
  float* leaf;         // [slots][leaf_cap][24]  the buckets again, as the search scans them: x[8] y[8] z[8] of the bucket that starts at
                       //                        tq position `first` in block first >> 2 (a bucket of a split cloud holds >= 4 points, so
                       //                        blocks are unique), unused entries = +inf (their distance is +inf: never a candidate)
  int32_t node_cap, seg_cap, leaf_cap;
  float max_error2;    // (1 + epsilon)^2
};

}  // namespace smhip
