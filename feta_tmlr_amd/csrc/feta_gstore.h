// Cache policy of the global stores of the training step's kernels, one per CLASS of tensor.
//
// At the end of a kernel the dirty lines of all eight XCD L2s are written back before the next kernel may start; what
// a launch stores and never reads again can leave for the memory side while the launch still runs (feta_device.h:
// kStWt).  The classes:
//   SAVED    written in the forward, read in the backward or returned: qkv, out, attn, attn_stats, h, cj / pooled, A / Bm
//   PARTIAL  split-K and statistics rows, final gradients: the FIRST store of a partial row (acc_to), dW / db, colsum
//   HANDOFF  rows the next launch reads: y1 / y2 / y_stats / sum_out / dx / dx_b, filt, the encoder output
// A class is write-through by default only where the headline measured faster with it (EXPERIMENTS.md, "Write-through
// stores"): SAVED and PARTIAL are, HANDOFF lost and is plain.  Never write-through: anything a launch reads back itself
// (the accumulate path of acc_to, running statistics, num_batches_tracked), LDS, spec_cat_bwd_graph_kernel (registers:
// filter.hip) and the streaming spec_fwd / spec_bwd_graph_kernel.
//
// Each class is a compile-time constant so that it can be A/B'd with -DFETA_ST_<CLASS>=0|1|2 (build.py: FETA_HIPCC_FLAGS).
#pragma once
#include <feta_device.h>

#ifndef FETA_ST_SAVED
#define FETA_ST_SAVED 1
#endif
#ifndef FETA_ST_PARTIAL
#define FETA_ST_PARTIAL 1
#endif
#ifndef FETA_ST_HANDOFF
#define FETA_ST_HANDOFF 0
#endif
#ifndef FETA_ST_BF16      // 1: the classes' policies also on tensors in bf16 storage (feta_lp.h); 0: those stay plain
#define FETA_ST_BF16 0
#endif

namespace feta {

constexpr int kStSaved = FETA_ST_SAVED, kStPartial = FETA_ST_PARTIAL, kStHandoff = FETA_ST_HANDOFF;

// fp32, GLOBAL memory: one element / four consecutive elements (16-byte aligned) of a lane
template <int POL>
__device__ __forceinline__ void gst1(float* p, float v) {
  gst_b32<POL>(p, v);
}
template <int POL>
__device__ __forceinline__ void gst2(float* p, float a, float b) {   // 8-byte aligned
  const float t[2] = {a, b};
  unsigned long long u;
  __builtin_memcpy(&u, t, 8);
  gst_b64<POL>(p, u);
}
template <int POL>
__device__ __forceinline__ void gst4(float* p, float a, float b, float c, float d) {
  f32x4 v;
  v[0] = a; v[1] = b; v[2] = c; v[3] = d;
  gst_b128<POL>(p, v);
}

}  // namespace feta
