// Graph-level readout of an evaluation batch in one launch (feta_readout_eval, include/feta_hip.h): what the task shells
// run after the encoder - masked mean pooling and the two-layer classifier (transformer/models.py, a dozen small library
// launches) - plus the per-graph loss and metric terms of train._evaluate.  Forward only.  Results go to split-level
// buffers indexed by the STORE id of the graph in the slot, and the number of live slots is read from device memory, so
// one captured launch serves every batch length up to B (train.StoreEvalStep).
//
// One workgroup of 256 lanes per slot.  Latency bound: at most N x 64 floats of rows, a 64 x 64 and a C x 64 matrix-vector
// product per graph; every operand is read once, 16 bytes per lane where it is aligned.
//   pooling   lane t owns columns [4 (t & 15), +4) of the rows t >> 4, t >> 4 + 16, ... (one row is 16 lanes = 256 bytes);
//             the 16 partial rows meet in LDS and lanes 0..63 add them in row-slot order
//   products  lane t owns a quarter of output t >> 2: the 16-byte pieces (t & 3) + 4 j of the weight row, so that the four
//             lanes of an output read 64 contiguous bytes per step; the quarters meet through two wave shuffles
//   terms     lane 0, serially over the C logits
// No atomics and one summation order: a result depends on the graph's own rows and the weights only, not on the batch
// it was evaluated in, and two launches are bit-equal.  Every result is written by the workgroup of its slot alone.
//
// The readout of a TRAINING batch (feta_readout_train_fwd / _bwd) is the same per-slot arithmetic - the phases below are
// shared - with the batch loss, its backward and the parameter gradients, in four launches:
//   readout_train_fwd_kernel   one workgroup per slot: scores by slot; pooled, the pre-activation z, the unscaled dlogit
//                              and (term, weight) into the workspace row of the slot
//   readout_train_loss_kernel  one workgroup: sum of the terms / sum of the weights over the live slots
//   readout_train_bwd_kernel   one workgroup per slot: dl = s dlogit, dz = (W2^T dl) act'(z), dpooled = W1^T dz, dy.  The
//                              transposed products walk a COLUMN of the weights: lane t owns column t & 63 of the rows
//                              t >> 6, t >> 6 + 4, ..., so the 64 lanes of a wave read one 256-byte row per step, and the four
//                              partial sums meet in LDS in wave order.  dy is written whole: zeros in the padded rows and
//                              in every row of a slot from *count on
//   readout_train_dw_kernel    the four parameter gradients, 16 output rows (64 columns each, plus their bias gradient) per
//                              workgroup; the slots are walked in ascending order in chunks of 64 staged in LDS, the next
//                              chunk's loads in flight while the current one is contracted
// Stores follow feta_gstore.h: scores, the saved part of the workspace (SAVED), the parameter gradients (PARTIAL), what
// the next launch reads - (term, weight), the loss, dl, dz, dy - (HANDOFF).
#include <cmath>

#include <feta_device.h>

#include "feta_abi_common.h"
#include "feta_gstore.h"

namespace feta {

constexpr int kReadoutThreads = 256, kReadoutD = 64, kReadoutSlots = kReadoutThreads / 16;
// LDS, in floats: the partial rows of the pooling, then pooled, h and the logits
constexpr int kReadoutLdsPooled = kReadoutSlots * kReadoutD, kReadoutLdsH = kReadoutLdsPooled + kReadoutD,
              kReadoutLdsLogit = kReadoutLdsH + kReadoutD, kReadoutLdsFloats = kReadoutLdsLogit + kReadoutD;
enum { kReadoutVecY = 1, kReadoutVecW1 = 2, kReadoutVecW2 = 4, kReadoutVecTerms = 8, kReadoutVecDy = 16 };

struct ReadoutArgs {
  feta_readout d;
  int vec;   // kReadoutVec* bits: strides and base pointers allow 16-byte accesses
};

__device__ __forceinline__ float4 readout_ld4(const float* p, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

// out[o] = sum_k w[o, k] x[k] for the lane's output o = t >> 2 (o < rows; the other lanes add zeros): every lane of a
// wave takes part in the shuffles, and the four lanes of an output end with the same sum
__device__ __forceinline__ float readout_dot(const float* w, const float* x, int rows, bool vec) {
  const int o = threadIdx.x >> 2, q = threadIdx.x & 3;
  float s = 0.0f;
  if (o < rows) {
#pragma unroll
    for (int j = 0; j < kReadoutD / 16; ++j) {
      const int k = 4 * (q + 4 * j);
      const float4 a = readout_ld4(w + o * kReadoutD + k, vec);
      s += a.x * x[k] + a.y * x[k + 1] + a.z * x[k + 2] + a.w * x[k + 3];
    }
  }
  s += shfl_xor(s, 1);
  s += shfl_xor(s, 2);
  return s;
}

// pooled[0..64) (LDS) = mean of the n real rows of the slot whose first row starts at `rows`; every lane of the workgroup
// calls it, and pooled is visible to all of them afterwards
__device__ __forceinline__ void readout_pool(const float* rows, int64_t row_sn, int n, bool vec, float* part, float* pooled) {
  const int t = threadIdx.x;
  {
    const int c = 4 * (t & 15), slot = t >> 4;
    const float* col = rows + c;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = slot; i < n; i += kReadoutSlots) {
      const float4 v = readout_ld4(col + (int64_t)i * row_sn, vec);
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
    float* p = part + slot * kReadoutD + c;
    p[0] = s.x;
    p[1] = s.y;
    p[2] = s.z;
    p[3] = s.w;
  }
  lds_barrier();
  if (t < kReadoutD) {
    float s = 0.0f;
    for (int slot = 0; slot < kReadoutSlots; ++slot) s += part[slot * kReadoutD + t];
    pooled[t] = s / (float)n;
  }
  lds_barrier();
}

// w x + bias for the lane's output t >> 2 (readout_dot); the value of the lanes with (t & 3) == 0 and t >> 2 < rows counts
__device__ __forceinline__ float readout_affine(const float* w, const float* bias, const float* x, int rows, bool vec) {
  const int t = threadIdx.x;
  float v = readout_dot(w, x, rows, vec);
  if ((t & 3) == 0 && (t >> 2) < rows && bias) v += bias[t >> 2];
  return v;
}

__device__ __forceinline__ float readout_act(float v, float slope) { return v > 0.0f ? v : slope * v; }

// the four terms of one slot (include/feta_hip.h) from its logits in LDS, one lane; m and s: the row maximum and the sum of
// exp(logit - m) of FETA_LOSS_CE (softmax[c] = exp(logit[c] - m) / s)
__device__ __forceinline__ float4 readout_terms(const float* logit, int C, int loss_kind, float label, int64_t cls, float& m,
                                                float& s) {
  float4 out = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  m = 0.0f;
  s = 1.0f;
  if (loss_kind == FETA_LOSS_L1) {
    const float e = logit[0] - label;
    out.x = fabsf(e);
    out.y = e * e;
  } else if (loss_kind == FETA_LOSS_BCE_LOGITS) {
    // (1 - y) x - log sigmoid(x), with log sigmoid(x) = min(x, 0) - log1p(exp(-|x|)): F.binary_cross_entropy_with_logits
    const float x = logit[0];
    const bool labelled = label == label;
    out.x = labelled ? (1.0f - label) * x + fmaxf(-x, 0.0f) + log1pf(expf(-fabsf(x))) : 0.0f;
    out.y = (x > 0.0f) == (label > 0.5f) ? 1.0f : 0.0f;
    out.w = labelled ? 1.0f : 0.0f;
  } else {
    // -log softmax[label] as log-sum-exp with the row maximum subtracted (F.cross_entropy); the first index wins a tie
    int best = 0;
    m = logit[0];
    for (int c = 1; c < C; ++c)
      if (logit[c] > m) {
        m = logit[c];
        best = c;
      }
    s = 0.0f;
    for (int c = 0; c < C; ++c) s += expf(logit[c] - m);
    const bool known = cls >= 0 && cls < C;     // (a label outside the classes: NaN, as a loss nobody defined)
    out.x = known ? m + logf(s) - logit[known ? cls : 0] : NAN;
    out.y = known && best == (int)cls ? 1.0f : 0.0f;
  }
  return out;
}

// the label of slot b as (float, class index)
__device__ __forceinline__ void readout_label(const void* labels, int label_kind, int b, float& label, int64_t& cls) {
  cls = 0;
  if (label_kind == FETA_LABELS_GRAPH_F32) {
    label = reinterpret_cast<const float*>(labels)[b];
  } else {
    cls = reinterpret_cast<const int64_t*>(labels)[b];
    label = (float)cls;
  }
}

__global__ __launch_bounds__(kReadoutThreads) void readout_eval_kernel(ReadoutArgs a) {
  const feta_readout& d = a.d;
  const int b = blockIdx.x, t = threadIdx.x;
  // (all three conditions are uniform over the workgroup: nobody is left behind at a barrier)
  if (b >= *d.count) return;
  const int g = d.ids[b], n = d.n_real[b];
  if (g < 0 || g >= d.G || n <= 0 || n > d.N) return;
  float* part = feta_lds;
  float* pooled = feta_lds + kReadoutLdsPooled;
  float* h = feta_lds + kReadoutLdsH;
  float* logit = feta_lds + kReadoutLdsLogit;

  // masked mean over the n real rows
  readout_pool(d.y + (int64_t)b * d.row_sb, d.row_sn, n, (a.vec & kReadoutVecY) != 0, part, pooled);
  {   // h = act(W1 pooled + b1)
    const float v = readout_affine(d.w1, d.b1, pooled, kReadoutD, (a.vec & kReadoutVecW1) != 0);
    if ((t & 3) == 0) h[t >> 2] = readout_act(v, d.slope);
  }
  lds_barrier();
  {   // logits = W2 h + b2
    const float v = readout_affine(d.w2, d.b2, h, d.C, (a.vec & kReadoutVecW2) != 0);
    if ((t & 3) == 0 && (t >> 2) < d.C) {
      logit[t >> 2] = v;
      d.scores[(int64_t)g * d.C + (t >> 2)] = v;
    }
  }
  lds_barrier();
  if (t != 0) return;

  float label, m, s;
  int64_t cls;
  readout_label(d.labels, d.label_kind, b, label, cls);
  const float4 out = readout_terms(logit, d.C, d.loss_kind, label, cls, m, s);
  float* row = d.terms + (int64_t)g * 4;
  if (a.vec & kReadoutVecTerms) {
    *reinterpret_cast<float4*>(row) = out;
  } else {
    row[0] = out.x;
    row[1] = out.y;
    row[2] = out.z;
    row[3] = out.w;
  }
}

// ---- training ---------------------------------------------------------------------------------------------------------

// workspace row of a slot, in floats (a multiple of 4: every piece of every row is 16-byte aligned)
constexpr int kRtPooled = 0, kRtZ = kReadoutD, kRtDlogit = 2 * kReadoutD, kRtDz = 3 * kReadoutD, kRtDl = 4 * kReadoutD,
              kRtTerm = 5 * kReadoutD, kRtRow = kRtTerm + 4;
// the parameter-gradient launch: output rows per workgroup, slots per staged chunk; LDS: the left factors [chunk][rows],
// then the right factors [chunk][64]
constexpr int kRtTile = 16, kRtChunk = 64, kRtLdsRight = kRtChunk * kRtTile,
              kRtDwLdsFloats = kRtLdsRight + kRtChunk * kReadoutD;

struct ReadoutTrainArgs {
  feta_readout_train d;
  int vec;
};

__device__ __forceinline__ bool readout_slot_ok(int n, int N) { return n >= 1 && n <= N; }

__global__ __launch_bounds__(kReadoutThreads) void readout_train_fwd_kernel(ReadoutTrainArgs a) {
  const feta_readout_train& d = a.d;
  const int b = blockIdx.x, t = threadIdx.x;
  if (b >= *d.count) return;     // (uniform over the workgroup, as every branch around a barrier below)
  const int n = d.n_real[b];
  float* ws = d.ws + (int64_t)b * kRtRow;
  if (!readout_slot_ok(n, d.N)) {   // an empty graph: nothing for the loss, nothing for the gradients
    if (t < kReadoutD) {
      gst1<kStSaved>(ws + kRtPooled + t, 0.0f);
      gst1<kStSaved>(ws + kRtZ + t, 0.0f);
      gst1<kStSaved>(ws + kRtDlogit + t, 0.0f);
      if (t < d.C) gst1<kStSaved>(d.scores + (int64_t)b * d.C + t, 0.0f);
      if (t < 4) gst1<kStHandoff>(ws + kRtTerm + t, 0.0f);
    }
    return;
  }
  float* part = feta_lds;
  float* pooled = feta_lds + kReadoutLdsPooled;
  float* h = feta_lds + kReadoutLdsH;
  float* logit = feta_lds + kReadoutLdsLogit;

  readout_pool(d.y + (int64_t)b * d.row_sb, d.row_sn, n, (a.vec & kReadoutVecY) != 0, part, pooled);
  if (t < kReadoutD) gst1<kStSaved>(ws + kRtPooled + t, pooled[t]);
  {
    const float v = readout_affine(d.w1, d.b1, pooled, kReadoutD, (a.vec & kReadoutVecW1) != 0);
    if ((t & 3) == 0) {
      h[t >> 2] = readout_act(v, d.slope);
      gst1<kStSaved>(ws + kRtZ + (t >> 2), v);
    }
  }
  lds_barrier();
  {
    const float v = readout_affine(d.w2, d.b2, h, d.C, (a.vec & kReadoutVecW2) != 0);
    if ((t & 3) == 0 && (t >> 2) < d.C) {
      logit[t >> 2] = v;
      gst1<kStSaved>(d.scores + (int64_t)b * d.C + (t >> 2), v);
    }
  }
  lds_barrier();

  float label;
  int64_t cls;
  readout_label(d.labels, d.label_kind, b, label, cls);
  float* stat = part;     // (the partial rows are spent) the row maximum and the sum of exponentials of FETA_LOSS_CE
  if (t == 0) {
    float m, s;
    const float4 out = readout_terms(logit, d.C, d.loss_kind, label, cls, m, s);
    gst1<kStHandoff>(ws + kRtTerm, out.x);
    gst1<kStHandoff>(ws + kRtTerm + 1, out.w);
    stat[0] = m;
    stat[1] = s;
    if (d.loss_kind == FETA_LOSS_L1) {
      const float e = logit[0] - label;
      gst1<kStSaved>(ws + kRtDlogit, (float)(e > 0.0f) - (float)(e < 0.0f));
    } else if (d.loss_kind == FETA_LOSS_BCE_LOGITS) {
      // sigmoid(x) without overflow: exp of a non-positive argument on either side
      const float x = logit[0], ex = expf(-fabsf(x));
      const float sig = x >= 0.0f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
      gst1<kStSaved>(ws + kRtDlogit, label == label ? sig - label : 0.0f);
    }
  }
  if (d.loss_kind != FETA_LOSS_CE) return;
  lds_barrier();
  if (t < d.C) {
    const bool known = cls >= 0 && cls < d.C;
    const float p = expf(logit[t] - stat[0]) / stat[1];
    gst1<kStSaved>(ws + kRtDlogit + t, known ? p - (t == (int)cls ? 1.0f : 0.0f) : NAN);
  }
}

// sum of v over the lanes t < live of the one workgroup, in ascending lane order within three fixed levels (each lane
// its own value, 16 lanes 16 values each, lane 0 the 16 sums); valid in lane 0
__device__ __forceinline__ float readout_ordered_sum(float v, float* buf) {
  const int t = threadIdx.x;
  buf[t] = v;
  lds_barrier();
  if (t < 16) {
    float s = 0.0f;
    for (int i = 0; i < 16; ++i) s += buf[16 * t + i];
    buf[kReadoutThreads + t] = s;
  }
  lds_barrier();
  float s = 0.0f;
  if (t == 0)
    for (int i = 0; i < 16; ++i) s += buf[kReadoutThreads + i];
  lds_barrier();
  return s;
}

__global__ __launch_bounds__(kReadoutThreads) void readout_train_loss_kernel(ReadoutTrainArgs a) {
  const feta_readout_train& d = a.d;
  const int t = threadIdx.x;
  int count = *d.count;
  count = count < 0 ? 0 : count > d.B ? d.B : count;
  // lane t owns the slots [t per, (t + 1) per), in ascending order
  const int per = (count + kReadoutThreads - 1) / kReadoutThreads;
  float term = 0.0f, weight = 0.0f;
  for (int b = t * per; b < (t + 1) * per && b < count; ++b) {
    const float* row = d.ws + (int64_t)b * kRtRow + kRtTerm;
    term += row[0];
    weight += row[1];
  }
  term = readout_ordered_sum(term, feta_lds);
  weight = readout_ordered_sum(weight, feta_lds);
  if (t == 0) {
    gst1<kStHandoff>(d.loss, term / weight);
    gst1<kStHandoff>(d.loss + 1, 1.0f / weight);
  }
}

// out[k] (LDS, k < 64) = sum_r w[r, k] x[r] over r < rows: lane t owns column t & 63 and the rows t >> 6, t >> 6 + 4, ...
// (a wave reads one 256-byte row per step); the four partial sums meet in `part` in wave order.  Every lane calls it.
__device__ __forceinline__ float readout_dot_t(const float* w, const float* x, int rows, float* part) {
  const int t = threadIdx.x, k = t & 63, q = t >> 6;
  float s = 0.0f;
  for (int r = q; r < rows; r += 4) s += w[r * kReadoutD + k] * x[r];
  part[q * kReadoutD + k] = s;
  lds_barrier();
  float v = 0.0f;
  if (t < kReadoutD) v = (part[t] + part[kReadoutD + t]) + (part[2 * kReadoutD + t] + part[3 * kReadoutD + t]);
  lds_barrier();
  return v;
}

__global__ __launch_bounds__(kReadoutThreads) void readout_train_bwd_kernel(ReadoutTrainArgs a) {
  const feta_readout_train& d = a.d;
  const int b = blockIdx.x, t = threadIdx.x;
  const bool counted = b < *d.count;
  int n = counted ? d.n_real[b] : 0;
  if (!readout_slot_ok(n, d.N)) n = 0;
  float* part = feta_lds;                          // [4][64] partial sums of the transposed products
  float* dl = feta_lds + 4 * kReadoutD;            // [64]
  float* dz = feta_lds + 5 * kReadoutD;            // [64]
  float* dp = feta_lds + 6 * kReadoutD;            // [64] dpooled / n
  if (counted) {
    float* ws = d.ws + (int64_t)b * kRtRow;
    const float s = *d.dloss * d.loss[1];
    if (t < kReadoutD) {
      const float v = t < d.C ? s * ws[kRtDlogit + t] : 0.0f;
      dl[t] = v;
      gst1<kStHandoff>(ws + kRtDl + t, v);
    }
    lds_barrier();
    {   // dz = (W2^T dl) act'(z)
      float v = readout_dot_t(d.w2, dl, d.C, part);
      if (t < kReadoutD) {
        v *= ws[kRtZ + t] > 0.0f ? 1.0f : d.slope;
        dz[t] = v;
        gst1<kStHandoff>(ws + kRtDz + t, v);
      }
    }
    lds_barrier();
    if (d.dy == nullptr) return;
    {   // dpooled = W1^T dz, and the mean's 1 / n
      const float v = readout_dot_t(d.w1, dz, kReadoutD, part);
      if (t < kReadoutD) dp[t] = n > 0 ? v / (float)n : 0.0f;
    }
    lds_barrier();
  }
  if (d.dy == nullptr) return;
  // dy: the slot's N rows, 16 lanes a row; dpooled / n in the real rows, zeros behind them (and in a slot nobody counts)
  const int c = 4 * (t & 15);
  float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (n > 0) g = make_float4(dp[c], dp[c + 1], dp[c + 2], dp[c + 3]);
  float* col = d.dy + (int64_t)b * d.drow_sb + c;
  for (int i = t >> 4; i < d.N; i += kReadoutSlots) {
    const float4 v = i < n ? g : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float* p = col + (int64_t)i * d.drow_sn;
    if (a.vec & kReadoutVecDy) {
      gst4<kStHandoff>(p, v.x, v.y, v.z, v.w);
    } else {
      gst1<kStHandoff>(p, v.x);
      gst1<kStHandoff>(p + 1, v.y);
      gst1<kStHandoff>(p + 2, v.z);
      gst1<kStHandoff>(p + 3, v.w);
    }
  }
}

// Workgroup `tile` < 4: rows [16 tile, +16) of dW1 and db1 (left factor dz, right factor pooled); the tiles behind them:
// rows [16 (tile - 4), +16) of dW2 and db2 (left factor dl, right factor h = act(z)).  Lane t owns the row t >> 4 of the tile
// and the columns [4 (t & 15), +4); the lanes of column group 0 carry the bias gradient of their row.
__global__ __launch_bounds__(kReadoutThreads) void readout_train_dw_kernel(ReadoutTrainArgs a) {
  const feta_readout_train& d = a.d;
  const int t = threadIdx.x;
  const bool second = blockIdx.x >= kReadoutD / kRtTile;
  const int row0 = kRtTile * (second ? blockIdx.x - kReadoutD / kRtTile : blockIdx.x), rows = second ? d.C : kReadoutD;
  float* dw = second ? d.dw2 : d.dw1;
  float* db = second ? d.db2 : d.db1;
  if (dw == nullptr && db == nullptr) return;
  int count = *d.count;
  count = count < 0 ? 0 : count > d.B ? d.B : count;
  const int left_off = second ? kRtDl : kRtDz, right_off = second ? kRtZ : kRtPooled;
  float* left = feta_lds;                  // [chunk][16]
  float* right = feta_lds + kRtLdsRight;   // [chunk][64]

  // staging: lane t loads the left factors of slot t >> 2, tile rows [4 (t & 3), +4), and the right factors of the
  // slots t >> 4 + 16 j, columns [4 (t & 15), +4)
  float4 ld_left, ld_right[kRtChunk / 16];
  auto fetch = [&](int b0) {
    const int bl = b0 + (t >> 2), r = row0 + 4 * (t & 3);
    ld_left = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (bl < count && r < rows) ld_left = *reinterpret_cast<const float4*>(d.ws + (int64_t)bl * kRtRow + left_off + r);
#pragma unroll
    for (int j = 0; j < kRtChunk / 16; ++j) {
      const int br = b0 + (t >> 4) + 16 * j;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (br < count) v = *reinterpret_cast<const float4*>(d.ws + (int64_t)br * kRtRow + right_off + 4 * (t & 15));
      if (second) {
        v.x = readout_act(v.x, d.slope);
        v.y = readout_act(v.y, d.slope);
        v.z = readout_act(v.z, d.slope);
        v.w = readout_act(v.w, d.slope);
      }
      ld_right[j] = v;
    }
  };
  auto stage = [&]() {
    float* l = left + (t >> 2) * kRtTile + 4 * (t & 3);
    l[0] = ld_left.x;
    l[1] = ld_left.y;
    l[2] = ld_left.z;
    l[3] = ld_left.w;
#pragma unroll
    for (int j = 0; j < kRtChunk / 16; ++j) {
      float* r = right + ((t >> 4) + 16 * j) * kReadoutD + 4 * (t & 15);
      r[0] = ld_right[j].x;
      r[1] = ld_right[j].y;
      r[2] = ld_right[j].z;
      r[3] = ld_right[j].w;
    }
  };

  const int row = t >> 4, c = 4 * (t & 15);
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float bias = 0.0f;
  fetch(0);
  for (int b0 = 0; b0 < count; b0 += kRtChunk) {
    stage();
    lds_barrier();
    if (b0 + kRtChunk < count) fetch(b0 + kRtChunk);
    const int live = count - b0 < kRtChunk ? count - b0 : kRtChunk;
    for (int i = 0; i < live; ++i) {
      const float l = left[i * kRtTile + row];
      const float* r = right + i * kReadoutD + c;
      acc.x += l * r[0];
      acc.y += l * r[1];
      acc.z += l * r[2];
      acc.w += l * r[3];
      bias += l;
    }
    lds_barrier();
  }
  if (row0 + row >= rows) return;
  if (dw) gst4<kStPartial>(dw + (row0 + row) * kReadoutD + c, acc.x, acc.y, acc.z, acc.w);
  if (db && c == 0) gst1<kStPartial>(db + row0 + row, bias);
}

}  // namespace feta

using namespace feta;

extern "C" int feta_readout_eval_supported(int d_model, int C) { return d_model == kReadoutD && C >= 1 && C <= 64 ? 1 : 0; }

extern "C" int feta_readout_eval(const feta_readout* dp, feta_stream_t stream) {
  FETA_REQUIRE(dp != nullptr, "readout_eval: null descriptor");
  const feta_readout& d = *dp;
  FETA_REQUIRE(d.B > 0 && d.N > 0 && d.G > 0, "readout_eval: B = %d, N = %d, G = %d must be positive", d.B, d.N, d.G);
  FETA_REQUIRE(feta_readout_eval_supported(d.d_model, d.C), "readout_eval: d_model = %d, C = %d (d_model = 64, 1 <= C <= 64)",
               d.d_model, d.C);
  FETA_REQUIRE(d.loss_kind >= FETA_LOSS_L1 && d.loss_kind <= FETA_LOSS_CE, "readout_eval: unknown loss_kind %d", d.loss_kind);
  FETA_REQUIRE(d.loss_kind == FETA_LOSS_CE || d.C == 1, "readout_eval: loss_kind %d needs C = 1, got C = %d", d.loss_kind, d.C);
  FETA_REQUIRE(d.label_kind == FETA_LABELS_GRAPH_F32 || d.label_kind == FETA_LABELS_GRAPH_I64,
               "readout_eval: label_kind %d (one label per graph: FETA_LABELS_GRAPH_F32 or FETA_LABELS_GRAPH_I64)", d.label_kind);
  FETA_REQUIRE(d.loss_kind != FETA_LOSS_CE || d.label_kind == FETA_LABELS_GRAPH_I64, "readout_eval: FETA_LOSS_CE needs int64 class labels");
  FETA_REQUIRE(d.y && d.n_real && d.ids && d.count && d.labels, "readout_eval: y, n_real, ids, count and labels are required");
  FETA_REQUIRE(d.w1 && d.w2 && d.scores && d.terms, "readout_eval: w1, w2, scores and terms are required");
  FETA_REQUIRE(d.row_sb >= 0 && d.row_sn >= 0, "readout_eval: negative row strides");
  ReadoutArgs args;
  args.d = d;
  args.vec = 0;
  if (aligned16(d.y) && d.row_sb % 4 == 0 && d.row_sn % 4 == 0) args.vec |= kReadoutVecY;
  if (aligned16(d.w1)) args.vec |= kReadoutVecW1;
  if (aligned16(d.w2)) args.vec |= kReadoutVecW2;
  if (aligned16(d.terms)) args.vec |= kReadoutVecTerms;
  hipLaunchKernelGGL(readout_eval_kernel, dim3(d.B), dim3(kReadoutThreads), kReadoutLdsFloats * sizeof(float),
                     (hipStream_t)stream, args);
  return check_launch("feta_readout_eval");
}

extern "C" int feta_readout_train_supported(int d_model, int C) { return feta_readout_eval_supported(d_model, C); }

extern "C" int64_t feta_readout_train_ws_floats(int B, int C) {
  return B > 0 && C >= 1 && C <= 64 ? (int64_t)B * kRtRow : 0;
}

// the checks both directions share; *args: the descriptor and the alignment bits of its forward operands
static int readout_train_args(const feta_readout_train* dp, const char* who, ReadoutTrainArgs* args) {
  FETA_REQUIRE(dp != nullptr, "%s: null descriptor", who);
  const feta_readout_train& d = *dp;
  FETA_REQUIRE(d.B > 0 && d.N > 0, "%s: B = %d, N = %d must be positive", who, d.B, d.N);
  FETA_REQUIRE(feta_readout_train_supported(d.d_model, d.C), "%s: d_model = %d, C = %d (d_model = 64, 1 <= C <= 64)", who,
               d.d_model, d.C);
  FETA_REQUIRE(d.loss_kind >= FETA_LOSS_L1 && d.loss_kind <= FETA_LOSS_CE, "%s: unknown loss_kind %d", who, d.loss_kind);
  FETA_REQUIRE(d.loss_kind == FETA_LOSS_CE || d.C == 1, "%s: loss_kind %d needs C = 1, got C = %d", who, d.loss_kind, d.C);
  FETA_REQUIRE(d.label_kind == FETA_LABELS_GRAPH_F32 || d.label_kind == FETA_LABELS_GRAPH_I64,
               "%s: label_kind %d (one label per graph: FETA_LABELS_GRAPH_F32 or FETA_LABELS_GRAPH_I64)", who, d.label_kind);
  FETA_REQUIRE(d.loss_kind != FETA_LOSS_CE || d.label_kind == FETA_LABELS_GRAPH_I64, "%s: FETA_LOSS_CE needs int64 class labels", who);
  FETA_REQUIRE(d.y && d.n_real && d.count && d.labels, "%s: y, n_real, count and labels are required", who);
  FETA_REQUIRE(d.w1 && d.w2 && d.scores && d.loss && d.ws, "%s: w1, w2, scores, loss and ws are required", who);
  FETA_REQUIRE(aligned16(d.ws), "%s: ws must be 16-byte aligned", who);
  FETA_REQUIRE(d.row_sb >= 0 && d.row_sn >= 0, "%s: negative row strides", who);
  args->d = d;
  args->vec = 0;
  if (aligned16(d.y) && d.row_sb % 4 == 0 && d.row_sn % 4 == 0) args->vec |= kReadoutVecY;
  if (aligned16(d.w1)) args->vec |= kReadoutVecW1;
  if (aligned16(d.w2)) args->vec |= kReadoutVecW2;
  return FETA_OK;
}

extern "C" int feta_readout_train_fwd(const feta_readout_train* dp, feta_stream_t stream) {
  ReadoutTrainArgs args;
  if (const int rc = readout_train_args(dp, "readout_train_fwd", &args)) return rc;
  hipLaunchKernelGGL(readout_train_fwd_kernel, dim3(args.d.B), dim3(kReadoutThreads), kReadoutLdsFloats * sizeof(float),
                     (hipStream_t)stream, args);
  if (const int rc = check_launch("feta_readout_train_fwd")) return rc;
  hipLaunchKernelGGL(readout_train_loss_kernel, dim3(1), dim3(kReadoutThreads), (kReadoutThreads + 16) * sizeof(float),
                     (hipStream_t)stream, args);
  return check_launch("feta_readout_train_fwd (loss)");
}

extern "C" int feta_readout_train_bwd(const feta_readout_train* dp, feta_stream_t stream) {
  ReadoutTrainArgs args;
  if (const int rc = readout_train_args(dp, "readout_train_bwd", &args)) return rc;
  const feta_readout_train& d = args.d;
  FETA_REQUIRE(d.dloss != nullptr, "readout_train_bwd: dloss is required");
  FETA_REQUIRE(d.dy == nullptr || (d.drow_sb >= 0 && d.drow_sn >= 0), "readout_train_bwd: negative dy strides");
  if (d.dy && aligned16(d.dy) && d.drow_sb % 4 == 0 && d.drow_sn % 4 == 0) args.vec |= kReadoutVecDy;
  FETA_REQUIRE((d.dw1 == nullptr || aligned16(d.dw1)) && (d.dw2 == nullptr || aligned16(d.dw2)),
               "readout_train_bwd: dw1 and dw2 must be 16-byte aligned");
  hipLaunchKernelGGL(readout_train_bwd_kernel, dim3(d.B), dim3(kReadoutThreads), 7 * kReadoutD * sizeof(float),
                     (hipStream_t)stream, args);
  if (const int rc = check_launch("feta_readout_train_bwd")) return rc;
  if (!(d.dw1 || d.db1 || d.dw2 || d.db2)) return FETA_OK;
  const int tiles = kReadoutD / kRtTile + (d.C + kRtTile - 1) / kRtTile;
  hipLaunchKernelGGL(readout_train_dw_kernel, dim3(tiles), dim3(kReadoutThreads), kRtDwLdsFloats * sizeof(float),
                     (hipStream_t)stream, args);
  return check_launch("feta_readout_train_bwd (parameter gradients)");
}
