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
#include <cmath>

#include <feta_device.h>

#include "feta_abi_common.h"

namespace feta {

constexpr int kReadoutThreads = 256, kReadoutD = 64, kReadoutSlots = kReadoutThreads / 16;
// LDS, in floats: the partial rows of the pooling, then pooled, h and the logits
constexpr int kReadoutLdsPooled = kReadoutSlots * kReadoutD, kReadoutLdsH = kReadoutLdsPooled + kReadoutD,
              kReadoutLdsLogit = kReadoutLdsH + kReadoutD, kReadoutLdsFloats = kReadoutLdsLogit + kReadoutD;
enum { kReadoutVecY = 1, kReadoutVecW1 = 2, kReadoutVecW2 = 4, kReadoutVecTerms = 8 };

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

  {   // masked mean over the n real rows
    const int c = 4 * (t & 15), slot = t >> 4;
    const float* col = d.y + (int64_t)b * d.row_sb + c;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = slot; i < n; i += kReadoutSlots) {
      const float4 v = readout_ld4(col + (int64_t)i * d.row_sn, (a.vec & kReadoutVecY) != 0);
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

  {   // h = act(W1 pooled + b1)
    float v = readout_dot(d.w1, pooled, kReadoutD, (a.vec & kReadoutVecW1) != 0);
    if ((t & 3) == 0) {
      if (d.b1) v += d.b1[t >> 2];
      h[t >> 2] = v > 0.0f ? v : d.slope * v;
    }
  }
  lds_barrier();
  {   // logits = W2 h + b2
    float v = readout_dot(d.w2, h, d.C, (a.vec & kReadoutVecW2) != 0);
    if ((t & 3) == 0 && (t >> 2) < d.C) {
      if (d.b2) v += d.b2[t >> 2];
      logit[t >> 2] = v;
      d.scores[(int64_t)g * d.C + (t >> 2)] = v;
    }
  }
  lds_barrier();
  if (t != 0) return;

  float label = 0.0f;
  int64_t cls = 0;
  if (d.label_kind == FETA_LABELS_GRAPH_F32) {
    label = reinterpret_cast<const float*>(d.labels)[b];
  } else {
    cls = reinterpret_cast<const int64_t*>(d.labels)[b];
    label = (float)cls;
  }
  float4 out = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  if (d.loss_kind == FETA_LOSS_L1) {
    const float e = logit[0] - label;
    out.x = fabsf(e);
    out.y = e * e;
  } else if (d.loss_kind == FETA_LOSS_BCE_LOGITS) {
    // (1 - y) x - log sigmoid(x), with log sigmoid(x) = min(x, 0) - log1p(exp(-|x|)): F.binary_cross_entropy_with_logits
    const float x = logit[0];
    const bool labelled = label == label;
    out.x = labelled ? (1.0f - label) * x + fmaxf(-x, 0.0f) + log1pf(expf(-fabsf(x))) : 0.0f;
    out.y = (x > 0.0f) == (label > 0.5f) ? 1.0f : 0.0f;
    out.w = labelled ? 1.0f : 0.0f;
  } else {
    // -log softmax[label] as log-sum-exp with the row maximum subtracted (F.cross_entropy); the first index wins a tie
    int best = 0;
    float m = logit[0];
    for (int c = 1; c < d.C; ++c)
      if (logit[c] > m) {
        m = logit[c];
        best = c;
      }
    float s = 0.0f;
    for (int c = 0; c < d.C; ++c) s += expf(logit[c] - m);
    const bool known = cls >= 0 && cls < d.C;     // (a label outside the classes: NaN, as a loss nobody defined)
    out.x = known ? m + logf(s) - logit[known ? cls : 0] : NAN;
    out.y = known && best == (int)cls ? 1.0f : 0.0f;
  }
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
