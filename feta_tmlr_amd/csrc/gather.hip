// One padded batch from the device-resident graph store in one launch (feta_batch_gather, include/feta_hip.h): what
// GraphDataset_v2.collate_fn builds on the host from Python lists (transformer/data.py:161-225) plus the cached
// per-graph encodings (transformer/position_encoding.py:35-49), gathered from flat device arrays by a list of graph
// ids that lives on the device too, so the launch can be replayed inside a captured training step.
//
// Pure streaming: workgroup (b, c) owns rows [64 c, 64 c + 64) of graph ids[b] in every per-row output and, c = 0, the
// per-graph ones.  Every element of every output is written - real values, or the padding value where the row or the
// column is behind n_real - so nothing is cleared between replays.  A field moves as 16-byte vectors when its width is a
// multiple of 4 and its pointers are aligned (the entry point decides per field; the store pitches the rows of pe to
// multiples of 4), element by element otherwise.  No LDS; the only cross-lane step is the prefix sum behind node_off.
//
// feta_batch_gather_ex is the same launch with the three additive fields of feta_gather_ex compiled in (EX): the dense
// scaled Laplacian of filter_mode='cheb' (lhat: the geometry and the block offsets of pe, always fp32) and a sign per
// column of lap.  feta_batch_gather keeps the kernels without them.
#include <cstddef>
#include <cstring>

#include "feta_abi_common.h"
#include "feta_bf16.h"

namespace feta {

constexpr int kGatherThreads = 256, kGatherRows = 64;
enum { kGatherVecX = 1, kGatherVecPe = 2, kGatherVecU = 4, kGatherVecLap = 8, kGatherVecLhat = 16 };

struct GatherArgs {
  feta_gather d;
  int vec;   // kGatherVec* bits: the field's widths and base pointers allow 16-byte loads
};
// what feta_gather_ex holds behind its feta_gather
struct GatherExtra {
  const float* s_lhat;
  float* lhat;
  const float* lap_sign;
};

__device__ __forceinline__ void gather_st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void gather_st4(bf16_t* p, const float4& v) {
  bf16x4_raw o;
  o.v[0] = f2bf(v.x);
  o.v[1] = f2bf(v.y);
  o.v[2] = f2bf(v.z);
  o.v[3] = f2bf(v.w);
  *reinterpret_cast<bf16x4_raw*>(p) = o;
}

// node count of the graph in slot j: 0 for an id outside the store or a graph that does not fit the padded size
__device__ __forceinline__ int gather_count(const feta_gather& d, int j, int* id_out = nullptr) {
  const int id = d.ids[j];
  if (id_out) *id_out = id;
  if (id < 0 || id >= d.G) return 0;
  const int n = d.s_n[id];
  return (n < 0 || n > d.N) ? 0 : n;
}

// dst[r, 0..W) for the rows [r0, r1) of one graph: src[r, c] (row pitch `pitch`) where r < n and c < wsrc, else 0.
// vec: W, pitch and wsrc are multiples of 4 and both sides are aligned for 4-element accesses.
// colscale [wsrc] or null: a factor per column of the real elements (the padding stays +0).
template <class T>
__device__ __forceinline__ void gather_rows(T* dst, int W, int r0, int r1, const float* src, int pitch, int wsrc, int n,
                                            bool vec, const float* colscale = nullptr) {
  if (vec) {
    const int w4 = W >> 2, items = (r1 - r0) * w4;
    for (int it = threadIdx.x; it < items; it += kGatherThreads) {
      const int q = it / w4, r = r0 + q, c = (it - q * w4) << 2;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (r < n && c < wsrc) {
        v = *reinterpret_cast<const float4*>(src + (int64_t)r * pitch + c);
        if (colscale) {
          v.x *= colscale[c];
          v.y *= colscale[c + 1];
          v.z *= colscale[c + 2];
          v.w *= colscale[c + 3];
        }
      }
      gather_st4(dst + (int64_t)r * W + c, v);
    }
  } else {
    const int items = (r1 - r0) * W;
    for (int it = threadIdx.x; it < items; it += kGatherThreads) {
      const int q = it / W, r = r0 + q, c = it - q * W;
      float v = 0.0f;
      if (r < n && c < wsrc) v = colscale ? src[(int64_t)r * pitch + c] * colscale[c] : src[(int64_t)r * pitch + c];
      Num<T>::st(dst + (int64_t)r * W + c, v);
    }
  }
}

template <class T, bool EX>
__device__ __forceinline__ void batch_gather_body(const GatherArgs& a, const GatherExtra& e) {
  const feta_gather& d = a.d;
  const int b = blockIdx.x, N = d.N;
  const int r0 = blockIdx.y * kGatherRows, r1 = min(N, r0 + kGatherRows);
  int id;
  const int n = gather_count(d, b, &id);
  const int64_t off = n > 0 ? d.s_node_off[id] : 0;   // (n == 0: no store row is addressed below)

  if (d.x) gather_rows(reinterpret_cast<T*>(d.x) + (int64_t)b * N * d.F, d.F, r0, r1, d.s_x + off * d.F, d.F, d.F, n,
                       (a.vec & kGatherVecX) != 0);
  if (d.pe) {
    const int64_t poff = n > 0 ? d.s_pe_off[id] : 0;
    const int pitch = (n + 3) & ~3;
    const bool vec = (a.vec & kGatherVecPe) != 0 && (poff & 3) == 0;
    gather_rows(reinterpret_cast<T*>(d.pe) + (int64_t)b * N * N, N, r0, r1, d.s_pe + poff, pitch, vec ? pitch : n, n, vec);
  }
  if (d.u) gather_rows(d.u + (int64_t)b * N * d.K, d.K, r0, r1, d.s_u + off * d.K, d.K, d.K, n, (a.vec & kGatherVecU) != 0);
  if (d.lap) gather_rows(d.lap + (int64_t)b * N * d.lap_dim, d.lap_dim, r0, r1, d.s_lap + off * d.lap_dim, d.lap_dim,
                         d.lap_dim, n, (a.vec & kGatherVecLap) != 0, EX ? e.lap_sign : nullptr);
  if (EX && e.lhat) {
    const int64_t poff = n > 0 ? d.s_pe_off[id] : 0;
    const int pitch = (n + 3) & ~3;
    const bool vec = (a.vec & kGatherVecLhat) != 0 && (poff & 3) == 0;
    gather_rows(e.lhat + (int64_t)b * N * N, N, r0, r1, e.s_lhat + poff, pitch, vec ? pitch : n, n, vec);
  }

  // one value per node
  for (int i = r0 + threadIdx.x; i < r1; i += kGatherThreads) {
    const bool real = i < n;
    if (d.mask) reinterpret_cast<unsigned char*>(d.mask)[(int64_t)b * N + i] = real ? 0 : 1;
    if (d.degree || d.degree_rows) {
      const float dg = real ? d.s_degree[off + i] : 0.0f;
      if (d.degree) d.degree[(int64_t)b * N + i] = dg;
      if (d.degree_rows) d.degree_rows[(int64_t)i * d.B + b] = dg;
    }
    if (d.labels && d.label_kind == FETA_LABELS_NODE_I64)
      reinterpret_cast<int64_t*>(d.labels)[(int64_t)b * N + i] =
          real ? reinterpret_cast<const int64_t*>(d.s_labels)[off + i] : (int64_t)-100;
  }
  if (blockIdx.y != 0) return;

  // one value (or row) per graph
  if (d.lam)
    for (int k = threadIdx.x; k < d.K; k += kGatherThreads) d.lam[(int64_t)b * d.K + k] = n > 0 ? d.s_lam[(int64_t)id * d.K + k] : 0.0f;
  if (threadIdx.x == 0) {
    if (d.n_real) d.n_real[b] = n;
    if (d.labels && d.label_kind == FETA_LABELS_GRAPH_F32)
      reinterpret_cast<float*>(d.labels)[b] = n > 0 ? reinterpret_cast<const float*>(d.s_labels)[id] : 0.0f;
    if (d.labels && d.label_kind == FETA_LABELS_GRAPH_I64)
      reinterpret_cast<int64_t*>(d.labels)[b] = n > 0 ? reinterpret_cast<const int64_t*>(d.s_labels)[id] : (int64_t)0;
  }
  // first node of graph b in the batch's node numbering: the counts of the slots in front of it, summed by wave 0
  // (as floats through the wave shuffle: exact, the entry point holds B * N below 2^24)
  if (d.node_off && threadIdx.x < 64) {
    float s = 0.0f;
    for (int j = threadIdx.x; j < b; j += 64) s += (float)gather_count(d, j);
    for (int m = 32; m > 0; m >>= 1) s += shfl_xor(s, m);
    if (threadIdx.x == 0) d.node_off[b] = (int32_t)s;
  }
}

template <class T>
__global__ __launch_bounds__(kGatherThreads) void batch_gather_kernel(GatherArgs a) {
  batch_gather_body<T, false>(a, GatherExtra{});
}

template <class T>
__global__ __launch_bounds__(kGatherThreads) void batch_gather_ex_kernel(GatherArgs a, GatherExtra e) {
  batch_gather_body<T, true>(a, e);
}

// the checks of both entry points, then the launch: with `e` the kernels that carry the fields of feta_gather_ex
static int gather_launch(const feta_gather& d, const GatherExtra* e, feta_stream_t stream, const char* what) {
  FETA_REQUIRE(d.B > 0 && d.N > 0 && d.G > 0, "batch_gather: B = %d, N = %d, G = %d must be positive", d.B, d.N, d.G);
  FETA_REQUIRE(d.dtype == FETA_F32 || d.dtype == FETA_BF16, "batch_gather: unknown dtype %d", d.dtype);
  FETA_REQUIRE(d.ids && d.s_n && d.s_node_off, "batch_gather: ids, s_n and s_node_off are required");
  FETA_REQUIRE(!d.x || (d.s_x && d.F > 0), "batch_gather: x needs s_x and F > 0");
  FETA_REQUIRE(!(d.degree || d.degree_rows) || d.s_degree, "batch_gather: degree / degree_rows need s_degree");
  FETA_REQUIRE(!d.pe || (d.s_pe && d.s_pe_off), "batch_gather: pe needs s_pe and s_pe_off");
  FETA_REQUIRE(!(d.u || d.lam) || (d.K >= 1 && d.K <= d.N), "batch_gather: K = %d with N = %d (1 <= K <= N)", d.K, d.N);
  FETA_REQUIRE(!d.u || d.s_u, "batch_gather: u needs s_u");
  FETA_REQUIRE(!d.lam || d.s_lam, "batch_gather: lam needs s_lam");
  FETA_REQUIRE(!d.lap || (d.s_lap && d.lap_dim > 0), "batch_gather: lap needs s_lap and lap_dim > 0");
  FETA_REQUIRE(d.label_kind >= FETA_LABELS_NONE && d.label_kind <= FETA_LABELS_NODE_I64,
               "batch_gather: unknown label_kind %d", d.label_kind);
  FETA_REQUIRE(!d.labels || (d.s_labels && d.label_kind != FETA_LABELS_NONE), "batch_gather: labels need s_labels and a label_kind");
  FETA_REQUIRE(!d.node_off || (int64_t)d.B * d.N < (1 << 24), "batch_gather: node_off needs B * N < 2^24");
  const int chunks = (d.N + kGatherRows - 1) / kGatherRows;
  FETA_REQUIRE(chunks <= 65535, "batch_gather: N = %d", d.N);
  GatherArgs args;
  args.d = d;
  const bool bf = d.dtype == FETA_BF16;
  auto out_ok = [bf](const void* p) { return bf ? (reinterpret_cast<uintptr_t>(p) & 7u) == 0 : aligned16(p); };
  args.vec = 0;
  if (d.x && d.F % 4 == 0 && aligned16(d.s_x) && out_ok(d.x)) args.vec |= kGatherVecX;
  if (d.pe && d.N % 4 == 0 && aligned16(d.s_pe) && out_ok(d.pe)) args.vec |= kGatherVecPe;
  if (d.u && d.K % 4 == 0 && aligned16(d.s_u) && aligned16(d.u)) args.vec |= kGatherVecU;
  if (d.lap && d.lap_dim % 4 == 0 && aligned16(d.s_lap) && aligned16(d.lap)) args.vec |= kGatherVecLap;
  if (e && e->lhat && d.N % 4 == 0 && aligned16(e->s_lhat) && aligned16(e->lhat)) args.vec |= kGatherVecLhat;
  const dim3 grid(d.B, chunks), block(kGatherThreads);
  if (e) {
    auto kern = bf ? batch_gather_ex_kernel<bf16_t> : batch_gather_ex_kernel<float>;
    hipLaunchKernelGGL(kern, grid, block, 0, (hipStream_t)stream, args, *e);
  } else if (bf) {
    auto kern = batch_gather_kernel<bf16_t>;
    hipLaunchKernelGGL(kern, grid, block, 0, (hipStream_t)stream, args);
  } else {
    auto kern = batch_gather_kernel<float>;
    hipLaunchKernelGGL(kern, grid, block, 0, (hipStream_t)stream, args);
  }
  return check_launch(what);
}

}  // namespace feta

using namespace feta;

extern "C" int feta_batch_gather(const feta_gather* dp, feta_stream_t stream) {
  FETA_REQUIRE(dp != nullptr, "batch_gather: null descriptor");
  return gather_launch(*dp, nullptr, stream, "feta_batch_gather");
}

// feta_gather_ex repeats the fields of feta_gather in front of its own (one layout, checked here)
static_assert(offsetof(feta_gather_ex, s_lhat) == sizeof(feta_gather) && offsetof(feta_gather_ex, labels) == offsetof(feta_gather, labels),
              "feta_gather_ex must begin with the fields of feta_gather");

extern "C" int feta_batch_gather_ex(const feta_gather_ex* dp, feta_stream_t stream) {
  FETA_REQUIRE(dp != nullptr, "batch_gather_ex: null descriptor");
  FETA_REQUIRE(!dp->lhat || (dp->s_lhat && dp->s_pe_off), "batch_gather_ex: lhat needs s_lhat and s_pe_off");
  FETA_REQUIRE(!dp->lap_sign || dp->lap, "batch_gather_ex: lap_sign needs lap");
  feta_gather d;
  memcpy(&d, dp, sizeof d);
  const GatherExtra e = {dp->s_lhat, dp->lhat, dp->lap_sign};
  return gather_launch(d, &e, stream, "feta_batch_gather_ex");
}
