// The whole encoder stack for INFERENCE in one launch (ABI 12, include/feta_hip.h: feta_encoder_infer): every layer of
// DiffTransformerEncoderLayer (contract transformer/models.py:166-167,179,244; body per upstream GraphiT, README.md:129)
// for one graph in one workgroup, the activations in LDS from the first layer's input to the last layer's output.
//
// In eval mode nothing couples two graphs - BatchNorm with running statistics is a per-channel affine, LayerNorm is
// row-local, attention is per graph - so the launch has no seam between workgroups, and nothing that only a backward
// pass would read (qkv, softmax statistics, pre-norm rows, h) is written.  Per layer, between workgroup barriers:
//   1. in_proj: q | k | v [NR][192] (v_mfma_f32_16x16x4_f32; weight rows are MFMA operands read from global memory -
//      128 KB per layer does not fit in LDS beside the activations, and every workgroup reads the same rows from L2);
//   2. attention per (head, 16-query tile) with the arithmetic of attn_block_fwd8_kernel (csrc/block.hip): scale
//      d_h^-1/2 on q, keys >= n_real masked, exp(s - rowmax), * pe, / max(rowsum, 1e-6); heads meet in the tile Os;
//   3. out_proj + bias, * degree, + residual - in place on the layer input (each element is read and written by the
//      same lane);  4. norm1;  5. linear1 + bias + relu -> h (aliases q | k | v), linear2 + bias + residual in place;
//   6. norm2: the rows are the next layer's input.
// The work items of a GEMM phase are (column tile, row tile) pairs, dealt in contiguous column-major runs (infer_gemm),
// of the attention phase (head, query tile) pairs, dealt round-robin to the waves.
//
// The kernel is written once against the storage policy of feta_lp.h, T in {float, bf16_t} (feta_encoder_infer_ex):
//   T = float   the tiles hold fp32 and every contraction is a chain of v_mfma_f32_16x16x4_f32 - feta_encoder_infer;
//   T = bf16_t  the evaluation of a model on bf16 storage (layers.set_storage_dtype): the tiles hold bf16 (pitch + 8:
//               53,248 B for 64 rows with pe, three workgroups per CU where fp32 has one), each group of four k-steps
//               is one v_mfma_f32_16x16x16_bf16, and accumulators, softmax, degree scale, residual adds and both norms
//               are fp32 - a value is rounded once, when it is written to a tile or becomes an operand.  Weights, biases,
//               norm parameters and running statistics stay the fp32 master tensors and are rounded in registers when a
//               wave loads them for its run of tiles (staging a layer's 64 KB of bf16 weights in LDS would cost two of
//               the three resident workgroups); x and pe arrive as fp32 or bf16 and are rounded while they are staged;
//               y, out and attn leave as fp32.  d_h = 16 only: bf16 storage has no d_h = 8 form anywhere in the package.
//
// The same kernel is the FORWARD OF A TRAINING STEP of a LayerNorm stack (feta_encoder_fwd_save): LayerNorm is row-local
// in training mode too, so its compile-time SAVE form runs the stack as above and every layer also writes what the
// backward kernels read - qkv, softmax statistics, concatenated heads, y1, h, y2 - from the phase that holds them.
//
// Eight waves (512 lanes), two per SIMD: one wave's VALU and LDS work issues under the other's 32-cycle MFMAs, and the
// phases have 12 NT, H NT, 4 NT and ff / 16 NT work items (NT = 16-row tiles of the graph: at the ZINC shape 36, 12 - 24,
// 12, 24) - sixteen waves would leave most of them idle in every phase but in_proj, four would put a single wave on a SIMD.
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "feta_abi_common.h"
#include "feta_colsum.h"
#include "feta_ln.h"

namespace feta {

constexpr int kInfD = 64;
constexpr int kInfWaves = 8, kInfThreads = 64 * kInfWaves;
constexpr int kInfMaxGrid = 512;        // graphs in flight (two workgroups per CU where the LDS allows); beyond that a
                                        // workgroup walks graphs b, b + grid, ...
constexpr int kInfMaxGridLp = 768;      // ... of the bf16 form: three workgroups per CU (LDS and registers).  Measured at
                                        // B = 1024, N = 64, 3 layers: 256 / 512 / 768 / 1024 -> 214 / 160 / 143 / 150 us

// LDS pitches in elements of T: a 64-wide row (fp32: 16-byte operand reads, bf16: 8-byte), a q | k | v row - the hidden
// rows h (pitch ff + PAD) reuse that tile
template <class T>
struct InfTile {
  static constexpr int P = kInfD + Lp<T>::PAD;
  static constexpr int QP = 3 * kInfD + Lp<T>::PAD;
};

// Kernel arguments: the layer table travels BY VALUE (no device table, no copy before the launch: capturable as is).
struct InferArgs {
  const void* x;     // fp32, or bf16 when in_bf16 (bf16 form only)
  const void* pe;
  const int32_t* n_real;
  const float* rowscale;
  float* y;
  float* out;
  float* attn;
  int64_t row_sb, row_sn;
  int B, N, L, norm;
  float scale;
  int in_bf16;
  feta_encoder_layer layers[FETA_ENCODER_MAX_LAYERS];
};
static_assert(sizeof(InferArgs) <= 4096, "the layer table must fit HIP's 4 KB of kernel arguments");

// The SAVE form (feta_encoder_fwd_save: the forward of a TRAINING step of a LayerNorm stack) also writes what the
// backward kernels read: one base pointer per kind, layer l at base + l * stride elements (no pointer table per layer: the
// arguments stay by value and within the 4 KB).  Layouts and storage type T are those of feta_attn_block_fwd / feta_ffn_fwd.
struct InferSave {
  void* qkv;            // [L][M,192] T
  void* out;            // [L][M,64]  T
  float* ast;           // [L][B,H,N,2]
  void* y1;             // [L][M,64]  T
  void* h;              // [L][M,FF]  T
  void* y2;             // [L][M,64]  T
  float* y2_last_f32;   // bf16 storage: the last layer's y2 as fp32 (feta_ffn.y_f32), instead of y2[L - 1]
  int qkv_sl, out_sl, ast_sl, y1_sl, h_sl, y2_sl;   // (elements per layer: the host checks that they fit 31 bits)
};
struct InferSaveArgs : InferArgs {
  InferSave s;
  ColsumPlan sums;   // pending column sums, reduced by the workgroups beyond main_grid (feta_colsum.h)
  int main_grid;
};
static_assert(sizeof(InferSaveArgs) <= 4096,
              "layer table, save pointers and column-sum plan must fit HIP's 4 KB of kernel arguments");

template <class T>
__host__ __device__ inline int infer_lds_bytes(int nt, bool pe) {
  const int nr = 16 * nt;
  return (int)sizeof(T) * (2 * nr * InfTile<T>::P + nr * InfTile<T>::QP + (pe ? nr * (nr + Lp<T>::PAD) : 0));
}

template <class T>
constexpr int infer_lds_bytes_min() {   // one 16-row tile, no pe
  return (int)sizeof(T) * (2 * 16 * InfTile<T>::P + 16 * InfTile<T>::QP);
}

// Operand of a contraction over K features from a row of an fp32 master weight in global memory, rounded to T in
// registers (chunk j: features 16 j + 4 g .. + 3, the bijection of feta_tiles.h)
template <class T, int K>
__device__ __forceinline__ void infer_load_w(RowOp<T, K>& t, const float* row, int g) {
#pragma unroll
  for (int j = 0; j < RowOp<T, K>::NJ; ++j) {
    const float4 x = *reinterpret_cast<const float4*>(row + 16 * j + 4 * g);
    t.o[j] = Lp<T>::mk(x.x, x.y, x.z, x.w);
  }
}

// The d_h features of one head of a q / k row in the q | k | v tile as ONE operand chunk; d_h = 8 is half a chunk
// (lanes g >= 2 carry zeros and read nothing)
template <class T, int DH>
__device__ __forceinline__ typename Lp<T>::Op infer_head_op(const T* row, int g) {
  static_assert(DH == 16 || DH == 8, "one operand chunk per head");
  if (DH == 16 || 4 * g < DH) return Lp<T>::ld(row + 4 * g);
  return Lp<T>::zero();
}
template <class T, int DH>
__device__ __forceinline__ typename Lp<T>::Op infer_head_op_scaled(const T* row, int g, float scale) {
  if (DH == 16 || 4 * g < DH) return Lp<T>::ld_scaled(row + 4 * g, scale);
  return Lp<T>::zero();
}

// element i of an operand kept where keep[i], zero elsewhere (bf16: on the packed bits, nothing is converted)
__device__ __forceinline__ Lp<float>::Op infer_keep4(const Lp<float>::Op& o, const bool (&keep)[4]) {
  return Lp<float>::mk(keep[0] ? o.v[0] : 0.0f, keep[1] ? o.v[1] : 0.0f, keep[2] ? o.v[2] : 0.0f, keep[3] ? o.v[3] : 0.0f);
}
__device__ __forceinline__ Lp<bf16_t>::Op infer_keep4(const Lp<bf16_t>::Op& o, const bool (&keep)[4]) {
  Lp<bf16_t>::Op r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.v[i] = keep[i] ? o.v[i] : (short)0;
  return r;
}

// rows . W^T over K features for all CT x NT output tiles, register r of a tile <-> (output column 16 ct + 4 g + r,
// row 16 rt + lq); epi(ct, rt, acc) consumes a tile.  Tiles are dealt to the waves in contiguous column-major runs, so a
// wave's consecutive tiles mostly share a column tile and its weight operand (read from global memory, rounded to T in
// registers) is loaded once per run, not once per tile.  skip(ct): column tiles nobody needs (wave-uniform).
template <class T, int K, int CT, int NT, class Skip, class Epi>
__device__ __forceinline__ void infer_gemm(const T* rows, int pitch, const float* w, int wave, int lq, int g,
                                           Skip skip, Epi epi) {
  constexpr int total = CT * NT, per = (total + kInfWaves - 1) / kInfWaves;
  RowOp<T, K> wf;
  int wct = -1;
  for (int t = wave * per; t < (wave + 1) * per && t < total; ++t) {
    const int ct = t / NT, rt = t - ct * NT;
    if (skip(ct)) continue;
    if (ct != wct) {
      infer_load_w<T, K>(wf, w + (int64_t)(16 * ct + lq) * K, g);
      wct = ct;
    }
    RowOp<T, K> xf;
    load_row_op<T, K>(xf, rows + (16 * rt + lq) * pitch, g);
    epi(ct, rt, dot_row_ops<T, K>(wf, xf, zero4()));
  }
}

__device__ __forceinline__ float4 infer_bias4(const float* b, int c) {
  return b != nullptr ? *reinterpret_cast<const float4*>(b + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// norm1 / norm2 of every staged row, in place: 16 lanes per row, four columns each (NR * 16 lanes are whole waves, so
// the DPP row sums of the LayerNorm run in complete waves); fp32 arithmetic on the tile's values, rounded on the store
template <class T, int NR>
__device__ __forceinline__ void infer_norm_rows(T* Xs, int norm, const float* gamma, const float* beta,
                                                const float* mean, const float* var, float eps) {
  for (int idx = threadIdx.x; idx < NR * 16; idx += kInfThreads) {
    const int c = 4 * (idx & 15);
    T* p = Xs + (idx >> 4) * InfTile<T>::P + c;
    float f[4];
    Lp<T>::ld4(p, f);
    if (norm == FETA_NORM_LAYER) {
      ln_apply<4>(f, gamma + c, beta + c, eps);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = (f[e] - mean[c + e]) * rsqrtf(var[c + e] + eps) * gamma[c + e] + beta[c + e];
    }
    Lp<T>::st4(p, f[0], f[1], f[2], f[3]);
  }
}

// SAVE form: layer l of a saved tensor, the row of node i of graph b, a 4-column group of a tile as it is
template <class T>
__device__ __forceinline__ T* save_ptr(void* base, int layer_stride, int l) {
  return static_cast<T*>(base) + (int64_t)l * layer_stride;
}
__device__ __forceinline__ int64_t save_row(const InferArgs& a, int b, int i) {
  return (int64_t)b * a.row_sb + (int64_t)i * a.row_sn;
}
__device__ __forceinline__ void save4(float* dst, const float* tile) {
  *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(tile);
}
__device__ __forceinline__ void save4(bf16_t* dst, const bf16_t* tile) {
  *reinterpret_cast<bf16x4_pk*>(dst) = *reinterpret_cast<const bf16x4_pk*>(tile);
}

// SAVE (compile time; feta_encoder_fwd_save, the forward of a TRAINING step): layer l also writes qkv, out, the softmax
// statistics, y1, h and y2 of its rows i < N - each from the phase whose lanes hold the values, in the storage type T,
// bf16 values as the tile holds them (what the forward itself goes on to use) - and the workgroups beyond main_grid
// reduce the pending column sums, as feta_attn_block_fwd_sums does.  The inference form has none of it.
template <class T, int NT, int DH, int FF, bool SAVE = false>
__global__ __launch_bounds__(kInfThreads) void encoder_infer_kernel(std::conditional_t<SAVE, InferSaveArgs, InferArgs> a) {
  int main_grid = 0;   // SAVE: the workgroups that walk graphs
  if constexpr (SAVE) {
    if ((int)blockIdx.x >= a.main_grid) {
      colsum_role<kInfThreads>(a.sums, (int)blockIdx.x - a.main_grid);
      return;
    }
    main_grid = a.main_grid;
  }
  typedef Lp<T> P;
  typedef typename Lp<T>::Op Op;
  constexpr bool kLp = !std::is_same<T, float>::value;
  static_assert(!kLp || DH == 16, "bf16 storage has no d_h = 8 form");
  constexpr int NR = 16 * NT, H = kInfD / DH, XP = InfTile<T>::P, QP = InfTile<T>::QP, PEP = NR + P::PAD, HP = FF + P::PAD;
  static_assert(HP <= QP, "the hidden rows reuse the q | k | v tile");
  T* Xs = reinterpret_cast<T*>(feta_lds);   // [NR][XP]  layer input -> y1 -> x1 -> y2 -> next layer's input
  T* QKV = Xs + NR * XP;             // [NR][QP]  q | k | v;  h [NR][HP] after the attention phase
  T* Os = QKV + NR * QP;             // [NR][XP]  concatenated heads
  T* Pe = Os + NR * XP;              // [NR][PEP] pe of the graph (zero outside N x N), when given
  T* Hs = QKV;
  const int tid = threadIdx.x;
  const bool has_pe = a.pe != nullptr;
  const bool in_lp = kLp && a.in_bf16 != 0;   // x and pe arrive as bf16 (wave-uniform)
  for (int b = blockIdx.x; b < a.B; b += SAVE ? main_grid : gridDim.x) {
    const int n = a.n_real[b];
    // ---- the graph's rows (rows >= N: zero, computed like the others and never stored) and its pe block ----
    for (int idx = tid; idx < NR * 16; idx += kInfThreads) {
      const int i = idx >> 4, c = 4 * (idx & 15);
      float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (i < a.N) {
        const int64_t off = ((int64_t)b * a.row_sb + (int64_t)i * a.row_sn) * kInfD + c;
        if (in_lp) Lp<bf16_t>::ld4(static_cast<const bf16_t*>(a.x) + off, v);
        else Lp<float>::ld4(static_cast<const float*>(a.x) + off, v);
      }
      P::st4(Xs + i * XP + c, v[0], v[1], v[2], v[3]);
    }
    if (has_pe) {
      for (int idx = tid; idx < NR * NR; idx += kInfThreads) {
        const int i = idx / NR, k = idx - i * NR;
        float v = 0.0f;
        if (i < a.N && k < a.N) {
          const int64_t off = ((int64_t)b * a.N + i) * a.N + k;
          v = in_lp ? bf2f(static_cast<const bf16_t*>(a.pe)[off]) : static_cast<const float*>(a.pe)[off];
        }
        P::st1(Pe + i * PEP + k, v);
      }
    }
    lds_barrier();
    for (int l = 0; l < a.L; ++l) {
      const feta_encoder_layer& p = a.layers[l];
      const bool last = l + 1 == a.L;
      // bf16 form: what a lane derives from its id is recomputed per layer, not held in registers across the whole
      // graph loop (the 80 registers of six waves per SIMD hold no such invariants without scratch)
      int tl = tid;
      if (kLp || SAVE) FETA_OPAQUE_LANE(tl);   // (SAVE: the row predicates of the stores would be held across the layer loop too)
      const int w = tl >> 6, lane = tl & 63, lq = lane & 15, g = lane >> 4;
      // ---- 1. in_proj ----
      const bool tie = p.tie_qk != 0;
      infer_gemm<T, kInfD, 12, NT>(Xs, XP, p.w_in, w, lq, g, [&](int ct) { return tie && ct >= 4 && ct < 8; },  // K is Q
                                   [&](int ct, int rt, f32x4 acc) {
        const float4 bv = infer_bias4(p.b_in, 16 * ct + 4 * g);
        P::st4(QKV + (16 * rt + lq) * QP + 16 * ct + 4 * g, acc[0] + bv.x, acc[1] + bv.y, acc[2] + bv.z, acc[3] + bv.w);
        if constexpr (SAVE) {   // on its way out long before phase 5 overwrites the tile
          if (16 * rt + lq < a.N)
            P::st4(save_ptr<T>(a.s.qkv, a.s.qkv_sl, l) + save_row(a, b, 16 * rt + lq) * (3 * kInfD) + 16 * ct + 4 * g,
                   acc[0] + bv.x, acc[1] + bv.y, acc[2] + bv.z, acc[3] + bv.w);
        }
      });
      lds_barrier();
      // ---- 2. attention: (head h, query tile qb) ----
      const T* Ks = QKV + (p.tie_qk ? 0 : kInfD);
      const T* Vs = QKV + 2 * kInfD;
      for (int t = w; t < H * NT; t += kInfWaves) {
        const int h = t % H, qb = t / H, q = 16 * qb + lq;
        const Op qf = infer_head_op_scaled<T, DH>(QKV + q * QP + DH * h, g, a.scale);
        f32x4 s[NT];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          s[kt] = zero4();
          if (16 * kt < n) {   // a key tile without a real node: nothing (wave-uniform)
            const Op kf = infer_head_op<T, DH>(Ks + (16 * kt + lq) * QP + DH * h, g);
            s[kt] = P::mma(kf, qf, zero4());   // (key 16 kt + 4 g + r, query q)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (16 * kt + 4 * g + r < n) m = fmaxf(m, s[kt][r]);
          }
        }
        m = fmaxf(m, shfl_xor(m, 16));
        m = fmaxf(m, shfl_xor(m, 32));
        float zs = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          if (16 * kt >= n) continue;
          float pr[4] = {1.0f, 1.0f, 1.0f, 1.0f};
          if (has_pe) P::ld4(Pe + q * PEP + 16 * kt + 4 * g, pr);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = 16 * kt + 4 * g + r < n ? fast_exp(s[kt][r] - m) * pr[r] : 0.0f;
            s[kt][r] = e;
            zs += e;
          }
        }
        zs += shfl_xor(zs, 16);
        zs += shfl_xor(zs, 32);
        const float rinv = 1.0f / fmaxf(zs, 1e-6f);
        if constexpr (SAVE) {   // row max of the scaled, masked scores; row sum before the clamp
          if (g == 0 && q < a.N) {
            float* st = a.s.ast + (int64_t)l * a.s.ast_sl + (((int64_t)b * H + h) * a.N + q) * 2;
            st[0] = m;
            st[1] = zs;
          }
        }
        f32x4 o = zero4();
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          if (16 * kt >= n) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) s[kt][r] *= rinv;
          // P (query lq, keys 16 kt + 4 g + r) as the A operand, V (those keys, column lq of the head) as B; padded
          // keys carry no value, lanes lq >= DH (d_h = 8: half a tile) feed columns nobody stores
          const int key = 16 * kt + 4 * g;
          const bool keep[4] = {key < n && lq < DH, key + 1 < n && lq < DH, key + 2 < n && lq < DH, key + 3 < n && lq < DH};
          const Op vf = infer_keep4(P::gather(Vs + key * QP + DH * h + (lq < DH ? lq : 0), QP), keep);
          o = P::mma(P::mk(s[kt]), vf, o);   // (query 16 qb + 4 g + r, column lq)
        }
        if (lq < DH) {
#pragma unroll
          for (int r = 0; r < 4; ++r) P::st1(Os + (16 * qb + 4 * g + r) * XP + DH * h + lq, o[r]);
        }
        if (last && a.attn != nullptr && q < a.N) {
          float* dst = a.attn + (((int64_t)b * H + h) * a.N + q) * a.N;
#pragma unroll
          for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (16 * kt + 4 * g + r < a.N) dst[16 * kt + 4 * g + r] = s[kt][r];
        }
      }
      lds_barrier();
      if constexpr (SAVE) {   // the concatenated heads, whole 4-column groups from the tile
        for (int idx = tid; idx < a.N * 16; idx += kInfThreads) {
          const int i = idx >> 4, c = 4 * (idx & 15);
          save4(save_ptr<T>(a.s.out, a.s.out_sl, l) + save_row(a, b, i) * kInfD + c, Os + i * XP + c);
        }
      }
      // ---- 3. out_proj + bias, * degree, + residual (in place) ----
      const auto none = [](int) { return false; };
      infer_gemm<T, kInfD, 4, NT>(Os, XP, p.w_out, w, lq, g, none, [&](int ct, int rt, f32x4 acc) {
        const int node = 16 * rt + lq, c0 = 16 * ct + 4 * g;
        const float4 bo = infer_bias4(p.b_out, c0);
        const float rs = (a.rowscale != nullptr && node < a.N)
                             ? a.rowscale[(int64_t)b * a.row_sb + (int64_t)node * a.row_sn] : 1.0f;
        T* xr = Xs + node * XP + c0;
        float x[4];
        P::ld4(xr, x);
        P::st4(xr, (acc[0] + bo.x) * rs + x[0], (acc[1] + bo.y) * rs + x[1], (acc[2] + bo.z) * rs + x[2],
               (acc[3] + bo.w) * rs + x[3]);
        if constexpr (SAVE) {   // y1: the rows before norm1
          if (node < a.N)
            P::st4(save_ptr<T>(a.s.y1, a.s.y1_sl, l) + save_row(a, b, node) * kInfD + c0, (acc[0] + bo.x) * rs + x[0],
                   (acc[1] + bo.y) * rs + x[1], (acc[2] + bo.z) * rs + x[2], (acc[3] + bo.w) * rs + x[3]);
        }
      });
      lds_barrier();
      // ---- 4. norm1 ----
      infer_norm_rows<T, NR>(Xs, a.norm, p.n1_gamma, p.n1_beta, p.n1_mean, p.n1_var, p.n1_eps);
      lds_barrier();
      // ---- 5. linear1 + relu -> h; linear2 + bias + residual (in place) ----
      infer_gemm<T, kInfD, FF / 16, NT>(Xs, XP, p.w1, w, lq, g, none, [&](int ct, int rt, f32x4 acc) {
        const float4 bv = infer_bias4(p.b1, 16 * ct + 4 * g);
        P::st4(Hs + (16 * rt + lq) * HP + 16 * ct + 4 * g, fmaxf(acc[0] + bv.x, 0.0f), fmaxf(acc[1] + bv.y, 0.0f),
               fmaxf(acc[2] + bv.z, 0.0f), fmaxf(acc[3] + bv.w, 0.0f));
        if constexpr (SAVE) {
          if (16 * rt + lq < a.N)
            P::st4(save_ptr<T>(a.s.h, a.s.h_sl, l) + save_row(a, b, 16 * rt + lq) * FF + 16 * ct + 4 * g,
                   fmaxf(acc[0] + bv.x, 0.0f), fmaxf(acc[1] + bv.y, 0.0f), fmaxf(acc[2] + bv.z, 0.0f), fmaxf(acc[3] + bv.w, 0.0f));
        }
      });
      lds_barrier();
      infer_gemm<T, FF, 4, NT>(Hs, HP, p.w2, w, lq, g, none, [&](int ct, int rt, f32x4 acc) {
        const int c0 = 16 * ct + 4 * g;
        const float4 bv = infer_bias4(p.b2, c0);
        T* xr = Xs + (16 * rt + lq) * XP + c0;
        float x[4];
        P::ld4(xr, x);
        P::st4(xr, x[0] + (acc[0] + bv.x), x[1] + (acc[1] + bv.y), x[2] + (acc[2] + bv.z), x[3] + (acc[3] + bv.w));
        if constexpr (SAVE) {   // y2: the rows before norm2 - the next layer's x0, LayerNorm applied on load
          if (16 * rt + lq < a.N) {
            const int64_t row = save_row(a, b, 16 * rt + lq);
            if (kLp && last) {   // bf16 storage: what leaves the stack is fp32 - the tile's (rounded) values, widened
              const Op yo = P::mk(x[0] + (acc[0] + bv.x), x[1] + (acc[1] + bv.y), x[2] + (acc[2] + bv.z), x[3] + (acc[3] + bv.w));
              *reinterpret_cast<float4*>(a.s.y2_last_f32 + row * kInfD + c0) =
                  make_float4(P::get(yo, 0), P::get(yo, 1), P::get(yo, 2), P::get(yo, 3));
            } else {
              P::st4(save_ptr<T>(a.s.y2, a.s.y2_sl, l) + row * kInfD + c0, x[0] + (acc[0] + bv.x), x[1] + (acc[1] + bv.y),
                     x[2] + (acc[2] + bv.z), x[3] + (acc[3] + bv.w));
            }
          }
        }
      });
      lds_barrier();
      // ---- 6. norm2 ----
      infer_norm_rows<T, NR>(Xs, a.norm, p.n2_gamma, p.n2_beta, p.n2_mean, p.n2_var, p.n2_eps);
      lds_barrier();
    }
    // ---- the last layer's output rows and concatenated heads (fp32 whatever T is) ----
    for (int idx = tid; idx < a.N * 16; idx += kInfThreads) {
      const int i = idx >> 4, c = 4 * (idx & 15);
      const int64_t row = (int64_t)b * a.row_sb + (int64_t)i * a.row_sn;
      float yv[4], ov[4];
      P::ld4(Xs + i * XP + c, yv);
      P::ld4(Os + i * XP + c, ov);
      *reinterpret_cast<float4*>(a.y + row * kInfD + c) = make_float4(yv[0], yv[1], yv[2], yv[3]);
      if (!SAVE || a.out != nullptr)   // (SAVE: NULL where the saved out of the last layer already is this tensor - fp32 storage)
        *reinterpret_cast<float4*>(a.out + row * kInfD + c) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    }
    lds_barrier();   // (the next graph's rows overwrite Xs)
  }
}

template <class T, int NT, int DH, int FF>
int launch_infer(const InferArgs& a, hipStream_t stream, const char* what) {
  const size_t lds = infer_lds_bytes<T>(NT, a.pe != nullptr);
  auto kern = encoder_infer_kernel<T, NT, DH, FF>;
  static LdsSeen lds_seen;
  allow_dynamic_lds(kern, lds, lds_seen);
  int cap = std::is_same<T, float>::value ? kInfMaxGrid : kInfMaxGridLp;   // FETA_INFER_MAX_GRID: tests force the walking loop
  if (const char* e = getenv("FETA_INFER_MAX_GRID")) cap = atoi(e) > 0 ? atoi(e) : cap;
  const int grid = a.B < cap ? a.B : cap;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kInfThreads), lds, stream, a);
  return check_launch(what);
}

template <class T, int NT, int DH>
int launch_infer_ff(const InferArgs& a, int ff, hipStream_t stream, const char* what) {
  return ff == 64 ? launch_infer<T, NT, DH, 64>(a, stream, what) : launch_infer<T, NT, DH, 128>(a, stream, what);
}

template <int NT>
int launch_infer_heads(const InferArgs& a, int dtype, int heads, int ff, hipStream_t stream, const char* what) {
  if (dtype == FETA_BF16) return launch_infer_ff<bf16_t, NT, 16>(a, ff, stream, what);
  return heads == 4 ? launch_infer_ff<float, NT, 16>(a, ff, stream, what) : launch_infer_ff<float, NT, 8>(a, ff, stream, what);
}

template <class T, int NT, int DH, int FF>
int launch_fwd_save(InferSaveArgs& a, const feta_colsum_seg* segs, int nseg, hipStream_t stream) {
  const size_t lds = infer_lds_bytes<T>(NT, a.pe != nullptr);   // (>= the 8 KB of the column-sum role: 16 rows of fp32 / bf16
                                                                //  tiles are 21 / 11 KB)
  static_assert(infer_lds_bytes_min<T>() >= 4 * colsum_role_lds_floats(kInfThreads), "the column-sum role's LDS");
  auto kern = encoder_infer_kernel<T, NT, DH, FF, true>;
  static LdsSeen lds_seen;
  allow_dynamic_lds(kern, lds, lds_seen);
  int cap = std::is_same<T, float>::value ? kInfMaxGrid : kInfMaxGridLp;
  if (const char* e = getenv("FETA_INFER_MAX_GRID")) cap = atoi(e) > 0 ? atoi(e) : cap;
  const int grid = a.B < cap ? a.B : cap;
  const int tiles = plan_colsum(segs, nseg, a.sums, kInfThreads);
  a.main_grid = grid;
  hipLaunchKernelGGL(kern, dim3(grid + tiles), dim3(kInfThreads), lds, stream, a);
  return check_launch("feta_encoder_fwd_save");
}

template <class T, int NT, int DH>
int launch_fwd_save_ff(InferSaveArgs& a, int ff, const feta_colsum_seg* segs, int nseg, hipStream_t stream) {
  return ff == 64 ? launch_fwd_save<T, NT, DH, 64>(a, segs, nseg, stream) : launch_fwd_save<T, NT, DH, 128>(a, segs, nseg, stream);
}

template <int NT>
int launch_fwd_save_heads(InferSaveArgs& a, int dtype, int heads, int ff, const feta_colsum_seg* segs, int nseg,
                          hipStream_t stream) {
  if (dtype == FETA_BF16) return launch_fwd_save_ff<bf16_t, NT, 16>(a, ff, segs, nseg, stream);
  return heads == 4 ? launch_fwd_save_ff<float, NT, 16>(a, ff, segs, nseg, stream)
                    : launch_fwd_save_ff<float, NT, 8>(a, ff, segs, nseg, stream);
}

// checks and argument block shared by the inference entry points and feta_encoder_fwd_save
int fill_infer_args(const struct feta_encoder_infer_ex* d, const char* what, InferArgs& a) {
  FETA_REQUIRE(d != nullptr, "%s: null descriptor", what);
  FETA_REQUIRE(d->dtype == FETA_F32 || d->dtype == FETA_BF16, "%s: dtype %d is neither FETA_F32 nor FETA_BF16", what, d->dtype);
  FETA_REQUIRE(d->in_dtype == FETA_F32 || d->in_dtype == FETA_BF16, "%s: in_dtype %d is neither FETA_F32 nor FETA_BF16",
               what, d->in_dtype);
  FETA_REQUIRE(d->dtype == FETA_F32 || d->H == 4, "%s: H=%d with dtype FETA_BF16 - the bf16 form has 4 heads (d_h = 16) only",
               what, d->H);
  FETA_REQUIRE(feta_encoder_infer_ex_supported(d->N, kInfD, d->H, d->FF, d->L, d->dtype),
               "%s: N=%d H=%d ff=%d L=%d outside 1 <= N <= 64, H in {4, 8}, ff in {64, 128}, 1 <= L <= %d",
               what, d->N, d->H, d->FF, d->L, FETA_ENCODER_MAX_LAYERS);
  FETA_REQUIRE(d->dtype == FETA_BF16 || d->in_dtype == FETA_F32, "%s: in_dtype FETA_BF16 needs dtype FETA_BF16 (the fp32 "
               "form reads fp32 x and pe)", what);
  FETA_REQUIRE(d->B > 0, "%s: B=%d", what, d->B);
  FETA_REQUIRE(d->norm == FETA_NORM_BATCH || d->norm == FETA_NORM_LAYER, "%s: norm kind %d", what, d->norm);
  FETA_REQUIRE(d->x && d->n_real && d->y && d->out && d->layers, "%s: null pointer", what);
  FETA_REQUIRE(aligned16(d->x) && aligned16(d->y) && aligned16(d->out), "%s: x, y, out must be 16-byte aligned", what);
  FETA_REQUIRE(d->row_sb >= 0 && d->row_sn >= 0, "%s: negative row strides", what);
  a.x = d->x;
  a.pe = d->pe;
  a.n_real = d->n_real;
  a.rowscale = d->rowscale;
  a.y = d->y;
  a.out = d->out;
  a.attn = d->attn;
  a.row_sb = d->row_sb;
  a.row_sn = d->row_sn;
  a.B = d->B;
  a.N = d->N;
  a.L = d->L;
  a.norm = d->norm;
  a.scale = (float)(1.0 / std::sqrt((double)(kInfD / d->H)));
  a.in_bf16 = d->in_dtype == FETA_BF16;
  for (int l = 0; l < d->L; ++l) {
    const feta_encoder_layer& p = d->layers[l];
    FETA_REQUIRE(p.w_in && p.w_out && p.w1 && p.w2 && p.n1_gamma && p.n1_beta && p.n2_gamma && p.n2_beta,
                 "%s: layer %d: null weight or norm parameter", what, l);
    FETA_REQUIRE(aligned16(p.w_in) && aligned16(p.b_in) && aligned16(p.w_out) && aligned16(p.b_out) && aligned16(p.w1) &&
                 aligned16(p.b1) && aligned16(p.w2) && aligned16(p.b2),
                 "%s: layer %d: weights and biases must be 16-byte aligned", what, l);
    FETA_REQUIRE(d->norm != FETA_NORM_BATCH || (p.n1_mean && p.n1_var && p.n2_mean && p.n2_var),
                 "%s: layer %d: BatchNorm needs running_mean and running_var", what, l);
    FETA_REQUIRE(p.n1_eps >= 0.0f && p.n2_eps >= 0.0f, "%s: layer %d: negative eps", what, l);
    a.layers[l] = p;
  }
  return FETA_OK;
}

// both entry points: `what` names the one that was called in every message
int run_infer(const struct feta_encoder_infer_ex* d, feta_stream_t stream, const char* what) {
  InferArgs a{};
  if (const int rc = fill_infer_args(d, what, a)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const char* name = d->dtype == FETA_BF16 ? "feta_encoder_infer_ex (bf16)" : "feta_encoder_infer";
  switch ((d->N + 15) / 16) {
    case 1: return launch_infer_heads<1>(a, d->dtype, d->H, d->FF, s, name);
    case 2: return launch_infer_heads<2>(a, d->dtype, d->H, d->FF, s, name);
    case 3: return launch_infer_heads<3>(a, d->dtype, d->H, d->FF, s, name);
    default: return launch_infer_heads<4>(a, d->dtype, d->H, d->FF, s, name);
  }
}

}  // namespace feta

using namespace feta;

extern "C" int feta_encoder_infer_supported(int N, int d_model, int heads, int ff, int L) {
  return (d_model == kInfD && (heads == 4 || heads == 8) && N >= 1 && N <= 64 && (ff == 64 || ff == 128) && L >= 1 &&
          L <= FETA_ENCODER_MAX_LAYERS) ? 1 : 0;
}

extern "C" int feta_encoder_infer_ex_supported(int N, int d_model, int heads, int ff, int L, int dtype) {
  if (dtype == FETA_F32) return feta_encoder_infer_supported(N, d_model, heads, ff, L);
  return (dtype == FETA_BF16 && heads == 4 && feta_encoder_infer_supported(N, d_model, heads, ff, L)) ? 1 : 0;
}

extern "C" int feta_encoder_infer(const struct feta_encoder_infer* d, feta_stream_t stream) {
  FETA_REQUIRE(d != nullptr, "encoder_infer: null descriptor");
  struct feta_encoder_infer_ex e{};
  e.x = d->x;
  e.row_sb = d->row_sb;
  e.row_sn = d->row_sn;
  e.pe = d->pe;
  e.n_real = d->n_real;
  e.rowscale = d->rowscale;
  e.y = d->y;
  e.out = d->out;
  e.attn = d->attn;
  e.B = d->B;
  e.N = d->N;
  e.H = d->H;
  e.FF = d->FF;
  e.L = d->L;
  e.norm = d->norm;
  e.layers = d->layers;
  e.dtype = e.in_dtype = FETA_F32;
  return run_infer(&e, stream, "encoder_infer");
}

extern "C" int feta_encoder_infer_ex(const struct feta_encoder_infer_ex* d, feta_stream_t stream) {
  return run_infer(d, stream, "encoder_infer_ex");
}

extern "C" int feta_encoder_fwd_save_supported(int N, int d_model, int heads, int ff, int L, int dtype, int tie_qk) {
  return (tie_qk == 0 && feta_encoder_infer_ex_supported(N, d_model, heads, ff, L, dtype)) ? 1 : 0;
}

extern "C" int feta_encoder_fwd_save(const struct feta_encoder_fwd_save* d, feta_stream_t stream) {
  return feta_encoder_fwd_save_sums(d, nullptr, 0, stream);
}

extern "C" int feta_encoder_fwd_save_sums(const struct feta_encoder_fwd_save* d, const feta_colsum_seg* segs, int nseg,
                                          feta_stream_t stream) {
  const char* what = "encoder_fwd_save";
  FETA_REQUIRE(d != nullptr, "%s: null descriptor", what);
  FETA_REQUIRE(nseg >= 0 && nseg <= FETA_COLSUM_MAX_SEGS && (nseg == 0 || segs != nullptr),
               "%s: 0..%d column-sum segments", what, FETA_COLSUM_MAX_SEGS);
  for (int i = 0; i < nseg; ++i) FETA_REQUIRE(colsum_seg_ok(segs[i]), "%s: bad segment %d", what, i);
  FETA_REQUIRE(d->norm == FETA_NORM_LAYER, "%s: norm kind %d - the training forward is one launch for LayerNorm stacks only "
               "(BatchNorm batch statistics couple the graphs)", what, d->norm);
  FETA_REQUIRE(d->dtype == FETA_F32 || d->dtype == FETA_BF16, "%s: dtype %d is neither FETA_F32 nor FETA_BF16", what, d->dtype);
  FETA_REQUIRE(d->dtype == FETA_F32 || d->H == 4, "%s: H=%d with dtype FETA_BF16 - the bf16 form has 4 heads (d_h = 16) only",
               what, d->H);
  FETA_REQUIRE(d->in_dtype == d->dtype, "%s: in_dtype %d differs from dtype %d - x is layer 0's saved x0, in the storage "
               "type the backward reads", what, d->in_dtype, d->dtype);
  FETA_REQUIRE(d->L >= 1 && d->L <= FETA_ENCODER_MAX_LAYERS && d->layers != nullptr, "%s: L=%d outside 1..%d or no layer table",
               what, d->L, FETA_ENCODER_MAX_LAYERS);
  for (int l = 0; l < d->L; ++l)
    FETA_REQUIRE(d->layers[l].tie_qk == 0, "%s: layer %d: tie_qk - feta_attn_block_bwd has no tied form", what, l);
  FETA_REQUIRE(d->qkv && d->out_save && d->attn_stats && d->y1 && d->h && d->y2, "%s: null save pointer", what);
  FETA_REQUIRE(d->dtype == FETA_F32 || d->y2_last_f32 != nullptr, "%s: dtype FETA_BF16 needs y2_last_f32 (the last layer's "
               "y2 leaves as fp32)", what);
  FETA_REQUIRE(d->dtype == FETA_F32 || d->out != nullptr, "%s: dtype FETA_BF16 needs out (the fp32 copy of the last layer's "
               "concatenated heads)", what);
  FETA_REQUIRE(aligned16(d->qkv) && aligned16(d->out_save) && aligned16(d->attn_stats) && aligned16(d->y1) && aligned16(d->h) &&
               aligned16(d->y2) && aligned16(d->y2_last_f32), "%s: save pointers must be 16-byte aligned", what);
  const int64_t strides[6] = {d->qkv_stride, d->out_stride, d->attn_stats_stride, d->y1_stride, d->h_stride, d->y2_stride};
  for (int i = 0; i < 6; ++i) {
    FETA_REQUIRE(d->L == 1 || strides[i] > 0, "%s: layer stride %d is %lld - L > 1 needs positive strides", what, i,
                 (long long)strides[i]);
    // (8 elements: 16 bytes of bf16, a multiple of 16 bytes of fp32 - every layer's view stays aligned)
    FETA_REQUIRE(strides[i] >= 0 && strides[i] % 8 == 0 && strides[i] <= 0x7fffffff,
                 "%s: layer stride %d is %lld - a non-negative multiple of 8 elements below 2^31", what, i, (long long)strides[i]);
  }
  struct feta_encoder_infer_ex e{};
  e.x = d->x;
  e.row_sb = d->row_sb;
  e.row_sn = d->row_sn;
  e.pe = d->pe;
  e.n_real = d->n_real;
  e.rowscale = d->rowscale;
  e.y = d->y;
  e.out = d->out != nullptr ? d->out : d->y;   // (fill_infer_args wants one; fp32 storage may leave it NULL - see below)
  e.attn = d->attn;
  e.B = d->B;
  e.N = d->N;
  e.H = d->H;
  e.FF = d->FF;
  e.L = d->L;
  e.norm = d->norm;
  e.layers = d->layers;
  e.dtype = d->dtype;
  e.in_dtype = d->in_dtype;
  InferSaveArgs a{};
  if (const int rc = fill_infer_args(&e, what, a)) return rc;
  a.out = d->out;
  a.s.qkv = d->qkv;
  a.s.out = d->out_save;
  a.s.ast = d->attn_stats;
  a.s.y1 = d->y1;
  a.s.h = d->h;
  a.s.y2 = d->y2;
  a.s.y2_last_f32 = d->y2_last_f32;
  a.s.qkv_sl = (int)d->qkv_stride;
  a.s.out_sl = (int)d->out_stride;
  a.s.ast_sl = (int)d->attn_stats_stride;
  a.s.y1_sl = (int)d->y1_stride;
  a.s.h_sl = (int)d->h_stride;
  a.s.y2_sl = (int)d->y2_stride;
  hipStream_t s = (hipStream_t)stream;
  switch ((d->N + 15) / 16) {
    case 1: return launch_fwd_save_heads<1>(a, d->dtype, d->H, d->FF, segs, nseg, s);
    case 2: return launch_fwd_save_heads<2>(a, d->dtype, d->H, d->FF, segs, nseg, s);
    case 3: return launch_fwd_save_heads<3>(a, d->dtype, d->H, d->FF, segs, nseg, s);
    default: return launch_fwd_save_heads<4>(a, d->dtype, d->H, d->FF, segs, nseg, s);
  }
}
