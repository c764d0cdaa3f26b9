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
// Eight waves (512 lanes), two per SIMD: one wave's VALU and LDS work issues under the other's 32-cycle MFMAs, and the
// phases have 12 NT, H NT, 4 NT and ff / 16 NT work items (NT = 16-row tiles of the graph: at the ZINC shape 36, 12 - 24,
// 12, 24) - sixteen waves would leave most of them idle in every phase but in_proj, four would put a single wave on a SIMD.
#include <cmath>
#include <cstdlib>

#include "feta_abi_common.h"
#include "feta_ln.h"

namespace feta {

constexpr int kInfD = 64;
constexpr int kInfP = kInfD + 4;        // LDS pitch of a 64-float row (16-byte operand reads)
constexpr int kInfQP = 3 * kInfD + 4;   // ... of a q | k | v row; the hidden rows h (pitch ff + 4) reuse that tile
constexpr int kInfWaves = 8, kInfThreads = 64 * kInfWaves;
constexpr int kInfMaxGrid = 512;        // graphs in flight (two workgroups per CU where the LDS allows); beyond that a
                                        // workgroup walks graphs b, b + grid, ...

// Kernel arguments: the layer table travels BY VALUE (no device table, no copy before the launch: capturable as is).
struct InferArgs {
  const float* x;
  const float* pe;
  const int32_t* n_real;
  const float* rowscale;
  float* y;
  float* out;
  float* attn;
  int64_t row_sb, row_sn;
  int B, N, L, norm;
  float scale;
  feta_encoder_layer layers[FETA_ENCODER_MAX_LAYERS];
};
static_assert(sizeof(InferArgs) <= 4096, "the layer table must fit HIP's 4 KB of kernel arguments");

__host__ __device__ inline int infer_lds_bytes(int nt, bool pe) {
  const int nr = 16 * nt;
  return 4 * (2 * nr * kInfP + nr * kInfQP + (pe ? nr * (nr + 4) : 0));
}

// rows . W^T over K features for all CT x NT output tiles, register r of a tile <-> (output column 16 ct + 4 g + r,
// row 16 rt + lq); epi(ct, rt, acc) consumes a tile.  Tiles are dealt to the waves in contiguous column-major runs, so a
// wave's consecutive tiles mostly share a column tile and its weight operand (read from global memory) is loaded once
// per run, not once per tile.  skip(ct): column tiles nobody needs (wave-uniform).
template <int K, int CT, int NT, class Skip, class Epi>
__device__ __forceinline__ void infer_gemm(const float* rows, int pitch, const float* w, int wave, int lq, int g,
                                           Skip skip, Epi epi) {
  constexpr int total = CT * NT, per = (total + kInfWaves - 1) / kInfWaves;
  Feat<K> wf;
  int wct = -1;
  for (int t = wave * per; t < (wave + 1) * per && t < total; ++t) {
    const int ct = t / NT, rt = t - ct * NT;
    if (skip(ct)) continue;
    if (ct != wct) {
      load_row<K>(wf, w + (int64_t)(16 * ct + lq) * K, g);
      wct = ct;
    }
    Feat<K> xf;
    load_row<K>(xf, rows + (16 * rt + lq) * pitch, g);
    epi(ct, rt, dot_rows<K>(wf, xf, zero4()));
  }
}

__device__ __forceinline__ float4 infer_bias4(const float* b, int c) {
  return b != nullptr ? *reinterpret_cast<const float4*>(b + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// norm1 / norm2 of every staged row, in place: 16 lanes per row, four columns each (NR * 16 lanes are whole waves, so
// the DPP row sums of the LayerNorm run in complete waves)
template <int NR>
__device__ __forceinline__ void infer_norm_rows(float* Xs, int norm, const float* gamma, const float* beta,
                                                const float* mean, const float* var, float eps) {
  for (int idx = threadIdx.x; idx < NR * 16; idx += kInfThreads) {
    const int c = 4 * (idx & 15);
    float4* p = reinterpret_cast<float4*>(Xs + (idx >> 4) * kInfP + c);
    const float4 v = *p;
    float f[4] = {v.x, v.y, v.z, v.w};
    if (norm == FETA_NORM_LAYER) {
      ln_apply<4>(f, gamma + c, beta + c, eps);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = (f[e] - mean[c + e]) * rsqrtf(var[c + e] + eps) * gamma[c + e] + beta[c + e];
    }
    *p = make_float4(f[0], f[1], f[2], f[3]);
  }
}

template <int NT, int DH, int FF>
__global__ __launch_bounds__(kInfThreads) void encoder_infer_kernel(InferArgs a) {
  constexpr int NR = 16 * NT, H = kInfD / DH, PEP = NR + 4, HP = FF + 4;
  static_assert(HP <= kInfQP, "the hidden rows reuse the q | k | v tile");
  float* Xs = feta_lds;              // [NR][kInfP]  layer input -> y1 -> x1 -> y2 -> next layer's input
  float* QKV = Xs + NR * kInfP;      // [NR][kInfQP] q | k | v;  h [NR][HP] after the attention phase
  float* Os = QKV + NR * kInfQP;     // [NR][kInfP]  concatenated heads
  float* Pe = Os + NR * kInfP;       // [NR][PEP]    pe of the graph (zero outside N x N), when given
  float* Hs = QKV;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lq = lane & 15, g = lane >> 4;
  const bool has_pe = a.pe != nullptr;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int n = a.n_real[b];
    // ---- the graph's rows (rows >= N: zero, computed like the others and never stored) and its pe block ----
    for (int idx = tid; idx < NR * 16; idx += kInfThreads) {
      const int i = idx >> 4, c = 4 * (idx & 15);
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (i < a.N) v = *reinterpret_cast<const float4*>(a.x + ((int64_t)b * a.row_sb + (int64_t)i * a.row_sn) * kInfD + c);
      *reinterpret_cast<float4*>(Xs + i * kInfP + c) = v;
    }
    if (has_pe) {
      for (int idx = tid; idx < NR * NR; idx += kInfThreads) {
        const int i = idx / NR, k = idx - i * NR;
        Pe[i * PEP + k] = (i < a.N && k < a.N) ? a.pe[((int64_t)b * a.N + i) * a.N + k] : 0.0f;
      }
    }
    lds_barrier();
    for (int l = 0; l < a.L; ++l) {
      const feta_encoder_layer& p = a.layers[l];
      const bool last = l + 1 == a.L;
      // ---- 1. in_proj ----
      const bool tie = p.tie_qk != 0;
      infer_gemm<kInfD, 12, NT>(Xs, kInfP, p.w_in, w, lq, g, [&](int ct) { return tie && ct >= 4 && ct < 8; },  // K is Q
                                [&](int ct, int rt, f32x4 acc) {
        const float4 bv = infer_bias4(p.b_in, 16 * ct + 4 * g);
        *reinterpret_cast<float4*>(QKV + (16 * rt + lq) * kInfQP + 16 * ct + 4 * g) =
            make_float4(acc[0] + bv.x, acc[1] + bv.y, acc[2] + bv.z, acc[3] + bv.w);
      });
      lds_barrier();
      // ---- 2. attention: (head h, query tile qb) ----
      const float* Ks = QKV + (p.tie_qk ? 0 : kInfD);
      const float* Vs = QKV + 2 * kInfD;
      for (int t = w; t < H * NT; t += kInfWaves) {
        const int h = t % H, qb = t / H, q = 16 * qb + lq;
        Feat<DH> qf;
        load_row<DH>(qf, QKV + q * kInfQP + DH * h, g, a.scale);
        f32x4 s[NT];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          s[kt] = zero4();
          if (16 * kt < n) {   // a key tile without a real node: nothing (wave-uniform)
            Feat<DH> kf;
            load_row<DH>(kf, Ks + (16 * kt + lq) * kInfQP + DH * h, g);
            s[kt] = dot_rows<DH>(kf, qf, zero4());   // (key 16 kt + 4 g + r, query q)
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
          float4 pv = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
          if (has_pe) pv = *reinterpret_cast<const float4*>(Pe + q * PEP + 16 * kt + 4 * g);
          const float pr[4] = {pv.x, pv.y, pv.z, pv.w};
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
        f32x4 o = zero4();
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          if (16 * kt >= n) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) s[kt][r] *= rinv;
          // P (query lq, key 16 kt + 4 g + r) as the A operand of step r, V (that key, column lq of the head) as B;
          // padded keys carry no value, lanes lq >= DH (d_h = 8: half a tile) feed columns nobody stores
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = 16 * kt + 4 * g + r;
            const float v = (key < n && lq < DH) ? Vs[key * kInfQP + DH * h + lq] : 0.0f;
            o = mfma16(s[kt][r], v, o);   // (query 16 qb + 4 g + r, column lq)
          }
        }
        if (lq < DH) {
#pragma unroll
          for (int r = 0; r < 4; ++r) Os[(16 * qb + 4 * g + r) * kInfP + DH * h + lq] = o[r];
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
      // ---- 3. out_proj + bias, * degree, + residual (in place) ----
      const auto none = [](int) { return false; };
      infer_gemm<kInfD, 4, NT>(Os, kInfP, p.w_out, w, lq, g, none, [&](int ct, int rt, f32x4 acc) {
        const int node = 16 * rt + lq, c0 = 16 * ct + 4 * g;
        const float4 bo = infer_bias4(p.b_out, c0);
        const float rs = (a.rowscale != nullptr && node < a.N)
                             ? a.rowscale[(int64_t)b * a.row_sb + (int64_t)node * a.row_sn] : 1.0f;
        float4* xr = reinterpret_cast<float4*>(Xs + node * kInfP + c0);
        const float4 x = *xr;
        *xr = make_float4((acc[0] + bo.x) * rs + x.x, (acc[1] + bo.y) * rs + x.y, (acc[2] + bo.z) * rs + x.z,
                          (acc[3] + bo.w) * rs + x.w);
      });
      lds_barrier();
      // ---- 4. norm1 ----
      infer_norm_rows<NR>(Xs, a.norm, p.n1_gamma, p.n1_beta, p.n1_mean, p.n1_var, p.n1_eps);
      lds_barrier();
      // ---- 5. linear1 + relu -> h; linear2 + bias + residual (in place) ----
      infer_gemm<kInfD, FF / 16, NT>(Xs, kInfP, p.w1, w, lq, g, none, [&](int ct, int rt, f32x4 acc) {
        const float4 bv = infer_bias4(p.b1, 16 * ct + 4 * g);
        *reinterpret_cast<float4*>(Hs + (16 * rt + lq) * HP + 16 * ct + 4 * g) =
            make_float4(fmaxf(acc[0] + bv.x, 0.0f), fmaxf(acc[1] + bv.y, 0.0f), fmaxf(acc[2] + bv.z, 0.0f),
                        fmaxf(acc[3] + bv.w, 0.0f));
      });
      lds_barrier();
      infer_gemm<FF, 4, NT>(Hs, HP, p.w2, w, lq, g, none, [&](int ct, int rt, f32x4 acc) {
        const int c0 = 16 * ct + 4 * g;
        const float4 bv = infer_bias4(p.b2, c0);
        float4* xr = reinterpret_cast<float4*>(Xs + (16 * rt + lq) * kInfP + c0);
        const float4 x = *xr;
        *xr = make_float4(x.x + (acc[0] + bv.x), x.y + (acc[1] + bv.y), x.z + (acc[2] + bv.z), x.w + (acc[3] + bv.w));
      });
      lds_barrier();
      // ---- 6. norm2 ----
      infer_norm_rows<NR>(Xs, a.norm, p.n2_gamma, p.n2_beta, p.n2_mean, p.n2_var, p.n2_eps);
      lds_barrier();
    }
    // ---- the last layer's output rows and concatenated heads ----
    for (int idx = tid; idx < a.N * 16; idx += kInfThreads) {
      const int i = idx >> 4, c = 4 * (idx & 15);
      const int64_t row = (int64_t)b * a.row_sb + (int64_t)i * a.row_sn;
      *reinterpret_cast<float4*>(a.y + row * kInfD + c) = *reinterpret_cast<const float4*>(Xs + i * kInfP + c);
      *reinterpret_cast<float4*>(a.out + row * kInfD + c) = *reinterpret_cast<const float4*>(Os + i * kInfP + c);
    }
    lds_barrier();   // (the next graph's rows overwrite Xs)
  }
}

template <int NT, int DH, int FF>
int launch_infer(const InferArgs& a, hipStream_t stream) {
  const size_t lds = infer_lds_bytes(NT, a.pe != nullptr);
  auto kern = encoder_infer_kernel<NT, DH, FF>;
  static LdsSeen lds_seen;
  allow_dynamic_lds(kern, lds, lds_seen);
  int cap = kInfMaxGrid;   // FETA_INFER_MAX_GRID: tests force the walking loop
  if (const char* e = getenv("FETA_INFER_MAX_GRID")) cap = atoi(e) > 0 ? atoi(e) : cap;
  const int grid = a.B < cap ? a.B : cap;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kInfThreads), lds, stream, a);
  return check_launch("feta_encoder_infer");
}

template <int NT, int DH>
int launch_infer_ff(const InferArgs& a, int ff, hipStream_t stream) {
  return ff == 64 ? launch_infer<NT, DH, 64>(a, stream) : launch_infer<NT, DH, 128>(a, stream);
}

template <int NT>
int launch_infer_heads(const InferArgs& a, int heads, int ff, hipStream_t stream) {
  return heads == 4 ? launch_infer_ff<NT, 16>(a, ff, stream) : launch_infer_ff<NT, 8>(a, ff, stream);
}

}  // namespace feta

using namespace feta;

extern "C" int feta_encoder_infer_supported(int N, int d_model, int heads, int ff, int L) {
  return (d_model == kInfD && (heads == 4 || heads == 8) && N >= 1 && N <= 64 && (ff == 64 || ff == 128) && L >= 1 &&
          L <= FETA_ENCODER_MAX_LAYERS) ? 1 : 0;
}

extern "C" int feta_encoder_infer(const struct feta_encoder_infer* d, feta_stream_t stream) {
  FETA_REQUIRE(d != nullptr, "encoder_infer: null descriptor");
  FETA_REQUIRE(feta_encoder_infer_supported(d->N, kInfD, d->H, d->FF, d->L),
               "encoder_infer: N=%d H=%d ff=%d L=%d outside 1 <= N <= 64, H in {4, 8}, ff in {64, 128}, 1 <= L <= %d",
               d->N, d->H, d->FF, d->L, FETA_ENCODER_MAX_LAYERS);
  FETA_REQUIRE(d->B > 0, "encoder_infer: B=%d", d->B);
  FETA_REQUIRE(d->norm == FETA_NORM_BATCH || d->norm == FETA_NORM_LAYER, "encoder_infer: norm kind %d", d->norm);
  FETA_REQUIRE(d->x && d->n_real && d->y && d->out && d->layers, "encoder_infer: null pointer");
  FETA_REQUIRE(aligned16(d->x) && aligned16(d->y) && aligned16(d->out), "encoder_infer: x, y, out must be 16-byte aligned");
  FETA_REQUIRE(d->row_sb >= 0 && d->row_sn >= 0, "encoder_infer: negative row strides");
  InferArgs a{};
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
  for (int l = 0; l < d->L; ++l) {
    const feta_encoder_layer& p = d->layers[l];
    FETA_REQUIRE(p.w_in && p.w_out && p.w1 && p.w2 && p.n1_gamma && p.n1_beta && p.n2_gamma && p.n2_beta,
                 "encoder_infer: layer %d: null weight or norm parameter", l);
    FETA_REQUIRE(aligned16(p.w_in) && aligned16(p.b_in) && aligned16(p.w_out) && aligned16(p.b_out) && aligned16(p.w1) &&
                 aligned16(p.b1) && aligned16(p.w2) && aligned16(p.b2),
                 "encoder_infer: layer %d: weights and biases must be 16-byte aligned", l);
    FETA_REQUIRE(d->norm != FETA_NORM_BATCH || (p.n1_mean && p.n1_var && p.n2_mean && p.n2_var),
                 "encoder_infer: layer %d: BatchNorm needs running_mean and running_var", l);
    FETA_REQUIRE(p.n1_eps >= 0.0f && p.n2_eps >= 0.0f, "encoder_infer: layer %d: negative eps", l);
    a.layers[l] = p;
  }
  hipStream_t s = (hipStream_t)stream;
  switch ((d->N + 15) / 16) {
    case 1: return launch_infer_heads<1>(a, d->H, d->FF, s);
    case 2: return launch_infer_heads<2>(a, d->H, d->FF, s);
    case 3: return launch_infer_heads<3>(a, d->H, d->FF, s);
    default: return launch_infer_heads<4>(a, d->H, d->FF, s);
  }
}
