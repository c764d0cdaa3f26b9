// The "dW" product of the coefficient generator's C x C linear (lin.hip: dW[n][k] = sum_r dy[r][n] x[r][k], db[n] = sum_r
// dy[r][n]) as a ROLE: trailing 512-thread workgroups of a launch that leaves CUs idle (the first layer's
// attn_block_bwd_kernel, block_bwd.hip: one workgroup per graph, half the chip at the BASELINE batch).
//
// Same chunk pipeline as lin_tiled_body (lin.hip): the contraction is staged through LDS in chunks of 64 rows, two register
// sets of staged chunks in flight in front of an LDS double buffer, ONE barrier per chunk, tile addresses computed from the
// buffer index.  What differs is the shape: 8 waves on a 128 x 64 output tile, every wave a 32 x 32 block = 2 x 2
// accumulator tiles, so that two 8-byte LDS reads feed four MFMAs (lin_tiled_body: three operand reads - one of them a
// four-scalar gather - per two MFMAs, 35 % pipe busy).  Both operands are [kk][outer] in memory and in LDS; a lane reads
// two ADJACENT outer indices per operand, i.e. row 2 m + a of the wave's block is row m of accumulator tile a (and the
// same for columns) - the permutation costs nothing and makes the result stores 8 bytes wide.
//
// Arithmetic: v_mfma_f32_16x16x4_f32, exact fp32; MFMA s of a chunk contracts rows 4 s .. 4 s + 3, chunks ascend - the
// same order for every output element whatever the grid: deterministic, independent of how many workgroups take part.
// db: fp32 sums of the staged dy values (the workgroups of the first tile column), fixed order.
#pragma once
#include "feta_abi_common.h"
#include <feta_device.h>
#include "feta_gstore.h"
#include "feta_tiles.h"

namespace feta {

constexpr int kDwThreads = 512;
constexpr int kDwI = 128, kDwJ = 64, kDwK = 64;      // output tile (dW rows x columns), contraction chunk
constexpr int kDwPP = kDwI + 4, kDwQP = kDwJ + 4;    // LDS pitches
constexpr int kDwPSZ = kDwK * kDwPP, kDwQSZ = kDwK * kDwQP;

__host__ __device__ constexpr int lin_dw_lds_bytes() { return 2 * (kDwPSZ + kDwQSZ) * (int)sizeof(float); }

struct LinDwPlan {
  const float* dy;   // [R][N]
  const float* x;    // [R][K]
  float* dw;         // [N][K]
  float* db;         // [N], nullable
  int R, K, N;
  int tj;            // tile columns, K / kDwJ
  int tiles;         // (N / kDwI) * tj
  int wgs;           // role workgroups: workgroup w takes tiles w, w + wgs, ...  (0: no role in this launch)
};

inline int lin_dw_tiles(int K, int N) { return (N / kDwI) * (K / kDwJ); }

inline bool lin_dw_shape_ok(int R, int K, int N) {
  return R >= kDwK && R % kDwK == 0 && K >= kDwJ && K % kDwJ == 0 && N >= kDwI && N % kDwI == 0;
}

// XCD-aware tile order (cf. lin_tile_of): workgroups are dealt round-robin to the 8 XCDs, so tiles t, t + 8, ... meet in one
// L2.  Tile t is element (t & 7) * tiles / 8 + (t >> 3) of the row-major tile list: an XCD walks a contiguous run of it,
// i.e. all its tiles share one (or few) tile rows - its dy columns are fetched from HBM once.  tiles % 8 != 0: row-major.
__device__ __forceinline__ void lin_dw_tile_of(int t, int tiles, int TJ, int& ti, int& tj) {
  const int lin = (tiles & 7) == 0 ? (t & 7) * (tiles >> 3) + (t >> 3) : t;
  ti = lin / TJ;
  tj = lin - ti * TJ;
}

// one chunk of an operand in registers: kDwK x COLS floats, COLS / 4 16-byte vectors per row, kDwThreads threads
template <int COLS>
struct DwStage {
  static constexpr int NV = kDwK * COLS / 4 / kDwThreads;   // 4 (P) or 2 (Q)
  f32x4 v0, v1, v2, v3;   // (the MFMA vector type: a float4 STRUCT that is only copied is moved by memcpy through private memory)
  __device__ __forceinline__ static const f32x4* at(const float* src, int64_t ld, int r0, int c0, int u) {
    const int idx = threadIdx.x + u * kDwThreads, rr = idx / (COLS / 4), c4 = idx % (COLS / 4);
    return reinterpret_cast<const f32x4*>(src + (int64_t)(r0 + rr) * ld + c0 + 4 * c4);
  }
  __device__ __forceinline__ void load(const float* src, int64_t ld, int r0, int c0) {
    v0 = *at(src, ld, r0, c0, 0);
    v1 = *at(src, ld, r0, c0, 1);
    if constexpr (NV > 2) {
      v2 = *at(src, ld, r0, c0, 2);
      v3 = *at(src, ld, r0, c0, 3);
    }
  }
  __device__ __forceinline__ static f32x4* slot(float* tile, int pitch, int u) {
    const int idx = threadIdx.x + u * kDwThreads, rr = idx / (COLS / 4), c4 = idx % (COLS / 4);
    return reinterpret_cast<f32x4*>(tile + rr * pitch + 4 * c4);
  }
  __device__ __forceinline__ void store(float* tile, int pitch) const {
    *slot(tile, pitch, 0) = v0;
    *slot(tile, pitch, 1) = v1;
    if constexpr (NV > 2) {
      *slot(tile, pitch, 2) = v2;
      *slot(tile, pitch, 3) = v3;
    }
  }
};

// one 128 x 64 tile of dW (and, first tile column, 128 elements of db); every thread of the workgroup calls it
__device__ __forceinline__ void lin_dw_tile(const LinDwPlan& a, int ti, int tj) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lq = lane & 15, g = lane >> 4;
  const int iw = wv & 3, jw = wv >> 2;   // the wave's 32 x 32 block of the tile
  float* base = feta_lds;
  const int i0 = kDwI * ti, j0 = kDwJ * tj;
  DwStage<kDwI> psA, psB;
  DwStage<kDwJ> qsA, qsB;
  const float* gp = a.dy;
  const float* gq = a.x;
  const int ldp = a.N, ldq = a.K;
  auto request = [gp, gq, ldp, ldq, i0, j0](DwStage<kDwI>& ps, DwStage<kDwJ>& qs, int c) __attribute__((always_inline)) {
    ps.load(gp, ldp, kDwK * c, i0);
    qs.load(gq, ldq, kDwK * c, j0);
  };
  // fp32 column sums of the staged dy values: this thread's float4s cover four consecutive i of the rows it stages
  // (scalars and four named accumulators below, not arrays: captured by reference, arrays stayed in private memory)
  float rs0 = 0.0f, rs1 = 0.0f, rs2 = 0.0f, rs3 = 0.0f;
  auto commit = [&rs0, &rs1, &rs2, &rs3, base](const DwStage<kDwI>& ps, const DwStage<kDwJ>& qs, int buf) __attribute__((always_inline)) {
    ps.store(base + buf * kDwPSZ, kDwPP);
    qs.store(base + 2 * kDwPSZ + buf * kDwQSZ, kDwQP);
    rs0 += ps.v0[0]; rs1 += ps.v0[1]; rs2 += ps.v0[2]; rs3 += ps.v0[3];
    rs0 += ps.v1[0]; rs1 += ps.v1[1]; rs2 += ps.v1[2]; rs3 += ps.v1[3];
    rs0 += ps.v2[0]; rs1 += ps.v2[1]; rs2 += ps.v2[2]; rs3 += ps.v2[3];
    rs0 += ps.v3[0]; rs1 += ps.v3[1]; rs2 += ps.v3[2]; rs3 += ps.v3[3];
  };
  f32x4 a00 = zero4(), a01 = zero4(), a10 = zero4(), a11 = zero4();
  auto compute = [&a00, &a01, &a10, &a11, base, iw, jw, lq, g](int buf) __attribute__((always_inline)) {
    const float* pt = base + buf * kDwPSZ + g * kDwPP + 32 * iw + 2 * lq;
    const float* qt = base + 2 * kDwPSZ + buf * kDwQSZ + g * kDwQP + 32 * jw + 2 * lq;
#pragma unroll
    for (int s = 0; s < kDwK / 4; ++s) {
      const float2 p = *reinterpret_cast<const float2*>(pt + 4 * s * kDwPP);   // dy[kk = 4 s + g][i = .. + 2 lq + {0, 1}]
      const float2 q = *reinterpret_cast<const float2*>(qt + 4 * s * kDwQP);   // x [kk][j = .. + 2 lq + {0, 1}]
      a00 = mfma16(p.x, q.x, a00);
      a01 = mfma16(p.x, q.y, a01);
      a10 = mfma16(p.y, q.x, a10);
      a11 = mfma16(p.y, q.y, a11);
    }
  };
  const int nc = a.R / kDwK;
  request(psA, qsA, 0);
  commit(psA, qsA, 0);
  if (1 < nc) request(psA, qsA, 1);
  if (2 < nc) request(psB, qsB, 2);
  __syncthreads();
  for (int c = 0; c < nc; c += 2) {
    // LDS buffer 0 holds chunk c; A: chunk c + 1, B: chunk c + 2 (in flight)
    compute(0);
    if (c + 1 < nc) commit(psA, qsA, 1);
    if (c + 3 < nc) request(psA, qsA, c + 3);
    __syncthreads();
    if (c + 1 < nc) {
      compute(1);
      if (c + 2 < nc) commit(psB, qsB, 0);
      if (c + 4 < nc) request(psB, qsB, c + 4);
      __syncthreads();
    }
  }
  // register r of accumulator (ta, tb) is dW[i0 + 32 iw + 2 (4 g + r) + ta][j0 + 32 jw + 2 lq + tb]
  float* out = a.dw + (int64_t)(i0 + 32 * iw + 8 * g) * a.K + j0 + 32 * jw + 2 * lq;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gst2<kStPartial>(out + (int64_t)(2 * r) * a.K, a00[r], a01[r]);
    gst2<kStPartial>(out + (int64_t)(2 * r + 1) * a.K, a10[r], a11[r]);
  }
  if (a.db != nullptr && tj == 0) {
    // thread (rr = tid / 32, c4 = tid % 32) summed rows rr, rr + 16, ... of columns i0 + 4 c4 ..: the 16 threads that
    // share c4 meet in LDS (the tiles are no longer needed: the loop ended on a barrier), fixed order
    float* red = feta_lds;   // [512][4]
    red[threadIdx.x * 4 + 0] = rs0; red[threadIdx.x * 4 + 1] = rs1;
    red[threadIdx.x * 4 + 2] = rs2; red[threadIdx.x * 4 + 3] = rs3;
    __syncthreads();
    if (threadIdx.x < kDwI) {
      const int c4 = threadIdx.x >> 2, e = threadIdx.x & 3;
      float sv = 0.0f;
      for (int k = 0; k < kDwThreads / 32; ++k) sv += red[(c4 + 32 * k) * 4 + e];
      gst1<kStPartial>(a.db + i0 + threadIdx.x, sv);
    }
  }
}

// role workgroup w of a.wgs
__device__ __forceinline__ void lin_dw_role(const LinDwPlan& a, int w) {
  for (int t = w; t < a.tiles; t += a.wgs) {
    if (t != w) __syncthreads();   // the previous tile's LDS reads are done
    int ti, tj;
    lin_dw_tile_of(t, a.tiles, a.tj, ti, tj);
    lin_dw_tile(a, ti, tj);
  }
}

// what a carrying kernel takes as its argument: the plan, or nothing (an instantiation that never carries the role)
template <bool ON>
struct LinDwHost {};
template <>
struct LinDwHost<true> {
  LinDwPlan p;
};

}  // namespace feta
