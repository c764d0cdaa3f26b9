/* feta_hip.h - C ABI of libfeta_hip.so: the MI355X (gfx950) kernels behind the FeTA
 * spectral-attention block (dense per-graph attention with a multiplicative
 * positional kernel -> attention-conditioned filter coefficients -> dynamic
 * Chebyshev / eigenbasis spectral filter), forward and backward.
 *
 * The reference (ansonb/FeTA_TMLR) has no FFI for this path - it is ~40 PyTorch /
 * torch-geometric ops per layer - so each entry point below cites the reference
 * Python text whose arithmetic it replaces (paths relative to the reference root).
 * The Python side (feta_tmlr_amd/_abi.py) binds exactly these symbols with ctypes.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller and valid until the
 *    given stream reaches the enqueue point; nothing is allocated or synchronised
 *    inside; kernels are stream-ordered and graph-capturable;
 *  - floating-point data is fp32 unless an entry point or a descriptor's `dtype` says bf16, row-major; `stream` is a
 *    hipStream_t;
 *  - "token tensors" (q/k/v, per-head outputs, filter input/output) are addressed
 *    as ptr[b*sb + i*sn + h*dh + c] with element strides sb (graph) and sn (node),
 *    so seq-first [N,B,d] and batch-first [B,N,d] storage both work without copies;
 *    base pointers and strides must be multiples of 4 elements (16 bytes);
 *  - n_real[b] (int32) is the number of real nodes of graph b, 1 <= n_real[b] <= N;
 *    padding is the suffix i >= n_real[b] (reference collate: transformer/data.py:210);
 *  - return 0 on success, a negative FETA_E_* code otherwise; feta_last_error()
 *    gives the message for the calling thread.
 */
#ifndef FETA_HIP_H_
#define FETA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FETA_ABI_VERSION 13

#define FETA_OK 0
#define FETA_E_ARG (-1)     /* bad shape / stride / alignment / unsupported size */
#define FETA_E_LAUNCH (-2)  /* the HIP runtime rejected a launch */

typedef void* feta_stream_t;

/* Storage type of the token tensors of the fused layer-stack descriptors (feta_attn_block, feta_attn_block_grad,
 * feta_ffn, feta_ffn_grad; ABI 7).  FETA_BF16: the tensors marked [T] in each descriptor hold bf16 (the pointers stay
 * typed float* in the structs; rows must be 16-byte aligned), the kernels stage bf16 tiles and run their contractions
 * on v_mfma_f32_16x16x16_bf16; weights, biases, BatchNorm parameter blocks and partial sums, softmax statistics, the
 * attention matrix, and every weight / bias gradient stay fp32.  The reference has no reduced-precision mode
 * (experiments/run_transformer_gengcn.py:115-164): this is the storage path of BASELINE configs 3 and 5. */
#define FETA_F32 0
#define FETA_BF16 1

int feta_version(void);
const char* feta_last_error(void);

/* Largest padded node count and head dim the tile templates are instantiated for. */
#define FETA_MAX_NODES 256
#define FETA_MAX_HEAD_DIM 64

/* ---- A1: attention core ---------------------------------------------------------
 * Replaces the score/softmax/weighted-sum of DiffTransformerEncoderLayer.self_attn
 * (source absent from the reference; contract from transformer/models.py:166-167,179,
 * 244,275; form witnesses LSPE/layers/graphit_gt_layer.py:39-43,120-131,164):
 *   s = scale * q.k^T ; keys >= n_real masked ; e = exp(s - rowmax) ; e *= pe (if pe) ;
 *   attn = e / max(rowsum(e), 1e-6) ; out = attn . v
 * q,k,v   token tensors (strides qkv_sb, qkv_sn), all N query rows are computed
 * pe      [B,N,N] or NULL (broadcast over heads)
 * out     token tensor (strides o_sb, o_sn): out_each_head[b,i,h,:]
 * attn    [B,H,N,N] or NULL (skip the write; backward recomputes from stats)
 * stats   [B,H,N,2]: (rowmax, un-clamped rowsum) per query row
 */
int feta_attn_fwd(const float* q, const float* k, const float* v,
                  int64_t qkv_sb, int64_t qkv_sn,
                  const float* pe, const int32_t* n_real,
                  float* out, int64_t o_sb, int64_t o_sn,
                  float* attn, float* stats, float scale,
                  int B, int N, int H, int dh, feta_stream_t stream);

/* Backward of feta_attn_fwd w.r.t. q,k,v given dout (same strides as out).
 * delta [B,H,N] is caller-provided scratch (rowsum(dout*out)).
 * dq,dk,dv use the q/k/v strides and are fully written (zeros on padded keys).
 * dout2 (nullable; N <= 64 and dh <= 16 only) is a second gradient into the same output, added to
 * dout on load (the filter path's gradient into out_each_head).
 * The gradient through the rowmax subtraction is dropped (it is exactly zero
 * unless the 1e-6 clamp is active). */
int feta_attn_bwd(const float* q, const float* k, const float* v,
                  int64_t qkv_sb, int64_t qkv_sn,
                  const float* pe, const int32_t* n_real,
                  const float* out, const float* dout, const float* dout2, int64_t o_sb, int64_t o_sn,
                  const float* stats, float* delta,
                  float* dq, float* dk, float* dv, float scale,
                  int B, int N, int H, int dh, feta_stream_t stream);

/* ---- A2: filter-coefficient generator ---------------------------------------------
 * Replaces DiffTransformerEncoderGenGCN.get_filter_coefficients up to (not including)
 * self.linear: transformer/models.py:240-283 with GCNConv semantics of
 * transformer/GenGCN.py:55-102,393-402, using the exact collapse
 * GCNConv(ones)[j] = c_j * colsum(W) + b   (SURVEY F7).
 *   block (h,b): w = attn[b,h,:n,:n] ; w_jj = 1 where attn_jj == 0 ;
 *   deg_j = sum_i w_ij ; c_j = sum_i deg_i^-1/2 w_ij deg_j^-1/2 ;
 *   pooled[h*B+b, :] = mean_j tanh(c_j * s + gcn_bias)
 * cj      [H*B, N] out (saved for backward; rows >= n are zero)
 * pooled  [H*B, C] out
 */
int feta_coeff_fwd(const float* attn, const int32_t* n_real,
                   const float* s, const float* gcn_bias,
                   float* cj, float* pooled,
                   int B, int N, int H, int C, feta_stream_t stream);

/* ds[c] = sum_{blk,j} dpooled*(1-z^2)*c_j/n ; dbias[c] likewise without c_j.
 * partial [G, 2, C] scratch with G = feta_coeff_bwd_groups(B,H); when dbias == ds + C both are
 * reduced by one launch.  ds == NULL (ABI 6): no reduction launch - the caller reduces the partials ([G, 2C]: ds from
 * columns 0..C-1, dbias from C..2C-1) with feta_colsum_multi, together with whatever else it has pending.  dw_dense (nullable) [dw_rows, C]: the gradient of gcn.weight itself - s = 1^T W,
 * so every row of dW equals ds; the reduction launch writes the rows (no broadcast copy afterwards). */
int feta_coeff_bwd_groups(int B, int H);
int feta_coeff_bwd(const float* cj, const int32_t* n_real,
                   const float* s, const float* gcn_bias, const float* dpooled,
                   float* partial, float* ds, float* dbias, float* dw_dense, int dw_rows,
                   int B, int N, int H, int C, feta_stream_t stream);

/* The same backward in two parts (ABI 13, additive).  Per channel ds[c] = sum_blk dpooled[blk,c] A[blk,c] and
 * dbias[c] = sum_blk dpooled[blk,c] Bm[blk,c] with
 *   A[blk,c] = (1/n_blk) sum_i (1 - z^2) c_i,  Bm[blk,c] = (1/n_blk) sum_i (1 - z^2),  z = tanh(c_i s[c] + gcn_bias[c]):
 * feta_coeff_dsum computes A and Bm ([H*B, C] each; zeros for a block with n_real = 0) from forward data alone - every tanh
 * of the backward -, feta_coeff_bwd_saved the part that depends on dpooled.  partial [G, 2, C] with
 * G = feta_coeff_bwd_saved_groups(B, H); ds / dbias / dw_dense as feta_coeff_bwd. */
int feta_coeff_dsum(const float* cj, const int32_t* n_real, const float* s, const float* gcn_bias,
                    float* A, float* Bm, int B, int N, int H, int C, feta_stream_t stream);
int feta_coeff_bwd_saved_groups(int B, int H);
int feta_coeff_bwd_saved(const float* dpooled, const float* A, const float* Bm,
                         float* partial, float* ds, float* dbias, float* dw_dense, int dw_rows,
                         int B, int H, int C, feta_stream_t stream);

/* out[c] = sum_r in[r, c]  (s = colsum(gcn.weight); also reduces per-block partials) */
int feta_colsum(const float* in, float* out, int R, int C, feta_stream_t stream);

/* Several independent column sums in one launch (bias gradients that become available together):
 * out[c] = sum_r in[r*ld + c], r < R, c < C (ld = 0: C); bcast_out (nullable) [bcast_rows, C] additionally
 * receives the result in every row. */
#define FETA_COLSUM_MAX_SEGS 12
typedef struct feta_colsum_seg {
  const float* in;
  float* out;
  int R, C, ld;
  float* bcast_out;
  int bcast_rows;
} feta_colsum_seg;
int feta_colsum_multi(const feta_colsum_seg* segs, int nseg, feta_stream_t stream);

/* ---- the C x C linear of the coefficient generator (ABI 6) ----
 * Replaces self.linear of DiffTransformerEncoderGenGCN (transformer/models.py:284; nn.Linear(C, C) applied to the
 * pooled [H*B, C] rows) and its autograd backward: y = x w^T + bias as one launch, and dx = dy w, dw = dy^T x,
 * db = colsum(dy) as ONE launch (workgroups take roles) that can also carry up to FETA_COLSUM_MAX_SEGS pending column
 * sums of the caller in trailing workgroups.  x [R,K], w [N,K], y / dy [R,N]; exact-fp32 MFMA, deterministic.
 * feta_lin_supported: R, K, N multiples of 4 and K, N >= 16 (else the caller uses a library GEMM).
 * dx and db may be NULL. */
int feta_lin_supported(int R, int K, int N);
int feta_lin_fwd(const float* x, const float* w, const float* bias, float* y, int R, int K, int N,
                 feta_stream_t stream);
int feta_lin_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int R, int K,
                 int N, const feta_colsum_seg* segs, int nseg, feta_stream_t stream);
/* the same with a compute type (ABI 7): FETA_BF16 = the fp32 operands are rounded to bf16 when they are staged and the
 * products run on v_mfma_f32_16x16x16_bf16 with fp32 accumulation (bf16 storage legs); outputs, bias gradient and the
 * pending column sums stay fp32.  Shapes whose dims are multiples of 64 (256 for K, N) take the LDS-tiled kernels -
 * one GFLOP per product at the BASELINE shape (R = 512, K = N = C = 1024), where they replace the library GEMMs. */
int feta_lin_fwd_ex(const float* x, const float* w, const float* bias, float* y, int R, int K, int N, int compute,
                    feta_stream_t stream);
int feta_lin_bwd_ex(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int R, int K,
                    int N, const feta_colsum_seg* segs, int nseg, int compute, feta_stream_t stream);

/* ---- A3: dynamic Chebyshev filter, direct recursion on a dense scaled Laplacian ----
 * Replaces ChebConvDynamic.forward + __norm__ (transformer/ChebNetDynamic.py:108-189)
 * and its head-stacking / gather / scatter glue (transformer/models.py:178-186,
 * 200-202,346-360):
 *   y[b,i,h,:] = sum_k (T_k(Lhat_b) x_bh)[i,:] . W_k^(h,b) + bias   for i < n_real[b],
 *   y = 0 on padded rows; W^(h,b) = coeff[h*B+b].reshape(P, dh, dh).
 * lhat   [B,N,N] dense operator of one propagate(): out = Lhat @ x
 * heads_share_graph  0 = reference-literal (only head 0 sees the graph, heads >= 1
 *                    use Lhat = 0: models.py:186); 1 = every head filtered
 * x, y   token tensors (x strides x_sb,x_sn ; y strides y_sb,y_sn)
 */
int feta_cheb_filter_fwd(const float* x, int64_t x_sb, int64_t x_sn,
                         const float* lhat, const float* coeff, const float* bias,
                         const int32_t* n_real,
                         float* y, int64_t y_sb, int64_t y_sn,
                         int B, int N, int H, int dh, int P, int heads_share_graph,
                         feta_stream_t stream);

/* dx (x strides), dcoeff [H*B, P*dh*dh], dbias_part [B*H, dh] (reduce with feta_colsum) */
int feta_cheb_filter_bwd(const float* x, int64_t x_sb, int64_t x_sn,
                         const float* lhat, const float* coeff, const int32_t* n_real,
                         const float* dy, int64_t y_sb, int64_t y_sn,
                         float* dx, float* dcoeff, float* dbias_part,
                         int B, int N, int H, int dh, int P, int heads_share_graph,
                         feta_stream_t stream);

/* ---- A3 (eigenbasis form): U^T.X -> g(Lambda) -> U.(.) ------------------------------
 * Same operator in the Laplacian eigenbasis:
 *   y = U [ sum_k diag(t_k(lam)) (U^T x) W_k ] + bias ,  t_0=1, t_1=lam, t_k=2 lam t_{k-1}-t_{k-2}
 * exact w.r.t. feta_cheb_filter_* iff K spans the graph (K >= n_real); K < n is the
 * truncated benchmark operator (BASELINE configs K=8/16/32).
 * u [B,N,K] (rows >= n_real zero), lam [B,K].
 */
int feta_spec_filter_fwd(const float* x, int64_t x_sb, int64_t x_sn,
                         const float* u, const float* lam,
                         const float* coeff, const float* bias, const int32_t* n_real,
                         float* y, int64_t y_sb, int64_t y_sn,
                         int B, int N, int H, int dh, int P, int K, int heads_share_graph,
                         feta_stream_t stream);

int feta_spec_filter_bwd(const float* x, int64_t x_sb, int64_t x_sn,
                         const float* u, const float* lam,
                         const float* coeff, const int32_t* n_real,
                         const float* dy, int64_t y_sb, int64_t y_sn,
                         float* dx, float* dcoeff, float* dbias_part,
                         int B, int N, int H, int dh, int P, int K, int heads_share_graph,
                         feta_stream_t stream);

/* ---- linear_cat folded into the per-graph eigenbasis filter (ABI 10) -------------------------------------------
 * transformer/models.py:223-224: output = linear_cat(cat(output, allout_filtered)).  With W_cat = [Wa | Wb] ([64][128]):
 *   out = xn Wa^T + filt Wb^T + b_cat,  filt = U Ytil + bias  =>  filt Wb^T = U (Ytil Wb^T) + bias Wb^T
 * - the filter half is a [K x 64] x [64 x 64] product in the eigen domain, the stack half the graph's own rows through a
 * 64 x 64 product: both are done by the workgroup that filters the graph.  feta_spec_cat_supported: two shapes of d = 64 -
 * 4 heads x 16 with N <= 128, or 8 heads x 8 with N <= 64 (a wave's 16-column tile then holds heads 2t and 2t + 1 and its
 * W_k tile is block-diagonal; coeff is [H*B][P*8*8] and bias [8] as for feta_spec_filter_fwd at dh = 8) -, order 4, K <= 32
 * (a multiple of 4), every head on the graph, fp32.  y (= filt) is still written (linear_cat's backward contracts it).
 * y2: the stack output rows [N*B][64], row(b, i) = b*y2_sb + i*y2_sn elements; seen through its last BatchNorm when
 * y2_stats (fresh partial sums [Gx + 1][2][64]: finalized here over M rows - workgroup 0 publishes bn_out [4][64] and
 * updates rmean / rvar / nbt, as feta_rowlin_fwd_ex does for its x operand) or y2_bn (a published block) is given, else
 * used as it is (LayerNorm stack).  Rows of padded nodes take part (filt is zero there).  out has y's strides. */
typedef struct feta_spec_cat {
  const float* y2;
  int64_t y2_sb, y2_sn;
  const float* y2_bn;
  const float* y2_stats;
  int Gx;
  const float* gamma;
  const float* beta;
  float* bn_out;
  float* rmean;
  float* rvar;
  int64_t* nbt;
  float momentum, eps;
  int M;
  const float* w_cat;
  const float* b_cat;
  float* out;
} feta_spec_cat;
int feta_spec_cat_supported(int N, int H, int dh, int P, int K, int heads_share_graph);
int feta_spec_filter_cat_fwd(const float* x, int64_t x_sb, int64_t x_sn, const float* u, const float* lam,
                             const float* coeff, const float* bias, const int32_t* n_real, float* y,
                             int64_t y_sb, int64_t y_sn, int B, int N, int H, int dh, int P, int K,
                             int heads_share_graph, const feta_spec_cat* cat, feta_stream_t stream);

/* The same launch with feta_coeff_dsum (its arguments; N <= 64) in trailing workgroups: the launch runs one workgroup per
 * graph and leaves most of the chip idle at small batches, and the tanh pass of the coefficient generator's backward needs
 * forward data only.  role == NULL: feta_spec_filter_cat_fwd.  y, out and bn_out do not depend on the role.  4 heads x 16
 * only: a role with H = 8 is FETA_E_ARG (8-head callers launch feta_spec_filter_cat_fwd and keep feta_coeff_bwd).
 * feta_spec_cat_fwd_coeff_fits(B, N, K, blocks): 1 if `blocks` role blocks fit beside the B main workgroups - the role takes
 * the resident slots the main grid leaves free of its last round and a role workgroup walks at most two blocks; the launch
 * with a role that does not fit is FETA_E_ARG (the caller then keeps feta_coeff_bwd). */
int feta_spec_cat_fwd_coeff_fits(int B, int N, int K, int blocks);
typedef struct feta_coeff_dsum_role {
  const float* cj; const int32_t* n_real; const float* s; const float* gcn_bias; float* A; float* Bm;
  int B, N, H, C;
} feta_coeff_dsum_role;
int feta_spec_filter_cat_fwd_coeff(const float* x, int64_t x_sb, int64_t x_sn, const float* u, const float* lam,
                                   const float* coeff, const float* bias, const int32_t* n_real, float* y,
                                   int64_t y_sb, int64_t y_sn, int B, int N, int H, int dh, int P, int K,
                                   int heads_share_graph, const feta_spec_cat* cat, const feta_coeff_dsum_role* role,
                                   feta_stream_t stream);

/* Backward of the same fold (ABI 11): feta_spec_filter_bwd with the backward of linear_cat inside - replaces
 * feta_rowlin_bwd_ex over [x_n | filt] (functional.RowLinearCat[BN]Fn.backward, transformer/models.py:223-224 under
 * autograd) + feta_spec_filter_bwd.  dout [N*B rows][64] = gradient w.r.t. linear_cat's output, rows addressed with the
 * strides of y2; filt = the forward's y (strides y_sb, y_sn); y2_bn = the block the forward published (or NULL: x_n = y2).
 * Outputs: dx / dcoeff / dbias_part as feta_spec_filter_bwd; dxn [rows][64] = dout W_a (gradient w.r.t. the NORMALISED
 * stack output); gs [R][2][64] = per-workgroup (sum dxn, sum dxn * xhat) for the BatchNorm backward of the stack's last norm
 * (NULL without y2_bn); partial [R][partial_ld] = [dW_cat 64 x 128 | db_cat 64] per workgroup, reduced by the caller's
 * feta_colsum_multi.  R = feta_spec_cat_bwd_rows(B) rows in gs and partial: one per graph up to 512 graphs, beyond that a
 * workgroup walks graphs blockIdx, blockIdx + 512, ... and leaves their sum.  feta_spec_cat_bwd_supported: P = 4, 4 heads x 16
 * or 8 heads x 8 (dcoeff [H*B][P*8*8], dbias_part [B*8][8]: the layouts of feta_spec_filter_bwd at dh = 8; dxn, gs and partial
 * keep theirs), N <= 64, K <= 32 (a multiple of 4), fp32, every head on the graph. */
typedef struct feta_spec_cat_grad {
  const float* dout;
  const float* y2;
  int64_t y2_sb, y2_sn;
  const float* y2_bn;
  const float* filt;
  const float* w_cat;
  float* dxn;
  float* gs;
  float* partial;
  int64_t partial_ld;
} feta_spec_cat_grad;
int feta_spec_cat_bwd_supported(int N, int H, int dh, int P, int K, int heads_share_graph);
int feta_spec_cat_bwd_rows(int B);
int feta_spec_filter_cat_bwd(const float* x, int64_t x_sb, int64_t x_sn, const float* u, const float* lam,
                             const float* coeff, const int32_t* n_real, int64_t y_sb, int64_t y_sn, float* dx,
                             float* dcoeff, float* dbias_part, int B, int N, int H, int dh, int P, int K,
                             int heads_share_graph, const feta_spec_cat_grad* cat, feta_stream_t stream);

/* ---- bf16 STORAGE variants of A1 and A3 (BASELINE configs 3 and 5) ----------------------------------
 * Same operators, same argument meaning as feta_attn_fwd/bwd and feta_spec_filter_fwd/bwd; `void*`
 * operands are bf16 (q, k, v, pe, out, attn, dout, dq, dk, dv; x, u, coeff, y, dy, dx, dcoeff), base
 * pointers 8-byte aligned, strides in elements (multiples of 4).  stats, delta, lam, bias and dbias_part
 * stay fp32; the contractions run on v_mfma_f32_16x16x16_bf16 with fp32 accumulation, softmax statistics
 * and t_k(lambda) in fp32.  The reference has no reduced-precision mode: parity of these entry points is
 * a stated tolerance against the fp64 oracle (tests/), the fp32 entry points are the reference arithmetic.
 * dh in {16, 32, 64} (attention), {16, 32} (filter); N <= FETA_MAX_NODES; K <= 64. */
int feta_attn_fwd_bf16(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                       const void* pe, const int32_t* n_real, void* out, int64_t o_sb, int64_t o_sn,
                       void* attn, float* stats, float scale, int B, int N, int H, int dh,
                       feta_stream_t stream);
int feta_attn_bwd_bf16(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                       const void* pe, const int32_t* n_real, const void* out, const void* dout,
                       int64_t o_sb, int64_t o_sn, const float* stats, float* delta,
                       void* dq, void* dk, void* dv, float scale, int B, int N, int H, int dh,
                       feta_stream_t stream);
int feta_spec_filter_fwd_bf16(const void* x, int64_t x_sb, int64_t x_sn, const void* u, const float* lam,
                              const void* coeff, const float* bias, const int32_t* n_real,
                              void* y, int64_t y_sb, int64_t y_sn,
                              int B, int N, int H, int dh, int P, int K, int heads_share_graph,
                              feta_stream_t stream);
int feta_spec_filter_bwd_bf16(const void* x, int64_t x_sb, int64_t x_sn, const void* u, const float* lam,
                              const void* coeff, const int32_t* n_real,
                              const void* dy, int64_t y_sb, int64_t y_sn,
                              void* dx, void* dcoeff, float* dbias_part,
                              int B, int N, int H, int dh, int P, int K, int heads_share_graph,
                              feta_stream_t stream);

/* ---- A1 with attention-probability dropout (step (6) of the reconstructed layer; the reference
 * scripts expose --dropout, default 0.0: experiments/run_transformer_gengcn.py:47) --------------------------
 * attn = dropout(softmax-like probabilities, p) (kept entries scaled by 1/(1-p)); out = attn . v; the written
 * attn is the dropped one (as nn.MultiheadAttention returns it).  The keep mask is a pure function of
 * (seed, offset, b, h, query, key): Philox4x32-10, key = seed, counter = (g, offset) with
 * g = ((b*H + h)*N + query) * ceil(N/4) + key/4, word key%4 of the output, keep iff word >= floor(p * 2^32);
 * backward regenerates it from the same (seed, offset) - no mask tensor.  dtype: FETA_DTYPE_F32 (float
 * operands, 16-byte aligned) or FETA_DTYPE_BF16 (as the *_bf16 entry points). */
#define FETA_DTYPE_F32 0
#define FETA_DTYPE_BF16 1
int feta_attn_fwd_drop(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                       const void* pe, const int32_t* n_real, void* out, int64_t o_sb, int64_t o_sn,
                       void* attn, float* stats, float scale, float p_drop, uint64_t seed, uint64_t offset,
                       int dtype, int B, int N, int H, int dh, feta_stream_t stream);
int feta_attn_bwd_drop(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                       const void* pe, const int32_t* n_real, const void* out, const void* dout,
                       int64_t o_sb, int64_t o_sn, const float* stats, float* delta,
                       void* dq, void* dk, void* dv, float scale, float p_drop, uint64_t seed, uint64_t offset,
                       int dtype, int B, int N, int H, int dh, feta_stream_t stream);
/* the same with the key DEVICE-RESIDENT (ABI 7): state = {seed, offset} (two uint64 in device memory), the mask of this
 * call is the one of (state[0], state[1] + offset_add), read when the kernel RUNS - a captured hipGraph (the reference's
 * --dropout > 0 inside train.GraphedTrainStep) draws fresh masks on every replay; the step advances state[1] itself. */
int feta_attn_fwd_drop_dev(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                           const void* pe, const int32_t* n_real, void* out, int64_t o_sb, int64_t o_sn,
                           void* attn, float* stats, float scale, float p_drop, const uint64_t* state,
                           uint64_t offset_add, int dtype, int B, int N, int H, int dh, feta_stream_t stream);
int feta_attn_bwd_drop_dev(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                           const void* pe, const int32_t* n_real, const void* out, const void* dout,
                           int64_t o_sb, int64_t o_sn, const float* stats, float* delta,
                           void* dq, void* dk, void* dv, float scale, float p_drop, const uint64_t* state,
                           uint64_t offset_add, int dtype, int B, int N, int H, int dh, feta_stream_t stream);

/* ---- A1 with a choice of exponent stabilisation (stab = {rowmax, clamp5}; ABI 7) --------------------
 * FETA_STAB_ROWMAX: e = exp(s - rowmax) - feta_attn_fwd / feta_attn_bwd (upstream GraphiT, README.md:129);
 * FETA_STAB_CLAMP5: e = exp(clamp(s, -5, 5)), the form of the in-tree DGL witnesses (LSPE/layers/graphit_gt_layer.py:
 * 39-43, LPE/layers/graph_transformer_spectra_layer.py:239-243): no row maximum (stats holds 0 for it), a clamped
 * score passes no gradient; everything else (key mask, * pe, / max(rowsum, 1e-6)) as feta_attn_fwd.  A1's source is
 * absent from the reference, so the open semantic choices are flags.  dtype as feta_attn_fwd_drop. */
#define FETA_STAB_ROWMAX 0
#define FETA_STAB_CLAMP5 1
int feta_attn_fwd_stab(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                       const void* pe, const int32_t* n_real, void* out, int64_t o_sb, int64_t o_sn,
                       void* attn, float* stats, float scale, int stab, int dtype, int B, int N, int H, int dh,
                       feta_stream_t stream);
int feta_attn_bwd_stab(const void* q, const void* k, const void* v, int64_t qkv_sb, int64_t qkv_sn,
                       const void* pe, const int32_t* n_real, const void* out, const void* dout,
                       int64_t o_sb, int64_t o_sn, const float* stats, float* delta,
                       void* dq, void* dk, void* dv, float scale, int stab, int dtype, int B, int N, int H, int dh,
                       feta_stream_t stream);

/* ---- A1/A4: row-wise linears of the encoder layer and BatchNorm1d --------------------------
 * Replaces the F.linear / relu / degree scaling / residual / BatchNorm1d sequence of
 * DiffTransformerEncoderLayer.forward (contract transformer/models.py:166-167; body per upstream
 * GraphiT, README.md:129) and linear_cat (transformer/models.py:223-224).  Activations are
 * [M, C] row-major, M = N*B rows.
 *   y = relu?(x W^T + bias) * rowscale[row]? + residual?        x [M,KI], W [NO,KI], y [M,NO]
 * stats (optional) receives per-block partial (sum, sumsq) of y: [feta_rowlin_blocks(M) + 1, 2, NO] (ABI 7: the last
 * row records the shift of the sums, feta_rowlin_ex.stats_shift - zero through this entry point),
 * the BatchNorm statistics of the result without a separate pass.
 * KI in {16,32,64,128,192,256}; NO a multiple of 16 (backward: NO in the same set).
 */
int feta_rowlin_blocks(int M);
int feta_rowlin_chunks(int M);
int feta_rowlin_fwd(const float* x, const float* w, const float* bias, const float* rowscale,
                    const float* residual, float* y, float* stats, int relu,
                    int M, int KI, int NO, feta_stream_t stream);
/* g = dy * rowscale? * [ysaved > 0]? ;  dx = g W ;  dwdb = [ g^T x  (NO*KI) | colsum g (NO) ].
 * partial: scratch [feta_rowlin_chunks(M), NO*KI + NO].  dX and the split-K weight gradient run
 * in one launch (blocks take roles), then one deterministic reduction of the partials. */
int feta_rowlin_bwd(const float* x, const float* w, const float* dy, const float* rowscale,
                    const float* ysaved, float* dx, float* partial, float* dwdb,
                    int M, int KI, int NO, feta_stream_t stream);

/* Extended form used by the fused encoder stack: the same two kernels with BatchNorm folded into
 * the operand loads and epilogues, so that BatchNorm never runs as a pass of its own.
 * "bn parameter block" = float[4][D]: scale = gamma*rstd, shift = beta - mean*scale, mean, rstd.
 * Unused pointers are NULL.  All tensors [M, .] row-major fp32. */
typedef struct feta_rowlin_ex {
  /* common */
  const float* x;         /* [M,KI] input (pre-norm values when x_bn / x_stats is set) */
  const float* w;         /* [NO,KI] */
  const float* bias;      /* [NO] */
  const float* rowscale;  /* [M] */
  int M, KI, NO, relu;
  /* forward:  y = relu?(BN?(x) W^T + bias) * rowscale? + BN?(residual)? */
  const float* residual;  /* [M,NO] */
  const float* res_bn;    /* bn parameter block [4][NO] through which residual is seen */
  float* y;               /* [M,NO] */
  float* stats;           /* [feta_rowlin_blocks(M) + 1,2,NO] partial (shifted) (sum, sumsq) of y + the shift row */
  const float* x_bn;      /* finalized bn parameter block [4][KI] of the input, or */
  const float* x_stats;   /* [Gx + 1,2,KI] partial statistics (+ shift row) to finalize here: needs x_gamma, x_beta, */
  int Gx;                 /*   x_bn_out (written by block 0), optional running stats */
  const float* x_gamma;
  const float* x_beta;
  float* x_bn_out;
  float* x_rmean;
  float* x_rvar;
  int64_t* x_nbt;         /* num_batches_tracked of that BatchNorm (+1 by block 0), or NULL */
  float momentum, eps;
  /* backward:  g = BNbwd?(dy) * rowscale? * [relu_y > 0]? ;  dx = g W (+ adds) ;  dW = g^T BN?(x) */
  const float* dy;        /* [M,NO] */
  const float* relu_y;    /* [M,NO] saved relu output */
  float* dx;              /* [M,KI] */
  float* partial;         /* [feta_rowlin_chunks(M), NO*KI + NO] scratch */
  int partial_ld;         /* row pitch of partial (0 = NO*KI+NO): lets several linears share one
                             [chunks, total] buffer that the caller reduces with ONE feta_colsum */
  const float* g_y;       /* [M,NO] pre-norm values of the BatchNorm whose backward is applied to dy */
  const float* g_bn;      /* its bn parameter block [4][NO] */
  const float* g_sum;     /* [Gs,2,NO] partial (sum dy, sum dy*xhat): finalized here, or */
  int Gs;
  const float* g_fin;     /* [2][NO] already finalized (mean dy, mean dy*xhat) */
  float* g_fin_out;       /* [2][NO] written by block 0 when g_sum is given */
  float* dgamma;          /* [NO] = sum dy*xhat   (written with g_sum) */
  float* dbeta;           /* [NO] = sum dy */
  const float* add_plain; /* [M,KI] added to dx */
  const float* add_dout;  /* [M,KI]: dx += BNbwd(add_dout) with add_y, add_bn [4][KI], add_fin [2][KI] */
  const float* add_y;
  const float* add_bn;
  const float* add_fin;
  const float* x2;        /* x is the virtual concatenation [x (x_split cols) | x2 (KI - x_split cols)]: */
  int x_split;            /*   linear_cat without materialising torch.cat; backward writes dx | dx2.  With x2,
                             x_bn / x_stats (and x_gamma ..) and sum_y / sum_bn / sum_out describe the BatchNorm
                             of the x part only: x_split columns instead of KI */
  float* dx2;
  const float* sum_y;     /* [M,KI] pre-norm values of the BatchNorm that produced x: emit */
  const float* sum_bn;    /*   sum_out [feta_rowlin_blocks(M),2,KI] = partial (sum dx, sum dx*xhat) */
  float* sum_out;
  const float* stats_shift; /* nullable [NO] (ABI 7): `stats` are SHIFTED sums - sum (y - K), sum (y - K)^2 with K = this
                               vector, the running mean of the BatchNorm that will consume them (0 if NULL) - and K is
                               recorded in one extra row: stats / x_stats / y_stats buffers hold G + 1 rows, row G =
                               [K | unused].  mean = K + S1 / M, var = S2 / M - (S1 / M)^2: the cancellation of
                               E[y^2] - mean^2 moves from |mean| to |mean - running mean| (csrc/feta_rowops.h) */
} feta_rowlin_ex;

int feta_rowlin_fwd_ex(const feta_rowlin_ex* d, feta_stream_t stream);
/* dwdb [NO*KI + NO] receives the reduced weight and bias gradient (NULL with partial_ld > 0:
 * partials only). */
int feta_rowlin_bwd_ex(const feta_rowlin_ex* d, float* dwdb, feta_stream_t stream);

/* out = BN(y) written explicitly (end of the stack), publishing the bn parameter block [4][D].
 * stats holds G_stats partial rows and, behind them, the shift row: [G_stats + 1][2][D] (G_stats = 0 means
 * feta_rowlin_blocks(M), the producer was a feta_rowlin_fwd*; feta_ffn_blocks(M) after feta_ffn_fwd;
 * feta_attn_block_stat_rows(B, N) after feta_attn_block_fwd). */
int feta_bn_apply_fwd_prm(const float* y, const float* stats, const float* gamma, const float* beta,
                          float* out, float* bn_prm, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float momentum, float eps, int M, int D, int G_stats,
                          feta_stream_t stream);
/* partial [feta_rowlin_blocks(M),2,D] = per-block (sum dout, sum dout*xhat), bn_prm [4][D]. */
int feta_bn_bwd_reduce(const float* y, const float* dout, const float* bn_prm, float* partial,
                       int M, int D, feta_stream_t stream);

/* Training-mode BatchNorm1d over the M rows (padded rows included, as nn.BatchNorm1d on the
 * [N*B, d] view does).  stats [feta_rowlin_blocks(M) + 1, 2, D] from feta_rowlin_fwd or feta_bn_stats:
 * G = feta_rowlin_blocks(M) partial rows PLUS ONE shift row (ABI 7: the sums are relative to the shift recorded in
 * row G; feta_bn_stats writes zeros there) - a caller that sizes the buffer with G rows gets a D-float overrun.
 * mean_rstd [2, D] is saved for backward; running_* (nullable) are updated with momentum and the
 * unbiased variance, num_batches_tracked (nullable, int64) is advanced by one, as nn.BatchNorm1d does. */
int feta_bn_stats(const float* y, float* stats, int M, int D, feta_stream_t stream);
/* ... with a shift (feta_rowlin_ex.stats_shift); either way stats has feta_rowlin_blocks(M) + 1 rows (ABI 7) */
int feta_bn_stats_shift(const float* y, const float* shift, float* stats, int M, int D, feta_stream_t stream);
int feta_bn_apply_fwd(const float* y, const float* stats, const float* gamma, const float* beta,
                      float* out, float* mean_rstd, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, float momentum, float eps, int M, int D, feta_stream_t stream);
/* partial: scratch [feta_rowlin_blocks(M), 2, D]; dgamma, dbeta [D]. */
int feta_bn_bwd(const float* y, const float* dout, const float* mean_rstd, const float* gamma,
                float* partial, float* dy, float* dgamma, float* dbeta,
                int M, int D, feta_stream_t stream);

/* ---- attention sub-block of one encoder layer in ONE launch --------------------------------
 * Replaces, for d_model = 64 = 4 heads x 16 or (ABI 13, field H) 8 heads x 8 and N <= 64 (feta_attn_block_supported), the sequence
 * feta_rowlin_fwd_ex (in_proj) -> feta_attn_fwd -> feta_rowlin_fwd_ex (out_proj + degree + residual
 * + BatchNorm statistics) of DiffTransformerEncoderLayer.forward (contract
 * transformer/models.py:166-167,179,244; body per upstream GraphiT, README.md:129).
 * One workgroup per graph; rows of the [M = B*N, .] activations are addressed as
 * row(b, i) = b*row_sb + i*row_sn (seq-first [N,B,d]: row_sb = 1, row_sn = B).
 * x is "seen through a BatchNorm" exactly as in feta_rowlin_ex: either x_bn (a published [4][64]
 * parameter block) or x_stats [Gx][2][64] fresh partial sums that this launch finalizes
 * (publishing x_bn_out and updating x_rmean / x_rvar), or neither (first layer).
 * Outputs: qkv [M,192] (in_proj result, for backward), out [M,64] (per-head attention outputs,
 * concatenated: out_each_head), attn_stats [B,H,N,2] (row max, un-clamped row sum), attn
 * [B,H,N,N] or NULL, y [M,64] = x_norm + rowscale * (out W_out^T + b_out), y_stats [G][2][64]
 * partial (sum, sum of squares) over the rows of y - padded rows included, as nn.BatchNorm1d over the
 * [N*B, d] view counts them; NULL (ABI 9): no statistics are taken (LayerNorm stack).
 * G = feta_attn_block_stat_rows(B, N) (ABI 8): one row per WORKGROUP - a graph is one
 * workgroup of eight waves (head x query-tile parity), or two such workgroups (query tiles split between them, K and V
 * projected by both) where a graph has more than two 16-row tiles and 2 B workgroups still fit the chip; the shift row
 * (y_shift) is row G. */
typedef struct feta_attn_block {
  const float* x;
  const float* x_bn;
  const float* x_stats;
  int Gx;
  const float* x_gamma;
  const float* x_beta;
  float* x_bn_out;
  float* x_rmean;
  float* x_rvar;
  int64_t* x_nbt;      /* num_batches_tracked of that BatchNorm (+1 by workgroup 0), or NULL */
  float momentum, eps;
  const float* w_in;   /* [192,64] */
  const float* b_in;   /* [192] or NULL */
  const float* w_out;  /* [64,64] */
  const float* b_out;  /* [64] or NULL */
  const float* pe;     /* [B,N,N] or NULL */
  const int32_t* n_real;
  const float* rowscale; /* [M] degree scale per row, or NULL */
  float* qkv;
  float* out;
  float* attn_stats;
  float* attn;
  float* y;
  float* y_stats;
  float scale;         /* d_h^-1/2 */
  int B, N, M;
  int64_t row_sb, row_sn;
  int tie_qk;
  int dtype;           /* FETA_F32 | FETA_BF16: storage type of x, pe, qkv, out, y [T] (ABI 7) */
  const float* y_shift; /* nullable [64]: shift of the y statistics = running mean of the BatchNorm that will normalise y
                           (feta_rowlin_ex.stats_shift); y_stats has G + 1 rows (G = feta_attn_block_stat_rows), row G
                           receives the shift */
  float* out_f32;      /* nullable: `out` once more, as fp32 [M,64] - the fp32 filter stage behind a bf16 stack reads it
                          (out_each_head of the last layer, transformer/models.py:179) without a cast launch */
  const float* x_ln_gamma; /* nullable [64] (ABI 9): x is seen through a LAYERNORM - the rows of x are the PRE-norm rows
                              (the previous layer's y2) and x_norm = (x - mean_row) * rstd_row * gamma + beta is computed
                              per row when the row is staged (eps: the field above; biased variance, as F.layer_norm):
                              LayerNorm is row-local, so its consumer applies it and no normalised tensor is ever
                              written (norm2 of DiffTransformerEncoderLayer with batch_norm=False, the reference's
                              default: experiments/run_transformer_gengcn_cv.py:56).  Excludes x_bn / x_stats. */
  const float* x_ln_beta;  /* [64], with x_ln_gamma */
  int H;               /* heads (ABI 13): 0 or 4 = 4 heads x 16, 8 = 8 heads x 8 (fp32 storage only; a 16-column tile of
                          the kernels then holds two heads and attn_stats / attn are [B,8,N,2] / [B,8,N,N]).  The
                          feta_attn_out_* entry points take 4 heads only. */
} feta_attn_block;

int feta_attn_block_supported(int N, int d_model, int heads);
int feta_attn_block_stat_rows(int B, int N);   /* partial rows a forward launch writes into y_stats (0: unsupported shape) */
int feta_attn_block_fwd(const feta_attn_block* d, feta_stream_t stream);
/* the same launch with up to FETA_COLSUM_MAX_SEGS independent column sums in trailing workgroups (ABI 6): at the
 * BASELINE batch the first launch of a forward pass leaves half the chip idle, and s = colsum(gcn.weight) of the
 * coefficient generator (transformer/models.py:280-282: the GCN only ever sees an all-ones input) depends on the
 * parameters alone. */
int feta_attn_block_fwd_sums(const feta_attn_block* d, const feta_colsum_seg* segs, int nseg, feta_stream_t stream);

/* ---- attention core + out_proj behind the in_proj launch, for graphs beyond feta_attn_block (ABI 8) -------------
 * (feta_attn_out_supported: d_model = 64, 4 heads, N <= 256.)  Replaces feta_attn_fwd -> feta_rowlin_fwd_ex
 * (out_proj + degree + residual + BatchNorm statistics) of DiffTransformerEncoderLayer.forward for config 4 (PATTERN,
 * experiments/run_transformer_gengcn_SBM_cv.py; contract transformer/models.py:166-167,179,244): one workgroup per
 * (graph, 32 query rows), the per-head outputs meet in LDS and are the out_proj operand.  Same descriptor as
 * feta_attn_block, read as follows: qkv [M,192] is an INPUT (the in_proj result), x is the residual (seen through the
 * published parameter block x_bn when given; x_stats must be NULL - the in_proj launch finalized them), w_in / b_in are
 * ignored; outputs out, out_f32, attn_stats, attn, y as there; y_stats (nullable) [G + 1][2][64] with
 * G = feta_attn_out_stat_rows(B, N) = B * ceil(N / 32) partial rows and the shift row behind them.  fp32 token tensors
 * (dtype = FETA_F32) only. */
int feta_attn_out_supported(int N, int d_model, int heads);
int feta_attn_out_stat_rows(int B, int N);
int feta_attn_out_fwd(const feta_attn_block* d, feta_stream_t stream);
/* ... with column sums in trailing workgroups, as feta_attn_block_fwd_sums (s = colsum(gcn.weight) in the first launch) */
int feta_attn_out_fwd_sums(const feta_attn_block* d, const feta_colsum_seg* segs, int nseg, feta_stream_t stream);

/* ---- backward of the attention sub-block in ONE launch ------------------------------------------------------
 * (feta_attn_block_bwd_supported: d_model = 64, 4 heads or - ABI 13, field H - 8 heads, N <= 64; K not tied to Q.)  Replaces
 * feta_rowlin_bwd_ex (out_proj) -> feta_attn_bwd -> feta_rowlin_bwd_ex (in_proj) of the layer's backward:
 *   g1 = BatchNorm-1 backward of dy (y1 [M,64], bn1 [4][64], partial sums g_sum [Gs][2][64] finalized here ->
 *        fin_out [2][64], dgamma, dbeta) - or dy itself when y1 is NULL (LayerNorm stack);
 *   dconcat = (rowscale * g1) W_out (+ dout2 [M,64], the filter branch's gradient into out_each_head);
 *   dq|dk|dv from q|k|v (qkv [M,192]), out [M,64], pe, attn_stats (feta_attn_bwd's arithmetic);
 *   dx [M,64] = dqkv W_in + g1;  sum_out (nullable) [2 * feta_attn_block_bwd_blocks(B)][2][64]: partial
 *        (sum dx, sum dx * xhat0), xhat0 from x0 (pre-norm) and bn0 [4][64];
 *   partial: one row per workgroup (feta_attn_block_bwd_blocks(B) rows: one workgroup per graph up to 256 graphs, beyond
 *        that the workgroups walk several graphs and add into their row; pitch partial_ld, 0: 4*64*64 + 4*64),
 *        columns [dW_out (64 x 64) | db_out (64) | dW_in (192 x 64) | db_in (192)], reduced by the caller;
 *        dW_in contracts dqkv with x0 seen through bn0 (scale, shift rows) when given.
 * Rows are addressed as in feta_attn_block: row(b, i) = b*row_sb + i*row_sn. */
typedef struct feta_attn_block_grad {
  const float* dy;
  const float* y1;
  const float* bn1;
  const float* g_sum;
  int Gs;
  float* fin_out;
  float* dgamma;
  float* dbeta;
  const float* rowscale;
  const float* w_out;
  const float* w_in;
  const float* qkv;
  const float* out;
  const float* dout2;
  const float* pe;
  const int32_t* n_real;
  const float* attn_stats;
  const float* x0;
  const float* bn0;
  float* dx;
  float* dx_b;       /* nullable: SPLIT form, two workgroups per graph (one per pair of heads): dx receives pair 0's part
                        (with the residual g1), dx_b pair 1's; the consumer adds them (feta_ffn_grad.dy_b); sum_out
                        rows then are partial sums of the two parts - same row count */
  float* sum_out;
  float* partial;
  int partial_ld;
  float scale;
  int B, N, M;
  int64_t row_sb, row_sn;
  int dtype;         /* FETA_F32 | FETA_BF16: storage type of dy, y1, qkv, out, dout2, pe, x0, dx, dx_b [T] (ABI 7) */
  int dout2_f32;     /* 1: dout2 is fp32 whatever dtype says (it comes from the fp32 filter stage) */
  const float* ln1_gamma;   /* nullable [64] (ABI 9): dy is the gradient w.r.t. LN1(y1) = norm1's output, and
                               g1 = LayerNorm backward of dy, computed per row when the gradient row is staged:
                               xhat = (y1 - mean_row) rstd_row, g = dy * gamma, g1 = rstd_row (g - mean_row(g) -
                               xhat mean_row(g xhat)); y1 = the pre-norm rows (bn1 / g_sum must be NULL).  The partial
                               row gains [dgamma1 (64) | dbeta1 (64)] = per-workgroup sums of (dy xhat, dy) behind
                               db_in (default pitch 4*64*64 + 4*64 + 128). */
  const float* x0_ln_gamma; /* nullable [64]: x0 holds PRE-norm rows, the in_proj operand is LayerNorm(x0) * gamma +
                               beta computed per row on load (feta_attn_block.x_ln_gamma); excludes bn0 */
  const float* x0_ln_beta;
  float ln_eps;
  int H;             /* heads (ABI 13): 0 or 4 = 4 heads x 16, 8 = 8 heads x 8 (fp32 storage only; attn_stats [B,8,N,2]);
                        SPLIT keeps its meaning per pair of 16-column tiles: workgroup 0 heads 0-3, workgroup 1 heads 4-7 */
} feta_attn_block_grad;

int feta_attn_block_bwd_supported(int N, int d_model, int heads);
int feta_attn_block_bwd_blocks(int B);
int feta_attn_block_bwd(const feta_attn_block_grad* d, feta_stream_t stream);
/* the same launch with up to FETA_COLSUM_MAX_SEGS independent column sums in trailing workgroups (ABI 8): the last launch
 * of a stack's backward leaves half the chip idle at the BASELINE batch while the split-K partials of everything behind it
 * are complete - reduced here, the final reduction launch is left with this launch's own partial columns. */
int feta_attn_block_bwd_sums(const feta_attn_block_grad* d, const feta_colsum_seg* segs, int nseg, feta_stream_t stream);
/* ... and, in front of them, the "dW" product of the coefficient generator's C x C linear as a role of the same launch
 * (additive, ABI 13): dw[n][k] = sum_r dy[r][n] x[r][k], db[n] = sum_r dy[r][n] (db nullable), exact fp32 MFMA with the
 * contraction index ascending - deterministic and independent of the grid.  512-thread workgroups on 128 x 64 tiles of dw,
 * dispatched behind the main workgroups and before the column-sum tiles; as many as the main grid leaves free of one round
 * of resident workgroups (CUs x occupancy of the instantiation), each walking several tiles where there are more tiles.
 * Carried by the one-workgroup-per-graph fp32 launches only (4 or 8 heads): dx_b (two workgroups per graph), bf16 storage
 * and more graphs than feta_attn_block_bwd_blocks(B) are rejected, as are R % 64, K % 64, N % 128 != 0, null or misaligned
 * (16 bytes) dy / x / dw.  Everything the main workgroups write is bit-identical with and without the role.  dw == NULL:
 * feta_attn_block_bwd_sums.
 *   feta_attn_block_bwd_dw_slots(B, N, heads): workgroup slots the launch for B graphs of N nodes leaves free (0: none, or
 *        no carrying instantiation);
 *   feta_attn_block_bwd_dw_tiles(K, N_out): tiles of the role for a [N_out, K] result (0: not a tiled shape) - with no more
 *        tiles than free slots the role takes one round;
 *   feta_attn_block_bwd_dw_supported(B, N, heads, R, K, N_out): the shape is tiled AND at least one slot is free.
 * The role has instantiations of its own (<..., DW = true>): a launch with dw == NULL runs the kernel it ran before. */
typedef struct feta_lin_dw {
  const float* dy; /* [R][N] gradient of the linear's output */
  const float* x;  /* [R][K] its input */
  float* dw;       /* [N][K] */
  float* db;       /* [N], nullable */
  int R, K, N;
} feta_lin_dw;
int feta_attn_block_bwd_dw_slots(int B, int N, int heads);
int feta_attn_block_bwd_dw_tiles(int K, int N_out);
int feta_attn_block_bwd_dw_supported(int B, int N, int heads, int R, int K, int N_out);
int feta_attn_block_bwd_sums_dw(const feta_attn_block_grad* d, const feta_colsum_seg* segs, int nseg, const feta_lin_dw* dw,
                                feta_stream_t stream);

/* ---- feed-forward half of one encoder layer in ONE launch -----------------------------------
 * x = BN1(y1) (x_bn | x_stats as in feta_rowlin_ex / feta_attn_block);  h = relu(x W1^T + b1);
 * y = x + h W2^T + b2;  y_stats [feta_ffn_blocks(M)][2][64] per-workgroup (sum, sum of squares).
 * Replaces the two feta_rowlin_fwd_ex launches of linear1 / linear2 for d_model = 64 and
 * dim_feedforward in {64,128,256} (feta_ffn_supported).  h [M,FF] is written for backward. */
typedef struct feta_ffn {
  const float* x;
  const float* x_bn;
  const float* x_stats;
  int Gx;
  const float* x_gamma;
  const float* x_beta;
  float* x_bn_out;
  float* x_rmean;
  float* x_rvar;
  int64_t* x_nbt;
  float momentum, eps;
  const float* w1;  /* [FF,64] */
  const float* b1;  /* [FF] or NULL */
  const float* w2;  /* [64,FF] */
  const float* b2;  /* [64] or NULL */
  float* h;
  float* y;
  float* y_stats;   /* or NULL */
  int M, FF;
  int dtype;        /* FETA_F32 | FETA_BF16: storage type of x, h, y [T] (ABI 7) */
  const float* y_shift; /* nullable [64]: shift of the y statistics (feta_attn_block.y_shift); y_stats has
                           feta_ffn_blocks(M) + 1 rows */
  int y_f32;        /* 1: y is written as fp32 whatever dtype says (last layer of a bf16 stack: its consumer, linear_cat
                       with the folded BatchNorm, transformer/models.py:223-224, is an fp32 kernel) */
  const float* x_ln_gamma; /* nullable [64] (ABI 9): x = LayerNorm(x rows) * gamma + beta, computed per row on load
                              (feta_attn_block.x_ln_gamma: norm1 with batch_norm=False); excludes x_bn / x_stats */
  const float* x_ln_beta;
  float* y_ln_out;          /* nullable [M,64] [T, or fp32 with y_ln_f32] (ABI 11): LayerNorm(y rows) * y_ln_gamma + y_ln_beta, */
  const float* y_ln_gamma;  /*   written beside y by the epilogue - norm2 of a LayerNorm stack where its consumer is not an */
  const float* y_ln_beta;   /*   on-load kernel (graphs beyond 64 nodes; the end of the stack).  Excludes y_stats. */
  float y_ln_eps;
  int y_ln_f32;
} feta_ffn;

int feta_ffn_supported(int d_model, int ff);
int feta_ffn_blocks(int M);
int feta_ffn_fwd(const feta_ffn* d, feta_stream_t stream);
/* the same launch with the FORWARD of the coefficient generator (feta_coeff_fwd's arguments) in trailing workgroups
 * (ABI 6): get_filter_coefficients (transformer/models.py:240-283) needs only the attention matrix of the last layer,
 * which the launch before this one wrote - two half-empty launches of a captured step become one. */
typedef struct feta_coeff_fwd_role {
  const float* attn; const int32_t* n_real; const float* s; const float* gcn_bias; float* cj; float* pooled;
  int B, N, H, C;
} feta_coeff_fwd_role;
int feta_ffn_fwd_coeff(const feta_ffn* d, const feta_coeff_fwd_role* c, feta_stream_t stream);

/* ---- backward of the feed-forward half in ONE launch ------------------------------------------------
 * (feta_ffn_bwd_supported: d_model = 64, dim_feedforward in {64,128}.)  Replaces the two feta_rowlin_bwd_ex
 * launches of linear2 and linear1 of DiffTransformerEncoderLayer (contract transformer/models.py:166-167;
 * y2 = x1 + linear2(relu(linear1(x1)))):
 *   g2 = BatchNorm-2 backward of dy (g_y = y2 [M,64], g_bn [4][64], partial sums g_sum [Gs][2][64] finalized
 *        here -> g_fin_out [2][64], dgamma, dbeta; or g_fin already finalized) - or dy itself when g_y is NULL
 *        (LayerNorm stack: dy is the gradient w.r.t. y2);
 *   dh = (g2 W2) * [h > 0] (never written to memory);  dx = g2 + dh W1;
 *   sum_out (nullable) [feta_ffn_bwd_blocks(M)][2][64]: partial (sum dx, sum dx * xhat) with xhat from x = y1
 *        (pre-norm) and x_bn [4][64], for the BatchNorm-1 backward;
 *   partial: one row per chunk - feta_ffn_bwd_chunks(M, FF) rows (ABI 11; feta_rowlin_chunks(M) or half of it) -, pitch partial_ld (0: 2*64*FF + 64 + FF), columns
 *        [dW2 (64 x FF) | db2 (64) | dW1 (FF x 64) | db1 (FF)], reduced by the caller (feta_colsum).
 * x is seen through x_bn (scale, shift rows) when given, else used as it is. */
typedef struct feta_ffn_grad {
  const float* dy;
  const float* dy_b;   /* nullable: second part of the gradient, added to dy on load (feta_attn_block_grad.dx_b) */
  const float* g_y;
  const float* g_bn;
  const float* g_sum;
  int Gs;
  const float* g_fin;
  float* g_fin_out;
  float* dgamma;
  float* dbeta;
  const float* h;    /* [M,FF] saved relu output */
  const float* w2;   /* [64,FF] */
  const float* w1;   /* [FF,64] */
  const float* x;    /* [M,64] */
  const float* x_bn; /* [4][64] or NULL */
  float* dx;         /* [M,64] */
  float* sum_out;
  float* partial;
  int partial_ld;
  int M, FF;
  int dtype;         /* FETA_F32 | FETA_BF16: storage type of dy, dy_b, g_y, h, x, dx [T] (ABI 7) */
  int g_f32;         /* 1: dy and g_y are fp32 whatever dtype says (last layer of a bf16 stack, see feta_ffn.y_f32) */
  const float* g_ln_gamma; /* nullable [64] (ABI 9): dy is the gradient w.r.t. LN2(y2) = norm2's output and
                              g2 = LayerNorm backward of dy per row, computed on load from g_y = y2 (pre-norm rows; g_bn /
                              g_sum / g_fin must be NULL), as feta_attn_block_grad.ln1_gamma.  The partial rows gain
                              [dgamma2 (64) | dbeta2 (64)] behind db1 (default pitch 2*64*FF + 64 + FF + 128). */
  const float* x_ln_gamma; /* nullable [64]: x holds PRE-norm rows (y1), the operand is LayerNorm(x) * gamma + beta per
                              row on load; excludes x_bn */
  const float* x_ln_beta;
  float ln_eps;
} feta_ffn_grad;

int feta_ffn_bwd_supported(int d_model, int ff);
int feta_ffn_bwd_blocks(int M);
int feta_ffn_bwd_chunks(int M, int ff);   /* split-K chunks = rows of `partial` a launch writes */
int feta_ffn_bwd(const feta_ffn_grad* d, feta_stream_t stream);
/* ... and the BACKWARD kernel of the coefficient generator (feta_coeff_bwd with ds = NULL: partial [G, 2, C] is left
 * for the caller's feta_colsum_multi) in trailing workgroups of the first launch of the layer stack's backward. */
typedef struct feta_coeff_bwd_role {
  const float* cj; const int32_t* n_real; const float* s; const float* gcn_bias; const float* dpooled; float* partial;
  int B, N, H, C;
} feta_coeff_bwd_role;
int feta_ffn_bwd_coeff(const feta_ffn_grad* d, const feta_coeff_bwd_role* c, feta_stream_t stream);
/* ... or its saved form (feta_coeff_bwd_saved with ds = NULL: A / Bm from feta_coeff_dsum, partial
 * [feta_coeff_bwd_saved_groups(B, H), 2, C]); these workgroups trail the main ones. */
typedef struct feta_coeff_bwd_saved_role {
  const float* dpooled; const float* A; const float* Bm; float* partial;
  int B, H, C;
} feta_coeff_bwd_saved_role;
int feta_ffn_bwd_coeff_saved(const feta_ffn_grad* d, const feta_coeff_bwd_saved_role* c, feta_stream_t stream);

/* ---- the whole encoder stack for inference in ONE launch (ABI 12) ------------------------------------------
 * Forward of L DiffTransformerEncoderLayers (contract transformer/models.py:166-167,179,244; body per upstream GraphiT,
 * README.md:129) with nothing saved for a backward pass: in eval mode nothing couples two graphs (BatchNorm with running
 * statistics is a per-channel affine, LayerNorm is row-local, attention is per graph), so one workgroup runs every layer
 * of one graph with the activations in LDS.  Per layer:
 *   qkv = x W_in^T (+ b_in); attention core exactly as feta_attn_fwd (scale d_h^-1/2, keys >= n_real masked,
 *   exp(s - rowmax), * pe, / max(rowsum, 1e-6)); y1 = x + rowscale * (concat W_out^T + b_out); x1 = norm1(y1);
 *   y2 = x1 + relu(x1 W1^T + b1) W2^T + b2; x = norm2(y2)
 * norm: FETA_NORM_BATCH (eval BatchNorm: (v - running_mean) * rsqrt(running_var + eps) * gamma + beta) or
 * FETA_NORM_LAYER (affine LayerNorm of the row, biased variance, as F.layer_norm).
 * Rows of the [M = B*N, 64] tensors x, y, out are row(b, i) = b*row_sb + i*row_sn (seq-first [N,B,64]: row_sb = 1,
 * row_sn = B); padded rows i >= n_real are computed like every other row.  Only the last layer writes: y (after norm2),
 * out (its concatenated heads: out_each_head, transformer/models.py:179) and attn [B,H,N,N] (nullable).
 * feta_encoder_infer_supported: d_model = 64, heads in {4, 8}, 1 <= N <= 64, ff in {64, 128},
 * 1 <= L <= FETA_ENCODER_MAX_LAYERS.  The layer table is copied into the kernel arguments: `layers` is a HOST pointer,
 * read during the call only (the launch stays capturable). */
#define FETA_ENCODER_MAX_LAYERS 16
#define FETA_NORM_BATCH 0
#define FETA_NORM_LAYER 1
typedef struct feta_encoder_layer {
  const float* w_in;      /* [192,64] */
  const float* b_in;      /* [192] or NULL */
  const float* w_out;     /* [64,64] */
  const float* b_out;     /* [64] or NULL */
  const float* n1_gamma;  /* [64] norm1 weight */
  const float* n1_beta;   /* [64] norm1 bias */
  const float* n1_mean;   /* [64] norm1 running_mean (BatchNorm; NULL for LayerNorm) */
  const float* n1_var;    /* [64] norm1 running_var (BatchNorm; NULL for LayerNorm) */
  const float* w1;        /* [ff,64] */
  const float* b1;        /* [ff] or NULL */
  const float* w2;        /* [64,ff] */
  const float* b2;        /* [64] or NULL */
  const float* n2_gamma;
  const float* n2_beta;
  const float* n2_mean;
  const float* n2_var;
  float n1_eps, n2_eps;
  int tie_qk;             /* 1: K = Q (before the scale); rows 64..127 of w_in / b_in are not read */
} feta_encoder_layer;

struct feta_encoder_infer {   /* (a struct tag only: the entry point has the same name) */
  const float* x;         /* [M,64] input of the first layer */
  int64_t row_sb, row_sn;
  const float* pe;        /* [B,N,N] or NULL (broadcast over heads) */
  const int32_t* n_real;  /* [B] */
  const float* rowscale;  /* [M] degree scale per row, or NULL */
  float* y;               /* [M,64] output of the last layer */
  float* out;             /* [M,64] concatenated heads of the last layer */
  float* attn;            /* [B,H,N,N] of the last layer, or NULL */
  int B, N, H, FF, L;
  int norm;               /* FETA_NORM_BATCH | FETA_NORM_LAYER, every layer alike */
  const feta_encoder_layer* layers;  /* HOST pointer to L layer structs */
};

int feta_encoder_infer_supported(int N, int d_model, int heads, int ff, int L);
int feta_encoder_infer(const struct feta_encoder_infer* d, feta_stream_t stream);

/* ... with a compute type (additive, like feta_rowlin_ex / feta_layernorm_*_ex): the evaluation of a model on bf16
 * storage in the same ONE launch.
 *   dtype = FETA_F32   exactly feta_encoder_infer (4 and 8 heads), bit for bit; in_dtype must be FETA_F32.
 *   dtype = FETA_BF16  the LDS tiles (layer rows, q | k | v, h, concatenated heads, pe) hold bf16 and every contraction
 *                      is v_mfma_f32_16x16x16_bf16; accumulators, softmax, degree scale, residual adds and both norms are
 *                      fp32, a value is rounded once, when it is written to a tile or becomes an operand.  Weights, biases,
 *                      norm parameters and running statistics are the fp32 master tensors (rounded as operands); y, out
 *                      and attn are fp32, as feta_ffn.y_f32 / feta_attn_block.out_f32 of the training stack.  4 heads
 *                      (d_h = 16) only: bf16 storage has no d_h = 8 form.
 *   in_dtype           type of x and pe in HBM (FETA_BF16 with dtype = FETA_BF16 only; x 16-byte aligned either way):
 *                      they are rounded while they are staged, no cast launch in front of the stack.
 * feta_encoder_infer_ex_supported: feta_encoder_infer_supported, and heads = 4 for FETA_BF16. */
struct feta_encoder_infer_ex {   /* (a struct tag only: the entry point has the same name) */
  const void* x;          /* [M,64] input of the first layer, in_dtype */
  int64_t row_sb, row_sn;
  const void* pe;         /* [B,N,N] or NULL, in_dtype */
  const int32_t* n_real;  /* [B] */
  const float* rowscale;  /* [M] or NULL */
  float* y;               /* [M,64] */
  float* out;             /* [M,64] */
  float* attn;            /* [B,H,N,N] or NULL */
  int B, N, H, FF, L;
  int norm;               /* FETA_NORM_BATCH | FETA_NORM_LAYER */
  const feta_encoder_layer* layers;  /* HOST pointer to L layer structs */
  int dtype;              /* FETA_F32 | FETA_BF16: tile / compute type */
  int in_dtype;           /* FETA_F32 | FETA_BF16: type of x and pe */
};

int feta_encoder_infer_ex_supported(int N, int d_model, int heads, int ff, int L, int dtype);
int feta_encoder_infer_ex(const struct feta_encoder_infer_ex* d, feta_stream_t stream);

/* ---- the same stack as the FORWARD OF A TRAINING STEP of a LayerNorm stack, in ONE launch (additive) --------------------
 * LayerNorm is row-local and attention is per graph, so nothing couples two graphs in training mode either: the kernel
 * of feta_encoder_infer_ex runs every layer of a graph in one workgroup and - its compile-time SAVE form - every layer l
 * also writes what the backward kernels (feta_ffn_bwd, feta_attn_block_bwd with the LayerNorm on load) read, in the
 * layouts, row addressing row(b, i) = b*row_sb + i*row_sn and storage type [T] (dtype) that feta_attn_block_fwd /
 * feta_ffn_fwd produce:
 *   qkv        [M,192] [T]   in_proj result incl. bias, unscaled
 *   out_save   [M,64]  [T]   concatenated heads
 *   attn_stats [B,H,N,2]     row max of the scaled, masked scores; row sum after * pe, before the 1e-6 clamp
 *   y1         [M,64]  [T]   rows before norm1
 *   h          [M,FF]  [T]   after relu
 *   y2         [M,64]  [T]   rows before norm2 (layer l + 1 reads them as its x0; layer 0's x0 is x itself)
 * Each is ONE base pointer, layer l at base + l * <kind>_stride ELEMENTS (a multiple of 8; > 0 when L > 1).  Rows i < N
 * are written, padded rows n_real <= i < N included (computed like every other row, as the training kernels do; k and v
 * of a key tile without a real node are written too).  bf16 storage: a saved value is the LDS tile's value - what the
 * forward itself went on to use; the last layer's y2 leaves as fp32 in y2_last_f32 (as feta_ffn.y_f32: y2[L-1] is not
 * written) and `out` is the fp32 copy of the last layer's concatenated heads (as feta_attn_block.out_f32).  fp32 storage:
 * `out` may be NULL (out_save + (L-1) * out_stride already is that tensor), y2_last_f32 is not read.
 * LayerNorm only (norm = FETA_NORM_LAYER), no tie_qk, in_dtype = dtype (x is layer 0's saved x0).  y (after norm2 of the
 * last layer) and attn leave as in feta_encoder_infer_ex.  _sums: up to FETA_COLSUM_MAX_SEGS pending column sums in
 * trailing workgroups, as feta_attn_block_fwd_sums.  Capturable: layer table, pointers and strides travel by value. */
struct feta_encoder_fwd_save {   /* (a struct tag only: the entry point has the same name) */
  const void* x;          /* [M,64] [T] input of the first layer */
  int64_t row_sb, row_sn;
  const void* pe;         /* [B,N,N] [T] or NULL */
  const int32_t* n_real;  /* [B] */
  const float* rowscale;  /* [M] or NULL */
  float* y;               /* [M,64] */
  float* out;             /* [M,64] fp32 concatenated heads of the last layer (fp32 storage: nullable) */
  float* attn;            /* [B,H,N,N] or NULL */
  int B, N, H, FF, L;
  int norm;               /* FETA_NORM_LAYER */
  const feta_encoder_layer* layers;  /* HOST pointer to L layer structs */
  int dtype;              /* FETA_F32 | FETA_BF16: tile / compute / storage type */
  int in_dtype;           /* = dtype */
  void* qkv;
  void* out_save;
  float* attn_stats;
  void* y1;
  void* h;
  void* y2;
  float* y2_last_f32;     /* [M,64] (FETA_BF16), else NULL */
  int64_t qkv_stride, out_stride, attn_stats_stride, y1_stride, h_stride, y2_stride;
};

int feta_encoder_fwd_save_supported(int N, int d_model, int heads, int ff, int L, int dtype, int tie_qk);
int feta_encoder_fwd_save(const struct feta_encoder_fwd_save* d, feta_stream_t stream);
int feta_encoder_fwd_save_sums(const struct feta_encoder_fwd_save* d, const feta_colsum_seg* segs, int nseg,
                               feta_stream_t stream);

/* ---- graph preprocessing -------------------------------------------------------------
 * Dense Lhat = -D^-1/2 A D^-1/2 per graph from the batched edge list, with the exact
 * edge-list semantics of ChebConvDynamic.__norm__ (transformer/ChebNetDynamic.py:108-130):
 * self loops removed, degree scattered on the source row, duplicates summed, flow
 * source -> target (Lhat[b, t, s] += w).  lhat [B,N,N] must be zeroed by the caller;
 * deg [n_tot] is zero-initialised scratch.
 * edge_index [2,E] int64 (global node ids), node_graph [n_tot] int64, node_off [B] int32
 * (first global node id of graph b).
 */
int feta_lhat_from_edges(const int64_t* edge_index, int64_t E,
                         const int64_t* node_graph, const int32_t* node_off,
                         float* deg, float* lhat, int B, int N, int64_t n_tot,
                         feta_stream_t stream);

/* ---- LayerNorm over the feature dimension (norm1 / norm2 of DiffTransformerEncoderLayer with
 * batch_norm=False, contract transformer/models.py:505-506; the default of the TU / molhiv / SBM
 * scripts, experiments/run_transformer_gengcn_cv.py:56) --------------------------------------
 * y, out, dout, dy [M,D] row-major, D a multiple of 4, <= 256; stats [M,2] = (mean, rstd) per row
 * (biased variance, eps inside the root, as torch.nn.LayerNorm).  Backward also returns
 * dgamma_dbeta [2,D]; partial [feta_layernorm_blocks(M), 2, D] is caller-provided scratch.
 * partial_ld > 0: row pitch of partial, so that several LayerNorms share one
 * [feta_layernorm_blocks(M), total] buffer which the caller reduces with ONE feta_colsum
 * (dgamma_dbeta = NULL then), as feta_rowlin_ex.partial_ld does for the weight gradients.
 */
int feta_layernorm_blocks(int M);
int feta_layernorm_fwd(const float* y, const float* gamma, const float* beta, float eps, float* out,
                       float* stats, int M, int D, feta_stream_t stream);
int feta_layernorm_bwd(const float* dout, const float* y, const float* stats, const float* gamma,
                       float* dy, float* partial, int partial_ld, float* dgamma_dbeta, int M, int D,
                       feta_stream_t stream);
/* the same kernels with a storage type per tensor (FETA_F32 | FETA_BF16; ABI 7): the LayerNorm stack on bf16 storage
 * normalises bf16 rows into bf16 rows (fp32 into the filter stage behind the last layer), statistics and the
 * dgamma / dbeta partials stay fp32. */
int feta_layernorm_fwd_ex(const void* y, const float* gamma, const float* beta, float eps, void* out,
                          float* stats, int M, int D, int y_dtype, int out_dtype, feta_stream_t stream);
int feta_layernorm_bwd_ex(const void* dout, const void* y, const float* stats, const float* gamma,
                          void* dy, float* partial, int partial_ld, float* dgamma_dbeta, int M, int D,
                          int dout_dtype, int y_dtype, int dy_dtype, feta_stream_t stream);
/* ... with `stats` nullable (ABI 9): the forward applied this LayerNorm on load (feta_ffn.x_ln_gamma) and saved no
 * statistics - mean / rstd are recomputed from the pre-norm rows y with `eps` (the row is in registers: two more sums). */
int feta_layernorm_bwd_eps(const void* dout, const void* y, const float* stats, float eps, const float* gamma,
                           void* dy, float* partial, int partial_ld, float* dgamma_dbeta, int M, int D,
                           int dout_dtype, int y_dtype, int dy_dtype, feta_stream_t stream);

/* ---- spectrum producer ------------------------------------------------
 * Batched symmetric eigendecomposition, one workgroup per graph, the matrix in LDS (N <= 192) or, for
 * 192 < N <= 256, in a caller-provided workspace of feta_eigh_sym_workspace_bytes(B, N) bytes (0 for N <= 192;
 * the largest ogbg-molhiv bucket, BASELINE config 5, has 222 nodes):
 *   a [B,N,N]: the real n_b x n_b block of graph b is decomposed; as numpy.linalg.eigh does, only
 *   the LOWER triangle is read.  a + shift*I must be positive definite (Lhat = -D^-1/2 A D^-1/2 has
 *   its spectrum in [-1,1]: shift 2; L_sym: shift 1) - the one-sided Jacobi iteration runs on that
 *   matrix and the shift is taken off the eigenvalues again.
 *   u [B,N,K]: eigenvectors of the K smallest eigenvalues as columns, ascending; rows >= n_b and
 *   columns >= n_b are zero; the entry of largest magnitude of every column is positive.
 *   lam [B,K]: eigenvalues (0 for columns >= n_b).  sweeps [B] (may be NULL): Jacobi sweeps used.
 *   max_sweeps <= 0: 16.  tol <= 0: 1e-6 (a pair is rotated while |g_p.g_q| > tol |g_p||g_q|).
 * Replaces the per-graph host eigendecomposition of transformer/position_encoding.py:127-161 and
 * feeds feta_spec_filter_fwd/bwd (u, lam) directly.
 */
int feta_eigh_sym_supported(int N);
int64_t feta_eigh_sym_workspace_bytes(int B, int N);
int feta_eigh_sym(const float* a, const int32_t* n_real, float shift, float* u, float* lam,
                  int32_t* sweeps, float* workspace, int B, int N, int K, int max_sweeps, float tol,
                  feta_stream_t stream);

/* Kernel function of the spectrum on the real block, zero elsewhere:
 *   out_b = U_b f(lam_b + lam_offset) U_b^T,   out [B,N,N], u [B,N,K], lam [B,K]
 *   FETA_SPECTRAL_DIFFUSION: f(x) = exp(-beta x)     (DiffusionEncoding, position_encoding.py:65-72)
 *   FETA_SPECTRAL_PSTEP:     f(x) = (1 - beta x)^max(p,1)   (PStepRWEncoding, :83-93: p - 1 products)
 * zero_diag: the diagonal is cleared (PositionEncoding.apply_to, position_encoding.py:25-27).
 * With (u, lam) of Lhat pass lam_offset = 1 for the kernels of L_sym = I + Lhat.
 */
#define FETA_SPECTRAL_DIFFUSION 0
#define FETA_SPECTRAL_PSTEP 1
int feta_spectral_kernel(const float* u, const float* lam, const int32_t* n_real, int mode,
                         float beta, int p, float lam_offset, int zero_diag, float* out,
                         int B, int N, int K, feta_stream_t stream);

/* ---- device-resident graph store: one padded batch per launch ----------------------------------------
 * A split lives on the device as flat per-graph arrays (transformer/store.py: DeviceGraphStore), its spectra computed
 * once; feta_batch_gather builds the padded batch of the graphs `ids` names - the tensors data.BatchStager.stage and
 * attach_device_spectrum emit - in ONE launch, so that it can sit inside a captured training step and the host sends
 * the ids only (replaces GraphDataset_v2.collate_fn, transformer/data.py:161-225, and the pickle cache of
 * transformer/position_encoding.py:35-49).
 *   store: graph g owns the rows [s_node_off[g], s_node_off[g] + s_n[g]) of the per-node arrays s_x [sumN,F],
 *   s_degree [sumN], s_u [sumN,K], s_lap [sumN,lap_dim] (and of s_labels for node labels) and row g of s_lam [G,K];
 *   its n x n kernel starts at s_pe + s_pe_off[g] with a row pitch of n rounded up to a multiple of 4, the columns
 *   behind n zero, and s_pe_off[g] a multiple of 4: every row starts on 16 bytes.
 *   ids [B] int32 ON THE DEVICE.  An id outside [0, G) or a graph with more than N nodes gives an empty graph
 *   (n_real 0, everything masked, zeros, label 0 / -100) and nothing of the store is read for it.
 *   outputs: every one may be NULL (skipped; its store array may then be NULL too); EVERY element of the others is
 *   written, the padding included, so no buffer has to be cleared between replays.
 * One workgroup per graph and 64-row chunk (grid B x ceil(N / 64)), no LDS.  16-byte loads where the widths (F, N, K,
 * lap_dim multiples of 4) and the pointers (16-byte aligned; bf16 outputs 8) allow, element-wise otherwise.
 * x / pe as FETA_BF16: rounded to nearest even from the stored fp32. */
#define FETA_LABELS_NONE 0
#define FETA_LABELS_GRAPH_F32 1   /* s_labels float [G]      -> labels float [B] */
#define FETA_LABELS_GRAPH_I64 2   /* s_labels int64 [G]      -> labels int64 [B] */
#define FETA_LABELS_NODE_I64 3    /* s_labels int64 [sumN]   -> labels int64 [B,N], -100 on the padded positions */
typedef struct feta_gather {
  const float* s_x;            /* [sumN,F] */
  const float* s_degree;       /* [sumN] */
  const void* s_labels;        /* label_kind */
  const int32_t* s_n;          /* [G] node counts */
  const int64_t* s_node_off;   /* [G] first row of each graph */
  const float* s_pe;           /* flat, see above */
  const int64_t* s_pe_off;     /* [G] n x n block offsets (feta_gather_ex: shared with s_lhat) */
  const float* s_u;            /* [sumN,K] */
  const float* s_lam;          /* [G,K] */
  const float* s_lap;          /* [sumN,lap_dim] */
  const int32_t* ids;          /* [B], device */
  int G, B, N, F, K, lap_dim;
  int dtype;                   /* FETA_F32 | FETA_BF16: storage type of the outputs x and pe [T] */
  int label_kind;              /* FETA_LABELS_* */
  void* x;                     /* [B,N,F] [T] */
  void* mask;                  /* [B,N] bytes, 1 = padding */
  float* degree;               /* [B,N] */
  float* degree_rows;          /* [N*B], row = node * B + graph */
  void* pe;                    /* [B,N,N] [T] */
  float* u;                    /* [B,N,K] */
  float* lam;                  /* [B,K] */
  float* lap;                  /* [B,N,lap_dim] */
  int32_t* n_real;             /* [B] */
  int32_t* node_off;           /* [B] exclusive prefix sum of n_real (B * N < 2^24) */
  void* labels;                /* label_kind */
} feta_gather;
int feta_batch_gather(const feta_gather* d, feta_stream_t stream);

/* ... with the dense scaled Laplacian of filter_mode='cheb' and the per-batch sign flip of the Laplacian eigenvector
 * features (additive, like feta_encoder_infer_ex): the fields of feta_gather, in its order, and behind them
 *   s_lhat    graph g's n x n block of Lhat (feta_lhat_from_edges) in the geometry of s_pe: it starts at
 *             s_lhat + s_pe_off[g], row pitch n rounded up to a multiple of 4, zero columns behind n.  s_pe_off holds
 *             "n x n block offsets" shared by both arrays and is required whenever pe or lhat is requested.
 *   lhat      [B,N,N], ALWAYS fp32 (the filter stage is fp32 on both storage types): rows and columns behind n_real
 *             zero, the whole block zero for an empty slot; every element is written on every launch.  16-byte vectors
 *             when N % 4 == 0, both pointers are 16-byte aligned and the block offset is a multiple of 4.
 *   lap_sign  [lap_dim] on the device or NULL: lap[b,i,c] = s_lap[.,c] * lap_sign[c] (train.lap_sign_flip, one draw per
 *             batch: experiments/run_transformer_gengcn.py:126-131); the padding stays zero.  Needs lap.
 * With s_lhat = lhat = lap_sign = NULL it writes what feta_batch_gather writes, bit for bit.  Same grid, no LDS. */
typedef struct feta_gather_ex {
  const float* s_x;
  const float* s_degree;
  const void* s_labels;
  const int32_t* s_n;
  const int64_t* s_node_off;
  const float* s_pe;
  const int64_t* s_pe_off;     /* [G] n x n block offsets, of s_pe and of s_lhat */
  const float* s_u;
  const float* s_lam;
  const float* s_lap;
  const int32_t* ids;
  int G, B, N, F, K, lap_dim;
  int dtype;
  int label_kind;
  void* x;
  void* mask;
  float* degree;
  float* degree_rows;
  void* pe;
  float* u;
  float* lam;
  float* lap;
  int32_t* n_real;
  int32_t* node_off;
  void* labels;
  const float* s_lhat;         /* flat, see above */
  float* lhat;                 /* [B,N,N] fp32 */
  const float* lap_sign;       /* [lap_dim] or NULL */
} feta_gather_ex;
int feta_batch_gather_ex(const feta_gather_ex* d, feta_stream_t stream);

/* ---- graph-level readout of an evaluation batch: pooling, classifier, loss and metric terms in one launch ----------
 * What the graph-level task shells run behind the encoder (masked mean pooling, Linear - activation - Linear:
 * transformer/models.py) and the per-graph arithmetic of the reference's eval_epoch, forward only, for a batch that
 * feta_batch_gather built: slot b holds the graph ids[b] of a split of G graphs.  For every slot b < *count with
 * 0 <= ids[b] < G and 1 <= n_real[b] <= N (every other slot writes NOTHING):
 *   pooled = mean of the rows y[i, b, :], i < n_real[b]        (row (i, b) starts at y + i * row_sn + b * row_sb)
 *   h      = act(w1 pooled + b1), act(v) = v > 0 ? v : slope * v  (slope 0: ReLU; slope 1: the molhiv shell's identity)
 *   scores[ids[b], 0..C) = w2 h + b2
 *   terms[ids[b], 0..4) by loss_kind, from the slot's label (label_kind FETA_LABELS_GRAPH_F32 | FETA_LABELS_GRAPH_I64):
 *     FETA_LOSS_L1          (|e|, e^2, 0, 1), e = logit - label                                            C = 1
 *     FETA_LOSS_BCE_LOGITS  (bce, hit, 0, w): bce the binary cross entropy with logits, hit = (logit > 0) == (label > 0.5),
 *                           w = 1; a NaN label (an unlabelled graph) gives bce = 0 and w = 0               C = 1
 *     FETA_LOSS_CE          (-log softmax[label], argmax == label, 0, 1): log-sum-exp with the row maximum subtracted, the
 *                           first index wins a tie; int64 labels; a label outside [0, C) gives (NaN, 0, 0, 1)
 * count lives ON THE DEVICE, so a captured launch serves every batch length up to B; scores and terms are indexed by the
 * graph's id in the split, so they do not depend on the order or the cut of the batches.  One workgroup per slot, no
 * atomics, one summation order: a graph's results are bit-equal from launch to launch and from batch to batch.  16-byte
 * loads where y (base and both strides), w1, w2 and terms are aligned for them. */
#define FETA_LOSS_L1 0
#define FETA_LOSS_BCE_LOGITS 1
#define FETA_LOSS_CE 2
typedef struct feta_readout {
  const float* y;              /* encoder output rows, fp32, 64 dense columns */
  int64_t row_sb, row_sn;      /* element strides of the graph and the node index ([N,B,64] contiguous: 64, 64 B) */
  const int32_t* n_real;       /* [B] */
  const int32_t* ids;          /* [B] graph id of each slot, device */
  const int32_t* count;        /* [1] live slots, device */
  const void* labels;          /* [B], label_kind */
  const float* w1;             /* [64,64] */
  const float* b1;             /* [64] or NULL */
  const float* w2;             /* [C,64] */
  const float* b2;             /* [C] or NULL */
  float* scores;               /* [G,C] */
  float* terms;                /* [G,4] */
  int B, N, G, C, d_model;
  int label_kind;              /* FETA_LABELS_GRAPH_F32 | FETA_LABELS_GRAPH_I64 */
  int loss_kind;               /* FETA_LOSS_* */
  float slope;
} feta_readout;
int feta_readout_eval_supported(int d_model, int C);   /* d_model = 64, 1 <= C <= 64 */
int feta_readout_eval(const feta_readout* d, feta_stream_t stream);

/* ---- graph-level readout of a TRAINING batch: pooling, classifier, loss and their backward in four launches ---------
 * The training counterpart of feta_readout_eval: the same pooled / h / logits arithmetic per slot (the same device
 * code), the batch loss of train.task_loss on the device, and the backward of all of it.  A slot b is LIVE when
 * b < *count and 1 <= n_real[b] <= N; a slot b < *count with another n_real is read as an empty graph (zero scores, term
 * and weight 0, zero gradient).  Slots b >= *count write nothing in the forward.
 *
 * feta_readout_train_fwd, two launches (one workgroup per slot, then one workgroup for the loss):
 *   scores[b, 0..C) = w2 h + b2                                                        (by SLOT, not by graph id)
 *   (term_b, weight_b) = the first and the last loss term of feta_readout_eval for loss_kind and the slot's label
 *   loss[0] = (sum_b term_b) / (sum_b weight_b), loss[1] = 1 / sum_b weight_b          (b < *count, ascending;
 *                                                                                        sum weight = 0: NaN and inf)
 *   ws: per slot pooled, the pre-activation z = w1 pooled + b1, the unscaled dlogit, (term, weight)
 *     dlogit  FETA_LOSS_L1 sign(e) with sign(0) = 0 | FETA_LOSS_BCE_LOGITS (sigmoid(x) - label) weight_b |
 *             FETA_LOSS_CE softmax - onehot (a label outside [0, C): NaN)
 * feta_readout_train_bwd, two launches (one workgroup per slot, then the parameter gradients), after the forward on the
 * same descriptor and ws; *dloss is the incoming gradient of loss[0], read ON THE DEVICE:
 *   s = *dloss * loss[1];  dl = s dlogit;  dz = (w2^T dl) * (z > 0 ? 1 : slope);  dpooled = w1^T dz
 *   dy[i, b, :] = dpooled / n_real[b] for i < n_real[b] of a live slot, ZERO in every other row of every slot b < B
 *   dw1 = sum_b dz_b (x) pooled_b, db1 = sum_b dz_b, dw2 = sum_b dl_b (x) h_b, db2 = sum_b dl_b   (b < *count, ascending)
 *   dy, dw1, db1, dw2, db2: NULL skips the output.  The parameter gradients are tiled over output rows (16 per
 *   workgroup) and walk the slots in chunks of 64.
 * No atomics, no library call, one summation order: two runs on the same operands are bit-equal.  ws holds
 * feta_readout_train_ws_floats(B, C) floats, 16-byte aligned, caller-owned, and must survive from the forward to the
 * backward.  16-byte accesses where y / dy (base and both strides), w1 and w2 are aligned for them. */
typedef struct feta_readout_train {
  const float* y;              /* encoder output rows, fp32, 64 dense columns */
  int64_t row_sb, row_sn;      /* element strides of y's graph and node index */
  const int32_t* n_real;       /* [B] */
  const int32_t* count;        /* [1] live slots, device */
  const void* labels;          /* [B], label_kind */
  const float* w1;             /* [64,64] */
  const float* b1;             /* [64] or NULL */
  const float* w2;             /* [C,64] */
  const float* b2;             /* [C] or NULL */
  float* scores;               /* [B,C] */
  float* loss;                 /* [2]: the batch loss, 1 / sum of the weights */
  float* ws;                   /* feta_readout_train_ws_floats(B, C) floats */
  const float* dloss;          /* [1] gradient of loss[0], device (backward only) */
  float* dy;                   /* backward: [N,B,64] rows with the strides below, or NULL */
  int64_t drow_sb, drow_sn;
  float* dw1;                  /* backward: [64,64] or NULL */
  float* db1;                  /* backward: [64] or NULL */
  float* dw2;                  /* backward: [C,64] or NULL */
  float* db2;                  /* backward: [C] or NULL */
  int B, N, C, d_model;
  int label_kind;              /* FETA_LABELS_GRAPH_F32 | FETA_LABELS_GRAPH_I64 */
  int loss_kind;               /* FETA_LOSS_* */
  float slope;
} feta_readout_train;
int feta_readout_train_supported(int d_model, int C);   /* d_model = 64, 1 <= C <= 64 */
int64_t feta_readout_train_ws_floats(int B, int C);
int feta_readout_train_fwd(const feta_readout_train* d, feta_stream_t stream);
int feta_readout_train_bwd(const feta_readout_train* d, feta_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FETA_HIP_H_ */
