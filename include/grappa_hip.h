/* grappa_hip.h -- C ABI of libgrappa_hip.so: the MI355X (gfx950) kernels of the Grappa hot path.
 *
 * The reference (hits-mbm-dev/grappa) has no native layer: every function below replaces a piece of
 * Python that today expands into torch/DGL device kernels.  Each entry point cites the reference
 * lines (relative to /root/reference/src/grappa/) whose arithmetic it computes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed / torch.cuda tensor storage) unless named h_*;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *   - no allocation, no mutable global state, re-entrant per stream and per host thread: every option of a call travels in its arguments
 *     (ABI 10 removed the four process-wide setters: plan override, tail launches, split-K reduction, dropout salt); scratch comes from the
 *     caller (`ws`, `ws_bytes`; sizes from the *_workspace_bytes() queries).  The library reads no environment variable: what used to be one
 *     is a constant of the build;
 *   - return 0 on success, a negative GRAPPA_ERR_* otherwise (never throws / aborts);
 *   - fp32 activations, int32 indices, row-major, leading dimensions in ELEMENTS.
 */
#ifndef GRAPPA_HIP_H
#define GRAPPA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRAPPA_OK 0
#define GRAPPA_ERR_ARG (-1)        /* unsupported shape / null pointer / bad enum */
#define GRAPPA_ERR_LAUNCH (-2)     /* hipGetLastError() != hipSuccess after the launch */
#define GRAPPA_ERR_WORKSPACE (-3)  /* ws_bytes too small */

#define GRAPPA_ABI_VERSION 11
int grappa_abi_version(void);
/* name of the offload arch the library was compiled for ("gfx950") */
const char* grappa_build_arch(void);
/* kernels this library has launched in this process since the last reset (reset != 0: returns the count and clears it); measurement only */
long long grappa_launch_count(int reset);

/* ------------------------------------------------------------------------------------------------
 * Dense blocks.  C = epilogue(opA(A) * opB(B)); the arithmetic of the product is grappa_gemm_desc.precision (below): the engine's default is
 * F32_F16X3 (fp32 operands as two fp16 pieces, three partial products on v_mfma_f32_32x32x16_f16), the native fp32 matrix instruction
 * (v_mfma_f32_32x32x2_f32) serves products with M or N <= 32 and precision F32_MFMA.
 *   A(m,k) = a_kcontig ? A[m*lda + k] : A[k*lda + m]
 *   B(n,k) = b_kcontig ? B[n*ldb + k] : B[k*ldb + n]
 *   forward  Y = X W^T      : a_kcontig=1 (X[M,K]),  b_kcontig=1 (W[N,K])   nn.Linear
 *   dgrad    dX = dY W      : a_kcontig=1 (dY[M,N']), b_kcontig=0 (W[N',K'])
 *   wgrad    dW = dY^T X    : a_kcontig=0 (dY[tok,N']), b_kcontig=0 (X[tok,K'])
 * epilogue, in this order, per element v = acc(m,n):
 *   v += pre[m,n]                          (pre != NULL: pre-activation addend, e.g. a second GEMM's result)
 *   v += bias[n]                           (bias != NULL)
 *   v  = elu(v)                            (act == GRAPPA_ACT_ELU)
 *   v *= (aux[m,n] > 0 ? 1 : aux[m,n]+1)   (aux != NULL: ELU'(z) from the saved ELU output)
 *   if (C2) { C[m,n] = v; }                (pre-dropout copy kept for the backward pass)
 *   v  = keep(seed, m*N+n) ? v/(1-p) : 0   (drop_p > 0; counter based, see grappa_dropout_keep)
 *   v += res[m,n]                          (res != NULL)
 *   v += OUT[m,n]                          (accumulate != 0)
 *   OUT[m,n] = v                           OUT = C2 ? C2 : C
 * Replaces: torch.nn.Linear / ELU / Dropout / residual adds in models/graph_attention.py:98-101,
 * :125-127, :261-272, :286-308; models/network_utils.py:44-54, :112-126 (in_proj/out_proj of
 * nn.MultiheadAttention); models/interaction_parameters.py:148-161; perm_equiv_transformer.py:231-264.
 */
#define GRAPPA_ACT_NONE 0
#define GRAPPA_ACT_ELU 1

/* Arithmetic of the product (grappa_gemm_desc.precision).  Inputs, outputs, epilogue and accumulation are fp32 in every mode.
 *   F32_MFMA    native fp32 matrix instruction (157 TFLOP/s peak; the value 0 of a zeroed descriptor -- the Python engine asks for F32_F16X3)
 *   F32_BF16X9  each fp32 operand split exactly into 3 bf16 pieces, all 9 partial products on the bf16 matrix cores: every
 *               partial product is exact, the result differs from an fp32 FMA chain only by accumulation order
 *   F32_BF16X6  the 6 largest partial products (drops terms <= 2^-24 |a||b|): fp32-grade, ~2 ulp per product
 *   BF16X3      2 pieces / 3 products (~2^-16 relative);  BF16: operands rounded to bf16 (the "bf16" trainer precision of
 *               the reference's configs, experiment/trainrun.py / Lightning `precision`)
 *   F32_F16X3   (ABI 4) each fp32 operand, scaled by a power of two per row of the product so that its largest magnitude lands in
 *               [2^14, 2^15), is split into 2 fp16 pieces (11 + 11 significant bits and a sign: a - hi - lo <= 2^-24 |a|); the 3
 *               products hi*hi + hi*lo + lo*hi run on the fp16 matrix cores (every product exact in fp32), the dropped lo*lo is
 *               <= 2^-24 |a||b|: fp32-grade like F32_BF16X6 at half the matrix instructions.  Needs a_amax / b_amax (below): the
 *               largest |element| of every row of the product's A (M values) and B (N values), from grappa_amax_f32.  Elements
 *               more than 2^16 below their row's maximum lose relative (never absolute: <= 2^-39 of the maximum) precision.
 * Shapes with M <= 32 or N <= 32 always take the native fp32 path. */
#define GRAPPA_GEMM_F32_MFMA 0
#define GRAPPA_GEMM_F32_BF16X9 1
#define GRAPPA_GEMM_F32_BF16X6 2
#define GRAPPA_GEMM_BF16X3 3
#define GRAPPA_GEMM_BF16 4
#define GRAPPA_GEMM_F32_F16X3 5

typedef struct grappa_gemm_desc {
    int M, N, K;
    int a_kcontig, b_kcontig;
    const float* A; int lda;
    const float* B; int ldb;
    float* C; int ldc;
    float* C2; int ldc2;          /* optional second output (see above) */
    const float* bias;            /* [N] or NULL */
    const float* res; int ldres;  /* [M,N] or NULL */
    const float* aux; int ldaux;  /* [M,N] or NULL */
    const float* pre; int ldpre;  /* [M,N] or NULL */
    float* a_colsum;              /* [M] or NULL; a_kcontig == 0 only: a_colsum[m] += sum_k A(m,k)  (bias gradient of a wgrad GEMM) */
    int act;
    float drop_p;
    uint64_t drop_seed;
    int accumulate;
    int precision;                /* GRAPPA_GEMM_* */
    /* ---- plane format (ABI 3; everything below may be 0 / NULL).  A matrix X "in planes" is three bf16 matrices P0, P1, P2 of
     * X's shape, P0 = bf16(X), P1 = bf16(X - P0), P2 = bf16(X - P0 - P1), X == P0 + P1 + P2 exactly; plane p starts
     * `*_plane_stride` ELEMENTS after plane 0, leading dimensions are in bf16 elements and multiples of 8, bases 16-byte aligned.
     * a_planes / b_planes != 0: A / B point to plane 0 (the pointer types above are then nominal).  Supported: b_planes alone
     * ("weight planes": A = fp32 activations [M][K] with K % 32 == 0, a_kcontig = b_kcontig = 1 -- forward with the planes of W,
     * dgrad with the planes of W^T; results are bit-identical to the split-in-kernel product) or both (a_kcontig = b_kcontig = 1,
     * or both 0 = the wgrad layout).  K-contiguous planes must be zero beyond K up to the next multiple of 32 (ld >= round_up(K, 32));
     * k-major operands need no padding (rows beyond K are taken from a page of zeros); rows * ld * element size < 2^32; M, N > 32.  The operands are
     * split ONCE by their producer (grappa_split_planes_f32, Cp below) instead of by every GEMM that reads them. */
    int a_planes, b_planes;
    size_t a_plane_stride, b_plane_stride;
    uint16_t* Cp; int ldcp; size_t cp_plane_stride;               /* planes of the FINAL value (what OUT receives); C may be NULL then */
    const uint16_t* resp; int ldresp; size_t resp_plane_stride;   /* residual given in planes (instead of res) */
    const uint16_t* auxp; int ldauxp; size_t auxp_plane_stride;   /* saved ELU output given in planes (instead of aux) */
    /* number of planes behind Cp / resp / auxp: 3 (0 means 3) = the exact fp32 split; 1 = a plain bf16 tensor (the bf16 storage
     * configuration: activations are kept in bf16 in HBM, precision GRAPPA_GEMM_BF16 reads plane 0 of both operands) */
    int cp_nplanes, resp_nplanes, auxp_nplanes;                   /* (Cp / C1p / resp / auxp are not available with F32_MFMA or M, N <= 32) */
    uint16_t* C1p; int ldc1p;                                     /* bf16 copy of the value C receives when C2 is used (before dropout / residual) */
    /* ---- ABI 4, precision F32_F16X3 only: bit patterns of max_k |A(m, k)| (M values) and max_k |B(n, k)| (N values); fp32 operands.
     * amax_bcast bit 0 / bit 1: a_amax / b_amax is ONE value for all rows (an upper bound of the whole operand; the weight-gradient
     * product, whose reduction runs over the tokens, takes max over the token maxima: elements more than 2^16 below the tensor's
     * largest lose relative precision gradually, absolute error <= 2^-39 of that largest) */
    const uint32_t* a_amax; const uint32_t* b_amax; int amax_bcast;
    /* any precision, optional: receives max_n |OUT(m, n)| (M values, fp32 bit patterns) of the final fp32 output, for a following
     * F32_F16X3 product that reads OUT as its A operand.  The row epilogue leaves per-segment maxima in the workspace (behind the
     * split-K slabs: grappa_gemm_f32_workspace_bytes includes them) and one small launch combines them; not with the grouped entry */
    uint32_t* out_amax;
    /* ---- ABI 5, the PAIR format: an fp32 matrix X[R][C] as fp16 (HI, LO) pairs plus one fp32 bit pattern per row, amax_r >= max_c
     * |X[r][c]| (the row's largest magnitude or an upper bound of it):
     *     s_r = 141 - exponent_field(amax_r),  HI = f16(X * 2^s_r),  LO = f16(X * 2^s_r - HI),  X = (HI + LO) * 2^-s_r
     * i.e. exactly the operand precision F32_F16X3 builds from fp32 rows inside every workgroup, built once by the tensor's producer
     * instead (grappa_split_pairs_f32; the *_pairs_* producers below) at the same 4 bytes per element.  Layout: a row is a sequence
     * of blocks of 16 consecutive k, each [16 x HI | 16 x LO] (one 64-byte granule): element (r, k) has HI at fp16 index
     * r * ld + 32 * (k / 16) + k % 16 and LO 16 further; ld (fp16 elements) >= 2 * round_up(C, 32) and a multiple of 8, base 16-byte
     * aligned, zeros beyond C up to the next multiple of 32.  precision F32_F16X3 with a_planes != 0 and b_planes != 0
     * (a_kcontig = b_kcontig = 1: forward with the pairs of W, dgrad with the pairs of W^T; lda / ldb = the rows' ld, plane strides
     * unused) reads both operands as pairs by LDS-DMA, a_amax / b_amax being the rows' amax_r; the result is bit-identical to the
     * fp32-operand F32_F16X3 product of the same scales and K split.  M, N > 32; rows * ld * 2 < 2^32.
     * b_planes != 0 alone ("weight pairs": A = fp32 activations [M][K], K % 16 == 0, lda % 4 == 0, 16-byte aligned, a_kcontig =
     * b_kcontig = 1) takes A as it is -- raw fp32 rows by LDS-DMA, each wavefront splits the fragments of its own 64 rows -- and gives
     * the same bits as the all-pairs product.  a_planes != 0 alone is refused. */
    /* ---- ABI 7: the residual given as the INPUT of a LayerNorm.  res_ln_mean != NULL: `res` holds x, the rows BEFORE normalisation, and the
     * epilogue adds LayerNorm(x)(m, n) = fma((x(m, n) - mean[m]) * rstd[m], gamma[n], beta[n]) -- the very bits grappa_layernorm_fwd_*
     * writes -- so that a producer that hands its normalised rows on in the pair format need not write them in fp32 as well (inference).
     * fp32 `res` (not resp), N % 4 == 0, gamma / beta 16-byte aligned, the split kernels only (M, N > 32, precision other than F32_MFMA; fp32
     * operands or both in the pair format): every epilogue form of those (straight-line classes, the generic row walk with C2 / activation,
     * the split-K reduction) adds the recomputed rows; anything else is refused (GRAPPA_ERR_ARG). */
    const float* res_ln_mean; const float* res_ln_rstd; const float* res_ln_gamma; const float* res_ln_beta;
    /* ---- ABI 8: operands of a WEIGHT-GRADIENT product (a_kcontig = b_kcontig = 0, precision F32_F16X3, grappa_gemm_f32_grouped only) in
     * the pair format.  a_planes != 0: A is the [K tokens][M features] matrix as its producer wrote it for the forward / input-gradient
     * products -- pairs, token row k scaled by its own maximum a_rowmax[k] (K values) -- lda in fp16 elements (>= 2 * M, % 8 == 0), M % 32
     * == 0, 16-byte aligned; a_amax (with amax_bcast bit 0) = the maximum over the token maxima.  The kernel moves every token row onto the
     * tensor's scale with exact fp16 multiplications by powers of two (the halves a fresh split under that scale would give, up to the
     * rounding of fp16 denormals).  b_planes / b_rowmax / bit 1: the same for B ([K tokens][N features]).  One operand may stay fp32.
     * The products of one grouped call may mix formats (one launch either way; a group of one combination runs the kernel specialised for it). */
    const uint32_t* a_rowmax; const uint32_t* b_rowmax;
    /* ---- ABI 8: row maxima of OUT left as the per-segment partials the epilogue writes anyway, combined by the CONSUMER.
     * out_amax_parts != NULL (instead of out_amax; the split kernels only: M, N > 32, precision other than F32_MFMA): receives
     * nseg = ceil(N / 32) arrays of M maxima, parts[seg * M + m].  A following product whose A operand is OUT (forward / input-gradient
     * layout, fp32 operands) passes a_amax = parts and a_amax_nseg = nseg and takes the maximum over the segments itself;
     * grappa_amax_reduce over all nseg * M values gives the whole-tensor maximum of a weight-gradient product. */
    uint32_t* out_amax_parts; int a_amax_nseg;
    /* ---- ABI 10: the options that used to be process-wide setters, per call (all 0 / NULL = the library's defaults).
     * plan_cfg: tuning and tests -- force the tile configuration index plan_cfg - 1 (0: the plan's own choice); plan_nsplit: force the split-K
     * factor (0: own choice).  plan_tail: the "tail launch" (when the tile grid is 256 q + rem workgroups, the rem tiles run as a second launch
     * with their K range cut): 0 = the default (allowed), 1 = allowed, 2 = never (a caller that keeps several
     * streams busy: the partial last round then runs beside another stream's kernels), 3 = forced where possible (tests).  Results differ only
     * in the summation order of the tail tiles' K slices.
     * splitk_reduce: where a split-K product of the fp32-operand split kernels sums its K slices -- 0 = default (a launch of the reduction kernel
     * behind the product), 1 = the reduction launch, 2 = inside the product's own launch
     * (the last workgroup of a tile to arrive adds the slabs in the fixed order 0, 1, ...).  Same bits either way.
     * drop_salt: one uint64 in DEVICE memory (or NULL: none) mixed into drop_seed when the kernel runs: seed + word * 0x9E3779B97F4A7C15.  A
     * train step captured in a hipGraph increments the word inside the graph: every replay draws fresh masks while forward and backward of
     * one replay agree.  (The row-wise kernels that draw the same masks take the same pointer as their last argument.) */
    int plan_cfg, plan_nsplit, plan_tail, splitk_reduce;
    const uint64_t* drop_salt;
} grappa_gemm_desc;

/* Largest magnitudes of an fp32 matrix x[R][C] (leading dimension ldx), as fp32 bit patterns: row_amax[r] = max_c |x[r][c]|,
 * col_amax[c] = max_r |x[r][c]| (either may be NULL), one pass over x.  A product's operand uses the array ALONG which it is
 * not reduced: forward x[tok][in] -> row_amax, W[out][in] -> row_amax; dgrad dY[tok][out] -> row_amax, W -> col_amax;
 * wgrad dY -> col_amax, x -> col_amax (or, with amax_bcast, the single maximum of each: grappa_amax_reduce over the row maxima).
 * NaN counts as larger than everything (the product is then NaN / Inf as in fp32).
 * ws: grappa_amax_f32_workspace_bytes(R, C) bytes (partial column maxima), needed only with col_amax. */
size_t grappa_amax_f32_workspace_bytes(int R, int C);
int grappa_amax_f32(void* stream, int R, int C, const float* x, int ldx, uint32_t* row_amax, uint32_t* col_amax, void* ws, size_t ws_bytes);
/* Row and column maxima of many small matrices in ONE launch (the weights of a model, refreshed once per optimiser step): matrix i is
 * handled by workgroup i.  `descs` is a DEVICE array; every matrix needs C % 4 == 0, C <= 2048, ld % 4 == 0 and a 16-byte aligned base
 * (the caller checks: the library cannot read the table). */
typedef struct grappa_amax_item {
    const float* x; int R, C, ld, pad_;
    uint32_t* row_amax; uint32_t* col_amax;
} grappa_amax_item;
int grappa_amax_f32_batched(void* stream, int count, const grappa_amax_item* descs);
/* out[b] = max_i in[b][i], i < n[b], for `count` arrays in one launch per 32 (bit patterns of magnitudes: unsigned order): whole-tensor
 * maxima from row maxima.  `in` and `n` are HOST arrays (of device pointers / lengths). */
int grappa_amax_reduce(void* stream, int count, const uint32_t* const* in, const int* n, uint32_t* out);
/* out[m] = max over seg of parts[seg * M + m]: the row maxima from a product's per-segment partials (grappa_gemm_desc.out_amax_parts), for a
 * consumer that needs them as one array */
int grappa_amax_combine(void* stream, int M, int nseg, const uint32_t* parts, uint32_t* out);

/* fp32 X[R][C] -> plane format: planes[p][r][c] (transpose == 0) or planes[p][c][r] (transpose != 0), p = 0..2, leading
 * dimension ldp, `plane_stride` elements between planes.  Only the R x C (C x R) block is written: padding the GEMM relies on
 * (zeros up to the next multiple of 32 along k) is the caller's (allocate zeroed).  Weights are split once per optimiser step
 * (grappa_amd/optim.py WeightPlanes), both orientations: W for the forward product, W^T for dgrad. */
int grappa_split_planes_f32(void* stream, int R, int C, const float* x, int ldx, uint16_t* planes, int ldp, size_t plane_stride,
                            int transpose);

/* ABI 5: fp32 X[R][C] -> pair format (see grappa_gemm_desc): row r of the output is row r of X (transpose == 0) or column r of X
 * (transpose != 0), leading dimension ldp fp16 elements.  amax: the bit patterns that define the scale of every OUTPUT row (R values,
 * or C values when transposing: grappa_amax_f32's row_amax / col_amax).  Only the elements of X are written; the zero padding along k
 * is the caller's (allocate zeroed).  Weights are split once per optimiser step, both orientations; activations by their producers. */
int grappa_split_pairs_f32(void* stream, int R, int C, const float* x, int ldx, const uint32_t* amax, uint16_t* pairs, int ldp, int transpose);
/* The same for many matrices in ONE launch (the weights of a model, both orientations, once per optimiser step).  `items` lives in DEVICE
 * memory; tile_begin = number of 32 x 32 tiles ((R + 31) / 32 * ((C + 31) / 32)) of the items before this one, total_tiles their sum;
 * amax = the row maxima of X (transpose == 0) or its column maxima (transpose != 0: the pairs of X^T, [C][R]). */
typedef struct grappa_split_pairs_item {
    const float* x; const uint32_t* amax; uint16_t* pairs;
    int R, C, ldx, ldp, transpose, tile_begin;
} grappa_split_pairs_item;
int grappa_split_pairs_f32_batched(void* stream, int count, int total_tiles, const grappa_split_pairs_item* items);

/* workspace of a product: enough for every plan the library may choose for this shape whatever plan_tail / splitk_reduce say (plan_cfg and
 * plan_nsplit = 0); a descriptor that forces a configuration or a split asks grappa_gemm_f32_workspace_bytes_desc */
size_t grappa_gemm_f32_workspace_bytes(int M, int N, int K);
size_t grappa_gemm_f32_workspace_bytes_desc(const grappa_gemm_desc* d);
/* host-only: the tile (tile_m x tile_n x 32) and split-K factor the launcher will use for this shape (default options), and the "tail": when
 * the tile grid is 256*q + rem workgroups, the rem tiles run as a second launch with their K range split tail_nsplit ways */
int grappa_gemm_f32_plan(int M, int N, int K, int precision, int* tile_m, int* tile_n, int* nsplit, int* tail_tiles, int* tail_nsplit);
/* ABI 10: the same for a descriptor's M, N, K, precision and plan options (operands taken as fp32) */
int grappa_gemm_f32_plan_desc(const grappa_gemm_desc* d, int* tile_m, int* tile_n, int* nsplit, int* tail_tiles, int* tail_nsplit);
int grappa_gemm_f32(void* stream, const grappa_gemm_desc* d, void* ws, size_t ws_bytes);

/* Grouped weight gradients: n <= GRAPPA_GEMM_GROUP_MAX independent products in the wgrad layout (a_kcontig = b_kcontig = 0, fp32
 * operands, M, N > 32, one common precision other than F32_MFMA) as ONE grid + one reduction.  A weight gradient alone has 8 - 24
 * output tiles and must cut its K (= tokens) 10 - 32 ways to fill the chip, i.e. write and re-read that many partial tiles per
 * output tile; a backward pass's gradients launched together need 3 - 11 cuts each.  Results per product are those of
 * grappa_gemm_f32 up to the summation order of the K chunks (fixed, reproducible).  The workspace also carries the device copies of
 * the descriptors.  Replaces nothing in the reference (torch.autograd runs one addmm per weight); used by ops._WgradQueue. */
#define GRAPPA_GEMM_GROUP_MAX 16
size_t grappa_gemm_f32_grouped_workspace_bytes(const grappa_gemm_desc* descs, int n);
int grappa_gemm_f32_grouped(void* stream, const grappa_gemm_desc* descs, int n, void* ws, size_t ws_bytes);
/* ABI 8: up to 4 FORWARD or INPUT-GRADIENT products in ONE launch -- the same product of the four writer heads (bond / angle / proper /
 * improper), which at small batches leaves most of the chip idle when launched head by head.  All descriptors: a_kcontig = 1, one
 * b_kcontig, one precision (not F32_MFMA), operands all fp32 or all in the pair format (both operands, b_kcontig = 1), M, N > 32, fp32 C
 * (no bf16 tensors, no a_colsum), operands that allow 16-byte loads; every product keeps its own epilogue (bias, activation, dropout,
 * residual incl. res_ln_*, C2, out_amax).  No split-K.  Anything else: GRAPPA_ERR_ARG (launch the products one by one). */
size_t grappa_gemm_f32_group_workspace_bytes(const grappa_gemm_desc* descs, int n);
int grappa_gemm_f32_group(void* stream, const grappa_gemm_desc* descs, int n, void* ws, size_t ws_bytes);

/* out[n] (+)= sum_m x[m*ldx + n]   (bias gradients) */
size_t grappa_colsum_workspace_bytes(int M, int N);
int grappa_colsum_f32(void* stream, int M, int N, const float* x, int ldx, float* out, int accumulate,
                      void* ws, size_t ws_bytes);

/* dz = dy * keep(seed,idx)/(1-p) * (y ? elu'(y) : 1)   elementwise over an [M,N] view (backward of the
 * act+dropout epilogue).  y == NULL: no activation.  dz may alias dy. */
int grappa_act_dropout_bwd_f32(void* stream, int M, int N, const float* dy, int lddy, const float* y, int ldy,
                               float drop_p, uint64_t drop_seed, float* dz, int lddz, const uint64_t* drop_salt);
/* ABI 4, *_amax_f32 variants of the producers of dense-product operands: the same kernel also writes the largest magnitude of every
 * row of its output (M fp32 bit patterns, as grappa_amax_f32's row_amax) -- the scales of a following F32_F16X3 product, without a
 * pass of their own.  A NULL array gives the plain kernel. */
int grappa_act_dropout_bwd_amax_f32(void* stream, int M, int N, const float* dy, int lddy, const float* y, int ldy,
                                    float drop_p, uint64_t drop_seed, float* dz, int lddz, uint32_t* dz_amax, const uint64_t* drop_salt);
/* (drop_salt, ABI 10: see grappa_gemm_desc.drop_salt; NULL = none)
 * ---- ABI 8: batched row-wise kernels.  The writer heads run layer-locked (one autograd node per transformer layer over all heads): their
 * products go out as one grouped launch (grappa_gemm_f32_group) and their row-wise kernels as ONE launch over up to
 * GRAPPA_ROW_BATCH_MAX independent tensors.  Same arithmetic per tensor as the single-tensor entry points (fp32, row maxima written). */
#define GRAPPA_ROW_BATCH_MAX 4
typedef struct grappa_ln_fwd_item {          /* = grappa_layernorm_fwd_amax_f32's arguments; y_amax may be NULL */
    int M, W; const float* x; int ldx; const float* gamma; const float* beta; float* y; int ldy; float* mean; float* rstd; uint32_t* y_amax;
} grappa_ln_fwd_item;
int grappa_layernorm_fwd_batched_f32(void* stream, const grappa_ln_fwd_item* items, int count);
typedef struct grappa_ln_bwd_item {          /* grappa_layernorm_bwd_amax_f32 with accumulate = 2: `part` receives grappa_layernorm_bwd_partial_rows(M)
                                              * rows of [dgamma | dbeta] partials (2 W floats each) for grappa_colsum_partials_batched; dx_amax may be NULL */
    int M, W; const float* dy; int lddy; const float* x; int ldx; const float* mean; const float* rstd; const float* gamma; float* dx; int lddx;
    float* part; uint32_t* dx_amax;
} grappa_ln_bwd_item;
int grappa_layernorm_bwd_batched_f32(void* stream, const grappa_ln_bwd_item* items, int count);
typedef struct grappa_act_dropout_item {     /* = grappa_act_dropout_bwd_amax_f32's arguments (N % 4 == 0, N <= 2048, 16-byte aligned rows); y may be NULL */
    int M, N; const float* dy; int lddy; const float* y; int ldy; float drop_p; uint64_t drop_seed; float* dz; int lddz; uint32_t* dz_amax;
    const uint64_t* drop_salt;               /* ABI 10 */
} grappa_act_dropout_item;
int grappa_act_dropout_bwd_batched_f32(void* stream, const grappa_act_dropout_item* items, int count);
typedef struct grappa_seqattn_item {         /* = grappa_seqattn_fwd_amax_f32 / grappa_seqattn_bwd_amax_f32's arguments; amax may be NULL */
    int s, T, nheads, dh; const float* qkv; float* out; const float* dout; float* dqkv; uint32_t* amax;
} grappa_seqattn_item;
int grappa_seqattn_fwd_batched_f32(void* stream, const grappa_seqattn_item* items, int count);      /* uses qkv, out, amax (of out) */
int grappa_seqattn_bwd_batched_f32(void* stream, const grappa_seqattn_item* items, int count);      /* uses qkv, dout, dqkv, amax (of dqkv) */
/* ABI 8: the same rows written in the PAIR format (pairs, ldp >= 2 * N fp16 elements, % 8 == 0; N % 32 == 0, N <= 2048; dz_amax = the
 * rows' scales, required); dz (fp32) may be NULL: the products behind -- the input gradient through grappa_gemm_f32's pair operands, the
 * weight gradient through ABI 8's -- read the pairs. */
int grappa_act_dropout_bwd_pairs_f32(void* stream, int M, int N, const float* dy, int lddy, const float* y, int ldy, float drop_p,
                                     uint64_t drop_seed, float* dz, int lddz, uint32_t* dz_amax, uint16_t* pairs, int ldp, const uint64_t* drop_salt);

/* y = x + z elementwise (used to merge gradient branches); y may alias x */
int grappa_add_f32(void* stream, size_t n, const float* x, const float* z, float* y);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension (eps = 1e-5, biased variance), one wavefront per row.
 * W % 4 == 0 and W <= 2048.  Replaces torch.nn.LayerNorm in graph_attention.py:258,:265;
 * network_utils.py:38,:98. */
int grappa_layernorm_fwd_f32(void* stream, int M, int W, const float* x, int ldx, const float* gamma, const float* beta,
                             float* y, int ldy, float* mean, float* rstd);
int grappa_layernorm_fwd_amax_f32(void* stream, int M, int W, const float* x, int ldx, const float* gamma, const float* beta,
                                  float* y, int ldy, float* mean, float* rstd, uint32_t* y_amax);
/* ABI 7: the same rows ALSO written in the pair format (grappa_gemm_desc, ABI 5: the A operand of a following F32_F16X3 product, split once
 * by the kernel that holds the whole row and its maximum): pairs[M][ldp] fp16, ldp >= 2 * W, ldp % 8 == 0, 16-byte aligned; W % 32 == 0.
 * y (fp32; NULL: not written), mean, rstd (NULL: not written) as above and bit-identical to them; y_amax is required (the pairs' scales).
 * Inference: LayerNorm -> product chains without a second pass over the activation and without a split in the product. */
int grappa_layernorm_fwd_pairs_f32(void* stream, int M, int W, const float* x, int ldx, const float* gamma, const float* beta,
                                   float* y, int ldy, float* mean, float* rstd, uint32_t* y_amax, uint16_t* pairs, int ldp);
size_t grappa_layernorm_bwd_workspace_bytes(int M, int W);
/* dx may alias dy.  dgamma/dbeta: accumulate = 1 adds to the existing values, 0 overwrites.  accumulate = 2 defers them: the
 * kernel leaves its per-block partial sums at the start of `ws` -- grappa_layernorm_bwd_partial_rows(M) rows of 2 W floats,
 * [dgamma | dbeta] -- and writes neither vector; the caller keeps that `ws` alive and later hands the partials of many LayerNorms to
 * ONE launch of grappa_colsum_partials_batched (a backward pass has ~50 LayerNorms: 100 small reduction launches otherwise). */
int grappa_layernorm_bwd_partial_rows(int M);
typedef struct {
    const float* part;   /* nrows x n, row-major, contiguous */
    int nrows, n;
    float* out;          /* columns [0, n_first) (all n when out2 is NULL) */
    float* out2;         /* columns [n_first, n), or NULL */
    int n_first;
    int accumulate;      /* != 0: add to the existing values */
} grappa_colsum_item;
/* out (+)= column sums of each item's partial rows, summed in a fixed order (the same bits every run); `items` is a HOST array, any
 * count; two items of one call must not share an output */
int grappa_colsum_partials_batched(void* stream, const grappa_colsum_item* items, int count);
int grappa_layernorm_bwd_f32(void* stream, int M, int W, const float* dy, int lddy, const float* x, int ldx,
                             const float* mean, const float* rstd, const float* gamma,
                             float* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                             void* ws, size_t ws_bytes);
int grappa_layernorm_bwd_amax_f32(void* stream, int M, int W, const float* dy, int lddy, const float* x, int ldx,
                                  const float* mean, const float* rstd, const float* gamma,
                                  float* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                                  void* ws, size_t ws_bytes, uint32_t* dx_amax);
/* ABI 9: the same with the dropout backward of the tensor this LayerNorm read fused in -- the reference's layers are
 * y = LN(x) + drop(f(LN(x))) chains (perm_equiv_transformer.py:127-151), so the gradient a LayerNorm backward produces is what the dropout
 * of the layer in front masks next: dz[r][c] = keep(drop_seed, r * W + c) ? dx[r][c] / (1 - drop_p) : 0 (the mask of grappa_act_dropout_bwd_f32
 * on an [M x W] tensor) and dz's row maxima, written while the row is in registers instead of by a launch of its own.  0 < drop_p < 1;
 * dx_amax may be NULL */
int grappa_layernorm_bwd_drop_f32(void* stream, int M, int W, const float* dy, int lddy, const float* x, int ldx,
                                  const float* mean, const float* rstd, const float* gamma,
                                  float* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                                  void* ws, size_t ws_bytes, uint32_t* dx_amax,
                                  float drop_p, uint64_t drop_seed, float* dz, int lddz, uint32_t* dz_amax, const uint64_t* drop_salt);

/* ------------------------------------------------------------------------------------------------
 * Graph attention message passing (DGL DotGatConv, graph_attention.py:249/:283 -> DGL u_dot_v +
 * edge_softmax + u_mul_e/sum): for every destination v and head h
 *     alpha_uv = softmax_{u in N(v)} <ft_u,ft_v>/sqrt(D),  out_v = sum_u alpha_uv ft_u.
 * CSR by destination: indptr[N+1], indices[E] (source ids).  F = H*D floats per row, D % 4 == 0,
 * D/4 a power of two <= 64, F <= 2048.  alpha[E,H] is written for the backward pass.
 * Backward (dft = dL/dft) uses rev[E] (slot of the reverse edge; the bond graph is symmetric) and
 * delta[N,H] scratch; it gathers -- no atomics, bitwise reproducible. */
int grappa_gat_fwd_f32(void* stream, int N, int E, int H, int D, const int* indptr, const int* indices,
                       const float* ft, float* out, float* alpha);
int grappa_gat_bwd_f32(void* stream, int N, int E, int H, int D, const int* indptr, const int* indices, const int* rev,
                       const float* ft, const float* out, const float* alpha, const float* dout,
                       float* dft, float* delta /* [N,H] scratch */);
/* DGL SAGEConv 'mean' aggregation (graph_attention.py:360-363,:391):
 * out_v = sum_{u in N(v)} x_u * (scale_by_neighbor ? 1/deg(u) : 1/deg(v)).
 * forward: scale_by_neighbor = 0; backward (symmetric graph): scale_by_neighbor = 1 on d(out). */
int grappa_neighbor_mean_f32(void* stream, int N, int F, const int* indptr, const int* indices,
                             const float* x, float* out, int scale_by_neighbor);
/* ABI 5, the bf16 storage configuration of the SAGE block: bf16 rows in (8-byte aligned), out bf16 (out_f32 == 0) or fp32 (16-byte aligned) */
int grappa_neighbor_mean_bf16(void* stream, int N, int F, const int* indptr, const int* indices,
                              const uint16_t* x, void* out, int out_f32, int scale_by_neighbor);

/* ------------------------------------------------------------------------------------------------
 * Input featurisation: sinusoidal encoding of the partial charge, graph_attention.py:428-444.
 * enc[n, 2j] = sin(s f_j), enc[n, 2j+1] = cos(s f_j), s = (clamp(q,lo,hi)+hi)/(hi-lo), f_j = 1e4^(-j/(dim/2)).
 * Written into out[n*ldo + col0 ...]. */
int grappa_charge_encoding_f32(void* stream, int N, const float* q, int dim, float lo, float hi, float* out, int ldo, int col0);

/* ------------------------------------------------------------------------------------------------
 * Tuple (n-body) stage.  Token table layout everywhere: row = pos*T + t  (the reference's
 * (n_seq, n_batch, n_feats) tensors, interaction_parameters.py:173-178).
 * gather : x[pos*T+t, 0:W] = a[idx[t*s+pos], 0:W]; if pe: x[.., W-1] = pe[pos]  (RepProjector gather
 *          + positional-encoding concat, perm_equiv_transformer.py:134-141).
 * gather_bwd: da[n, 0:W] = sum over rows r in inv_rows[inv_ptr[n] : inv_ptr[n+1]] of dx[r, 0:W]
 *          (column W-1 zeroed when has_pe). */
int grappa_tuple_gather_fwd_f32(void* stream, int T, int s, int W, const float* a, int lda, const int* idx,
                                const float* pe, float* x, int ldx);
int grappa_tuple_gather_bwd_f32(void* stream, int N, int W, const int* inv_ptr, const int* inv_rows,
                                const float* dx, int lddx, float* da, int ldda, int has_pe, int accumulate);

/* nn.MultiheadAttention over the s <= 4 tokens of each tuple (network_utils.py:105,:122):
 * qkv[pos*T+t, 3F] = [q|k|v], head h = columns h*dh.. of each third; out[pos*T+t, F].
 * dh % 4 == 0, dh/4 a power of two, F = nheads*dh <= 1024. */
int grappa_seqattn_fwd_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv, float* out);
int grappa_seqattn_bwd_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv, const float* dout, float* dqkv);
/* ABI 4: the same kernels, also writing the largest magnitude of every row of out (s*T values) / of dqkv (s*T values) */
int grappa_seqattn_fwd_amax_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv, float* out, uint32_t* out_amax);
/* ABI 7: the attention output in the pair format only (inference: nothing but the out-projection product reads it): pairs[s*T][ldp],
 * F = nheads * dh <= 512, F % 32 == 0, ldp >= 2 * F; out_amax (s*T values, required) = the rows' scales; values bit-identical to
 * grappa_seqattn_fwd_amax_f32 followed by grappa_split_pairs_f32 */
int grappa_seqattn_fwd_pairs_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv, uint16_t* pairs, int ldp, uint32_t* out_amax);
int grappa_seqattn_bwd_amax_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv, const float* dout, float* dqkv,
                                uint32_t* dqkv_amax);
/* The same attention kernels reading q | k | v through a row index (the first layer of a head computed on (atom, position) table rows):
 * the q | k | v row of token (pos, t) is qkv_tab[row_idx[t*s + pos]] (row_idx: int32 (T, s), required) instead of qkv[pos*T + t]; every
 * output (out / pairs / dqkv and the row maxima) stays token-level at pos*T + t.  Same limits and the same bits as the entry points above
 * run on the gathered copy; out_amax / dqkv_amax may be NULL except for the pair format. */
int grappa_seqattn_fwd_idx_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv_tab, const int* row_idx, float* out,
                               uint32_t* out_amax);
int grappa_seqattn_fwd_pairs_idx_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv_tab, const int* row_idx, uint16_t* pairs,
                                     int ldp, uint32_t* out_amax);
int grappa_seqattn_bwd_idx_f32(void* stream, int s, int T, int nheads, int dh, const float* qkv_tab, const int* row_idx, const float* dout,
                               float* dqkv, uint32_t* dqkv_amax);
/* gather_bwd with several incident rows in flight per wavefront (each element is still summed over its list in ascending order: the bits
 * of grappa_tuple_gather_bwd_f32), optionally writing the largest magnitude of every destination row (da_amax: N fp32 bit patterns with
 * the sign cleared, as grappa_amax_f32's row maxima; the zeroed column W-1 of has_pe does not enter it; NULL: not wanted), and optionally
 * summing a second table of another width over the SAME incidence in the same launch (W2 > 0: dx2 -> da2, da2_amax; has_pe and
 * accumulate apply to both). */
int grappa_tuple_gather_bwd2_f32(void* stream, int N, const int* inv_ptr, const int* inv_rows, int has_pe, int accumulate,
                                 int W, const float* dx, int lddx, float* da, int ldda, uint32_t* da_amax,
                                 int W2, const float* dx2, int lddx2, float* da2, int ldda2, uint32_t* da2_amax);

/* Symmetriser input (perm_equiv_transformer.py:248-261): z[p*T+t, j*F+f] = x[perm[p*s+j]*T+t, f].
 * bwd: dx[i*T+t, f] = sum_p dz[p*T+t, inv_p(i)*F+f].  h_perm is a HOST array (P*s ints). */
int grappa_perm_concat_fwd_f32(void* stream, int s, int T, int F, int P, const int* h_perm, const float* x, float* z);
int grappa_perm_concat_bwd_f32(void* stream, int s, int T, int F, int P, const int* h_perm, const float* dz, float* dx);

/* Output maps (interaction_parameters.py:252-266, :347-362, :536-560; final_layer.py:52,:91-97;
 * network_utils.py:144-145).  o[P*T, ldo] is the symmetriser MLP output for all P permuted copies;
 * c = sum_p o[p*T+t, :].
 *   kind BOND : eq = std_e*(elu(mos_e + c0 - 1)+1)+min_e ; k = std_k*(elu(mos_k + c1 - 1)+1)+min_k
 *   kind ANGLE: eq = max*sigmoid(som*c0)                 ; k as above
 *   kind TORSION: gated ? k_n = c_n*sigmoid(c_{np+n})*k_std[n] : k_n = c_n*k_std[n]+k_mean[n];
 *                 k_n = |k_n| > cutoff ? k_n : 0
 * consts (device, float): BOND  [mos_e,std_e,min_e,mos_k,std_k,min_k];
 *                         ANGLE [som,max,0,mos_k,std_k,min_k];  TORSION [k_std[np] | k_mean[np]]. */
#define GRAPPA_OUT_BOND 0
#define GRAPPA_OUT_ANGLE 1
#define GRAPPA_OUT_TORSION 2
int grappa_param_out_fwd_f32(void* stream, int kind, int T, int P, int n_per, int gated, float cutoff,
                             const float* o, int ldo, const float* consts, float* k, float* eq);
int grappa_param_out_bwd_f32(void* stream, int kind, int T, int P, int n_per, int gated, float cutoff,
                             const float* o, int ldo, const float* consts, const float* dk, const float* deq,
                             float* d_o);
/* ABI 4, learnable_statistics=True (reference models/final_layer.py:21-44, :64-88; interaction_parameters.py:463-470): d_consts[i] =
 * dL/d consts[i] of the same map (6 values for bonds / angles, 2 * n_per for torsions; entries of constants that are buffers in the
 * reference -- min_, max -- are computed but meaningless).  Fixed-order two-stage sum: reproducible. */
size_t grappa_param_out_stats_workspace_bytes(int T);
int grappa_param_out_bwd_stats_f32(void* stream, int kind, int T, int P, int n_per, int gated, float cutoff, const float* o, int ldo,
                                   const float* consts, const float* dk, const float* deq, float* d_consts, void* ws, size_t ws_bytes);

/* ------------------------------------------------------------------------------------------------
 * Molecular-mechanics energy / force and its backward (models/internal_coordinates.py:15-125,:150-210;
 * models/energy.py:8-71,:99-145).  xyz[N,C,3].  Per level: idx[T,s], k (T or T*n_per), eq (T), mol_ptr[B+1].
 *   energy  : E[b,c] = sum of 1/2 k (x-eq)^2 (bonds, angles) + sum_n k_n cos(n phi) (+|k_n| if offset)
 *             per-term totals term_energy[4,B,C]; optional per-tuple energies tuple_e[l] (T_l,C).
 *   gradient: G[a,c,:] = dE/dxyz via the atom->tuple incidence (inc_ptr[N+1], inc_code = t<<4|level<<2|pos).
 *   backward: given gE[B,C] and gG[N,C,3] (either may be NULL): gk, geq per tuple (closed form of the
 *             double backward through autograd.grad(create_graph=True), energy.py:139).
 * conf_mask[B,C] (NULL = all ones) is NOT applied here; dummy conformations are handled by the loss. */
typedef struct grappa_mm_desc {
    int N, C, B;
    const float* xyz;
    int T[4];                 /* n2, n3, n4, n4_improper */
    const int* idx[4];
    const float* k[4];
    const float* eq[4];       /* [2],[3] unused */
    const int* mol_ptr[4];
    int n_per[4];             /* [0],[1] unused */
    int offset_torsion;
    const int* inc_ptr;
    const int* inc_code;
    const int* atom_molptr;   /* [B+1] */
} grappa_mm_desc;

int grappa_mm_energy_fwd_f32(void* stream, const grappa_mm_desc* d, float* energy, float* term_energy,
                             float* const tuple_e[4], float* const tuple_x[4]);
int grappa_mm_gradient_fwd_f32(void* stream, const grappa_mm_desc* d, float* grad);
int grappa_mm_bwd_f32(void* stream, const grappa_mm_desc* d, const float* gE, const float* gG,
                      float* const gk[4], float* const geq[4]);

/* ------------------------------------------------------------------------------------------------
 * Nonbonded energy and gradient (additions to ABI 11): OpenMM's NonbondedForce with NoCutoff, in Angstrom, kcal/mol and elementary
 * charges.  For every molecule b (atoms atom_molptr[b] .. atom_molptr[b+1]-1, atom_molptr[B] == N) and conformation c:
 *   E[b,c] = sum_{i<j, (i,j) no exception} 4 eps_ij ((s_ij/r)^12 - (s_ij/r)^6) + K q_i q_j / r
 *          + sum_{exceptions p=(i,j)}      4 eps_p  ((s_p /r)^12 - (s_p /r)^6) + K qq_p / r
 *   s_ij = (sigma_i + sigma_j)/2, eps_ij = sqrt(eps_i eps_j), K = 138.93545764438198 * 10 / 4.184;  G[a,c,:] = +dE/dxyz[a,c,:].
 * Atoms of different molecules never interact.  An exception REPLACES the pair's interaction; with eps_p == 0 and qq_p == 0 it is an
 * exclusion, which is not evaluated (two excluded atoms may coincide).  A non-excluded pair at zero distance gives inf / NaN.
 * The exception table is a CSR over the atoms with batch-global partner indices, ascending per atom, every exception stored on both
 * of its atoms (partners outside the atom's molecule are ignored).  The five exc_* arrays must be non-NULL (one unused element when
 * the table is empty).  term_energy[2,B,C] = the Lennard-Jones and the Coulomb part (NULL: not written); grad NULL: not written.
 * Fixed-order sums, no atomics: same input, same bits, and a molecule's results do not depend on its place in the batch.
 * No gradients with respect to charge / sigma / epsilon; no periodic box or PME (a cutoff: grappa_nonbonded_fwd_cut_f32 below).
 * GRAPPA_ERR_ARG: a NULL required pointer or a negative size; N == 0, C == 0 or B == 0: returns 0 without a launch. */
#define GRAPPA_NB_IBLOCK 64      /* i-atoms per workgroup: molecule sizes around its multiples are the kernel's edges */
typedef struct grappa_nb_desc {
    int N, C, B;
    const float* xyz;            /* [N,C,3] */
    const int*   atom_molptr;    /* [B+1] */
    const float *charge, *sigma, *epsilon;   /* [N] */
    const int*   exc_ptr;        /* [N+1]: exceptions of atom a = exc_*[exc_ptr[a] .. exc_ptr[a+1]) */
    const int*   exc_atom;       /* partner, batch-global index, ascending per atom; every exception is stored on both of its atoms */
    const float *exc_qq, *exc_sigma, *exc_eps;
} grappa_nb_desc;
int grappa_nonbonded_iblock(void);       /* GRAPPA_NB_IBLOCK of the library that is loaded */
size_t grappa_nonbonded_workspace_bytes(int N, int C, int B);
int grappa_nonbonded_fwd_f32(void* stream, const grappa_nb_desc* d, float* energy /*[B,C]*/, float* term_energy /*[2,B,C] LJ, Coulomb; may be NULL*/,
                             float* grad /*[N,C,3]; may be NULL*/, void* ws, size_t ws_bytes);
/* The same with the work-item list built on the HOST, once per (batch, C), instead of by a setup launch per call (the entry point above
 * cannot read atom_molptr, which is device memory).  grappa_nonbonded_plan reads a HOST copy of atom_molptr and writes the table as ints:
 * [n_items, n_blocks, 0, 0 | blk_ptr[B+1] padded to a multiple of 4 | 4 ints per item]; it returns the table's length in ints (table ==
 * NULL: only that), GRAPPA_ERR_ARG for C < 1, B < 1 or ranges that do not ascend inside [0, N], GRAPPA_ERR_WORKSPACE for a table that is too
 * short.  The caller copies the table to 16-byte aligned device memory and passes it with table[0] and table[1]; the pairs grid is then
 * exactly n_items and the workspace holds only the partial energies (16 * n_blocks * C bytes).  Same items, same bits as the entry point above. */
long long grappa_nonbonded_plan(int N, int C, int B, const int* atom_molptr_host, int* table, long long table_ints);
int grappa_nonbonded_fwd_planned_f32(void* stream, const grappa_nb_desc* d, const int* table_dev, int n_items, int n_blocks, float* energy,
                                     float* term_energy, float* grad, void* ws, size_t ws_bytes);

/* ------------------------------------------------------------------------------------------------
 * The same with a cutoff (additions to ABI 11): the conventions of OpenMM's NonbondedForce with CutoffNonPeriodic, stated in full.
 * With rc = cutoff, rs = switch_distance and eps = rf_dielectric, a pair that is NOT an exception contributes, for r < rc,
 *   E_lj = S(r) 4 eps_ij ((s_ij/r)^12 - (s_ij/r)^6),  S = 1 for r <= rs or rs == 0, else 1 - 10 u^3 + 15 u^4 - 6 u^5, u = (r - rs)/(rc - rs)
 *   E_c  = K q_i q_j (1/r + k_rf r^2 - c_rf),  k_rf = (eps - 1) / ((2 eps + 1) rc^3),  c_rf = 3 eps / ((2 eps + 1) rc)   (E_c(rc) = 0)
 * and the exact derivative of these, the dS/dr term included; for r >= rc nothing, by a branch: the test is r2 < rc2 with r2 the fp32
 * value the pair code forms and rc2 rounded once from (double)rc * rc (a NaN r2 is evaluated and gives a non-finite gradient, as
 * today).  EXCEPTIONS ARE NOT CUT: an exception is evaluated at any distance with the plain formulas above, without reaction field and
 * without switch; an exclusion is skipped.  term_energy[0] = the switched Lennard-Jones part, term_energy[1] = the Coulomb part with
 * the reaction-field terms.  Planned form only: table_dev, n_items, n_blocks are grappa_nonbonded_plan's (table and ws 16-byte aligned).
 * Tiles.  The work item of i-block I walks its molecule's atoms in tiles of GRAPPA_NB_IBLOCK j-atoms; tile J of a molecule is its
 * block J (counted from the molecule's first atom).  With prune == 1 an item skips the tiles that cannot hold a pair within rc:
 *   boxes  : for each (block, conformation), lo and hi = the exact fp32 minimum and maximum of the block's coordinates per axis.
 *   range  : for each block I, [e_lo, e_hi] = the first and last tile of the molecule that holds an exception partner of one of the
 *            block's atoms, taken from the first and last entry of each atom's (ascending) partner list with the partner clamped
 *            into the molecule; empty if no atom of the block has an entry.
 *   rule   : tile (I, J) of an item is evaluated iff  prune == 0,  or  e_lo(I) <= J <= e_hi(I),  or  for some conformation of the
 *            item (in the dynamics: some conformation that still runs)  NOT d2 > thr,  where
 *            d2 = ((gx * gx) + (gy * gy)) + (gz * gz),  g_axis = max(0, lo_I - hi_J, lo_J - hi_I),  every operation rounded to fp32,
 *            thr = (float)((double)rc2 * (1 + 2^-18)).  A non-finite box compares as near.
 * One launch writes boxes and ranges into the workspace, the next reads them; the decision is uniform over the workgroup.  A skipped
 * tile holds only pairs the branch above rejects (the margin 2^-18 covers the rounding of r2 and of d2: DESIGN.md section 17), so
 * prune == 0 and prune == 1 give the same bits.  tiles[k] (NULL: not written) = the tiles item k evaluated, written by its thread 0.
 * GRAPPA_ERR_ARG, nothing launched and nothing written: the cases of grappa_nonbonded_fwd_planned_f32, a NULL cut, a cutoff that is not
 * finite and > 0, a switch_distance that is neither 0 nor inside (0, cutoff), an rf_dielectric that is not finite and >= 1, a prune
 * other than 0 or 1, a table or workspace that is not 16-byte aligned.  ws_bytes below grappa_nonbonded_cut_workspace_bytes(C, n_blocks)
 * (about 56 n_blocks C bytes): GRAPPA_ERR_WORKSPACE.  3 launches.  No periodic box, no PME, no long-range Lennard-Jones correction. */
typedef struct grappa_nb_cut {
    float cutoff;           /* A, finite, > 0 */
    float switch_distance;  /* 0: none; else 0 < switch_distance < cutoff */
    float rf_dielectric;    /* finite, >= 1 (1: k_rf = 0, a shifted Coulomb) */
    int   prune;            /* 1: skip far tiles; 0: evaluate every tile -- the same bits */
} grappa_nb_cut;
size_t grappa_nonbonded_cut_workspace_bytes(int C, int n_blocks);
int grappa_nonbonded_fwd_cut_f32(void* stream, const grappa_nb_desc* d, const grappa_nb_cut* cut, const int* table_dev, int n_items,
                                 int n_blocks, float* energy, float* term_energy, float* grad, int* tiles /*[n_items] or NULL*/, void* ws,
                                 size_t ws_bytes);

/* ------------------------------------------------------------------------------------------------
 * Generalized-Born implicit solvent with a surface-area term (additions to ABI 11): GB/SA in the Onufriev-Bashford-Case form (OpenMM's
 * GBSAOBCForce), in Angstrom, kcal/mol and elementary charges, K as above.  Per atom: the charge q_i of grappa_nb_desc, a radius R_i and
 * a scale S_i.  GB knows no exceptions and no exclusions: every ordered pair i != j of a molecule counts, bonded or not (of nb only xyz,
 * charge and atom_molptr are read).  With o_i = R_i - offset, s_j = S_j o_j, r = |x_i - x_j|:
 *   I_i   = sum_{j != i} H(r, o_i, s_j);   H = 0 if o_i >= r + s_j, else with L = max(o_i, |r - s_j|), l = 1/L, u = 1/(r + s_j)
 *           H = l - u + r (u^2 - l^2)/4 + ln(u/l)/(2r) + s_j^2 (l^2 - u^2)/(4r)   [+ 2 (1/o_i - l) if o_i < s_j - r]
 *   psi_i = o_i I_i / 2;   B_i = 1 / (1/o_i - tanh(alpha psi - beta psi^2 + gamma psi^3) / R_i)          (the Born radius)
 *   E_pol = -(K/2) (1/eps_in - 1/eps_out) sum_{i,j, i = j included} q_i q_j / f_ij,   f_ij = sqrt(r^2 + B_i B_j exp(-r^2 / (4 B_i B_j)))
 *   E_sa  = sum_i 4 pi surface_tension (R_i + probe)^2 (R_i / B_i)^6
 * obc2 is (alpha, beta, gamma) = (1, 0.8, 4.85), obc1 is (0.8, 0, 2.909125).  grad = +d(E_pol + E_sa)/dxyz, exactly: the part at fixed
 * B, the chain through B_i into every r_ij of its own integral, and the chain through B_j into the same r_ij with the roles swapped.
 * dH/dr = -(l^2 - u^2)(1 + s_j^2/r^2)/4 - ln(u/l)/(2 r^2) on every branch (H is stationary in l and u where they move with r); at the
 * three branch borders, where H has a kink, one of the two one-sided values.
 * Three passes over the work items of grappa_nonbonded_plan (planned form only; table and ws 16-byte aligned), each pass a launch,
 * because a pass reads what EVERY item of the one before has written: born (I_i -> B_i and dB_i/dI_i), pair (the 1/f sums -> the
 * gradient at fixed B, dE/dB_i, both energies per block in double), chain (the two chain parts, added to the gradient by its owner);
 * then the blocks' energies are added per molecule.  4 launches, 3 with grad == NULL (no chain pass).  Fixed-order sums, no atomics,
 * one writer per word and launch: same input, same bits, and a molecule's results do not depend on its place in the batch.
 * Arithmetic: fp32; 1/x and 1/sqrt(x) are the hardware's approximations with one Newton step (half an ulp), exp and log the
 * library's 1-ulp expf and logf, tanh as (1 - e)/(1 + e) and 1 - tanh^2 as 4 e/(1 + e)^2 from ONE e = expf(-2 |.|), so that the
 * derivative keeps its relative accuracy where tanh saturates.  r = 0 between two distinct atoms or a NaN coordinate gives a
 * non-finite gradient.  term_energy[2,B,C] = E_pol, E_sa; born[N,C] = B_i; each may be NULL: not written.
 * GRAPPA_ERR_ARG, nothing launched and nothing written: a NULL required pointer (nb, nb->xyz, charge, atom_molptr, gb, radius, scale,
 * energy, table_dev, ws), negative sizes, n_blocks > N / GRAPPA_NB_IBLOCK + B, a table or workspace that is not 16-byte aligned,
 * options that are not finite, eps_in or eps_out <= 0, surface_tension < 0, probe < 0.  ws_bytes below
 * grappa_gb_obc_workspace_bytes: GRAPPA_ERR_WORKSPACE.  radius and scale are device memory, which the host cannot read: an atom with
 * radius <= offset or scale <= 0 (or either non-finite) makes every result of its molecule NaN -- the Python layer refuses such
 * parameters before anything is uploaded.  A table made for another batch is walked away from item by item, as in the calls above.
 * N == 0, C == 0 or B == 0: returns 0 without a launch.  Not here: HCT / GBn, a salt term (a cutoff with tile pruning: grappa_gb_cut
 * below). */
typedef struct grappa_gb_desc {
    const float *radius, *scale;      /* [N], device: R_i in A (> offset), S_i (> 0) */
    float offset;                     /* A; OpenMM: 0.09 */
    float alpha, beta, gamma;
    float eps_in, eps_out;            /* solute and solvent dielectric, > 0 */
    float surface_tension;            /* kcal/mol/A^2, >= 0; OpenMM's 2.25936 kJ/mol/nm^2 = 0.0054 */
    float probe;                      /* A, >= 0; 1.4 */
} grappa_gb_desc;
size_t grappa_gb_obc_workspace_bytes(int N, int C, int n_blocks);
int grappa_gb_obc_fwd_f32(void* stream, const grappa_nb_desc* nb, const grappa_gb_desc* gb, const int* table_dev, int n_items, int n_blocks,
                          float* energy /*[B,C]*/, float* term_energy /*[2,B,C] polar, SA; may be NULL*/, float* grad /*[N,C,3]; may be NULL*/,
                          float* born /*[N,C]; may be NULL*/, void* ws, size_t ws_bytes);

/* GB/SA under a cutoff (additions to ABI 11): the pairwise truncation of OpenMM's GBSAOBCForce under CutoffNonPeriodic.  The energy is
 * grappa_gb_desc's with every sum over j != i restricted to the pairs inside:
 *   I_i   = sum_{j != i, inside} H(r, o_i, s_j);   psi_i, B_i as above
 *   E_pol = -(K/2) (1/eps_in - 1/eps_out) (sum_i q_i^2 / B_i + sum_{i != j, inside} q_i q_j / f_ij)      (the terms i = j are not cut)
 *   E_sa  = sum_i 4 pi surface_tension (R_i + probe)^2 (R_i / B_i)^6                                           (not cut)
 * A pair is inside unless r2 >= rc2, with the fp32 r2 = ((dx dx + dy dy) + dz dz) of d = x_i - x_j, products and sums rounded one by
 * one in that order, and rc2 = (float)((double)cutoff * cutoff): a NaN r2 is therefore evaluated and found as a non-finite result, as
 * above.  All three passes form this one r2 (one device function), test it the same way and use it in the pair's arithmetic, so that
 * the chain rule differentiates the energy that born and pair evaluated: grad is the exact derivative of the energy above wherever no
 * pair sits at the cutoff.  Nothing is shifted or switched: the energy JUMPS by the pair's terms where a pair crosses the cutoff (its H
 * in both Born integrals and what they move, and its q_i q_j / f_ij), and the Born radii under a short cutoff differ from the
 * all-pairs ones (an integral over fewer spheres: larger radii).
 * prune: tile (i-block I, j-block J) of a work item is evaluated iff prune == 0 or, for a conformation of the item, NOT d2 > thr, with
 * d2 the squared gap of the blocks' bounding boxes as grappa_nb_cut forms it (fp32, rounded one by one) and thr = (float)(rc2 (1 +
 * 2^-18)); GB has no exceptions, so the boxes alone decide.  Every pair of a skipped tile has r2 >= rc2 (r2 has at most five roundings
 * beside the gap's), so prune = 0 and prune = 1 give the same bits -- for finite coordinates: a NaN in ONE axis
 * of a far block zeroes that axis' gap only, so its tile may still be skipped under prune = 1 where prune = 0 spreads the NaN to the
 * far rows too (the NaN's own molecule is non-finite either way; grappa_nb_cut behaves alike).  tiles[k]: the tiles item k evaluated (the
 * same in all three passes; the born pass writes it).
 * One launch writes the boxes of every (block, conformation), then the passes follow as above: 5 launches, 4 with grad == NULL.
 * GRAPPA_ERR_ARG, nothing launched and nothing written: gbcut == NULL, a cutoff that is not finite and > 0 or whose square overflows, a
 * prune other than 0 or 1, n_blocks * C > INT_MAX, and every refusal of grappa_gb_obc_fwd_f32.  ws_bytes below
 * grappa_gb_obc_cut_workspace_bytes (the words of grappa_gb_obc_workspace_bytes and behind them 32 n_blocks C bytes of boxes):
 * GRAPPA_ERR_WORKSPACE. */
typedef struct grappa_gb_cut {
    float cutoff;   /* A, finite, > 0 */
    int   prune;    /* 1: skip far tiles; 0: evaluate every tile -- the same bits */
} grappa_gb_cut;
size_t grappa_gb_obc_cut_workspace_bytes(int N, int C, int n_blocks);
int grappa_gb_obc_fwd_cut_f32(void* stream, const grappa_nb_desc* nb, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                              const int* table_dev, int n_items, int n_blocks, float* energy, float* term_energy, float* grad, float* born,
                              int* tiles /*[n_items] or NULL*/, void* ws, size_t ws_bytes);

/* ------------------------------------------------------------------------------------------------
 * Relaxation under the full MM force field (additions to ABI 11): FIRE (Bitzek et al. 2006) with unit masses and semi-implicit Euler,
 * one workgroup per (molecule b, conformation c), the whole minimisation in one launch.  E = the bonded energy of
 * grappa_mm_energy_fwd_f32 (+ the energy of grappa_nonbonded_fwd_f32 if nb != NULL; nb->xyz is ignored), g = +dE/dxyz, start = mm->xyz:
 *   x = start; v = 0; h = dt_start; a = alpha_start; npos = 0; steps = 0; g = grad E(x)
 *   loop: gmax = max_i |g_i|_2;  not finite: status 2, stop;  gmax <= tolerance: status 1, stop;  steps == max_steps: status 0, stop
 *         F = -g; P = sum F.v; Fn = |F|; vn = |v|
 *         P > 0: v = (1-a) v + a (vn/Fn) F; then, if npos >= n_min: h = min(h f_inc, dt_max), a = a f_alpha;  npos += 1
 *         else : v = 0; h = h f_dec; a = alpha_start; npos = 0
 *         v += h F; d = h v; s = min(1, max_disp / max_i |d_i|_2) (1 if that maximum is 0); x += s d; v = s v; steps += 1; g = grad E(x)
 * Outputs per item: xyz_out[N,C,3] (the coordinates held when the item stopped), energy[B,C] (total, at xyz_out), gmax[B,C] (inf for
 * status 2), steps[B,C], status[B,C]; optional (NULL: not written) grad[N,C,3] at xyz_out and term_energy[6,B,C] = bonds, angles,
 * propers, impropers, Lennard-Jones, Coulomb.  A molecule without atoms writes nothing; a single atom stops at step 0 with status 1 and
 * xyz_out bit-equal to its input.  A molecule of more than grappa_relax_max_atoms() atoms gets status 3 and NOTHING else is written for
 * it (the limit is checked by the kernel on atom_molptr, which is device memory; a caller with a host copy refuses before the launch,
 * as HipBackend.relax_fire does).  Fixed-order sums, no atomics, no communication between workgroups: same input, same bits, and an
 * item's results depend neither on its place in the batch nor on how long its neighbours run.  max_steps bounds the loop.
 * GRAPPA_ERR_ARG: a NULL required pointer or a negative size; nb disagreeing with mm in N, C or B; B * C >= 2^31; dt_start, dt_max,
 * max_disp, f_inc, f_dec or f_alpha not positive and finite; alpha_start outside [0, 1]; tolerance negative or not finite; n_min < 0;
 * max_steps < 0 or > 1,000,000.  N == 0, C == 0 or B == 0: returns 0 without a launch. */
typedef struct grappa_relax_opts {
    float tolerance;             /* kcal/mol/A, on the largest atomic gradient norm */
    int   max_steps;
    float dt_start, dt_max, max_disp;      /* max_disp: Angstrom, the largest displacement of an atom in one step */
    int   n_min;
    float f_inc, f_dec, alpha_start, f_alpha;
} grappa_relax_opts;
int grappa_relax_max_atoms(void);        /* atoms per molecule at most (>= 512) */
int grappa_relax_fire_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o, float* xyz_out,
                          float* energy, float* term_energy, float* grad, float* gmax, int* steps, int* status);

/* ------------------------------------------------------------------------------------------------
 * The same relaxation with restraints (additions to ABI 11): frozen atoms, harmonic tethers to the start coordinates and periodic
 * dihedral restraints with one target per conformation -- what a relaxed torsion scan needs (the grid points are the conformations of
 * one molecule, one workgroup each, one launch).  The loop, the options, the item and the size limit are those of grappa_relax_fire_f32,
 * word for word, on the objective E_ff + E_r with E_ff the energy above and
 *   E_r = sum_r dih_k_r (1 - cos(phi_r - dih_target_r,c)) + sum_i 0.5 pos_k_i |x_i - start_i|^2        (start = mm->xyz)
 * phi: the dihedral of grappa_mm_energy_fwd_f32 (the reference's sign convention), radians; the restraint is periodic and smooth (no
 * wrap-around case) and about 0.5 k dphi^2 near its target.  Units: dih_k kcal/mol, pos_k kcal/mol/A^2, targets rad.  The gradient the
 * loop sees is formed per atom in a fixed order: g = grad E_ff as grappa_relax_fire_f32 forms it; + dih_k_r sin(phi_r - target) dphi_r/dx
 * for the atom's restraints in ascending r; + pos_k_i (x_i - start_i); then replaced by 0 for a frozen atom before anything reads it
 * (gmax, the non-finite test, P, |F|^2, the velocity).  A frozen atom keeps the bits of its input coordinates; a molecule frozen
 * entirely stops at step 0 with status 1.
 * Outputs: xyz_out, steps, status as above; energy and term_energy are the FORCE FIELD's six terms only (what a scan plots);
 * restraint_energy[B,C] = E_r at xyz_out, thread partials added in double in thread order like the six terms; grad and gmax are those of
 * the objective; dih_phi[R,C] (NULL: not written) the restrained dihedrals at xyz_out.
 * The tables are device memory: the kernel vets an item's before it writes anything for it.  An atom index outside [0, n), a dihedral
 * whose four atoms are not distinct, a dih_k that is negative or not finite, a target of the item's conformation that is not finite, a
 * pos_k that is negative or not finite, or more than GRAPPA_RELAX_MAX_DIHEDRALS restrained dihedrals on the molecule: status 5 = the
 * item's tables are refused and NOTHING else is written for it (as for grappa_md_langevin_cons_f32).  Statuses 0 to 3 are unchanged;
 * a molecule above grappa_relax_max_atoms() gets status 3.  Same input, same bits, whatever the neighbours do.
 * r == NULL, or R == 0 with frozen == NULL and pos_k == NULL: the launch of grappa_relax_fire_f32 itself, hence its bits, and
 * restraint_energy = 0 for every molecule that has atoms and is within the size limit.
 * GRAPPA_ERR_ARG: the cases of grappa_relax_fire_f32; R < 0; a NULL dih_molptr, dih_atoms, dih_k or dih_target with R > 0; a NULL
 * restraint_energy; R * C >= 2^31. */
#define GRAPPA_RELAX_MAX_DIHEDRALS 16        /* restrained dihedrals per molecule at most */
typedef struct grappa_relax_restr {
    const int*   frozen;       /* [N] or NULL: nonzero = the atom is frozen */
    const float* pos_k;        /* [N] or NULL: kcal/mol/A^2, 0 = none; tethers the atom to its START position mm->xyz */
    const int*   dih_molptr;   /* [B+1]: the restrained dihedrals of molecule b (NULL iff R == 0) */
    const int*   dih_atoms;    /* [R,4]: atom indices WITHIN the molecule */
    const float* dih_k;        /* [R] kcal/mol */
    const float* dih_target;   /* [R,C] rad: one target per conformation */
    int R;
} grappa_relax_restr;
int grappa_relax_max_dihedrals(void);    /* 16 */
int grappa_relax_fire_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                                const grappa_relax_restr* r, float* xyz_out, float* energy, float* term_energy, float* grad, float* gmax,
                                int* steps, int* status, float* restraint_energy /*[B,C]*/, float* dih_phi /*[R,C] or NULL*/);

/* ------------------------------------------------------------------------------------------------
 * The same relaxation for molecules of ANY size, stepwise (additions to ABI 11): the loop, the energy, the options and the outputs are
 * those of grappa_relax_fire_f32 above, but a molecule spans many workgroups, the minimiser's state lives in a caller-owned workspace
 * and a step is a fixed sequence of four launches.  The decomposition is grappa_nonbonded_plan's (a work item = molecule, block of at
 * most GRAPPA_NB_IBLOCK i-atoms, nc conformations): the caller passes that table (device memory, 16-byte aligned) with table[0] =
 * n_items and table[1] = n_blocks to all three calls, also when nb == NULL (the plan is about atoms, not about parameters).
 *   init   : x = mm->xyz, v = 0, h = dt_start, a = alpha_start, npos = 0, steps = 0; n_running_dev[0] = the number of (molecule,
 *            conformation) items with at least one atom; g = grad E(x) and the block partials of P, |F|^2, |v|^2, max |g_i|.  2 launches.
 *   run    : enqueues exactly n_steps iterations of the loop, 4 launches each and nothing else: no sync, no allocation, safe to capture.
 *            decide (one workgroup per item: adds the block partials in ascending block order in double, takes the stop tests and FIRE's
 *            decisions, writes the item's scalars; the thread that stops an item subtracts 1 from n_running_dev[0]), vel (v and the
 *            blocks' largest |h v_i|), move (the maximum over the item's blocks, x += s h v, v = s v), force (g and the partials at the
 *            new x in ONE launch: the bonded gather and the Lennard-Jones / Coulomb pair loop).  The host reads n_running_dev[0]
 *            whenever it likes -- typically once per chunk of steps -- and stops enqueueing when it is 0.
 *   finish : applies the stop tests once more (an item still running ends with status 0), then writes xyz_out, energy, gmax, steps,
 *            status and the optional grad and term_energy[6,B,C] as grappa_relax_fire_f32 defines them.  The six terms come from the
 *            kernels of grappa_mm_energy_fwd_f32 and grappa_nonbonded_fwd_planned_f32 at xyz_out: the same bits as those entry points
 *            give there; energy is their sum, added in double in term order.  A workspace that was finished is not run again.
 * Hazards.  Workgroups of one molecule exchange data only across launch boundaries: partials are written by one launch and read by
 * the next, and the per-item scalars (h, a, npos, steps, status, the step's mixing factors) have ONE writer, the decide launch, which no
 * other launch overlaps.  No cooperative launch, no flag that is waited on, no float atomics; the only atomic is the integer count.
 * Every launch leaves an item whose status is final alone before touching its x, v, g or state: the outputs do not depend on how many
 * steps were enqueued after an item stopped, nor on n_steps per call.  A non-finite gradient stops an item at once with status 2,
 * gmax = inf and the coordinates it held.  A molecule without atoms writes nothing; a single atom stops at step 0 with status 1 and
 * xyz_out bit-equal to its input.  Fixed-order sums: same input, same bits, and a molecule's bits do not depend on its place in the batch
 * (they differ from grappa_relax_fire_f32's, which adds in another order).  With max_steps == 0 (init, finish) xyz_out is the input
 * bit for bit with energy, grad and gmax at it.
 * Limits.  N * C * 3, n_blocks * C and B * C below 2^31 and n_blocks <= N / GRAPPA_NB_IBLOCK + B, GRAPPA_ERR_ARG otherwise; the other
 * GRAPPA_ERR_ARG cases are those of grappa_relax_fire_f32, plus a NULL table_dev, ws or n_running_dev, a table or workspace that is not 16-byte
 * aligned, a negative n_items or n_blocks and n_steps < 1.  ws_bytes below grappa_relax_steps_workspace_bytes(N, C, B, n_blocks): GRAPPA_ERR_WORKSPACE, nothing launched.
 * N == 0, C == 0 or B == 0: returns 0 without a launch.  The workspace holds about 36 N C + 68 B C + 52 n_blocks C bytes. */
size_t grappa_relax_steps_workspace_bytes(int N, int C, int B, int n_blocks);
int grappa_relax_steps_init_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                                const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int* n_running_dev);
int grappa_relax_steps_run_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                               const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int n_steps, int* n_running_dev);
int grappa_relax_steps_finish_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_relax_opts* o,
                                  const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* energy,
                                  float* term_energy, float* grad, float* gmax, int* steps, int* status);
/* The stepwise minimiser under a nonbonded cutoff (additions to ABI 11): the three calls above with `const grappa_nb_cut* cut` after nb.
 * cut == NULL forwards to the call above, with its launches and its bits; cut != NULL needs nb (else GRAPPA_ERR_ARG) and bad options in
 * cut are GRAPPA_ERR_ARG, nothing launched and nothing written.  The conventions are grappa_nb_cut's, stated there: the nonbonded force
 * is that of grappa_nonbonded_fwd_cut_f32 (same formulas, same skip rule; a conformation that has stopped is not looked at by the rule),
 * and the loop minimises that energy.  A step stays FOUR launches: the move launch's work item writes the box of its own (block,
 * conformations) after moving -- it is the box's only writer, and a stopped conformation keeps its box as it keeps its x -- and the force
 * launch reads all boxes across the launch boundary.  init gains one launch (boxes and ranges at the start coordinates): 3.  finish's
 * terms 4 and 5 come from the kernels of grappa_nonbonded_fwd_cut_f32 at xyz_out: its bits there.  Pass the same cut to all three
 * calls.  The workspace is grappa_relax_steps_cut_workspace_bytes(N, C, B, n_blocks): the one above plus about 88 n_blocks C; ws_bytes
 * below it is GRAPPA_ERR_WORKSPACE, nothing launched. */
size_t grappa_relax_steps_cut_workspace_bytes(int N, int C, int B, int n_blocks);
int grappa_relax_steps_init_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                    const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes,
                                    int* n_running_dev);
int grappa_relax_steps_run_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                   const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes,
                                   int n_steps, int* n_running_dev);
int grappa_relax_steps_finish_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                      const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws,
                                      size_t ws_bytes, float* xyz_out, float* energy, float* term_energy, float* grad, float* gmax,
                                      int* steps, int* status);
/* The stepwise minimiser in GB/SA implicit solvent (additions to ABI 11): the three _cut_ calls with `const grappa_gb_desc* gb` after
 * cut, and `float* esolv` at the end of finish.  gb == NULL: each forwards to the call above (the _cut_ one if cut != NULL, else the plain
 * one) -- its launches, its bits.  With gb the minimised energy is the one above plus E_pol + E_sa of grappa_gb_obc_fwd_f32 (nb is
 * required: it carries the charges; its exceptions do not touch the solvent term), cut must be NULL (GB under a cutoff is not
 * implemented) and the force launch is followed by the three passes of that entry under the stopped-conformation mask:
 *   step   : decide, vel, move, force (as they are), born, pair, chain -- the chain launch's epilogue adds the three gradients in the order
 *            (bonded + nonbonded) + fixed-B part + chain parts, writes g and rewrites the block's partials of P, |F|^2, |v|^2 and
 *            max |g_i| from the sum and the unchanged v, by the arithmetic of the force launch's epilogue.  7 launches per step; init
 *            gains the same three: 5.  decide stays the only writer of the per-item state: a non-finite sum ends the item with status 2
 *            as a non-finite force gradient does.  The decide, vel, move and force kernels are the ones a call without solvent launches.
 *   finish : the sequence above (decide, the six terms, the copy kernel), grappa_gb_obc_fwd_f32 at xyz_out in a workspace region of
 *            its own, and one small launch: energy = the eight terms (six as before, E_pol, E_sa) added in double in that order, esolv
 *            [B,C] (NULL: not written) = E_pol + E_sa alone, and term_energy, if given, is [8,B,C] with E_pol and E_sa in rows 6 and 7
 *            (the entry's bits).  grad is the total gradient.  9 launches (5 without solvent).
 * The workspace is grappa_relax_steps_gb_workspace_bytes(N, C, B, n_blocks): the words of a call without solvent first (the plain
 * layout, unchanged), behind them B, dBdI, w [N,C], the fixed-B gradient [N,C,3], [3,B,C] energies and the workspace of
 * grappa_gb_obc_fwd_f32, each piece on a 256-byte boundary; ws_bytes below it is GRAPPA_ERR_WORKSPACE, nothing launched.
 * GRAPPA_ERR_ARG before anything else is looked at, nothing launched and nothing written: cut != NULL together with gb, nb == NULL or
 * without charges, NULL radius or scale, options grappa_gb_obc_fwd_f32 refuses.  r = 0 between two distinct atoms (bonded or not: GB
 * has no exclusions) gives status 2; a radius <= offset or a scale <= 0 makes its molecule's gradient NaN: status 2.  Not here: the fused
 * minimiser, restraints (the stepwise DYNAMICS take them: grappa_md_steps_*_restr_f32), a cutoff, the HCT / GBn models, a salt term. */
size_t grappa_relax_steps_gb_workspace_bytes(int N, int C, int B, int n_blocks);
int grappa_relax_steps_init_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                   const grappa_gb_desc* gb, const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks,
                                   void* ws, size_t ws_bytes, int* n_running_dev);
int grappa_relax_steps_run_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                  const grappa_gb_desc* gb, const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks,
                                  void* ws, size_t ws_bytes, int n_steps, int* n_running_dev);
int grappa_relax_steps_finish_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                     const grappa_gb_desc* gb, const grappa_relax_opts* o, const int* table_dev, int n_items, int n_blocks,
                                     void* ws, size_t ws_bytes, float* xyz_out, float* energy, float* term_energy, float* grad, float* gmax,
                                     int* steps, int* status, float* esolv);

/* ------------------------------------------------------------------------------------------------
 * Langevin molecular dynamics under the full MM force field (additions to ABI 11): BAOAB (Leimkuhler and Matthews 2013; on-step
 * velocities, one force evaluation per step), one workgroup per (molecule b, conformation c), n_steps steps in one launch.  The energy,
 * the gradient g = +dE/dxyz, the descriptors and the size limit are those of grappa_relax_fire_f32 (start = mm->xyz, nb->xyz ignored, nb
 * == NULL: bonded terms only).  Units: Angstrom, kcal/mol, amu, ps, K; ACC = 418.4 (1 kcal/mol = 418.4 amu A^2 / ps^2), kB = 0.0019872041
 * kcal/mol/K.  mass[N] in amu; w_i = 1 / m_i, and a mass that is not positive makes a FROZEN atom (OpenMM's convention for mass 0): w_i =
 * 0, its coordinates come back bit for bit and its velocity is 0, whatever vel_in holds for it.
 *   c1 = exp(-friction dt); c2 = sqrt(1 - c1^2); s_i = sqrt(ACC kB temperature w_i); g = grad E(x)
 *   v = vel_in, or, if vel_in == NULL, v_i = sqrt(ACC kB init_temperature w_i) z(first_step, purpose 1) (0 for init_temperature == 0)
 *   repeat n_steps times, t = first_step + k, k = 0, 1, ..:
 *       g not finite: status 2, stop with the x and v held and steps = k
 *       v -= (dt/2) ACC w_i g;  x += (dt/2) v
 *       if friction > 0: v = c1 v + c2 s_i z(t, purpose 0)
 *       x += (dt/2) v;  g = grad E(x);  v -= (dt/2) ACC w_i g
 *       if save_every > 0 and (k + 1) % save_every == 0: write frame (k + 1) / save_every - 1
 *   g not finite: status 2 (the gradient that closes the last step is tested too; with n_steps == 0 the one at the start)
 * With friction == 0 this is velocity Verlet and no random number is drawn.  dt/2, (dt/2) ACC, c1, c2, ACC kB temperature and ACC kB
 * init_temperature are formed in double on the host and rounded once.  A gradient is "not finite" by the test of grappa_relax_fire_f32.
 * The step that found it has been completed with it (frozen atoms excepted, its velocities are then not finite either), and a frame
 * that fell on that step has been written; no later frame is.
 * Random numbers have no state: z(t, purpose) of atom i (its index WITHIN the molecule) and conformation c is a function of
 * (mol_key[b], i, c, t, purpose) alone.  Philox4x32-10 (Salmon et al. 2011, Random123's constants) with key = (low, high half of
 * mol_key[b]) and counter = (i, c, t, purpose) gives w0..w3; with u(w) = ((w >> 8) + 0.5) 2^-24, r(w) = sqrt(-2 ln u(w)) and
 * a(w) = 2 pi (w >> 8) 2^-24:  z = (r(w0) cos a(w1), r(w0) sin a(w1), r(w2) cos a(w3)).  u is never 0; the logarithm is taken of an
 * argument fp32 holds exactly (u below 1/2, 1 - u through log1p above).  A molecule's trajectory therefore depends on its key, not on
 * its place in the batch, and a run of a + b steps gives the same bits of x, v and frames as a run of a steps (a a multiple of
 * save_every) followed by one of b steps with mm->xyz = xyz_out, vel_in = vel_out and first_step + a: the gradient recomputed at the
 * start is the one that was held.  first_step + n_steps must stay below 2^32.
 * Outputs per item: xyz_out, vel_out [N,C,3]; epot[B,C] (total potential energy at xyz_out: thread partials in fp32, added in double in
 * a fixed order, the code path of grappa_relax_fire_f32's energy); ekin[B,C] = 0.5 / ACC sum m_i v_i^2, added the same way; steps[B,C];
 * status[B,C]: 0 = ran n_steps steps, 2 = non-finite gradient, 3 = more than grappa_relax_max_atoms() atoms and NOTHING else written.
 * Optional (NULL: not written): frames_xyz[F,N,C,3] with F = n_steps / save_every, each frame in the layout of mm->xyz;
 * frames_epot[F,B,C] and frames_ekin[F,B,C], the bits epot and ekin of a run that ended there would have.  The potential energy is
 * computed at frames and at the end only.  A molecule without atoms writes nothing.  n_steps == 0 returns the input bit for bit (the
 * velocities of frozen atoms zeroed) with epot and ekin at it.  No atomics, no communication between workgroups: same input, same bits,
 * and an item's bits depend neither on its place in the batch nor on its neighbours.
 * GRAPPA_ERR_ARG, nothing written: a NULL required pointer or a negative size; nb disagreeing with mm in N, C or B; B * C >= 2^31; dt not
 * positive and finite; temperature, friction or init_temperature negative or not finite; n_steps < 0 or > 1,000,000; save_every < 0;
 * first_step + n_steps >= 2^32.  N == 0, C == 0 or B == 0: returns 0 without a launch.  Cutoffs and periodic boxes are
 * not supported; X-H bond constraints are grappa_md_langevin_cons_f32's below; molecules above the limit go through grappa_md_steps_*_f32.
 * grappa_md_philox: the generator itself on the host (no device, no launch).  grappa_md_noise_f32: one small launch that writes
 * out[N,C,3] = z(step, purpose) of every (atom, conformation) exactly as grappa_md_langevin_f32 draws it (atom_molptr[B+1] and
 * mol_key[B] are device memory; N * C < 2^31). */
typedef struct grappa_md_opts {
    float dt;                    /* ps */
    float temperature;           /* K, of the thermostat */
    float friction;              /* 1/ps; 0: no thermostat (velocity Verlet) */
    float init_temperature;      /* K, of the start velocities when vel_in == NULL */
    int   n_steps, save_every;   /* save_every == 0: no frames */
    unsigned first_step;         /* the global index of this call's first step: the random stream's position */
} grappa_md_opts;
int grappa_md_langevin_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                           const float* mass /*[N]*/, const unsigned long long* mol_key /*[B]*/, const float* vel_in /*[N,C,3] or NULL*/,
                           float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps, int* status,
                           float* frames_xyz, float* frames_epot, float* frames_ekin);
void grappa_md_philox(unsigned long long key, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned out[4]);
int grappa_md_noise_f32(void* stream, const unsigned long long* mol_key, const int* atom_molptr, int N, int C, int B, unsigned step,
                        unsigned purpose, float* out /*[N,C,3]*/);

/* ------------------------------------------------------------------------------------------------
 * The same dynamics with X-H bond constraints (additions to ABI 11): g-BAOAB (Leimkuhler and Matthews 2016) with one geodesic
 * sub-step.  Everything that grappa_md_langevin_f32 states holds (units, frozen atoms, c1, c2, s_i, z and its counters -- the noise an
 * atom draws does not depend on whether it is constrained --, the outputs, the frames, the size limit), except the loop.
 * Constraints come as STAR CLUSTERS: a centre atom 0 and L leaves 1..L, 1 <= L <= GRAPPA_MD_CONS_MAX_LEAVES = 4, with one length d_k > 0
 * per leaf (X-H, XH2, XH3, XH4).  Every atom belongs to at most one cluster, so a molecule has at most 256 clusters.  cluster_molptr[B+1]:
 * the clusters of molecule b; cluster_atoms[K,5]: the centre, then the leaves, as atom indices WITHIN the molecule, -1 = no leaf;
 * cluster_d[K,4] in Angstrom.  h2 = dt/2, hk = (dt/2) ACC.  A leaf with w_0 + w_k == 0 (both ends frozen) is treated as absent.
 *   P(x, v), the velocity projection, direct:  r_k = x_k - x_0;  solve sum_l A_kl mu_l = r_k . (v_k - v_0) with
 *       A_kl = w_0 (r_k . r_l) + delta_kl w_k (r_k . r_k);  v_k -= w_k mu_k r_k;  v_0 += w_0 sum_l mu_l r_l.
 *   S(xref, x, v), the position constraint, cluster-wise Newton on the multipliers (M-SHAKE), on vectors relative to the centre:
 *       rref_k = xref_k - xref_0;  rt_k = x_k - x_0;  lambda = 0;  repeat:
 *           r_k = rt_k - w_k lambda_k rref_k - w_0 sum_l lambda_l rref_l;  sigma_k = r_k . r_k - d_k^2
 *           converged when every |sigma_k| <= 2 tolerance d_k^2 (a sigma that is not finite: not converged)
 *           else lambda -= J^-1 sigma with J_kl = -2 r_k . (delta_kl w_k rref_k + w_0 rref_l),
 *       at most GRAPPA_MD_CONS_MAX_ITER = 8 updates.  Then x_0 += w_0 sum_l lambda_l rref_l;  x_k = x_0 (new) + r_k;
 *       v_k -= w_k lambda_k rref_k / h2;  v_0 += w_0 sum_l lambda_l rref_l / h2 (a frozen atom is not touched).  Without convergence
 *       the same updates are made with the last lambda, if it is finite, and the item's constraint-failure flag is set.
 *   start:  if constrain_start: S(x, x, -) (the velocities are set afterwards);  v = vel_in or drawn;  P
 *           else: x and vel_in are taken as they are (a continued run); drawn velocities are projected in either case
 *           g = grad E(x)
 *   repeat n_steps times:
 *           g not finite or the flag set: stop
 *           v -= hk w g;  P
 *           xr = x;  x += h2 v;  S(xr, x, v);  P
 *           if friction > 0: v = c1 v + c2 s z(t, purpose 0);  P
 *           xr = x;  x += h2 v;  S(xr, x, v);  P
 *           g = grad E(x);  v -= hk w g;  P
 *           frame if due
 * An atom in no cluster moves exactly as in grappa_md_langevin_f32.  The potential energy is unchanged: the constrained bonds' terms are
 * still evaluated.  The flag is reduced with the non-finite-gradient flag at the next force evaluation, so the step that found either
 * has been completed with it and its frame, if due, written.  status 4 = a position constraint did not converge (it wins over 2): the
 * state is the one held after that step, and steps = the steps completed BEFORE it (0 when the start's S failed) -- the steps whose
 * constraints held; status 2 counts as in grappa_md_langevin_f32.  status 5 = the item's tables are refused and NOTHING else is written
 * for it: the tables are device memory, so the kernel checks, before it writes anything, that a cluster's indices lie in [0, n) and are
 * distinct, that it has at least one leaf, that no atom is in two clusters, that every used d is finite and positive and that the
 * molecule has at most 256 clusters.  NOT checked: a cluster that its frozen atoms over-determine (a moving centre with four frozen
 * leaves: the projection's system is singular) is unsupported; its item ends with status 2 or 4.  grappa_amd's front ends refuse it.
 * A run of a + b steps gives the bits of a run of a steps followed by one of b steps with constrain_start = 0, mm->xyz = xyz_out,
 * vel_in = vel_out and first_step + a.  Same input, same bits; an item's bits depend neither on its place nor on its neighbours.
 * GRAPPA_ERR_ARG: the cases of grappa_md_langevin_f32, plus K < 0, a NULL table with K > 0, and a tolerance that is not finite, below
 * 2^-20 or above 2^-7.  cons == NULL or K == 0: the launch of grappa_md_langevin_f32 itself, hence its bits.  Constraints other than
 * these stars (rigid water, SETTLE) are not supported.  Molecules above the size limit, and a nonbonded cutoff, go through
 * grappa_md_steps_*_cons_f32 below. */
#define GRAPPA_MD_CONS_MAX_LEAVES 4
#define GRAPPA_MD_CONS_MAX_ITER 8
typedef struct grappa_md_cons {
    const int*   cluster_molptr;   /* [B+1] device: clusters of molecule b */
    const int*   cluster_atoms;    /* [K,5] device: centre, leaves; atom index WITHIN the molecule; -1 = no leaf */
    const float* cluster_d;        /* [K,4] device: A */
    int   K;
    float tolerance;               /* relative, on d: converged when |r^2 - d^2| <= 2 tol d^2 */
    int   constrain_start;         /* 1: constrain the input first; 0: a continued run */
} grappa_md_cons;
int grappa_md_cons_max_leaves(void);   /* 4 */
int grappa_md_cons_max_iter(void);     /* 8 */
int grappa_md_langevin_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                                const grappa_md_cons* cons, const float* mass /*[N]*/, const unsigned long long* mol_key /*[B]*/,
                                const float* vel_in /*[N,C,3] or NULL*/, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps,
                                int* status, float* frames_xyz, float* frames_epot, float* frames_ekin);

/* ------------------------------------------------------------------------------------------------
 * The same dynamics for molecules of ANY size, stepwise (additions to ABI 11): the loop, the units, the frozen-atom rule, the random
 * stream, the options and the outputs are, word for word, those of grappa_md_langevin_f32 above, but a molecule spans many workgroups,
 * the integrator's state lives in a caller-owned workspace and a step is a fixed sequence of TWO launches, whatever the shape.  The
 * decomposition is grappa_nonbonded_plan's, exactly as grappa_relax_steps_*_f32 use it: the caller passes that table (device memory,
 * 16-byte aligned) with n_items and n_blocks to all three calls, also when nb == NULL; a table made for another batch is walked away
 * from, not followed.  opts is the run's: opts->n_steps its total number of steps, opts->save_every its frame period, opts->first_step
 * the global index of its first step; pass the same opts to all three calls.
 *   init   : x = mm->xyz; v = vel_in with frozen atoms zeroed, or, if vel_in == NULL, the draw at init_temperature (purpose 1 at
 *            first_step); every (molecule, conformation) with atoms is running, steps = 0; g = grad E(x) with the blocks' flags of a
 *            non-finite gradient and kinetic partials at it.  2 launches.
 *   run    : enqueues the steps step0 .. step0 + n_steps - 1 of the run (the noise of step k is z(first_step + step0 + k, purpose 0)), 2
 *            launches each and nothing else: no sync, no allocation, safe to capture.  The caller advances step0.
 *            move  (a thread per (atom, conformation); every workgroup of a molecule ORs the flags of all the molecule's blocks and
 *                  leaves a flagged conformation untouched, otherwise v -= (dt/2) ACC w g; x += (dt/2) v; the thermostat; x += (dt/2) v
 *                  on its atoms of positive mass.  The workgroup of the molecule's first block writes the item's status and steps.)
 *            force (g at the new x in ONE launch: the bonded gather and the Lennard-Jones / Coulomb pair loop of the stepwise
 *                  minimiser, slices added in slice order; then per atom the closing kick v -= (dt/2) ACC w g and the non-finite test, per
 *                  (block, conformation) the flag and sum m v^2 over the block's atoms in ascending order in double, and on a frame step
 *                  the frame's coordinates.  It leaves an item alone whose status, written by the move launch before it, is final.)
 *            Frames: this call's frame pointers address the frames step0 / save_every .. (each NULL or the slice for this call's
 *            frames, in the layouts of grappa_md_langevin_f32); step0 must be a multiple of save_every when one is given.  Only on a
 *            frame step, and only if frames_epot or frames_ekin is given, the energy launches are added: without frames a call adds
 *            exactly 2 n_steps launches.
 *   finish : takes the stop decision once more (the gradient that closed the last step), then writes xyz_out, vel_out, epot, ekin, steps
 *            and status as grappa_md_langevin_f32 defines them: steps = the steps completed, status 0 or 2; status 3 does not occur.
 * Energies.  epot and frames_epot come from the kernels of grappa_mm_energy_fwd_f32 and grappa_nonbonded_fwd_planned_f32 at the
 * coordinates held: the six terms those entry points give there, added in double in term order -- the arrangement and the bits of
 * grappa_relax_steps_finish_f32's energy.  ekin and frames_ekin are 0.5 / ACC times the blocks' partials, added in ascending block
 * order in double.  frames_*[f] are the bits xyz_out, epot and ekin of a run that ended at that step would have.
 * Stopping.  A non-finite gradient (the test of grappa_relax_fire_f32) stops an item with status 2, the x and v it held and steps =
 * the steps completed, the one that found it included; a frame that fell on that step has been written, no later one is; steps
 * enqueued after an item stopped do not touch it.
 * Hazards.  Workgroups of one molecule exchange data only across launch boundaries, every word has one writer per launch, and no
 * workgroup reads in a launch what a sibling writes in it: move reads the flags and writes status, force reads status and writes the
 * flags.  No cooperative launch, no flag that is waited on, no atomics.
 * Bits.  Same input, same bits.  A molecule's bits depend on its key and its own input, not on its place in the batch nor on its
 * neighbours, and not on how the steps are dealt out to run calls.  They differ from grappa_md_langevin_f32's, which adds in another
 * order.  A run of a + b steps equals a run of a steps (a a multiple of save_every) followed by init / run / finish of b steps from
 * its outputs with first_step + a.  n_steps == 0 (init, finish): the input back bit for bit (the velocities of frozen atoms zeroed)
 * with epot and ekin at it.  A molecule without atoms writes nothing.
 * GRAPPA_ERR_ARG, nothing launched and nothing written: the cases of grappa_md_langevin_f32 (a NULL required pointer -- mass and mol_key
 * for init and run, the six outputs for finish --, bad options, nb disagreeing with mm) and of grappa_relax_steps_*_f32 (a NULL
 * table_dev or ws, a table or workspace that is not 16-byte aligned, a negative n_items or n_blocks, n_blocks > N / GRAPPA_NB_IBLOCK + B;
 * N * C * 3, n_blocks * C or B * C at or above 2^31); on run also n_steps < 1, step0 < 0, step0 + n_steps > opts->n_steps and a step0
 * that is no multiple of save_every with a frame pointer given.  first_step + opts->n_steps must stay below 2^32.  ws_bytes below
 * grappa_md_steps_workspace_bytes(N, C, B, n_blocks): GRAPPA_ERR_WORKSPACE, nothing launched.  N == 0, C == 0 or B == 0: returns 0
 * without a launch.  The workspace holds about 36 N C + 40 B C + 28 n_blocks C bytes. */
size_t grappa_md_steps_workspace_bytes(int N, int C, int B, int n_blocks);
int grappa_md_steps_init_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                             const float* mass /*[N]*/, const unsigned long long* mol_key /*[B]*/, const float* vel_in /*[N,C,3] or NULL*/,
                             const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes);
int grappa_md_steps_run_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                            const float* mass, const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks, void* ws,
                            size_t ws_bytes, int step0, int n_steps, float* frames_xyz, float* frames_epot, float* frames_ekin);
int grappa_md_steps_finish_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_md_opts* o,
                               const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* vel_out,
                               float* epot, float* ekin, int* steps, int* status);
/* The stepwise dynamics under a nonbonded cutoff (additions to ABI 11): the three calls above with `const grappa_nb_cut* cut` after nb.
 * cut == NULL forwards to the call above, with its launches and its bits; cut != NULL needs nb (else GRAPPA_ERR_ARG) and bad options in
 * cut are GRAPPA_ERR_ARG, nothing launched and nothing written.  The force is then that of grappa_nonbonded_fwd_cut_f32 (same formulas,
 * same skip rule; a conformation that has stopped is not looked at by the rule).  A step stays TWO launches: the move launch's work item
 * writes the box of its own (block, conformations) after moving -- it is the box's only writer, and a stopped conformation keeps its box
 * as it keeps its x -- and the force launch reads all boxes across the launch boundary.  init gains one launch (boxes and ranges): 3.
 * epot and frames_epot come from the kernels of grappa_nonbonded_fwd_cut_f32 at the held coordinates: its bits there.  Pass the same cut
 * to all three calls.  The workspace is grappa_md_steps_cut_workspace_bytes(N, C, B, n_blocks): the one above plus about 88 n_blocks C. */
size_t grappa_md_steps_cut_workspace_bytes(int N, int C, int B, int n_blocks);
int grappa_md_steps_init_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                 const grappa_md_opts* o, const float* mass, const unsigned long long* mol_key, const float* vel_in,
                                 const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes);
int grappa_md_steps_run_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                const grappa_md_opts* o, const float* mass, const unsigned long long* mol_key, const int* table_dev,
                                int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps, float* frames_xyz,
                                float* frames_epot, float* frames_ekin);
int grappa_md_steps_finish_cut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                   const grappa_md_opts* o, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes,
                                   float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps, int* status);
/* The stepwise dynamics with X-H bond constraints (additions to ABI 11): the `_cut_` calls above with `const grappa_md_cons* cons` after
 * the options; cut may be NULL (all pairs).  cons == NULL or K == 0 forwards to the `_cut_` call (which forwards to the plain one for
 * cut == NULL): its launches, its bits.  Otherwise the loop is, word for word, the one stated at grappa_md_langevin_cons_f32 -- the star
 * clusters, P, S with at most GRAPPA_MD_CONS_MAX_ITER updates, the tolerance range, constrain_start (read by init alone), the noise
 * counters, the frozen-atom rules, status 4 with steps = the steps completed before the failing one (0 when the start's S failed), status
 * 5, the frame rule -- for molecules of ANY size and any number of clusters: "at most 256 clusters" does not apply, "an atom is in at most
 * one cluster" does.  Pass the same cut and cons tables to all three calls.
 *   decomposition : a cluster is integrated, all its atoms together, by the thread that its CENTRE has in the work item of the centre's
 *            block; its leaves may lie in any block of the molecule, so no order is asked of the table.  A clustered atom is skipped by
 *            its ordinary owner in the integration; a free atom moves exactly as in grappa_md_steps_run_f32.
 *   run    : a step is THREE launches, FOUR under a cutoff, whatever the shape, and nothing else without frames:
 *            move  (clusters: v -= hk w g, P | A S P | O P | A S P; free atoms as above; the flags' OR, status and steps as above, where
 *                  a set constraint flag gives status 4 and takes back the count of the failing step -- the first block's workgroup is the
 *                  only writer of both words; per (block, conformation) the constraint-failure word of the block's own clusters, fresh
 *                  each launch)
 *            boxes (only with cut: a block's atoms may have been moved by a sibling, so the boxes need the launch boundary)
 *            force (as above, with the closing kick of EVERY atom by its owner; the block's flag word also takes the block's
 *                  constraint-failure word, so the flags stay the one array that move reads, and stay sticky)
 *            close (clusters: the closing P; per (block, conformation) the kinetic partial, here the sum in double over the block's atoms
 *                  in ascending order where a free atom gives m v^2, a centre the sum over its cluster's moving atoms -- the centre, then
 *                  its leaves in table order -- and a leaf nothing.  ekin stays the ascending-block sum.)
 *   init   : the launches of the `_cut_` init plus the table vet (3: claim words cleared, written, read back), the start's S and P (1,
 *            unless constrain_start == 0 with vel_in given), and the kinetic partials (1): 6 or 7 launches, one more under a cutoff.
 *   tables : vetted on the device during init: per cluster the checks of grappa_md_langevin_cons_f32; "no atom in two clusters" through
 *            one claim word per atom in the workspace: a launch has every cluster store its index to its atoms' words with plain stores,
 *            the next has it read them back, and of two clusters that hold one atom at least one sees the other.  A refused item gets
 *            status 5 and nothing else: its xyz_out, vel_out, epot, ekin, steps and frames are untouched; its neighbours run.
 *   finish : as above; the stop decision taken once more includes the constraint flag (status 4 with the failing step taken back), so
 *            the failure flag survives any number of run calls: it lives in the workspace.
 * Hazards: the rule above holds launch by launch: every word has one writer per launch and no workgroup reads in a launch what a sibling
 * writes in it.  Bits: same input, same bits; they depend neither on the item's place or neighbours, nor on how steps are dealt to run
 * calls, nor on where frames fall; they differ from the fused kernel's.  The continuation rule is grappa_md_langevin_cons_f32's
 * (constrain_start = 0, first_step + a).  GRAPPA_ERR_ARG, nothing launched: the cases of the `_cut_` calls, plus K < 0, a NULL table with
 * K > 0 and a tolerance that is not finite, below 2^-20 or above 2^-7.  The workspace is
 * grappa_md_steps_cons_workspace_bytes(N, C, B, n_blocks, K, with_cut): that of the call forwarded to for K == 0, else 4 N + 4 n_blocks C
 * bytes more; below it: GRAPPA_ERR_WORKSPACE, nothing launched. */
size_t grappa_md_steps_cons_workspace_bytes(int N, int C, int B, int n_blocks, int K, int with_cut);
int grappa_md_steps_init_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                  const grappa_md_opts* o, const grappa_md_cons* cons, const float* mass, const unsigned long long* mol_key,
                                  const float* vel_in, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes);
int grappa_md_steps_run_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                 const grappa_md_opts* o, const grappa_md_cons* cons, const float* mass, const unsigned long long* mol_key,
                                 const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps,
                                 float* frames_xyz, float* frames_epot, float* frames_ekin);
int grappa_md_steps_finish_cons_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                    const grappa_md_opts* o, const grappa_md_cons* cons, const int* table_dev, int n_items, int n_blocks,
                                    void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps,
                                    int* status);

/* The stepwise dynamics in GB/SA implicit solvent (additions to ABI 11): the _cons_ calls with `const grappa_gb_desc* gb` after cons.
 * gb == NULL: each forwards to its _cons_ call -- the launches and the bits of a run without solvent.  With gb the potential is the one
 * above plus E_pol + E_sa of grappa_gb_obc_fwd_f32 (nb is required: it carries the charges; its exceptions do not touch the solvent
 * term) and the force launch is followed by the three passes of that entry under the stopped-conformation mask:
 *   step : move, force (as it is, without its closing kick), born, pair, chain -- the chain launch's epilogue adds the three gradients in
 *          the order (bonded + nonbonded) + fixed-B part + chain parts, gives the closing kick, and tests the sum: a non-finite sum ends
 *          the item with status 2 as a non-finite force gradient does.  5 launches, 6 with constraints (close follows); init gains 3.
 *          The force kernels are the ones a run without solvent launches: nothing of them was changed for the solvent.
 * epot includes the solvent term: the eight terms (six as before, E_pol, E_sa) added in double in that order, each from the library's
 * own energy entry at the held coordinates; esolv [B,C] / frames_esolv [F,B,C] (NULL: not written) = E_pol + E_sa alone, written where
 * epot is.  The workspace is grappa_md_steps_gb_workspace_bytes (the words of a run without solvent first, the solvent's behind them).
 * GRAPPA_ERR_ARG before anything else is looked at: cut != NULL together with gb (GB under a cutoff is not implemented), nb == NULL,
 * NULL radius or scale, options grappa_gb_obc_fwd_f32 refuses.  r = 0 between two distinct atoms (bonded or not: GB has no exclusions)
 * gives status 2.  Not here: the fused dynamics, the fused minimiser (restraints: grappa_md_steps_*_restr_f32 below). */
size_t grappa_md_steps_gb_workspace_bytes(int N, int C, int B, int n_blocks, int K);
int grappa_md_steps_init_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const float* mass,
                                const unsigned long long* mol_key, const float* vel_in, const int* table_dev, int n_items, int n_blocks,
                                void* ws, size_t ws_bytes);
int grappa_md_steps_run_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                               const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const float* mass,
                               const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes,
                               int step0, int n_steps, float* frames_xyz, float* frames_epot, float* frames_ekin, float* frames_esolv);
int grappa_md_steps_finish_gb_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                  const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const int* table_dev,
                                  int n_items, int n_blocks, void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot,
                                  float* ekin, int* steps, int* status, float* esolv);

/* The stepwise dynamics with the solvent under ITS cutoff (additions to ABI 11): the _gb_ calls with `const grappa_gb_cut* gbcut`
 * directly after gb.  gbcut == NULL: each forwards to its _gb_ call -- its launches, its bits, its refusals, that of cut together with
 * gb included.  With gbcut, gb is required, the solvent term is the truncated energy of grappa_gb_cut (born, pair and chain are the
 * cut instantiations of the bodies grappa_gb_obc_fwd_cut_f32 launches, under the stopped-conformation mask), and cut, the NONBONDED
 * cutoff, may be given too: the force launch is then what it is under a nonbonded cutoff without solvent, else what it is without one
 * -- untouched either way.  A reaction field already screens; OpenMM runs GB with the reaction-field dielectric 1, so a grappa_nb_cut
 * with rf_dielectric = 1 is the usual companion (the caller's choice: nothing is overridden).
 * ONE set of boxes serves both cutoffs, written once per step by the launch that writes them under a nonbonded cutoff: the move
 * launch, or with constraints the box launch behind the constrained move; in init the box launch in front of the force.
 *   step : move (with the boxes), force, born, pair, chain: 5 launches as above; with constraints move, boxes, force, born, pair,
 *          chain, close: 7 (the box launch is the one a nonbonded cutoff adds to a constrained step; giving cut as well adds nothing
 *          more).  init gains the box launch.
 * epot and esolv: the solvent's terms come from grappa_gb_obc_fwd_cut_f32 itself at the held coordinates, in a workspace region of its
 * own; with cut the six others from grappa_nonbonded_fwd_cut_f32 as in the _cut_ calls.  No second energy path.
 * The truncated energy jumps where a pair crosses the solvent's cutoff, so a run under it does not conserve energy (DESIGN.md section
 * 22 gives the size of a jump).  The workspace is grappa_md_steps_gbcut_workspace_bytes (it holds the boxes and the region of
 * grappa_nonbonded_fwd_cut_f32 whether cut is given or not); ws_bytes below what the call needs: GRAPPA_ERR_WORKSPACE.
 * GRAPPA_ERR_ARG before anything else is looked at: gbcut without gb, a cutoff or prune grappa_gb_obc_fwd_cut_f32 refuses, options of
 * cut that grappa_md_steps_*_cut_f32 refuses, and every refusal of the _gb_ calls but that of cut. */
size_t grappa_md_steps_gbcut_workspace_bytes(int N, int C, int B, int n_blocks, int K);
int grappa_md_steps_init_gbcut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                   const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                   const float* mass, const unsigned long long* mol_key, const float* vel_in, const int* table_dev, int n_items,
                                   int n_blocks, void* ws, size_t ws_bytes);
int grappa_md_steps_run_gbcut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                  const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                  const float* mass, const unsigned long long* mol_key, const int* table_dev, int n_items, int n_blocks,
                                  void* ws, size_t ws_bytes, int step0, int n_steps, float* frames_xyz, float* frames_epot,
                                  float* frames_ekin, float* frames_esolv);
int grappa_md_steps_finish_gbcut_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                     const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                     const grappa_gb_cut* gbcut, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes,
                                     float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps, int* status, float* esolv);

/* The stepwise dynamics with restraints (additions to ABI 11): the _gbcut_ calls with `const grappa_md_restr* r` directly after gbcut.
 * cut, cons, gb and gbcut are each optional under the _gbcut_ family's own rules (gbcut == NULL: the rules of the _gb_ calls, gb == NULL:
 * those of the _cons_ calls, and so on down).  The integrator sees the gradient of E_ff (+ solvent) + E_r,
 *   E_r(b,c) = sum_r dih_k_r (1 - cos(phi_r - dih_target_{r,c})) + sum_i 0.5 pos_k_i |x_{i,c} - ref_{i,c}|^2,
 * the restraint energy of grappa_relax_fire_restr_f32 with an explicit reference; phi is the library's dihedral.  Per (atom,
 * conformation) the gradient is formed in a fixed order: the force field's, exactly as the force launch forms it; + dih_k_r sin(phi_r -
 * target) dphi_r/dx_i for the molecule's rows that name the atom, in ascending r; + pos_k_i (x_i - ref_i).  It is added in the force
 * launch's epilogue, before g is written, before the closing kick and before the non-finite test, so every launch behind it (the
 * solvent's chain, the constrained close, the next move) reads it: a step gains no launch.  Same input, same bits; no atomics; an item's
 * bits do not depend on its place in the batch.
 *   ref    : pos_ref [N,C,3], or NULL: mm->xyz as init receives it.  init copies it into the workspace; run and finish read that copy.
 *            A run continued with first_step must pass the ORIGINAL reference: with NULL the tethers move to the start of the
 *            continuing call.  There is no `frozen`: a mass of 0 freezes an atom.
 *   vet    : one launch of init, per (molecule, conformation): atom indices in [0, n) and the four of a row distinct, dih_k finite and
 *            >= 0, the conformation's targets finite, pos_k finite and >= 0, at most GRAPPA_RELAX_MAX_DIHEDRALS rows on the molecule,
 *            dih_molptr monotone and within [0, R].  A refused item gets status 5 (constraint or restraint tables refused) and never
 *            runs: its xyz_out, vel_out, epot, ekin, steps, erestr, dih_phi and frames are untouched, its neighbours run.  A NaN target
 *            refuses its conformation only.  A non-finite pos_ref under a positive pos_k has no check of its own: it makes the gradient
 *            non-finite, which is status 2 by the force launch's own test.
 *   energy : epot / frames_epot stay the force field's (plus the solvent's).  erestr [B,C] (required) and dih_phi [R,C] (NULL: not
 *            written) = E_r and the restrained dihedrals at xyz_out; frames_erestr [F,B,C] and frames_phi [F,R,C] (NULL: not written)
 *            the same on frame steps, for running items.  One workgroup per (molecule, conformation): the tethers in double (thread t
 *            the atoms t, t + 256, .. ascending, the 256 rows added in order), then the dihedral rows in ascending r.
 * r == NULL, or R == 0 with pos_k == NULL, is the _gbcut_ call itself: its launches, its bits, its refusals; erestr is then written as
 * 0 for molecules that have atoms and the frames' restraint outputs are not written.  GRAPPA_ERR_ARG, nothing launched and nothing
 * written: R < 0, a NULL dih_* table with R > 0, pos_ref without pos_k, a NULL erestr (finish), R * C >= 2^31.  The workspace is
 * grappa_md_steps_restr_workspace_bytes(N, C, B, n_blocks, K, with_cut, with_gb, with_gbcut): the layout of the call without
 * restraints, unchanged, and the reference behind it.  Not here: restraints in the fused dynamics, anything in the minimisers, distance,
 * angle or flat-bottomed restraints, more than GRAPPA_RELAX_MAX_DIHEDRALS dihedrals per molecule, time-dependent targets. */
typedef struct grappa_md_restr {
    const float* pos_k;      /* [N] or NULL */
    const float* pos_ref;    /* [N,C,3] or NULL: mm->xyz as init receives it */
    const int*   dih_molptr; /* [B+1], NULL iff R == 0 */
    const int*   dih_atoms;  /* [R,4] within the molecule */
    const float* dih_k;      /* [R] */
    const float* dih_target; /* [R,C] */
    int R;
} grappa_md_restr;
size_t grappa_md_steps_restr_workspace_bytes(int N, int C, int B, int n_blocks, int K, int with_cut, int with_gb, int with_gbcut);
int grappa_md_steps_init_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                   const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                   const grappa_md_restr* r, const float* mass, const unsigned long long* mol_key, const float* vel_in,
                                   const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes);
int grappa_md_steps_run_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                  const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                                  const grappa_md_restr* r, const float* mass, const unsigned long long* mol_key, const int* table_dev,
                                  int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps, float* frames_xyz,
                                  float* frames_epot, float* frames_ekin, float* frames_esolv, float* frames_erestr, float* frames_phi);
int grappa_md_steps_finish_restr_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                                     const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb,
                                     const grappa_gb_cut* gbcut, const grappa_md_restr* r, const int* table_dev, int n_items, int n_blocks,
                                     void* ws, size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps,
                                     int* status, float* esolv, float* erestr, float* dih_phi);

/* Temperature ladders and replica exchange on the stepwise dynamics (additions to ABI 11): the _restr_ calls with
 * `const grappa_md_remd* x` directly after r; cut, cons, gb, gbcut and r are each optional under the _restr_ family's own rules.
 *   ladder : temperatures[C], fp32 in kelvin, in device memory.  Slot s has kt_s = (float)(ACC kB (double)T_s): the expression of the
 *            scalar temperature, the same bits.
 *   replica: every (molecule b, conformation c) is a replica.  It keeps its coordinates, its noise stream (keyed by c, as ever) and its
 *            index c for the whole run; what moves is the SLOT it holds.  The workspace keeps per item slot[b,c], its inverse
 *            who[b,s], kt_item[b,c] and scale[b,c].  Each molecule of a batch has its own ladder state over the same temperatures.
 *            Start: slot[b,c] = c, or slots_in[B,C], which must be a permutation of 0 .. C-1 per molecule.
 *   vet    : one launch of init, per molecule: every temperature finite and >= 0 (with exchanges: > 0), the molecule's slots_in row a
 *            permutation.  A refused molecule's items get status 5 and never run; their outputs are untouched, their neighbours run.
 *   O step : reads kt_item[b,c] in place of ACC kB temperature; c1, c2, the noise and B, A, O, A are what they were.  o->temperature
 *            must still be valid and is otherwise unused.
 *   start  : with vel_in == NULL the velocities are drawn at the replica's slot temperature if init_at_ladder != 0, at the scalar
 *            o->init_temperature otherwise.
 *   attempt: with exchange_every = K > 0, behind the step whose global index g = first_step + step0 + s + 1 is a multiple of K, after
 *            that step's own frame outputs.  The attempt's number is a = g / K; its pairs are the slots (s, s + 1) with s = a (mod 2),
 *            0 <= s <= C - 2.  K == 0: a ladder without exchanges.
 *   energy : with lo = who[b,s], hi = who[b,s+1]: U = (double)epot + (double)erestr, the fp32 values a frame at this step reports (the
 *            force field plus the solvent; E_r, 0 without restraints), by the launches a frame uses, into workspace scratch -- or the
 *            frame's own rows where the frame of the same step asked for them: nothing is evaluated twice.
 *   decision: beta = 1 / (kB (double)T); D = (beta_s - beta_{s+1}) (U_lo - U_hi); u = ((double)w0 + 0.5) 2^-32 with w0 word 0 of
 *            Philox4x32-10(key = mol_key[b], counter = (s, 0, g, 2)) -- purpose 2, which no other draw uses; accepted iff D >= 0 or
 *            u < exp(D), all in double.  A pair is not attempted if either replica no longer runs (its status, or a flag that the
 *            step's launches set on one of its blocks) or either U is not finite.
 *   swap   : on acceptance the two replicas swap slot, who and kt_item, and the velocities of each are multiplied by
 *            f = (float)sqrt((double)T_new / (double)T_old).  x and g are untouched: no force is recomputed.  The kinetic partials of
 *            the replica's blocks are multiplied by (double)f * f, so an ekin reported before the next step agrees with
 *            sum m v^2 / 2 within rounding, NOT bit for bit.
 *   logs   : exch_slot, exch_epot, exch_erestr [X,B,C], each NULL: not written; X = the attempts of the call, row i belongs to attempt
 *            (first_step + step0) / K + 1 + i, and with a log (first_step + step0) % K != 0 is GRAPPA_ERR_ARG of THAT run call (it
 *            launches and writes nothing; init has run by then, as with a step0 off the period of save_every).  Without logs a run
 *            call may begin anywhere.  exch_slot holds the
 *            slots after the attempt, the energies are those the decision read (NaN for a replica that no longer runs; a refused
 *            item's rows are untouched).
 *   finish : slots_out [B,C] (required): the slot every item holds, for molecules with atoms but refused items.
 * Launches: init gains one (the vet); a step gains none; a step with an attempt gains the energy launches a frame with epot (and E_r)
 * at that step makes, unless that frame is written anyway, plus two (exchange, rescale); finish gains one (slots_out).
 * Same input, same bits; no atomics; every word has one writer per launch (the pairs of an attempt are disjoint); a replica's bits
 * depend neither on the batch around its molecule nor on how the steps are dealt out to run calls.
 * x == NULL is the _restr_ call itself: its launches, its bits, its refusals; slots_out is then written as c.  GRAPPA_ERR_ARG, nothing
 * launched and nothing written: NULL temperatures, exchange_every < 0, exchange_every > 0 with friction == 0 (exchanges need a
 * thermostat), a NULL slots_out (finish), every refusal of the _restr_ calls; of the run call alone, the log boundary above.  The
 * workspace is grappa_md_remd_workspace_bytes: the
 * layout of the call without a ladder, unchanged, and the ladder's words behind it.  Not here: Hamiltonian exchange between umbrella
 * windows, the fused dynamics, coordinate exchange, non-neighbour pairs, per-replica friction or dt, annealing schedules. */
typedef struct grappa_md_remd {
    const float* temperatures;   /* [C] device */
    const int*   slots_in;       /* [B,C] device or NULL */
    int exchange_every;          /* 0: ladder only */
    int init_at_ladder;
} grappa_md_remd;
size_t grappa_md_remd_workspace_bytes(int N, int C, int B, int n_blocks, int K, int with_cut, int with_gb, int with_gbcut, int with_restr);
int grappa_md_remd_init_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                            const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                            const grappa_md_restr* r, const grappa_md_remd* x, const float* mass, const unsigned long long* mol_key,
                            const float* vel_in, const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes);
int grappa_md_remd_run_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                           const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                           const grappa_md_restr* r, const grappa_md_remd* x, const float* mass, const unsigned long long* mol_key,
                           const int* table_dev, int n_items, int n_blocks, void* ws, size_t ws_bytes, int step0, int n_steps,
                           float* frames_xyz, float* frames_epot, float* frames_ekin, float* frames_esolv, float* frames_erestr,
                           float* frames_phi, int* exch_slot, float* exch_epot, float* exch_erestr);
int grappa_md_remd_finish_f32(void* stream, const grappa_mm_desc* mm, const grappa_nb_desc* nb, const grappa_nb_cut* cut,
                              const grappa_md_opts* o, const grappa_md_cons* cons, const grappa_gb_desc* gb, const grappa_gb_cut* gbcut,
                              const grappa_md_restr* r, const grappa_md_remd* x, const int* table_dev, int n_items, int n_blocks, void* ws,
                              size_t ws_bytes, float* xyz_out, float* vel_out, float* epot, float* ekin, int* steps, int* status,
                              float* esolv, float* erestr, float* dih_phi, int* slots_out);

/* ------------------------------------------------------------------------------------------------
 * MolwiseLoss (training/loss.py:45-167 with utils/graph_utils.py:35-86), one workgroup per molecule:
 *  l_m = wE*mean_c((E-<E>)-(Eref-<Eref>))^2 + wG*mean_{a,c,xyz}(G-Gref)^2   over real conformations
 *  loss_mol[b] = l_m ; gE = d(sum_m l_m * inv_B)/dE ; gG likewise.  is_dummy may be NULL. */
int grappa_loss_ef_fwd_bwd_f32(void* stream, int B, int C, int N, const int* atom_molptr,
                               const float* energy, const float* energy_ref, const float* is_dummy,
                               const float* grad, const float* grad_ref, float wE, float wG, float inv_B,
                               float* loss_mol, float* gE, float* gG);
/* parameter MSE vs classical parameters (NaN references masked) + L2 on torsion k, per molecule:
 *  loss_mol[b] += pw[b] * sum_levels fac_l^2 sum (p-pref)^2 / (#entries) + reg terms; d/dp written to gp[l]
 *  (every entry of gp[l] is overwritten).  levels: 0 n2_k, 1 n2_eq, 2 n3_k, 3 n3_eq, 4 n4_k, 5 n4_improper_k.
 *  ref[l] may be NULL (level skipped in the MSE); width[l] = columns; ref_width[l] = columns of ref. */
typedef struct grappa_ploss_desc {
    int B;
    const int* mol_ptr[6];
    const float* p[6];
    const float* ref[6];
    int width[6];
    int ref_width[6];
    float fac[6];
    float reg[6];             /* L2 prefactor per level (only [4],[5] non-zero in the reference) */
    const float* pw;          /* [B] parameter weight per molecule, or NULL = no MSE term */
    float inv_B;
} grappa_ploss_desc;
int grappa_loss_param_fwd_bwd_f32(void* stream, const grappa_ploss_desc* d, float* loss_mol, float* const gp[6]);

/* Device-side collate (replaces the per-batch host work of data/GraphDataLoader.py:23-73 collate_fn,
 * utils/dgl_utils.py:11-60 batch and :132-171 set_number_confs for a dataset that is resident in HBM).
 * A table is an array of 4-byte elements (int32 / float32; an int64 column counts as two) with `width` elements per row.
 * Workgroup (j, t) copies the rows of batch slot j of table t:
 *   rows  dst_row[j] .. dst_row[j+1]-1 of dst   <-   rows src_row[j] .. of src          (all arrays are DEVICE pointers)
 * and transforms them according to `mode`:
 *   COPY      verbatim (features, charges, reference parameters)
 *   ADD       int32 + p0[j]                       (CSR columns / tuple indices + atom offset, reverse-edge slots + edge offset)
 *   INV_ROWS  local token row pos*p0[j] + t  ->  pos*c0 + p1[j] + t     (p0 = tuples of the molecule, p1 = tuple offset of the
 *             slot, c0 = tuples of the batch at this level; width 1)
 *   INC_CODE  packed incidence code (tuple << 4 | level << 2 | pos) + (p0[4*j + level] << 4)
 *   CONF      conformation selection: a source row holds (p0[j], width) values, a batch row (c0, width);
 *             dst[row][c][e] = src[src_row[j] + (row*p0[j] + p1[j*c0 + c])*width + e]  -- src_row[j] is an ELEMENT offset here;
 *             p1 = selected conformation per (slot, output conformation): sub-sampling and dummy padding alike. */
#define GRAPPA_COLLATE_COPY 0
#define GRAPPA_COLLATE_ADD 1
#define GRAPPA_COLLATE_INV_ROWS 2
#define GRAPPA_COLLATE_INC_CODE 3
#define GRAPPA_COLLATE_CONF 4
typedef struct grappa_collate_desc {
    const int32_t* src;
    int32_t* dst;
    const int64_t* src_row;   /* [B] */
    const int64_t* dst_row;   /* [B+1] */
    const int32_t* p0;
    const int32_t* p1;
    int64_t c0;
    int32_t width;
    int32_t mode;
} grappa_collate_desc;
/* descs_device: the n_tables descriptors in device memory (read by the kernel); descs_host: the same array in host memory
 * (validated before the launch).  One launch, grid (B, n_tables). */
int grappa_collate_batch(void* stream, const grappa_collate_desc* descs_device, const grappa_collate_desc* descs_host, int n_tables, int B);

/* FastEvaluator.step (training/evaluation.py:53-113; get_energies / get_gradients utils/graph_utils.py:35-86), one workgroup
 * per molecule instead of dgl.unbatch + a Python loop:  out[b*4 + {0,1,2,3}] = { sum over real conformations of the squared
 * difference of the per-molecule-centred energies, number of real conformations, sum over atoms x real conformations x xyz of
 * (G - G_ref)^2, atoms x real conformations }.  grad / grad_ref may both be NULL (FastEvaluator(gradients=False)). */
int grappa_eval_se_f32(void* stream, int B, int C, int N, const int* atom_molptr, const float* energy, const float* energy_ref,
                       const float* is_dummy, const float* grad, const float* grad_ref, float* out);

/* The bootstrapped Evaluator (training/evaluation.py:164-386: step :207-261, collect :264-311, pool :314-355, get_metrics :358-386)
 * on per-molecule moments.  Every metric of get_metrics is a function of a few sums over the molecules of a (resampled) dataset, so a
 * bootstrap replicate gathers and adds rows instead of torch.cat over thousands of per-molecule tensors.  (Additions to ABI 11.)
 *
 * grappa_eval_moments_f32 replaces Evaluator.step's unbatch + per-molecule slicing: same inputs as grappa_eval_se_f32, one workgroup per
 * molecule, fp32 inputs, every operation from the first subtraction on in double, fixed-order sums without atomics (same input, same
 * bits).  out[b][GRAPPA_EVAL_NMOM] (16-byte aligned; a row is 80 bytes), over the REAL conformations of molecule b:
 *   0 n_E       real conformations                         5 n_V        atoms x real conformations (3-vectors)
 *   1 sum d^2   d = centred prediction - centred reference  6 sum |dg|^2  dg = G - G_ref of one atom and conformation
 *   2 sum |d|                                              7 sum |dg|
 *   3 sum r     r = centred reference energy                8 sum g       all components of G_ref
 *   4 sum r^2                                              9 sum g^2
 * (energies centred per molecule over its real conformations, utils/graph_utils.py:35-63).  grad == grad_ref == NULL: columns 5..9 are 0. */
#define GRAPPA_EVAL_NMOM 10
/* metrics per dataset, in get_metrics' order (:368-377): std_energies (unbiased std of r), std_gradients (unbiased std of all components
 * of G_ref, x sqrt 3), rmse_energies, mae_energies, rmse_gradients = sqrt(sum |dg|^2 / n_V), crmse_gradients = sqrt(sum |dg|^2 / 3 n_V),
 * mae_gradients = sum |dg| / n_V.  A zero count gives NaN, as torch's mean / std of an empty tensor.  The two stds come from raw moments
 * (sum, sum of squares): their relative error is that of a double sum times (1 + mean^2 / variance) -- centred energies have mean 0, and
 * the components of forces average to zero over a molecule at rest. */
#define GRAPPA_EVAL_NMETRICS 7
int grappa_eval_moments_f32(void* stream, int B, int C, int N, const int* atom_molptr, const float* energy, const float* energy_ref,
                            const float* is_dummy, const float* grad, const float* grad_ref, double* out);
/* grappa_eval_bootstrap_f64 replaces collect(bootstrap_seed) + get_metrics per replicate and pool's mean / np.std over the replicates
 * (:320-351).  mom[M][GRAPPA_EVAL_NMOM]: the moment rows grouped by dataset, dataset d = rows ds_ptr[d] .. ds_ptr[d+1]-1 (ds_ptr[n_ds+1],
 * DEVICE memory).  The call covers the replicates rep0 <= r < rep1 of n_rep; idx[rep1-rep0][M] (int32, DEVICE memory) holds THEIR
 * resamples: replicate rep0 + i of dataset d sums the rows ds_ptr[d] + idx[i][ds_ptr[d] + j], j < ds_ptr[d+1] - ds_ptr[d], in a fixed
 * order (one workgroup per (dataset, replicate), no atomics) and writes rep_metrics[rep0 + i][d][GRAPPA_EVAL_NMETRICS].  The call whose
 * range ends at n_rep adds a second launch: mean[d][..] and std[d][..] (population std, np.std) of every metric over all n_rep
 * replicates, which earlier calls on the same stream must have written.  At most 65535 replicates per call.
 * GRAPPA_ERR_ARG: a NULL pointer, M < 1, n_ds < 1, n_rep < 1, an empty or misplaced range.  ds_ptr and idx live in device memory, which
 * the entry point cannot read: an index outside [0, rows of its dataset) is CLAMPED into the dataset by the kernel, and ds_ptr into
 * [0, M]; the front end (grappa_amd.backend.HipBackend.eval_bootstrap) refuses host-side index tables that are out of range. */
int grappa_eval_bootstrap_f64(void* stream, const double* mom, int M, int n_ds, const int* ds_ptr, const int* idx, int n_rep, int rep0,
                              int rep1, double* rep_metrics, double* mean, double* stdev);

/* ------------------------------------------------------------------------------------------------
 * Optimiser (training/lightning_model.py:297-299 Adam; lightning_trainer.py:92 gradient_clip_val=10):
 * sumsq: out[0] (+)= sum x^2.  adam: p -= lr * mhat/(sqrt(vhat)+eps) with g scaled by
 * clip = min(1, max_norm/(sqrt(*sumsq)+1e-6)) when sumsq != NULL; grad_scale multiplies g first. */
size_t grappa_sumsq_workspace_bytes(size_t n);
int grappa_sumsq_f32(void* stream, size_t n, const float* x, float* out, int accumulate, void* ws, size_t ws_bytes);
int grappa_adam_step_f32(void* stream, size_t n, float* p, const float* g, float* m, float* v,
                         float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         float grad_scale, const float* sumsq, float max_norm);
/* ABI 8, for a train step captured in a hipGraph: the same update with the learning rate (lr_dev[0]) and the step count (step_dev[0] >= 1,
 * for the bias corrections) read from DEVICE memory at execution time. */
int grappa_adam_step_dyn_f32(void* stream, size_t n, float* p, const float* g, float* m, float* v, const float* lr_dev, float beta1, float beta2,
                             float eps, float weight_decay, const int* step_dev, float grad_scale, const float* sumsq, float max_norm);
/* ------------------------------------------------------------------------------------------------
 * bf16 storage configuration (BASELINE configs[2]: "bf16, MFMA dense heads"; the reference's Lightning `precision` / its
 * torch.set_float32_matmul_precision('medium'), training/trainrun.py:3): activations and activation gradients are kept as bf16
 * in HBM (uint16_t bit patterns, round to nearest even on every store), half the bytes of every HBM-bound kernel; statistics,
 * softmax, accumulation, parameters, parameter gradients, energies and forces stay fp32.  Same semantics and argument meaning
 * as the *_f32 entry points above; rows 8-byte aligned.  The dense products take precision GRAPPA_GEMM_BF16 with a_planes /
 * b_planes = 1 and *_nplanes = 1 (grappa_gemm_desc): one plane = the bf16 tensor itself. */
int grappa_layernorm_fwd_bf16(void* stream, int M, int W, const uint16_t* x, int ldx, const float* gamma, const float* beta,
                              uint16_t* y, int ldy, float* mean, float* rstd);
int grappa_layernorm_bwd_bf16(void* stream, int M, int W, const uint16_t* dy, int lddy, const uint16_t* x, int ldx,
                              const float* mean, const float* rstd, const float* gamma, uint16_t* dx, int lddx,
                              float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes);
int grappa_act_dropout_bwd_bf16(void* stream, int M, int N, const uint16_t* dy, int lddy, const uint16_t* y, int ldy,
                                float drop_p, uint64_t drop_seed, uint16_t* dz, int lddz, const uint64_t* drop_salt);
int grappa_gat_fwd_bf16(void* stream, int N, int E, int H, int D, const int* indptr, const int* indices,
                        const uint16_t* ft, uint16_t* out, float* alpha);
int grappa_gat_bwd_bf16(void* stream, int N, int E, int H, int D, const int* indptr, const int* indices, const int* rev,
                        const uint16_t* ft, const uint16_t* out, const float* alpha, const uint16_t* dout,
                        uint16_t* dft, float* delta);
int grappa_tuple_gather_fwd_bf16(void* stream, int T, int s, int W, const uint16_t* a, int lda, const int* idx,
                                 const float* pe, uint16_t* x, int ldx);
int grappa_tuple_gather_bwd_bf16(void* stream, int N, int W, const int* inv_ptr, const int* inv_rows,
                                 const uint16_t* dx, int lddx, uint16_t* da, int ldda, int has_pe, int accumulate);
int grappa_seqattn_fwd_bf16(void* stream, int s, int T, int nheads, int dh, const uint16_t* qkv, uint16_t* out);
int grappa_seqattn_bwd_bf16(void* stream, int s, int T, int nheads, int dh, const uint16_t* qkv, const uint16_t* dout, uint16_t* dqkv);
int grappa_perm_concat_fwd_bf16(void* stream, int s, int T, int F, int P, const int* h_perm, const uint16_t* x, uint16_t* z);
int grappa_perm_concat_bwd_bf16(void* stream, int s, int T, int F, int P, const int* h_perm, const uint16_t* dz, uint16_t* dx);
/* element-type conversion of a [M,N] view (round to nearest even), for the few places where the two configurations meet */
int grappa_convert_f32_to_bf16(void* stream, int M, int N, const float* x, int ldx, uint16_t* y, int ldy);
int grappa_convert_bf16_to_f32(void* stream, int M, int N, const uint16_t* x, int ldx, float* y, int ldy);

/* ------------------------------------------------------------------------------------------------
 * ABI 11: the FUSED writer-head layer (SURVEY section 8(b) "grappa_writer_head_fwd/bwd"): one kernel per transformer layer of a writer head,
 * one workgroup per tile of 64 token rows (= every token of 32 / 21 / 16 tuples), the 512-wide activations resident in LDS:
 *     x1 = LN(x; n1);  qkv = x1 W_in^T + b_in;  a = multi-head attention over the s tokens of each tuple (nheads x 64, softmax over the s keys);
 *     x2 = drop(a W_o^T + b_o; seed1) + x1;  x3 = LN(x2; nf);  u = ELU(x3 W_1^T + b_1);  out = drop(u W_2^T + b_2; seed2) + x3
 * Replaces: models/network_utils.py:112-133 (DottedAttWithMLP.forward) with :44-54 (FeedForwardLayer.forward), one layer of the stack of
 * models/perm_equiv_transformer.py:121-151; nn.MultiheadAttention's in_proj / out_proj as in grappa_gemm_f32 above.
 * Token rows as everywhere: row = pos * T + t, tensors contiguous with F = 512 columns (qkv: 1536).  Dropout as grappa_gemm_f32 (element index
 * row * 512 + column).  dtype GRAPPA_WRITER_BF16: x, out and the saved activations are bf16 (the bf16 storage configuration), products on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation, LayerNorm / softmax / ELU in fp32; every stored tensor is rounded exactly where the
 * unfused kernels round it.  Weights travel PACKED in MFMA fragment order (grappa_writer_pack_weight, once per optimiser step).
 * save_* (all or none; training): the tensors the backward pass reads -- x1, qkv, att, x2, x3, u and the statistics of both LayerNorms -- are
 * written as by-products.  Supported: F = 512, nheads = 8, s = 2, 3, 4; anything else GRAPPA_ERR_ARG (the caller runs the unfused sequence). */
#define GRAPPA_WRITER_BF16 1
typedef struct grappa_writer_layer_desc {
    int s, T, F, nheads, dtype;
    const void* x;                                        /* (s*T, F) */
    void* out;                                            /* (s*T, F) */
    const void *w_in_pk, *w_o_pk, *w1_pk, *w2_pk;         /* packed (3F x F), (F x F), (F x F), (F x F) */
    const float *b_in, *b_o, *b1, *b2;                    /* 3F, F, F, F */
    const float *n1_gamma, *n1_beta, *nf_gamma, *nf_beta; /* F each */
    float drop_p;
    uint64_t seed1, seed2;
    const uint64_t* drop_salt;                            /* device word mixed into both seeds, or NULL (grappa_gemm_desc.drop_salt) */
    float *save_mean1, *save_rstd1, *save_meanf, *save_rstdf;      /* (s*T) each, or NULL */
    void *save_x1, *save_qkv, *save_att, *save_x2, *save_x3, *save_u;      /* (s*T, F), qkv (s*T, 3F), or NULL */
    /* GATHER mode (gather_idx != NULL; the first layer of a head whose LayerNorm and q | k | v were computed once per (atom, position) TABLE row,
       reference models/interaction_parameters.py:155-180 + network_utils.py:112-133 on tokens that depend on their tuple only through (atom, position)):
       x1 and q | k | v are GATHERED -- token (pos, t) takes row gather_idx[t * s + pos] of x1_tab (rows x F, already normalised) and of qkv_tab
       (rows x 3F, bias included) -- instead of computed; x, n1_*, w_in_pk, save_x1 / save_qkv / save_mean1 / save_rstd1 are not used */
    const int* gather_idx;
    const void *x1_tab, *qkv_tab;
    int x2_tiled;      /* != 0: save_x2 holds grappa_writer_head_tiles(s, T) * 64 rows in the TILE order of grappa_writer_head_bwd (x2_tiled there too):
                          per tile and lane the 16 accumulator quads behind one another; 0: plain rows (what grappa_layernorm_bwd_bf16 reads) */
} grappa_writer_layer_desc;
int grappa_writer_head_fwd(void* stream, const grappa_writer_layer_desc* d);
/* The backward pass of the same layer: the whole input-gradient chain in one kernel per tile of 64 token rows
 *     dz2 = mask2(dout);  dz1 = (dz2 W_2) * ELU'(u);  dx3 = dz1 W_1 + dout;  dx2 = LN'(dx3; x2, nf);  dzo = mask1(dx2);  datt = dzo W_o;
 *     dqkv = attention'(qkv, datt);  dx1 = dqkv W_in + dx2;  dx = LN'(dx1; x, n1)
 * (the derivative of models/network_utils.py:112-133 with :44-54; mask1 / mask2: the forward's dropout masks, regenerated from seed1 / seed2).
 * Rounded to bf16 where the unfused kernels store a tensor: the five outputs dz2, dz1, dzo, dqkv, dx AND the intermediates dx3, dx2, datt, dx1,
 * which the unfused sequence writes to memory and this kernel keeps in registers / LDS (the LayerNorm partials sum the rounded dx3 / dx1).
 * The four weight (and bias) gradients are ordinary grouped weight-gradient products (grappa_gemm_f32_grouped) over the operands this kernel
 * writes as by-products -- dz2, dz1, dzo (s*T, F), dqkv (s*T, 3F) -- and the activations the forward saved (u, x3, att, x1).  LayerNorm parameter
 * gradients: per-tile partial sums, ln*_part[tile][0][F] = dgamma, [tile][1][F] = dbeta, grappa_writer_head_tiles(s, T) tiles (the layout
 * grappa_colsum_partials_batched reduces).  Weights packed TRANSPOSED (grappa_writer_pack_weight(F, 3F or F, W, ld, 1, ...)). */
typedef struct grappa_writer_layer_bwd_desc {
    int s, T, F, nheads, dtype;
    const void* dout;                                     /* (s*T, F): gradient of the layer's output */
    const void *x, *qkv, *x2, *u;                         /* the layer's input and what grappa_writer_head_fwd saved */
    const float *mean1, *rstd1, *meanf, *rstdf;
    const float *n1_gamma, *nf_gamma;
    const void *w_in_tpk, *w_o_tpk, *w1_tpk, *w2_tpk;     /* packed W_in^T (F x 3F), W_o^T, W_1^T, W_2^T (F x F) */
    float drop_p;
    uint64_t seed1, seed2;
    const uint64_t* drop_salt;
    void* dx;                                             /* (s*T, F): gradient of the layer's input */
    void *dz2, *dz1, *dzo, *dqkv;
    float *ln1_part, *lnf_part;                           /* (tiles, 2, F) each */
    int x2_tiled;                                         /* the layout of x2: see grappa_writer_layer_desc */
    const int* gather_idx;                                /* GATHER mode: `qkv` is the (rows x 3F) TABLE read through gather_idx; the chain ends behind the attention:
                                                             `dqkv` (token rows) and `dx` = the skip branch's gradient dx2 (token rows) are the outputs, x / mean1 / rstd1 /
                                                             n1_gamma / w_in_tpk / ln1_part are not used */
} grappa_writer_layer_bwd_desc;
int grappa_writer_head_bwd(void* stream, const grappa_writer_layer_bwd_desc* d);
int grappa_writer_head_tiles(int s, int T);
/* W (N x K fp32, rows ldw elements apart; transpose != 0: the operand is W^T, i.e. W is K x N) in the fragment order of the fused layer: block
 * (n / 16, k / 32) is one contiguous KB, 16 bytes per lane.  N % 16 == 0, K % 32 == 0; `out` holds grappa_writer_pack_bytes(N, K, dtype) bytes. */
size_t grappa_writer_pack_bytes(int N, int K, int dtype);
int grappa_writer_pack_weight(void* stream, int N, int K, const float* W, int ldw, int transpose, int dtype, void* out);

/* the dropout decision used by every kernel above, exposed for tests: 1 = keep */
int grappa_dropout_keep(uint64_t seed, uint64_t index, float p);

#ifdef __cplusplus
}
#endif
#endif /* GRAPPA_HIP_H */
