/*
 * fsg_hip.h -- C ABI of libfsg_hip.so: the MI355X (gfx950) hot path of kaftanski/fissure-segmentation.
 *
 * The reference has no FFI of its own: its seam is the Python nn.Module API.  This
 * header is the boundary that sits UNDER that API; each entry point names the reference code it
 * replaces (paths relative to the reference checkout).  Conventions:
 *   - plain C, no torch types; every pointer is a DEVICE pointer owned by the caller (hipMalloc'd /
 *     torch storage) unless marked "host"; nothing is allocated or freed inside the library;
 *   - row-major contiguous tensors unless explicit element strides are passed;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on that stream and
 *     keep no global state, so the library is re-entrant per stream (one process per GPU under DDP);
 *   - return value: FSG_OK or an FSG_ERR_* code; fsg_last_error() gives the text for the calling
 *     thread.  Nothing throws across the boundary.
 */
#ifndef FSG_HIP_H
#define FSG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_OK 0
#define FSG_ERR_ARG 1         /* bad shape / NULL pointer / unsupported size */
#define FSG_ERR_HIP 2         /* a HIP runtime call or launch failed          */
#define FSG_ERR_UNSUPPORTED 3 /* valid request this build cannot serve        */

#define FSG_KNN_FIX_DIAG 1   /* force d(i,i) = 0          -- utils/general_utils.py:52            */
#define FSG_KNN_DROP_FIRST 2 /* select k+1, drop column 0 -- utils/general_utils.py:317,320-322   */

#define FSG_KNN_FORCE_ROWS 4 /* use the general "rows in LDS" kernel even where the MFMA kernel applies (tests) */

#define FSG_KNN_FORCE_MFMA 8 /* (experimental kernels: libfsg_hip_experiments.so only; rejected by libfsg_hip.so)     */
/* Higher bits of `flags` are debug / cross-check selectors for tests and tools (csrc/knn_internal.h has the meanings); a bit that
 * is not listed here is FSG_ERR_ARG.  Tests, tools and bench.py pass the numbers: the values are fixed. */
#define FSG_KNN_DBG_HALF_CHUNKS (1 << 11)
#define FSG_KNN_DBG_TWO_PHASE (1 << 21)
#define FSG_KNN_DBG_ALL_SLOW (1 << 22)
#define FSG_KNN_DBG_STATS (1 << 25)
#define FSG_KNN_DBG_STAMPS (1 << 28)
#define FSG_KNN_DBG_ONE_LAUNCH (1 << 29)
#define FSG_KNN_DBG_BF16 (1 << 30)

#define FSG_KNN_MAX_K 64

typedef void *fsg_stream_t;

int fsg_version(void);
const char *fsg_last_error(void);

/*
 * Dense kNN graph build: replaces utils/general_utils.py:43-53 (pairwise_dist), :315-327 (knn) and
 * models/dgcnn_opensrc.py:34-40 (knn; flags = 0).  The (B,N,N) distance matrix is never materialised.
 *   x        (B, C, N) fp32, element strides (stride_b, stride_c, 1) -- a channel slice x[:, :3]
 *            is passed without a copy; only channels [0, c_knn) enter the distance
 *   idx_out  (B, N, k) int32, ascending (distance, index)
 *   dist_out (B, N, k) fp32 or NULL
 *   xx_scratch (B, N) fp32 scratch for the squared norms, or NULL (then only the general kernel is used)
 * Arithmetic: d = (xx_i - 2 * dot_ij) + xx_j, dot/xx as channel-ordered fp32 fma chains.
 * Limits: 1 <= k, k + drop <= min(N, FSG_KNN_MAX_K); N <= 32768.
 */
int fsg_knn_dense_f32(const float *x, int B, int N, int64_t stride_b, int64_t stride_c, int c_knn,
                      int k, int flags, int32_t *idx_out, float *dist_out, float *xx_scratch,
                      fsg_stream_t stream);

/*
 * The same graph build with a caller-owned workspace (what the nn.Module layer calls).  Inside 1024 <= N <= 8192 with
 * c_knn <= 64 (N <= 4096 for 64 < c_knn <= 128) and k + drop <= 64 the graph comes from the coarse-sweep + exact-refine kernel
 * (csrc/knn_split.hip): coarse products on the matrix cores -- ONE fp16 image of the points centred on a sampled mean and
 * scaled by a power of two above 4 channels (v_mfma_f32_32x32x16_f16), two bf16 pieces / three products up to 4 channels
 * (v_mfma_f32_32x32x16_bf16) -- only NOMINATE candidates under a rigorous error bound (~25 per query at k = 20), and only the
 * nominees get the arithmetic above: indices AND distance bits equal fsg_knn_dense_f32's.  Other shapes: fsg_knn_dense_f32 with
 * the workspace as xx_scratch.  workspace may be NULL (then as fsg_knn_dense_f32 with xx_scratch = NULL).
 */
size_t fsg_knn_dense_workspace_bytes(int B, int N, int c_knn);
int fsg_knn_dense_ws_f32(const float *x, int B, int N, int64_t stride_b, int64_t stride_c, int c_knn,
                         int k, int flags, int32_t *idx_out, float *dist_out, void *workspace,
                         size_t workspace_bytes, fsg_stream_t stream);

/*
 * fsg_knn_dense_ws_f32 over points of up to FOUR channels, plus their per-point product with a small weight:
 * pq_out (B, N, rows_pq) = x^T w_pq^T with w_pq (rows_pq, c_knn) row-major -- the "one plain GEMM" of the FIRST EdgeConv's
 * contract (models/dgcnn.py:212-243: its first 1x1 conv, decomposed per point; fsg_edge_weights_many_f32 makes the weight), a
 * K <= 4 product no matrix unit is needed for.  Where the graph build reads the (B, C, N) points itself (N = 2048, rows
 * addressable in 16-byte pieces) the rows come out of its first launch; otherwise a small launch follows the build.
 * 1 <= c_knn <= 4, rows_pq divides 256.
 */
int fsg_knn_dense_ws_pq_f32(const float *x, int B, int N, int64_t stride_b, int64_t stride_c, int c_knn, int k, int flags,
                            int32_t *idx_out, float *dist_out, void *workspace, size_t workspace_bytes, const float *w_pq,
                            int rows_pq, float *pq_out, fsg_stream_t stream);

/*
 * The same graph build when the PRODUCER of the points has already prepared it: fsg_edgeconv_apply_f32 (below) with a
 * knn_workspace emits the squared norms, the centred norms and the fp16 operand image of its output on the way, so the build
 * starts at its main kernel (one launch and ~11 us less per feature-space graph of DGCNN-seg).  x_pm = the point-major
 * (B, N, c_knn) copy of the points (the producer's out_pm), workspace = the one handed to the producer
 * (fsg_knn_dense_workspace_bytes(B, N, c_knn) bytes).  Same result bits as fsg_knn_dense_f32 on the same points.
 * c_knn in {16, 32, 64}, N % 64 == 0, 1024 <= N <= 8192, k + drop <= 64; FSG_ERR_UNSUPPORTED otherwise.
 */
int fsg_knn_dense_prepared_f32(const float *x_pm, int B, int N, int c_knn, int k, int flags, int32_t *idx_out, float *dist_out,
                               void *workspace, size_t workspace_bytes, fsg_stream_t stream);

/*
 * Edge features: replaces models/dgcnn.py:31-36 (create_neighbor_features: take_along_dim, repeat,
 * cat) and models/dgcnn_opensrc.py:43-66 (get_graph_feature).
 *   x (B,C,N) fp32, idx (B,N,k) int32 -> edge (B,2C,N,k): [x_j - x_i ; x_i]
 * _bwd is the autograd transpose: grad_edge (B,2C,N,k) -> grad_x (B,C,N), overwritten.
 */
int fsg_edge_gather_fwd_f32(const float *x, const int32_t *idx, float *edge, int B, int C, int N,
                            int k, fsg_stream_t stream);
int fsg_edge_gather_bwd_f32(const float *grad_edge, const int32_t *idx, float *grad_x, int B, int C,
                            int N, int k, fsg_stream_t stream);
/* create_neighbor_features (models/dgcnn.py:15-36) in one call: dynamic kNN graph over channels [0, c_knn) with the point
 * itself as neighbour 0 (:26-27) + the edge tensor.  x (B,C,N) contiguous; idx_out (B,N,k) int32; edge (B,2C,N,k);
 * xx_scratch (B,N) fp32.  (Reference-semantic op: the training path uses the fused fsg_edgeconv* entries instead.) */
int fsg_knn_gather_fused_f32(const float *x, int B, int C, int N, int k, int c_knn, int32_t *idx_out, float *edge,
                             float *xx_scratch, fsg_stream_t stream);
/* ... with the workspace of fsg_knn_dense_workspace_bytes(B, N, c_knn): the graph then comes from fsg_knn_dense_ws_f32 */
int fsg_knn_gather_fused_ws_f32(const float *x, int B, int C, int N, int k, int c_knn, int32_t *idx_out, float *edge,
                                void *workspace, size_t workspace_bytes, fsg_stream_t stream);
/* bf16 storage of the same op (BASELINE configs 3-5; SURVEY 8d counts the edge tensor at 2 bytes per element):
 * x, edge and grad_edge are bf16 (raw 16-bit patterns), the difference is formed in fp32 and rounded once;
 * grad_x is accumulated and returned in FP32 (B,C,N). */
int fsg_edge_gather_fwd_bf16(const void *x, const int32_t *idx, void *edge, int B, int C, int N, int k,
                             fsg_stream_t stream);
int fsg_edge_gather_bwd_bf16(const void *grad_edge, const int32_t *idx, float *grad_x, int B, int C, int N,
                             int k, fsg_stream_t stream);

/*
 * Reverse graph (CSR by destination) of a kNN graph -- needed by the gather-style backward below.
 *   idx (B,N,k) int32 -> rowptr (B,N+1) int32, col (B,N*k) int32 with col = (source point << 6) | slot.
 *   The in-edges of a destination are sorted ascending by (source, slot) -- the backward that walks them is then
 *   reproducible from run to run.  Destinations with more than 1024 in-edges (hub points) are sorted through a copy in
 *   the workspace; without a workspace they keep the order they were filled in.
 *   workspace: fsg_graph_reverse_csr_workspace_bytes(B,N,k) bytes, or NULL (then one workgroup per cloud builds the
 *   graph; with the workspace 16 workgroups per cloud share the edge list: count / scan / fill).
 */
size_t fsg_graph_reverse_csr_workspace_bytes(int B, int N, int k);
int fsg_graph_reverse_csr(const int32_t *idx, int B, int N, int k, int32_t *rowptr, int32_t *col,
                          void *workspace, fsg_stream_t stream);

/*
 * Weight of the per-point GEMM behind the fused EdgeConv: the first 1x1 conv over [x_j - x_i ; x_i] with
 * W = [W_rel | W_ctr] (Co, 2C) (models/dgcnn.py:234-241, :282-323) equals P_j + Q_i with [P | Q] = x [W_rel ; W_ctr - W_rel]^T.
 *   _fwd: W (Co,2C) -> Wt (2Co,C);   _bwd: grad_Wt (2Co,C) -> grad_W (Co,2C) (overwritten)
 */
int fsg_edge_weights_fwd_f32(const float *W, int Co, int C, float *Wt, fsg_stream_t stream);
int fsg_edge_weights_bwd_f32(const float *grad_Wt, int Co, int C, float *grad_W, fsg_stream_t stream);
/* the same for up to 8 layers in ONE launch (the transforms depend on the weights only): src/dst per layer are W -> Wt
 * (backward == 0) or grad_Wt -> grad_W (backward != 0); `jobs` is read on the host during the call */
#define FSG_EDGE_WEIGHT_MAX_JOBS 8
typedef struct fsg_edge_weight_jobs {
    const float *src[FSG_EDGE_WEIGHT_MAX_JOBS];
    float *dst[FSG_EDGE_WEIGHT_MAX_JOBS];
    int Co[FSG_EDGE_WEIGHT_MAX_JOBS];
    int C[FSG_EDGE_WEIGHT_MAX_JOBS];
    int n;
} fsg_edge_weight_jobs;
int fsg_edge_weights_many_f32(const fsg_edge_weight_jobs *jobs, int backward, fsg_stream_t stream);
/* The backward transform of fsg_edge_weights_many_f32 fed with UNREDUCED weight gradients: a job with S > 1 reads src as the
 * [S][2Co * C] split partials that fsg_gemm_small_deferred_f32 left in its workspace for the product grad_Wt (2Co, C), sums
 * them in the order fsg_gemm_small_f32's own reduction uses for that S (bit-identical to reducing first), then transforms;
 * a job with S <= 1 reads src as a finished grad_Wt.  One launch, no atomics. */
typedef struct fsg_edge_weight_fold_jobs {
    const float *src[FSG_EDGE_WEIGHT_MAX_JOBS];
    float *dst[FSG_EDGE_WEIGHT_MAX_JOBS];
    int Co[FSG_EDGE_WEIGHT_MAX_JOBS];
    int C[FSG_EDGE_WEIGHT_MAX_JOBS];
    int S[FSG_EDGE_WEIGHT_MAX_JOBS];
    int n;
} fsg_edge_weight_fold_jobs;
int fsg_edge_weights_bwd_folded_f32(const fsg_edge_weight_fold_jobs *jobs, fsg_stream_t stream);

/*
 * Last pass of the fused EdgeConv forward on its own: out (B,Co,N) [+ out_pm (B,N,Co)] = LeakyReLU(BatchNorm(ysel)) from the
 * selected pre-norm values, for callers that ran fsg_edgeconv{1,2}_fwd_* with out == NULL (those then stop after the
 * statistics).  knn_workspace != NULL (Co == 64, N % 64 == 0, both layouts): the pass also prepares the feature-space graph
 * build of the NEXT layer over its own output -- see fsg_knn_dense_prepared_f32.
 */
int fsg_edgeconv_apply_f32(const float *ysel, const float *gamma, const float *beta, const float *mean, const float *invstd,
                           int B, int N, int Co, float slope, float *out, float *out_pm, void *knn_workspace,
                           size_t knn_workspace_bytes, fsg_stream_t stream);

/*
 * The same pass (knn_workspace required) that ALSO emits the per-point rows of the next fused EdgeConv over this block's
 * output: pq_next (B, N, rows_next) = out_pm w_next^T with w_next (rows_next, Co) row-major = the [W_rel ; W_ctr - W_rel] weight
 * of the next block's first conv (fsg_edge_weights_many_f32) -- the "one plain GEMM" of fsg_edgeconv{1,2}_fwd_f32's contract
 * (models/dgcnn.py:212-243: the next EdgeConv's first 1x1 conv, decomposed per point), computed on the tile the pass holds in
 * LDS by the exact fp32 matrix instruction instead of by a library launch.  Co == 64, rows_next == 128, N % 64 == 0.
 */
int fsg_edgeconv_apply_pq_f32(const float *ysel, const float *gamma, const float *beta, const float *mean, const float *invstd,
                              int B, int N, int Co, float slope, float *out, float *out_pm, void *knn_workspace,
                              size_t knn_workspace_bytes, const float *w_next, int rows_next, float *pq_next,
                              fsg_stream_t stream);

/*
 * Fused EdgeConv with ONE shared-MLP layer: replaces models/dgcnn.py:234-241 (gather, 1x1 Conv2d, BatchNorm2d,
 * LeakyReLU, max over k) and the get_graph_feature -> conv -> max blocks of models/folding_net.py:120-133.
 * The caller supplies the per-point rows of the decomposed conv (W = [W_rel | W_ctr]):
 *   pq (B,N,2*Co) = [ x^T W_rel^T | x^T (W_ctr - W_rel)^T ]      (one plain GEMM), Co % 64 == 0, k <= 64.
 * Forward outputs: out (B,Co,N) and, if non-NULL, out_pm (B,N,Co) (the same values point-major, the layout the
 *   point-wise head consumes); saved for backward: ysel (B,N,Co) selected pre-BN value, arg (B,N,Co) uint8
 *   selected slot, ssum (B,N,Co) = sum_s y (training only), mean/invstd (Co) (outputs when training, inputs
 *   -- running statistics -- otherwise).  running_mean/var (nullable) are updated in place when training.
 *   workspace: fsg_edgeconv1_workspace_bytes() floats-as-bytes (training only).
 * Backward: grad_out (B,Co,N) and/or up to two point-major gradients grad_out_pm / grad_out_pm2 (B,N,Co) with row strides
 *   ld_pm / ld_pm2 >= Co in elements (any of the three may be NULL; they are summed) -> grad_pq (B,N,2*Co), grad_gamma, grad_beta (Co); h_scratch (B,N,Co) and
 *   workspace (2*Co*B*ceil(N/64) floats) are caller-provided scratch.
 */
size_t fsg_edgeconv1_workspace_bytes(int B, int N, int Co);
int fsg_edgeconv1_fwd_f32(const float *pq, const int32_t *idx, const float *gamma, const float *beta,
                          float *running_mean, float *running_var, int B, int N, int k, int Co, int training,
                          float momentum, float eps, float slope, float *out, float *out_pm, float *ysel,
                          uint8_t *arg, float *ssum, float *mean, float *invstd, float *workspace,
                          fsg_stream_t stream);
int fsg_edgeconv1_bwd_f32(const float *grad_out, const float *grad_out_pm, int64_t ld_pm, const float *grad_out_pm2,
                          int64_t ld_pm2, const float *pq, const int32_t *rowptr, const int32_t *col,
                          const float *gamma, const float *beta, const float *mean, const float *invstd,
                          const float *ysel, const uint8_t *arg, const float *ssum, int B, int N, int k, int Co,
                          int training, float slope, float *grad_pq, float *grad_gamma, float *grad_beta,
                          float *h_scratch, float *workspace, fsg_stream_t stream);

/*
 * Fused EdgeConv with TWO shared-MLP layers (2C -> 64 -> C2, C2 = 64 or 128): replaces models/dgcnn.py:234-241 for
 * len(shared_mlp) == 2 (ec1 of DGCNNSeg, the EdgeConv of the SpatialTransformer).  Layer 1 arrives decomposed as
 * pq (B,N,128) = [P | Q] like fsg_edgeconv1; w2 (C2,64) is the second 1x1 conv; *1 / *2 are the two BatchNorms.
 * Forward saves ssum1 (B,N,64), mean1/invstd1, ysel2/arg2/ssum2 (B,N,C2), mean2/invstd2 for the backward
 * (mean/invstd are INPUTS -- running statistics -- when training == 0).  Backward (output gradients as for
 * fsg_edgeconv1_bwd_f32) returns grad_pq (B,N,128),
 * grad_w2 (C2,64) and the four BatchNorm parameter gradients.  Workspaces: fsg_edgeconv2_workspace_bytes /
 * fsg_edgeconv2_bwd_workspace_bytes (the backward one holds the only per-edge tensor, du1 (B*N*k, 64)).
 */
size_t fsg_edgeconv2_workspace_bytes(int B, int N, int k, int C2);
size_t fsg_edgeconv2_bwd_workspace_bytes(int B, int N, int k, int C2);
int fsg_edgeconv2_fwd_f32(const float *pq, const int32_t *idx, const float *w2, const float *gamma1,
                          const float *beta1, float *running_mean1, float *running_var1, const float *gamma2,
                          const float *beta2, float *running_mean2, float *running_var2, int B, int N, int k, int C2,
                          int training, float momentum1, float momentum2, float eps1, float eps2, float slope,
                          float *out, float *out_pm, float *ssum1, float *mean1, float *invstd1, float *ysel2,
                          uint8_t *arg2, float *ssum2, float *mean2, float *invstd2, void *workspace,
                          fsg_stream_t stream);
int fsg_edgeconv2_bwd_f32(const float *grad_out, const float *grad_out_pm, int64_t ld_pm, const float *grad_out_pm2,
                          int64_t ld_pm2, const float *pq, const int32_t *idx,
                          const int32_t *rowptr, const int32_t *col, const float *w2, const float *gamma1,
                          const float *beta1, const float *mean1, const float *invstd1, const float *ssum1,
                          const float *gamma2, const float *beta2, const float *mean2, const float *invstd2,
                          const float *ysel2, const uint8_t *arg2, int B, int N, int k, int C2, int training,
                          float slope, float *grad_pq, float *grad_w2, float *grad_gamma1, float *grad_beta1,
                          float *grad_gamma2, float *grad_beta2, void *workspace, fsg_stream_t stream);
/* bf16 operand mode of the same two entry points (same arguments, every tensor fp32): the per-edge 64 x C2 contraction
 * of the forward and the three per-tile products of the backward (y2 recompute, dz1 = dy2 W2, dW2 += dy2^T z1) run on
 * v_mfma_f32_32x32x16_bf16 -- operands rounded to bf16 (once, on their way INTO the LDS operand image at C2 = 64; at every
 * fragment read at C2 = 128), fp32 accumulation; gathers, BatchNorm statistics, selection and all stored tensors are
 * unchanged.  The graph (idx) is always built in fp32.  (The fp32 entry points run the same kernels at C2 = 64 with three
 * bf16 pieces per operand and six products -- fp32-grade, see fsg_pw_* below; v_mfma_f32_32x32x2_f32 at C2 = 128.) */
int fsg_edgeconv2_fwd_bf16(const float *pq, const int32_t *idx, const float *w2, const float *gamma1,
                           const float *beta1, float *running_mean1, float *running_var1, const float *gamma2,
                           const float *beta2, float *running_mean2, float *running_var2, int B, int N, int k, int C2,
                           int training, float momentum1, float momentum2, float eps1, float eps2, float slope,
                           float *out, float *out_pm, float *ssum1, float *mean1, float *invstd1, float *ysel2,
                           uint8_t *arg2, float *ssum2, float *mean2, float *invstd2, void *workspace,
                           fsg_stream_t stream);
int fsg_edgeconv2_bwd_bf16(const float *grad_out, const float *grad_out_pm, int64_t ld_pm, const float *grad_out_pm2,
                           int64_t ld_pm2, const float *pq, const int32_t *idx,
                           const int32_t *rowptr, const int32_t *col, const float *w2, const float *gamma1,
                           const float *beta1, const float *mean1, const float *invstd1, const float *ssum1,
                           const float *gamma2, const float *beta2, const float *mean2, const float *invstd2,
                           const float *ysel2, const uint8_t *arg2, int B, int N, int k, int C2, int training,
                           float slope, float *grad_pq, float *grad_w2, float *grad_gamma1, float *grad_beta1,
                           float *grad_gamma2, float *grad_beta2, void *workspace, fsg_stream_t stream);

/*
 * Fused BatchNorm + LeakyReLU on point-major rows (M, C), C % 64 == 0: the stage behind every 1x1 conv of the
 * point-wise head (models/dgcnn.py:282-323 ConvBlock: conv -> BatchNorm -> LeakyReLU; slope 1 = no activation,
 * slope 0 = ReLU).  Forward: y -> out, plus mean/invstd (outputs when training, inputs otherwise) and the in-place
 * running-statistics update; backward: grad_out, y -> grad_y, grad_gamma, grad_beta.
 * workspace: fsg_bn_act_workspace_bytes(M, C) bytes.  One statistics record per 128 rows: ceil(M / 128) <= 65535
 * (M <= 8388480), anything larger is rejected as a bad shape.
 */
size_t fsg_bn_act_workspace_bytes(long M, int C);
int fsg_bn_act_fwd_f32(const float *y, const float *gamma, const float *beta, float *running_mean, float *running_var,
                       long M, int C, int training, float momentum, float eps, float slope, float *out, float *mean,
                       float *invstd, float *workspace, fsg_stream_t stream);
int fsg_bn_act_bwd_f32(const float *grad_out, const float *y, const float *gamma, const float *beta, const float *mean,
                       const float *invstd, long M, int C, int training, float slope, float *grad_y, float *grad_gamma,
                       float *grad_beta, float *workspace, fsg_stream_t stream);

/*
 * BatchNorm + LeakyReLU + max over the N points of each cloud in one stage: the global feature of DGCNNSeg
 * (models/dgcnn.py:134-137: SharedFullyConnected(192,1024) -> AdaptiveMaxPool1d(1)) without materialising the
 * (B*N, C) activation.  y (B,N,C) pre-norm rows -> out (B,C); saved: ysel (B,C) selected pre-norm value, arg (B,C)
 * its point index.  Backward: grad_out (B,C) -> grad_y (B,N,C) (dense: BN statistics terms), grad_gamma, grad_beta.
 * One record per (cloud, 128 points): B * ceil(N / 128) <= 65535, anything larger is rejected as a bad shape
 * (fsg_bn_act_maxavg_* below has the same limit).
 */
size_t fsg_bn_act_max_workspace_bytes(int B, int N, int C);
int fsg_bn_act_max_fwd_f32(const float *y, const float *gamma, const float *beta, float *running_mean,
                           float *running_var, int B, int N, int C, int training, float momentum, float eps,
                           float slope, float *out, float *ysel, int32_t *arg, float *mean, float *invstd,
                           float *workspace, fsg_stream_t stream);
int fsg_bn_act_max_bwd_f32(const float *grad_out, const float *y, const float *ysel, const int32_t *arg,
                           const float *gamma, const float *beta, const float *mean, const float *invstd, int B, int N,
                           int C, int training, float slope, float *grad_y, float *grad_gamma, float *grad_beta,
                           fsg_stream_t stream);

/*
 * BatchNorm + LeakyReLU + [max | mean] over the N points of each cloud: the global feature of the upstream DGCNN
 * (models/dgcnn_opensrc.py:158-164: conv5 = Conv1d -> BatchNorm1d -> LeakyReLU, then
 * cat(adaptive_max_pool1d, adaptive_avg_pool1d)).  y (B,N,C) pre-norm rows, C % 64 == 0 -> out (B,2C) =
 * [max_n a | mean_n a], a = LeakyReLU(BN(y)); saved: arg (B,C) the point of the max (lowest index on ties).
 * mean/invstd are outputs when training (batch statistics over B*N rows, running statistics updated in place with
 * momentum), inputs otherwise.  Two reads of y; the activation is never written.
 * Backward: grad_out (B,2C) -> grad_y (B,N,C) = BN-backward of f'(u) (g_max [n = arg] + g_avg / N), grad_gamma,
 * grad_beta (fixed-order sums, no atomics).  workspace: fsg_bn_act_maxavg_workspace_bytes(B, N, C) bytes, both passes.
 */
size_t fsg_bn_act_maxavg_workspace_bytes(int B, int N, int C);
int fsg_bn_act_maxavg_fwd_f32(const float *y, const float *gamma, const float *beta, float *running_mean,
                              float *running_var, int B, int N, int C, int training, float momentum, float eps,
                              float slope, float *out, int32_t *arg, float *mean, float *invstd, float *workspace,
                              fsg_stream_t stream);
int fsg_bn_act_maxavg_bwd_f32(const float *grad_out, const float *y, const int32_t *arg, const float *gamma,
                              const float *beta, const float *mean, const float *invstd, int B, int N, int C,
                              int training, float slope, float *grad_y, float *grad_gamma, float *grad_beta,
                              float *workspace, fsg_stream_t stream);

/*
 * Chamfer nearest neighbour, one direction: replaces the pytorch3d.loss.chamfer_distance call of
 * losses/chamfer_loss.py:19 (and losses/mesh_loss.py:29-31, train_pc_ae.py:88).
 *   x (B,N,3), y (B,M,3) fp32 -> dist (B,N) = min_j |x_i - y_j|^2, arg (B,N) int32 (lowest j on ties)
 * _bwd: given g = dLoss/d dist (B,N) and arg, ACCUMULATES into grad_x (B,N,3) and grad_y (B,M,3)
 *   grad_x[i] += 2 g_i (x_i - y_arg) ; grad_y[arg] -= 2 g_i (x_i - y_arg)      (caller zero-fills)
 *   workspace (fsg_chamfer_nn_bwd_workspace_bytes, 4-byte aligned): grad_y is summed per target in ascending query order
 *   through the reverse graph of arg (reproducible); NULL: scattered with hardware fp32 atomics.
 */
size_t fsg_chamfer_nn_bwd_workspace_bytes(int B, int N, int M);
int fsg_chamfer_nn_f32(const float *x, const float *y, int B, int N, int M, float *dist,
                       int32_t *arg, fsg_stream_t stream);
int fsg_chamfer_nn_bwd_f32(const float *x, const float *y, const int32_t *arg, const float *g_dist,
                           int B, int N, int M, float *grad_x, float *grad_y, void *workspace,
                           fsg_stream_t stream);

/*
 * Unsigned point-to-triangle-mesh distance: replaces the open3d RaycastingScene.compute_distance call of metrics.py:20-24
 * (under assd / batch_assd / pseudo_symmetric_point_to_mesh_distance).  Brute force over all faces, exact in the
 * seven-region sense: the closest point lies in the face interior, on an edge or at a vertex.
 *   pts (B,P,3), verts (B,V,3) fp32, faces (Bf,F,3) int32 with Bf == 1 (one face list shared by all meshes) or Bf == B
 *   -> dist2 (B,P) = min over faces of the squared distance (lowest face index on ties),
 *      face (B,P) int32 a face that attains it (NULL: not written), closest (B,P,3) that closest point (NULL: not written)
 * Faces without area are legal: they yield the distance to their longest edge, or to the point if all three vertices coincide;
 * never NaN or Inf for finite input.  Face indices are NOT checked against V (the caller validates them once per face list).
 * P, V, F > 0.  One launch, no workspace.
 */
int fsg_point_mesh_dist_f32(const float *pts, const float *verts, const int32_t *faces, int B, int P, int V, int F,
                            int Bf, float *dist2, int32_t *face, float *closest, fsg_stream_t stream);

/*
 * Triangle meshes -> voxel label maps: replace mesh2labelmap_dist (data_processing/surface_fitting_optimization.py:332-358)
 * and the surface sampling of o3d_mesh_to_labelmap / mesh2labelmap_sampling (data_processing/surface_fitting.py:144-169,
 * :19-39).  All meshes of a call are packed: verts (V,3) fp32 in the axis order of the volume (d0, d1, d2), faces (F,3) int32
 * into verts, labels (F,) int32 = the mesh m >= 0 of every face.  One wave per face scans the voxels of the face's bounding
 * box, which is clipped to the volume in float before any index is formed; coordinates outside the volume, Inf included,
 * are legal, and a face with a NaN vertex takes part in nothing.  Face indices are NOT checked against V (the caller does).
 * Faces without area are legal (their longest edge, or the point).  V, F, d0, d1, d2 > 0, d0 d1 d2 < 2^31, spacings positive
 * and finite; all of this is checked before anything is launched.
 *
 * fsg_mesh_labelmap_dist_f32: voxel (i0,i1,i2) has the centre (i0 s0, i1 s1, i2 s2); out (d0,d1,d2) int64 = 1 + m of the
 *   mesh of smallest distance (the arithmetic of fsg_point_mesh_dist_f32; the lowest m on an exact tie) if that distance is
 *   <= dist_threshold (>= 0; compared as squares) and mask (d0,d1,d2) uint8, NULL = all set, is non-zero there; else 0.
 *   keys: d0 d1 d2 uint64 of scratch, initialised here.  Memset + two launches; bitwise reproducible.
 * fsg_mesh_labelmap_cover_f32: cell (i0,i1,i2) is the box [i s, (i + 1) s) per axis; out = the highest 1 + m among the
 *   meshes with a triangle that intersects the cell (separating axes), 0 if none.  Memset + one launch, no scratch.
 */
int fsg_mesh_labelmap_dist_f32(const float *verts, const int32_t *faces, const int32_t *labels, int V, int F, int d0, int d1,
                               int d2, float s0, float s1, float s2, float dist_threshold, const uint8_t *mask, uint64_t *keys,
                               int64_t *out, fsg_stream_t stream);
int fsg_mesh_labelmap_cover_f32(const float *verts, const int32_t *faces, const int32_t *labels, int V, int F, int d0, int d1,
                                int d2, float s0, float s1, float s2, int64_t *out, fsg_stream_t stream);

/*
 * Segmentation loss, value and gradient: replaces losses/nnu_loss.py:6-19, i.e.
 * nn.CrossEntropyLoss(class_weights) + GDL(softmax over dim 1, batch_dice=True, do_bg=True, smooth=1, weights 1/volume)
 * of losses/dice_loss.py:24-96 (the criterion train.py:38 builds for the default --loss nnunet).
 *   logits (B,C,N) fp32 with element strides (stride_b, stride_c, stride_n) -- class-major or point-major alike;
 *   labels (B,N) int64 contiguous, values in [0,C); class_weights (C) fp32 or NULL (= all ones); 2 <= C <= 32
 *   loss_out[4] = { w_ce*ce + w_dice*gdl, ce, gdl, number of labels outside [0,C) (those points are skipped) }
 *   grad (nullable) = d loss_out[0] / d logits, written with its own element strides
 *   workspace: fsg_nnu_loss_workspace_bytes(C) bytes, 8-byte aligned.  Reproducible: no atomics, fixed reduction order.
 */
size_t fsg_nnu_loss_workspace_bytes(int C);
int fsg_nnu_loss_f32(const float *logits, int64_t stride_b, int64_t stride_c, int64_t stride_n,
                     const int64_t *labels, const float *class_weights, int B, int C, int N, float w_ce,
                     float w_dice, float smooth, float *loss_out, float *grad, int64_t gstride_b,
                     int64_t gstride_c, int64_t gstride_n, void *workspace, fsg_stream_t stream);

/*
 * Packed-segment kNN query: replaces pointops_cuda.knnquery_cuda behind
 * models/pointtransformer/pointops.py:42-62.
 *   xyz (n,3), new_xyz (m,3) fp32; offset / new_offset (b) int32 cumulative segment ends
 *   idx (m,nsample) int32 global row numbers, dist2 (m,nsample) SQUARED distances, ascending
 *   (the Python wrapper returns sqrt, as pointops.py:60 does).  Segments shorter than nsample are
 *   padded with (first row of the segment, 1e10).   nsample <= 64.
 */
int fsg_knn_segment_f32(const float *xyz, const float *new_xyz, const int32_t *offset,
                        const int32_t *new_offset, int b, int n, int m, int nsample, int32_t *idx,
                        float *dist2, fsg_stream_t stream);

/*
 * Farthest point sampling per segment: replaces pointops_cuda.furthestsampling_cuda behind
 * models/pointtransformer/pointops.py:16-39.   tmp: (n) fp32 scratch (the reference's `tmp`),
 * idx: (new_offset[b-1]) int32.  First sample of a segment = its first row; ties -> lowest index.
 */
int fsg_fps_f32(const float *xyz, const int32_t *offset, const int32_t *new_offset, int b, int n,
                float *tmp, int32_t *idx, fsg_stream_t stream);

/*
 * Row gather / scatter-add by neighbour index: replaces the fancy-index grouping of
 * models/pointtransformer/pointops.py:114-118 (and pointops_cuda.grouping_*, :78,:94).
 *   feat (n,c), idx (m,ns) -> out (m,ns,c) = feat[idx]       ; bwd ACCUMULATES into grad_feat (n,c)
 */
int fsg_group_gather_fwd_f32(const float *feat, const int32_t *idx, float *out, int n, int c, int m,
                             int ns, fsg_stream_t stream);
int fsg_group_gather_bwd_f32(const float *grad_out, const int32_t *idx, float *grad_feat, int n,
                             int c, int m, int ns, fsg_stream_t stream);

/* pointops.queryandgroup(use_xyz=True) (reference: models/pointtransformer/pointops.py:100-123) as one launch: out (m, ns, 3 + c)
 * = [ xyz[idx] - new_xyz | feat[idx] ].  Backward: the feature columns of grad_out (m, ns, 3 + c) are scattered into grad_feat
 * (n, c), which the caller ZEROES (atomics); coordinates carry no gradient here. */
int fsg_group_xyz_feat_fwd_f32(const float *xyz, const float *new_xyz, const float *feat, const int32_t *idx, float *out, int n,
                               int c, int m, int ns, fsg_stream_t stream);
int fsg_group_xyz_feat_bwd_f32(const float *grad_out, const int32_t *idx, float *grad_feat, int n, int c, int m, int ns,
                               fsg_stream_t stream);

/* max over the ns neighbour rows of x (m, ns, c) with its arg-max (TransitionDown's MaxPool1d, reference: models/pointtransformer/
 * seg_model.py:77-83); the backward writes the whole (m, ns, c) gradient in one launch. */
int fsg_rows_max_fwd_f32(const float *x, float *out, int32_t *arg, int m, int ns, int c, fsg_stream_t stream);
int fsg_rows_max_bwd_f32(const float *grad_out, const int32_t *arg, float *grad_x, int m, int ns, int c, fsg_stream_t stream);

/* pointops.interpolation (reference: models/pointtransformer/pointops.py:198-215) as one launch each way: out (m, c) =
 * sum_j feat[idx[i, j]] w_ij with w_ij = 1 / (sqrt(dist2[i, j]) + 1e-8) normalised over the k neighbours (k <= 8); idx / dist2
 * (m, k) from fsg_knn_segment_f32.  Backward: grad_feat (n, c) must be ZEROED by the caller (atomic accumulation). */
int fsg_interp_fwd_f32(const float *feat, const int32_t *idx, const float *dist2, float *out, int n, int c, int m, int k,
                       fsg_stream_t stream);
int fsg_interp_bwd_f32(const float *grad_out, const int32_t *idx, const float *dist2, float *grad_feat, int n, int c, int m, int k,
                       fsg_stream_t stream);


/*
 * Vector-attention aggregate: replaces models/pointtransformer/seg_model.py:50-52 (and
 * pointops_cuda.aggregation_*, pointops.py:161-195), fused with the value gather:
 *   out[i, ch] = sum_j (v[idx[i,j], ch] + pos[i,j,ch]) * w[i, j, ch mod cw]        cw = c / share_planes
 *   v (n,c), pos (n,ns,c), w (n,ns,cw), idx (n,ns) -> out (n,c)
 * _bwd: grad_out (n,c) -> grad_v (n,c) ACCUMULATED (caller zero-fills), grad_pos (n,ns,c) and
 *   grad_w (n,ns,cw) overwritten.
 */
int fsg_vec_attn_fwd_f32(const float *v, const float *pos, const float *w, const int32_t *idx,
                         float *out, int n, int ns, int c, int cw, fsg_stream_t stream);
int fsg_vec_attn_bwd_f32(const float *v, const float *pos, const float *w, const int32_t *idx,
                         const float *grad_out, float *grad_v, float *grad_pos, float *grad_w, int n,
                         int ns, int c, int cw, fsg_stream_t stream);

/*
 * BatchNorm1d (+ residual) (+ ReLU) over packed point rows: the `relu(bn(linear(x)))` / `relu(bn(linear(y)) + identity)`
 * glue of models/pointtransformer/seg_model.py (:66, :82, :92-99, :138-141, :168).
 *   x, residual (nullable), out: (M,C) fp32 row-major, C in {32,64,128,256,512};  out = [relu]( bn(x) [+ residual] )
 *   training: batch statistics (fp64 sums, fixed order), running buffers updated with torch's rule (nullable);
 *   eval: the caller provides mean / rstd.  workspace: fsg_bn_rows_workspace_bytes(M,C), 8-byte aligned.
 * _bwd: grad_out (M,C) -> grad_x, grad_residual (nullable; = grad_out masked by the ReLU), grad_gamma, grad_beta,
 *   all overwritten; `out` is the forward result (the ReLU mask), needed when relu != 0.
 */
size_t fsg_bn_rows_workspace_bytes(long M, int C);
int fsg_bn_rows_fwd_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                        float *running_mean, float *running_var, long M, int C, int training, float momentum,
                        float eps, int relu, float *out, float *mean, float *rstd, void *workspace,
                        fsg_stream_t stream);
int fsg_bn_rows_bwd_f32(const float *grad_out, const float *x, const float *out, const float *gamma,
                        const float *mean, const float *rstd, long M, int C, int training, int relu,
                        float *grad_x, float *grad_residual, float *grad_gamma, float *grad_beta,
                        void *workspace, fsg_stream_t stream);

/*
 * Small / skinny fp32 GEMM:  C[i,j] = sum_k A(i,k) * B(k,j) (+ bias[j]),  A(i,k) = A[i*sa_i + k*sa_k],
 * B(k,j) = B[k*sb_k + j*sb_j] (element strides: any transposition), C row-major with row stride ldc.
 * Carries the point-wise Linears of models/pointtransformer/seg_model.py (:25-33, :64-69, :92-99, :128-134, :168-169)
 * and their dX / dW products, for which the vendor GEMM launches a single workgroup (see csrc/small_gemm.hip).
 * Reproducible (split reductions are summed in a fixed order).  workspace: fsg_gemm_small_workspace_bytes(I,J,K)
 * bytes (0 when the shape needs no split), 4-byte aligned.
 */
size_t fsg_gemm_small_workspace_bytes(int I, int J, int K);
int fsg_gemm_small_f32(const float *A, int64_t sa_i, int64_t sa_k, const float *B, int64_t sb_k, int64_t sb_j,
                       const float *bias, float *C, int64_t ldc, int I, int J, int K, void *workspace,
                       fsg_stream_t stream);
/* The same product with a by-product: rowsum[i] = sum_k A(i, k) (NULL: none).  With A = dY^T (the weight gradient
 * dW = dY^T X of a Linear, models/pointtransformer/seg_model.py) that is the layer's bias gradient -- one launch instead of the
 * product plus a column reduction.  Same workspace, same fixed summation order. */
int fsg_gemm_small_rowsum_f32(const float *A, int64_t sa_i, int64_t sa_k, const float *B, int64_t sb_k, int64_t sb_j,
                              const float *bias, float *C, int64_t ldc, int I, int J, int K, float *rowsum, void *workspace,
                              fsg_stream_t stream);

/* Deferred split reduction (PointTransformer backward: 50 weight gradients per step, each a tiny output behind a reduction over
 * all points).  fsg_gemm_small_deferred_f32 runs the product only: *splits = S > 1 when the S partial products (and row-sum
 * partials) were left in `workspace`, which the caller keeps alive; 0 when C / rowsum are already final.
 * fsg_gemm_small_reduce_many_f32 then sums up to FSG_GEMM_REDUCE_MAX_JOBS such products in ONE launch, in split order
 * (reproducible).  `blocks` is filled by the callee. */
#define FSG_GEMM_REDUCE_MAX_JOBS 48
typedef struct fsg_gemm_reduce_jobs {
    const float *part[FSG_GEMM_REDUCE_MAX_JOBS];
    float *C[FSG_GEMM_REDUCE_MAX_JOBS];
    float *rowsum[FSG_GEMM_REDUCE_MAX_JOBS];
    int64_t ldc[FSG_GEMM_REDUCE_MAX_JOBS];
    int32_t S[FSG_GEMM_REDUCE_MAX_JOBS], I[FSG_GEMM_REDUCE_MAX_JOBS], J[FSG_GEMM_REDUCE_MAX_JOBS], blocks[FSG_GEMM_REDUCE_MAX_JOBS];
    int32_t n;
} fsg_gemm_reduce_jobs;
int fsg_gemm_small_deferred_f32(const float *A, int64_t sa_i, int64_t sa_k, const float *B, int64_t sb_k, int64_t sb_j, float *C,
                                int64_t ldc, int I, int J, int K, float *rowsum, void *workspace, int *splits,
                                fsg_stream_t stream);
int fsg_gemm_small_reduce_many_f32(const fsg_gemm_reduce_jobs *jobs, fsg_stream_t stream);
/* fsg_gemm_small_deferred_f32 for up to FSG_GEMM_SMALL_MAX_JOBS products in ONE launch (no row sums): every product keeps the
 * tiles, splits and arithmetic it has alone, so C / the partials in workspace[j] carry the same bits.  splits[j] is filled by
 * the callee as fsg_gemm_small_deferred_f32 fills *splits; `jobs` is read and written on the host during the call. */
#define FSG_GEMM_SMALL_MAX_JOBS 8
typedef struct fsg_gemm_small_jobs {
    const float *A[FSG_GEMM_SMALL_MAX_JOBS];
    int64_t sa_i[FSG_GEMM_SMALL_MAX_JOBS], sa_k[FSG_GEMM_SMALL_MAX_JOBS];
    const float *B[FSG_GEMM_SMALL_MAX_JOBS];
    int64_t sb_k[FSG_GEMM_SMALL_MAX_JOBS], sb_j[FSG_GEMM_SMALL_MAX_JOBS];
    float *C[FSG_GEMM_SMALL_MAX_JOBS];
    int64_t ldc[FSG_GEMM_SMALL_MAX_JOBS];
    int32_t I[FSG_GEMM_SMALL_MAX_JOBS], J[FSG_GEMM_SMALL_MAX_JOBS], K[FSG_GEMM_SMALL_MAX_JOBS];
    void *workspace[FSG_GEMM_SMALL_MAX_JOBS];
    int32_t splits[FSG_GEMM_SMALL_MAX_JOBS];
    int32_t n;
} fsg_gemm_small_jobs;
int fsg_gemm_small_many_deferred_f32(fsg_gemm_small_jobs *jobs, fsg_stream_t stream);
/* bf16 operand mode of fsg_gemm_small_rowsum_f32 (splits == NULL) / fsg_gemm_small_deferred_f32 (splits != NULL, bias NULL): both
 * operands are rounded to bf16 (nearest even) on their way into LDS, products on v_mfma_f32_32x32x16_bf16, fp32 accumulation,
 * fp32 output.  The nn.Linear products of the PointTransformer in bf16 mode (reference: autocast, model_trainer.py:75-76,157). */
int fsg_gemm_small_bf16(const float *A, int64_t sa_i, int64_t sa_k, const float *B, int64_t sb_k, int64_t sb_j, const float *bias,
                        float *C, int64_t ldc, int I, int J, int K, float *rowsum, void *workspace, int *splits,
                        fsg_stream_t stream);


/*
 * Fused PointTransformerLayer body: replaces models/pointtransformer/seg_model.py:38-53 after the three
 * q/k/v Linears (:37), i.e. neighbour grouping of keys, values and coordinates, linear_p (Linear(3,3) -> BatchNorm1d(3)
 * -> ReLU -> Linear(3,c)), w = k_j - q_i + p_r, linear_w (BatchNorm1d(c) -> ReLU -> Linear(c,c/8) -> BatchNorm1d(c/8) ->
 * ReLU -> Linear(c/8,c/8)), softmax over the nsample neighbours and the shared-plane aggregate
 *     out[i,ch] = sum_s (v[idx[i,s],ch] + p_r[i,s,ch]) * softmax_s(w)[i,s,ch mod c/8]
 * without any (n,nsample,c) tensor in HBM.  Train-mode BatchNorm statistics run over all n*nsample edges (one pass per
 * BatchNorm, fp64 sums, fixed order) and update the running buffers with torch's rule (unbiased variance).
 *   p (n,3) fp32; idx (n,ns) int32 rows of p/q/k/v (every entry valid -- fsg_knn_segment_f32 pads short segments);
 *   q, k, v (n,c) fp32 with a common row stride ld (in elements: 3c when they are slices of one (n,3c) GEMM output);
 *   c in {32,64,128,256,512}, 1 <= ns <= 16, share_planes = 8.
 *   stats [2*(3+c+c/8)] = mean|rstd of the three BatchNorms (written in training, read in eval: the caller fills them
 *   from the running buffers); u1 (n,ns,c/8) pre-BatchNorm output of the first linear_w Linear and sm (n,ns,c/8) the
 *   softmax weights are kept for the backward; workspace: fsg_pt_attn_workspace_bytes(n, ns, c), 8-byte aligned.
 * _bwd: grad_out (n,c) -> grad_q (n,c, row stride ldg) overwritten; grad_k, grad_v ACCUMULATED (caller zero-fills);
 *   every pointer of `grads` overwritten (same shapes as the parameters); grad_p (n,3) nullable, ACCUMULATED (the
 *   coordinates are network inputs, seg_model.py:202-231: pass NULL unless the input itself needs a gradient).
 */
typedef struct fsg_pt_layer_params {
    const float *lp1_w, *lp1_b;               /* linear_p.0: (3,3), (3) */
    const float *bnp_g, *bnp_b;               /* linear_p.1: (3) */
    float *bnp_rm, *bnp_rv;                   /*   running mean / var, nullable */
    const float *lp2_w, *lp2_b;               /* linear_p.3: (c,3), (c) */
    const float *bn1_g, *bn1_b;               /* linear_w.0: (c) */
    float *bn1_rm, *bn1_rv;
    const float *lw1_w, *lw1_b;               /* linear_w.2: (c/8,c), (c/8) */
    const float *bn2_g, *bn2_b;               /* linear_w.3: (c/8) */
    float *bn2_rm, *bn2_rv;
    const float *lw2_w, *lw2_b;               /* linear_w.5: (c/8,c/8), (c/8) */
    float eps_p, eps_1, eps_2;
    float mom_p, mom_1, mom_2;                /* momentum of this call for the running buffers */
} fsg_pt_layer_params;

typedef struct fsg_pt_layer_grads {
    float *lp1_w, *lp1_b, *bnp_g, *bnp_b, *lp2_w, *lp2_b, *bn1_g, *bn1_b, *lw1_w, *lw1_b, *bn2_g, *bn2_b, *lw2_w,
        *lw2_b;
} fsg_pt_layer_grads;

size_t fsg_pt_attn_workspace_bytes(int n, int ns, int c);
int fsg_pt_attn_fwd_f32(const float *p, const int32_t *idx, const float *q, const float *k, const float *v,
                        int64_t ld, const fsg_pt_layer_params *params, int n, int ns, int c, int training,
                        float *out, float *stats, float *u1, float *sm, void *workspace, fsg_stream_t stream);
int fsg_pt_attn_bwd_f32(const float *p, const int32_t *idx, const float *q, const float *k, const float *v,
                        int64_t ld, const fsg_pt_layer_params *params, int n, int ns, int c, int training,
                        const float *grad_out, const float *stats, const float *u1, const float *sm,
                        float *grad_q, float *grad_k, float *grad_v, int64_t ldg, float *grad_p,
                        const fsg_pt_layer_grads *grads, void *workspace, fsg_stream_t stream);

/*
 * Adam over one flat fp32 buffer -- replaces torch.optim.Adam(model.parameters(), lr, weight_decay) of
 * model_trainer.py:57 once the parameters live in one contiguous buffer (optim.FlatAdam).  Update rule of
 * torch/optim/adam.py (L2 weight decay, no amsgrad, no maximize).  All four arrays (n) 16-byte aligned, updated in place.
 *   state: 8 bytes, 8-byte aligned, zero-initialised by the caller once: { float step; uint32 ticket } -- the step count
 *          lives on the device and is incremented by the call itself (the call is replayable inside a hipGraph).
 *   lr_dev: nullable; when given, the learning rate is read from device memory (a scheduler can change it between
 *          replays), otherwise `lr` is used.
 */
int fsg_adam_flat_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, void *state, int64_t n,
                      float lr, const float *lr_dev, float beta1, float beta2, float eps, float weight_decay,
                      fsg_stream_t stream);
/* The same update with the gradient read where autograd left it, one segment per parameter: `count` floats at grad[s] belong
 * at flat offset[s].  The segments tile [0, n) in order; every grad[s] is 16-byte aligned and every count a multiple of 4.
 * The gradients read are also stored into `flat_grad` (n), which afterwards holds their concatenation -- what the caller of
 * fsg_adam_flat_f32 had to build with a copy of its own beforehand.  Same arithmetic per element, same `state`.
 * `segments` is read on the host during the call. */
#define FSG_ADAM_MAX_SEGMENTS 128
typedef struct fsg_adam_segments {
    const float *grad[FSG_ADAM_MAX_SEGMENTS];
    int64_t offset[FSG_ADAM_MAX_SEGMENTS], count[FSG_ADAM_MAX_SEGMENTS];
    int32_t n;
} fsg_adam_segments;
int fsg_adam_flat_segments_f32(float *param, float *flat_grad, float *exp_avg, float *exp_avg_sq, void *state, int64_t n,
                               const fsg_adam_segments *segments, float lr, const float *lr_dev, float beta1, float beta2,
                               float eps, float weight_decay, fsg_stream_t stream);

/*
 * Accumulation step of the test-time ensembling `predict_full_pointcloud` (models/point_seg_net.py:21-48; the loop body
 * `softmax_accumulation[..., perm] += softmax(net(pc[..., perm]))` of :27-29 and :40-44) for R runs at once:
 *   logits (R,B,cls,S) fp32 contiguous -- the net's output for the R subsets, run as one batch of R*B clouds
 *   pts    (R,S) int64 -- the point indices of every run (indices outside [0,n_points) are ignored)
 *   acc    (B,cls,n_points) fp32, updated in place:  acc[b,:,pts[r,s]] += softmax_c(logits[r,b,:,s]),  runs applied in
 *          the order r = 0..R-1 per point (same association as the reference's loop; no float atomics).  When a run
 *          names a point more than once, the highest slot s is the one added (the reference's indexed += also adds one).
 *   cls <= 32.  workspace: fsg_ensemble_accumulate_workspace_bytes(R, n_points), 4-byte aligned.
 */
size_t fsg_ensemble_accumulate_workspace_bytes(int R, int64_t n_points);
int fsg_ensemble_accumulate_f32(const float *logits, int R, int B, int cls, int S, const int64_t *pts, int64_t n_points,
                                float *acc, void *workspace, fsg_stream_t stream);

/*
 * On-device sampling + augmentation, the step in front of the path: data.py:435-460 (random `sample_points` subset of an
 * item) after augmentations.py:52-113 (random rotation / scale / translation of the coordinate rows), one pass:
 *   x (B,C,N) fp32;  sample (B,S) int64 column indices in [0,N), or NULL (then S == N: identity subset);
 *   affine (B,12) fp32 = row-major [A | t] (3 x 4, column-vector form  x' = A x + t) applied to rows 0..2, or NULL;
 *   out (B,C,S):  out[b,0:3,i] = A_b x[b,0:3,sample[b,i]] + t_b,  out[b,3:,i] = x[b,3:,sample[b,i]].
 */
int fsg_sample_transform_f32(const float *x, int B, int C, int64_t N, const int64_t *sample, int S, const float *affine,
                             float *out, fsg_stream_t stream);

/*
 * Shape-model decode + similarity transform, DG-SSM's step behind its backbone: replaces shape_model/ssm.py:74-83
 * (SSM.decode: mean + eigenvectors x weights, vector2shape) and, with v / s / tr, models/dg_ssm.py:133-135
 * (augmentations.py:78-88 compose_transform: so3_exp_map, rotate, scale, translate; :103-113 transform_points) in ONE launch:
 *   w (B,M) mode weights;  mean (3P);  evec (3P,M) row-major;  v, s, tr (B,3) axis-angle rotation, scaling, translation
 *   x[b,p,:]   = mean[p,:] + sum_m evec[3p..3p+2, m] w[b,m]
 *   R_b        = I + a K + b K^2,  K = hat(v_b),  t = sqrt(max(|v_b|^2, 1e-4)),  a = sin t / t,  b = (1 - cos t) / t^2
 *   out[b,p,:] = (x[b,p,:] R_b) * s_b + tr_b            (B,P,3), row-vector convention
 *   v == NULL (then s == tr == NULL): out = x, the decode alone (predict_affine_params=False).
 * _bwd (two launches): grad_out (B,P,3) -> grad_w (B,M), grad_v, grad_s, grad_tr (B,3), all overwritten; x is recomputed;
 *   grad_v is the closed-form derivative of R_b, with t constant where |v_b|^2 < 1e-4 (as torch.clamp makes it); v == NULL:
 *   grad_w only (s and the three small gradients NULL).  mean and evec get no gradient (shape_model/ssm.py:33).  Every sum
 *   over the points runs in a fixed order without atomics.  workspace: the _workspace_bytes query, 4-byte aligned.
 * Limits: P >= 1, B <= 65535, 1 <= M <= FSG_SSM_MAX_MODES (FSG_ERR_UNSUPPORTED above).
 */
#define FSG_SSM_MAX_MODES 64
size_t fsg_ssm_decode_bwd_workspace_bytes(int B, int P, int M);
int fsg_ssm_decode_fwd_f32(const float *w, const float *mean, const float *evec, const float *v, const float *s,
                           const float *tr, int B, int P, int M, float *out, fsg_stream_t stream);
int fsg_ssm_decode_bwd_f32(const float *grad_out, const float *w, const float *mean, const float *evec, const float *v,
                           const float *s, int B, int P, int M, float *grad_w, float *grad_v, float *grad_s, float *grad_tr,
                           void *workspace, size_t workspace_bytes, fsg_stream_t stream);

/*
 * Column sums of a narrow row-major matrix: out[c] = sum_m x[m*C + c], C a power of two <= 32 -- the bias gradient of the
 * last point-wise layer (models/dgcnn.py:146, Conv1d(128, num_classes) with bias) over B*N rows.  One workgroup, fixed
 * summation order.
 */
int fsg_colsum_narrow_f32(const float *x, int64_t M, int C, float *out, fsg_stream_t stream);

/*
 * First layer of a folding MLP (models/folding_net.py:205-221): Conv1d(E + cp, Cout, 1) over cat([code repeated over the m
 * points, pts]) (+ ReLU) with the code part already reduced to per_cloud (B,Cout) = code W[:, :E]^T + bias by the caller:
 *   out[b,i,:] = [relu]( per_cloud[b,:] + sum_{j<cp} pts[b,i,j] * w[:,j] ),   pts (B,m,cp), cp in 1..3, w (Cout,cp) with row
 *   stride ldw (the W[:, E:] slice of the conv weight), out (B,m,Cout) written once.  Cout % 4 == 0, 16-byte aligned rows.
 */
int fsg_fold_layer1_f32(const float *pts, int cp, const float *w, int64_t ldw, const float *per_cloud, int B, int m, int Cout,
                        int relu, float *out, fsg_stream_t stream);

/*
 * Point-wise layers of the DGCNN head on the bf16 matrix pipe with fp32-grade results (csrc/pointwise.hip): replaces the
 * Conv1d(kernel 1) products of models/dgcnn.py:123-137,156-160,282-323.  Every fp32 operand is split into three bf16 pieces
 * (x = h + m + l, exact to 2^-27 |x|) and a product is six v_mfma_f32_32x32x16_bf16 products with fp32 accumulation: as
 * close to real arithmetic as an fp32 fma chain, at 2.7x the rate of the fp32 matrix instruction.
 *
 * fsg_pw_weight_image_f32: the (N, K) matrix W(n, k) = W[n*stride_n + k*stride_k] * scale -> the register image of the MFMA's
 *   B operand (fsg_pw_weight_image_bytes(N, K) bytes; rows and columns padded with zeros).  An image may concatenate several
 *   matrices along k: this call fills k-steps [ks0, ks0 + ceil(K/16)) of an image with KS k-steps per 32-row block.
 * fsg_pw_linear_f32: C (M, N) = A (M, K) W^T (+ bias), A fp32 rows with stride lda (multiple of 4, 16-byte aligned),
 *   K % 32 == 0, W given as its image.  tile: 0 = chosen by shape, 1 = 128x128, 2 = 64x128, 3 = 64x64, 4 = 128x64.
 * fsg_pw_weight_images_f32: up to FSG_PW_MAX_IMAGE_JOBS images in one launch (the weights of a whole head, both orientations).
 */
#define FSG_PW_MAX_IMAGE_JOBS 10
typedef struct fsg_pw_image_jobs {
    const float *W[FSG_PW_MAX_IMAGE_JOBS];
    int64_t stride_n[FSG_PW_MAX_IMAGE_JOBS], stride_k[FSG_PW_MAX_IMAGE_JOBS];
    int N[FSG_PW_MAX_IMAGE_JOBS], K[FSG_PW_MAX_IMAGE_JOBS], ks0[FSG_PW_MAX_IMAGE_JOBS], KS[FSG_PW_MAX_IMAGE_JOBS];
    float scale[FSG_PW_MAX_IMAGE_JOBS];
    void *image[FSG_PW_MAX_IMAGE_JOBS];
    int n;
} fsg_pw_image_jobs;
int fsg_pw_weight_images_f32(const fsg_pw_image_jobs *jobs, fsg_stream_t stream);
size_t fsg_pw_weight_image_bytes(int N, int K);
int fsg_pw_weight_image_f32(const float *W, int64_t stride_n, int64_t stride_k, int N, int K, float scale, int ks0, int KS,
                            void *image, fsg_stream_t stream);
int fsg_pw_linear_f32(const float *A, int64_t lda, const void *image, const float *bias, float *C, int64_t ldc, int M, int N,
                      int K, int tile, fsg_stream_t stream);

/*
 * bf16 operand mode of the same kernels (BASELINE configs 3-5 name bf16; the reference trains under autocast,
 * model_trainer.py:75-76,157): ONE bf16 piece per fp32 operand (round-to-nearest-even), one v_mfma_f32_32x32x16_bf16 product,
 * fp32 accumulation, fp32 storage.  Carries the nn.Linear products of models/pointtransformer/seg_model.py (:25-33, :64-69,
 * :92-99, :128-134, :168-169) when functional.set_mfma_operands("bf16") / an ambient autocast(bfloat16) is on.
 *   fsg_pw_weight_image_bf16: (N, K) weight -> one-piece image of fsg_pw_weight_image_bytes(N, K) / 3 bytes
 *   fsg_pw_linear_bf16:       C (M, N) = bf16(A) bf16(W)^T (+ bias), K % 32 == 0; tile 0 = by shape, 2 = 64 x 128, 3 = 64 x 64
 *   fsg_pw_tn_bf16:           C1 (N1a, N2) = bf16(L1)^T bf16(R) over the M rows (plain single-segment operands of fsg_pw_tn_args),
 *                             tile 2 = 64 x 128, 3 = 64 x 64
 */
int fsg_pw_weight_image_bf16(const float *W, int64_t stride_n, int64_t stride_k, int N, int K, void *image, fsg_stream_t stream);
int fsg_pw_linear_bf16(const float *A, int64_t lda, const void *image, const float *bias, float *C, int64_t ldc, int M, int N,
                       int K, int tile, fsg_stream_t stream);

/*
 * The members of the family behind the fused DGCNN head (`functional.seg_head`; models/dgcnn.py:123-162 of the reference).
 * Tile codes: 1 = 128 x 128, 2 = 64 x 128, 3 = 64 x 64, 4 = 128 x 64, 5 = 64 x 192 (rows x columns of C; 5 only with the BatchNorm-backward prologue + bias epilogue); fsg_pw_tile_rows(tile) = rows.
 *
 * fsg_pw_rowgemm_f32:  C (M, N) = pro(A) (M, K1 + K2) . B,  B given as a weight image with (K1 + K2) / 16 k-steps.
 *   prologue `pro` on segment 1 of A (segment 2 is always plain):
 *     0 none
 *     1 BatchNorm + LeakyReLU of the producing layer:  a = lrelu(alpha[k] A1[m,k] + delta[cloud(m)][k])
 *     2 BatchNorm backward:  a = alpha[k] A1[m,k] f'(alpha[k] Y1[m,k] + delta[cloud][k]) - P[cloud][k] - Q[k] Y1[m,k]
 *       (A1 = gradient w.r.t. the layer's activation, Y1 = its pre-BatchNorm values; P, Q from fsg_pw_bnbwd_finalize_f32)
 *     per-cloud tables have `tstride` floats between clouds (0: one row for all), cloud(m) = m / rows_per_cloud
 *   epilogue `epi` = OR of
 *     1  STORE     columns >= store_n0 go to C[m * ldc + n - store_n0]
 *     2  STATS     rec (M / rows, 3, N): (n, mean, M2) of every column over the tile's rows (train-mode BatchNorm statistics)
 *     4  SEL       columns < sel_n: sel_val (M / rows, sel_n) = max over the tile's rows of sgn[n] * c, sel_arg = its row inside
 *                  the cloud, lowest row on ties (the global max-pool through the monotone BatchNorm + LeakyReLU)
 *     8  BWDSTATS  rec2 (M / rows, 2, N): sums over the tile's rows of h = c f'(ealpha Yp + edelta[cloud]) and
 *                  h (Yp - emu[cloud]) er  (BatchNorm backward sums of the layer whose activation gradient C is)
 *     16 BIAS      bias[n] added on the way out (with STORE)
 *   K1, K2 multiples of 32; A rows 16-byte aligned with strides that are multiples of 4; reducing epilogues need M and
 *   rows_per_cloud to be multiples of the tile's rows.  Only the combinations the head uses are instantiated
 *   (FSG_ERR_UNSUPPORTED otherwise).
 */
#define FSG_PW_PRO_NONE 0 /* the prologue codes `pro` above */
#define FSG_PW_PRO_BNACT 1
#define FSG_PW_PRO_BNBWD 2
#define FSG_PW_STORE 1 /* the epilogue bits `epi` above */
#define FSG_PW_STATS 2
#define FSG_PW_SEL 4
#define FSG_PW_BWDSTATS 8
#define FSG_PW_BIAS 16
typedef struct fsg_pw_rowgemm_args {
    const float *A1, *Y1, *A2;
    int64_t lda1, lda2;
    int K1, K2;
    const void *Bimg;
    int M, N, rows_per_cloud;
    const float *alpha, *delta, *P, *Q;
    int tstride;
    float slope;
    float *C;
    int64_t ldc;
    int store_n0;
    const float *bias;
    float *rec;
    const float *sgn;
    float *sel_val;
    int32_t *sel_arg;
    int sel_n;
    const float *Yp;
    int64_t ldyp;
    const float *ealpha, *edelta, *emu, *er;
    int etstride;
    float *rec2;
} fsg_pw_rowgemm_args;
int fsg_pw_tile_rows(int tile);
int fsg_pw_rowgemm_f32(const fsg_pw_rowgemm_args *args, int pro, int epi, int tile, fsg_stream_t stream);

/*
 * fsg_pw_tn_f32:  [C1 ; C2] (N1a + N1b, N2) = sum_m L'(m, :)^T R'(m, :)  -- weight gradients dW = dy^T a and the Gram matrix
 *   of the global-feature backward; contraction over the M rows, split into slices of rows_per_slice rows (multiple of 32)
 *   whose partial products are summed in slice order (reproducible).  Left operand = [segment 1 | segment 2]: segment 1
 *   (N1a columns) with prologue lpro = 0 or 2 (as above: L1 = gradient, LY1 = pre-BatchNorm values), segment 2 (N1b columns,
 *   N1a % 64 == 0 then) plain; right operand (N2 columns) with rpro = 0 or 1.  Rows of the result below N1a go to C1, the
 *   others to C2.  tile: 1 = 128 x 128, 2 = 64 x 128, 3 = 64 x 64, 5 = 128 x 192 (N1 x N2).  workspace:
 *   fsg_pw_tn_workspace_bytes(N1a + N1b, N2, M, rows_per_slice) bytes.
 *   C1 == NULL: the slices are left in the workspace, to be folded later by fsg_pw_tn_reduce_f32 -- the reductions of several
 *   products in ONE launch (job j: S = ceil(M / rows_per_slice) slices of (N1, N2) in workspace[j]; rows < N1a -> C1, others -> C2).
 */
typedef struct fsg_pw_tn_args {
    const float *L1, *LY1, *L2;
    int64_t ldl1, ldl2;
    int N1a, N1b, lpro;
    const float *lalpha, *ldelta, *lP, *lQ;
    int lts;
    const float *R;
    int64_t ldr;
    int N2, rpro;
    const float *ralpha, *rdelta;
    int rts;
    float slope;
    int M, rows_per_cloud, rows_per_slice;
    int ones;      /* 1: one more left column (behind segment 2) that is all ones: result row N1a + N1b = column sums of R' */
} fsg_pw_tn_args;
#define FSG_PW_MAX_REDUCE_JOBS 6
typedef struct fsg_pw_tn_reduce_jobs {
    const void *workspace[FSG_PW_MAX_REDUCE_JOBS];
    float *C1[FSG_PW_MAX_REDUCE_JOBS], *C2[FSG_PW_MAX_REDUCE_JOBS];
    int64_t ldc1[FSG_PW_MAX_REDUCE_JOBS], ldc2[FSG_PW_MAX_REDUCE_JOBS];
    int S[FSG_PW_MAX_REDUCE_JOBS], N1[FSG_PW_MAX_REDUCE_JOBS], N2[FSG_PW_MAX_REDUCE_JOBS], N1a[FSG_PW_MAX_REDUCE_JOBS];
    int n;
} fsg_pw_tn_reduce_jobs;
int fsg_pw_tn_reduce_f32(const fsg_pw_tn_reduce_jobs *jobs, fsg_stream_t stream);
size_t fsg_pw_tn_workspace_bytes(int N1, int N2, int M, int rows_per_slice);
int fsg_pw_tn_f32(const fsg_pw_tn_args *args, int tile, void *workspace, size_t workspace_bytes, float *C1, int64_t ldc1,
                  float *C2, int64_t ldc2, fsg_stream_t stream);
int fsg_pw_tn_bf16(const fsg_pw_tn_args *args, int tile, void *workspace, size_t workspace_bytes, float *C1, int64_t ldc1,
                   fsg_stream_t stream);

/*
 * fsg_pw_bn_finalize_f32: STATS records (R, 3, ldn), columns [c0, c0 + C) -> train-mode BatchNorm statistics (Chan's merge in
 *   fp64; `shift` (B, C) or NULL is added to the mean of every record of its cloud: y = y0 + shift[cloud]), torch's running
 *   update (unbiased variance), and the tables of the consumers: alpha = gamma invstd, delta (B or 1, C) = alpha (shift - mean)
 *   + beta, emu (B or 1, C) = mean - shift (nullable), cloud_mean (B, C) = unshifted per-cloud mean (nullable).
 *   training == 0: mean / invstd are inputs (running statistics), only the tables are written.
 *   gfeat (B, CG) != NULL: the shift is computed in the kernel first, shift[b][c] = sum_j gfeat[b][j] Wglob[c * ldwg + j] (the
 *   per-cloud constant of the first head layer, models/dgcnn.py:159-160), and written to shift_out == shift (B <= 64).
 * fsg_pw_cloud_linear_f32: out (B, C0) = x (B, CG) W^T, W (C0, CG) with row stride ldw -- the per-cloud constant of the first head
 *   layer (its global-feature block times the max-pooled feature, models/dgcnn.py:159-160); one wave per output.
 * fsg_pw_max_finish_f32: SEL records (B * tiles, C) -> out (B, C) = lrelu(alpha ysel + delta), ysel, arg (row inside the cloud).
 * fsg_pw_bnbwd_finalize_f32: BWDSTATS records (R, 2, C) -> dbeta, dgamma, P (B or 1, C), Q (C) of prologue 2, and (first head
 *   layer, dc != NULL) dc (B, C) = per-cloud column sums of dy = the gradient of the per-cloud constant.
 * fsg_pw_logits_bwd_f32: last layer (Conv1d(C, classes) + bias): da (M, C) = g (M, classes) W3, stored, + BWDSTATS records
 *   (ceil(M / 32), 2, C) of the BatchNorm in front of it.
 */
int fsg_pw_bn_finalize_f32(const float *rec, int R, int ldn, int c0, int C, const float *shift, int B, int training,
                           const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                           float *running_var, float *mean, float *invstd, float *alpha, float *delta, float *emu,
                           float *cloud_mean, const float *gfeat, const float *Wglob, int64_t ldwg, int CG, float *shift_out,
                           fsg_stream_t stream);
int fsg_pw_cloud_linear_f32(const float *x, const float *W, int64_t ldw, int B, int C0, int CG, float *out, fsg_stream_t stream);
int fsg_pw_max_finish_f32(const float *sel_val, const int32_t *sel_arg, const float *sgn, const float *alpha, const float *delta,
                          int B, int tiles, int C, float slope, float *out, float *ysel, int32_t *arg, fsg_stream_t stream);
/* fsg_pw_bn_finalize_f32 (no per-cloud shift) and fsg_pw_max_finish_f32 as ONE launch: the statistics of the BatchNorm in front
 * of the global max-pool and the pool's finish from the SEL records of the same product (models/dgcnn.py:134-137,156); B <= 64. */
int fsg_pw_bn_finalize_max_f32(const float *rec, int R, int ldn, int c0, int C, int B, int training, const float *gamma,
                               const float *beta, float eps, float momentum, float *running_mean, float *running_var, float *mean,
                               float *invstd, float *alpha, float *delta, const float *sel_val, const int32_t *sel_arg,
                               const float *sgn, int tiles, float slope, float *out, float *ysel, int32_t *arg, fsg_stream_t stream);

int fsg_pw_bnbwd_finalize_f32(const float *rec2, int R, int C, int B, int64_t M, int training, const float *alpha,
                              const float *invstd, const float *emu, int emu_per_cloud, const float *cloud_mean, float *dbeta,
                              float *dgamma, float *P, float *Q, float *dc, fsg_stream_t stream);
int fsg_pw_logits_bwd_f32(const float *g, int classes, const float *W3, const float *y, const float *alpha, const float *delta,
                          const float *mean, const float *invstd, int64_t M, int C, float slope, float *da, float *rec2,
                          fsg_stream_t stream);

/*
 * Global-feature layer, backward in its Gram form (the (M, 1024) activation gradient is never formed): after the max over the
 * points only B * C entries of dY are "selected", the BatchNorm terms are affine in y = X W^T, so with G = X^T X, s = sum_m X_m:
 *   dX = selected rows - 1 (W^T P)^T - X (W^T diag(Q) W),   dW = selected rows - P s^T - diag(Q) W G.
 * fsg_pw_gf_prep_f32: per channel dbeta, dgamma, P, Q and coef (B, C) = weight of the selected row in dy.  The gradient of the
 *   global feature is either given (dg (B, C), dc == NULL) or formed here from the gradient dc (B, C0) of the first head layer's
 *   per-cloud constant: dg = dc W0g (W0g (C0, C), row stride ldw0), together with dW0g (C0, C) = dc^T gfeat (B <= 32).
 *   Wq != NULL: also the rows [Q[c] W[c, :] | -P[c]] (C, K + 1) with row stride ldwq -- the left operand of the row contraction
 *   [M1 ; npvec] = [Q o W | -P]^T W (fsg_pw_tn_f32 over the C channel rows).
 * fsg_pw_scatter_rows_f32: dX[b Npts + arg[b,c], :] += coef[b,c] W[c, :], summed per destination row in channel order
 *   (C <= 4096; workspace fsg_pw_scatter_rows_workspace_bytes(B, C) bytes for the sorted selection keys).
 * fsg_pw_gf_dw_f32: dW[c, :] = sum_b coef[b,c] X[b Npts + arg[b,c], :] - P[c] s - Q[c] (W G)[c, :]  (G (K, K) contiguous).
 *   (s = column sums of X and G come out of ONE row contraction: fsg_pw_tn_f32 with `ones` = 1.)
 */
int fsg_pw_gf_prep_f32(const float *dc, const float *W0g, int64_t ldw0, int C0, const float *gfeat, float *dW0g, int64_t lddw0,
                       const float *dg, const float *ysel, const float *alpha, const float *delta, const float *mean,
                       const float *invstd, int B, int C, int64_t M, int training, float slope, float *dbeta, float *dgamma,
                       float *P, float *Q, float *coef, const float *W, int64_t ldw, int K, float *Wq, int64_t ldwq,
                       fsg_stream_t stream);
size_t fsg_pw_scatter_rows_workspace_bytes(int B, int C);
int fsg_pw_scatter_rows_f32(const float *coef, const int32_t *arg, const float *W, int64_t ldw, int B, int C, int K, int Npts,
                            float *dX, int64_t ldx, void *workspace, fsg_stream_t stream);
int fsg_pw_gf_dw_f32(const float *coef, const int32_t *arg, const float *X, int64_t ldx, const float *s, const float *W,
                     int64_t ldw, const float *G, const float *P, const float *Q, int B, int C, int K, int Npts, float *dW,
                     int64_t lddw, fsg_stream_t stream);

/*
 * The tail of the head's backward with four launches folded into their neighbours.  Every entry computes what the sequence it
 * replaces computes, BIT FOR BIT (same operations, same order; tests/test_pw_tail_gpu.py compares with torch.equal):
 * fsg_pw_logits_bwd_bias_f32 = fsg_pw_logits_bwd_f32 + fsg_colsum_narrow_f32(g, M, classes) -> db, one more workgroup of the
 *   same launch (classes a power of two).
 * fsg_pw_gf_prep_sort_f32 = fsg_pw_gf_prep_f32 (dc form) + the key sort of fsg_pw_scatter_rows_f32 in the second launch
 *   (512 < C <= 1024): sorted (B, 1024) keys (arg << 12 | channel) ascending, padded with 0xFFFFFFFF -- what that entry leaves
 *   in its workspace -- and first (B, Npts / 64 + 1): first[b][t] = number of channels of cloud b with arg < 64 t.
 * fsg_pw_tn_reduce_image_f32 = the fold of fsg_pw_tn_f32 (called with C1 == NULL: slices left in `workspace`, S of them, N1 x N2
 *   each) + fsg_pw_weight_image_f32(rows < NI as an (NI, N2) matrix, scale, ks0, KS) -> image; rows [NI, N1) -> C2 (fp32).
 * fsg_pw_rowgemm_scatter_f32 = fsg_pw_rowgemm_f32(PRO_BNBWD, PW_STORE | PW_BIAS, tile 5) + fsg_pw_scatter_rows_f32 on its output
 *   (K = N <= 192, Npts = rows_per_cloud, a multiple of 64 that divides M; sorted / first from fsg_pw_gf_prep_sort_f32): the
 *   workgroup that owns 64 rows adds their selected sums before it stores them.  A tile walks its own entries alone: up to C
 *   of them when every channel of a cloud selects rows of one tile.
 */
int fsg_pw_logits_bwd_bias_f32(const float *g, int classes, const float *W3, const float *y, const float *alpha,
                               const float *delta, const float *mean, const float *invstd, int64_t M, int C, float slope,
                               float *da, float *rec2, float *db, fsg_stream_t stream);
int fsg_pw_gf_prep_sort_f32(const float *dc, const float *W0g, int64_t ldw0, int C0, const float *gfeat, float *dW0g, int64_t lddw0,
                            const float *ysel, const float *alpha, const float *delta, const float *mean, const float *invstd,
                            int B, int C, int64_t M, int training, float slope, float *dbeta, float *dgamma, float *P, float *Q,
                            float *coef, const float *W, int64_t ldw, int K, float *Wq, int64_t ldwq, const int32_t *arg, int Npts,
                            void *sorted, int32_t *first, fsg_stream_t stream);
int fsg_pw_tn_reduce_image_f32(const void *workspace, int S, int N1, int N2, int NI, float scale, int ks0, int KS, void *image,
                               float *C2, int64_t ldc2, fsg_stream_t stream);
int fsg_pw_rowgemm_scatter_f32(const fsg_pw_rowgemm_args *args, const void *sorted, const int32_t *first, const float *coef,
                               const float *W, int64_t ldw, int C, fsg_stream_t stream);

/*
 * Image front end on single-channel fp32 volumes (B, D, H, W), contiguous: Foerstner keypoints
 * (data_processing/foerstner.py:62-108) and MIND descriptors (data_processing/point_features.py:86-150).  Everything here is
 * an evaluation primitive, not differentiable.  `weights` (HOST, N odd <= 9 floats) are the taps of utils/image_utils.py:
 * smooth; the host computes them the way the reference does and the kernels apply them along axes 0, 1, 2 with replicate
 * padding.  All intermediate volumes of the torch composition (gradients, products, squared differences, partially smoothed
 * channels) live in LDS only.
 *
 * Distinctiveness: out (B, D, H, W) = 1 / trace(inverse(smoothed structure tensor of the 5-tap central-difference gradient)),
 *   in the reference's operation order; NaN where the tensor is singular (constant regions), exactly like the reference.
 *
 * Non-maximum suppression: window maximum of utils/image_utils.py: nms over [i - (d - d/2 - 1), i + d/2] per axis (even d is
 *   asymmetric), replicate padding, NaN propagates through the window.  maxout (B, D, H, W) fp32 or NULL; flags (B, D, H, W)
 *   bytes or NULL: flags = eroded(mask) & (max == dist) & (dist >= thresh), where a voxel survives the erosion iff its six face
 *   neighbours inside the volume are all set in `mask` (bytes, NULL = all set) -- the voxel's OWN mask value does not count
 *   (foerstner.py:93-104).  d <= 13.
 *
 * MIND: `shifts` (HOST, nch x 2 x 3 ints in {-1, 0, 1}) are the two voxels of every channel's pair, scaled by `dilation`
 *   (1..4).  box != 0 selects the general form the reference's ssc = False kernels need (point_features.py:129-132):
 *   `shifts` is then nch x 2 ints, each a 27-bit subset of the dilated 3 x 3 x 3 stencil (bit (kz * 3 + ky) * 3 + kx), and
 *   the two operands of a channel are the sums over their subsets.  nch is 6 or 12.  `outch` (HOST, nch ints) is the output position of
 *   channel c.  The statistics pass writes mean (DEVICE, 1 float) = mean over all voxels of mean_c(ssd_c - min_c ssd_c),
 *   reduced in a fixed order through `workspace` (fsg_mind_stats_workspace_bytes) -- deterministic, no float atomics, no
 *   feature volume.  The evaluation passes read it and write exp(-(ssd - min) / clamp(mean_c, 0.001 mean, 1000 mean)) for
 *   the whole volume (out (B, nch, D, H, W)) or for K voxels kp (K, 3) int64 (z, y, x) of ONE volume (out (nch, K));
 *   coordinates outside the volume are clamped).  Both run the same code, so the values are bitwise equal.
 */
#define FSG_FRONTEND_MAX_TAP_RADIUS 4 /* `weights`: N <= 2 * 4 + 1 taps */
int fsg_foerstner_dist_f32(const float *img, int B, int D, int H, int W, const float *weights, int N, float *out,
                           fsg_stream_t stream);
int fsg_nms_keypoints(const float *dist, const uint8_t *mask, int B, int D, int H, int W, int d, float thresh, float *maxout,
                      uint8_t *flags, fsg_stream_t stream);
size_t fsg_mind_stats_workspace_bytes(int B, int D, int H, int W);
int fsg_mind_stats_f32(const float *img, int B, int D, int H, int W, int dilation, int nch, int box, const int *shifts,
                       const float *weights, int N, void *workspace, float *mean, fsg_stream_t stream);
int fsg_mind_eval_f32(const float *img, int B, int D, int H, int W, int dilation, int nch, int box, const int *shifts,
                      const int *outch, const float *weights, int N, const float *mean, float *out, fsg_stream_t stream);
int fsg_mind_eval_kp_f32(const float *img, int D, int H, int W, int dilation, int nch, int box, const int *shifts,
                         const int *outch, const float *weights, int N, const float *mean, const int64_t *kp, int K, float *out,
                         fsg_stream_t stream);

/* Hessian fissure enhancement and its keypoint candidates (csrc/fissure_enhance.hip).  Volumes are (B, 1, D, H, W) fp32,
 * DEVICE; tap vectors are HOST pointers.
 *
 * fsg_fissure_enhance_f32 replaces HessianEnhancementFilter.forward + fissure_filter of the reference
 *   (data_processing/fissure_enhancement.py:47-99, 149-180) and, with `mask`, the lung-mask product of
 *   get_enhanced_fissure_image (:213-214).  k1 / k2 (N taps each, N odd, 3..9) are the first- and second-derivative
 *   Gaussian taps of utils/image_utils.py:53-58 in fp32; k1 must be antisymmetric and k2 symmetric, bit for bit.  Per voxel:
 *   H[a][a] = k2 along axis a, H[a][b] = k1 along a then k1 along b (a < b), replicate padding; the eigenvalues sorted by
 *   absolute value, descending; P = (|l1| - |l2|) / (|l1| + |l2|) where l1 < 0, else 0; out = exp(-(img - mu)^2 /
 *   (2 sigma_hu^2)) * P, times (mask != 0) when mask (bytes) is given.  planeness / hu_weight (NULL or DEVICE, the shape of
 *   out) receive P and the HU weight (return_intermediate).  Where the (2R + 1)^3 support of a voxel is constant, out and P
 *   are exactly 0.  No intermediate volume is written.
 *
 * fsg_smooth_threshold_f32 is the dense part of get_hessian_fissure_enhancement_kpts (data_processing/
 *   keypoint_extraction.py:134-141): separable smoothing with per-axis taps wz, wy, wx (odd counts, at most 9; axis order
 *   0, 1, 2; replicate padding), then out = s > thresh ? s : 0 and flags (bytes) = s > thresh.  Either output may be NULL.
 */
#define FSG_ENHANCE_MAX_TAP_RADIUS 4 /* k1 / k2 and wz / wy / wx: at most 2 * 4 + 1 taps each (derivation sigma <= 1) */
int fsg_fissure_enhance_f32(const float *img, const uint8_t *mask, int B, int D, int H, int W, const float *k1, const float *k2,
                            int N, float mu, float sigma_hu, float *out, float *planeness, float *hu_weight,
                            fsg_stream_t stream);
int fsg_smooth_threshold_f32(const float *vol, int B, int D, int H, int W, const float *wz, int Nz, const float *wy, int Ny,
                             const float *wx, int Nx, float thresh, float *out, uint8_t *flags, fsg_stream_t stream);

/* Coherent point drift, E-step without the (M, N) responsibility matrix (csrc/cpd.hip).  Serves the pycpd registrations of the
 * reference, shape_model/point_cloud_registration.py:101-116,231-232 (register_cpd_deformable and the joint rigid
 * pre-registration), whose expectation step is dense numpy on the CPU, one case at a time.
 *   X (N, 3) fixed points of item b at X + b * x_batch_stride floats (0: one cloud shared by the batch); TY (B, M, 3) the
 *   transformed moving points; sigma2 (B) DEVICE, > 0; w in [0, 1) the outlier weight.  All fp32, contiguous rows.
 *   P[m,n] = exp(-|x_n - ty_m|^2 / 2 sigma2) / (sum_m' exp(-|x_n - ty_m'|^2 / 2 sigma2) + c),
 *   c = (2 pi sigma2)^(3/2) * w / (1 - w) * M / N, evaluated relative to every column's smallest distance (no underflow of a
 *   column sum; where the rescaled c overflows, the column is 0).  Distances are sums of squared differences.
 *   P1 (B, M) = sum_n P, Pt1 (B, N) = sum_m P, PX (B, M, 3) = sum_n P x_n, Np (B) = sum_mn P (added up over Pt1).
 * Two launches, no atomics: the same inputs give the same bits, and an item's outputs do not depend on the rest of the batch.
 * The exponentials are fp32; distances, exponents and sums are carried in fp64.  Any N, M >= 1.  workspace:
 * fsg_cpd_estep_workspace_bytes(B, N, M) bytes (16 N per item), 8-byte aligned. */
size_t fsg_cpd_estep_workspace_bytes(int B, int N, int M);
int fsg_cpd_estep_f32(const float *X, int64_t x_batch_stride, const float *TY, const float *sigma2, float w, int B, int N, int M,
                      float *P1, float *Pt1, float *PX, float *Np, void *workspace, size_t workspace_bytes,
                      fsg_stream_t stream);

/* Lloyd's k-means on 3-D points, batched and bit-reproducible (csrc/kmeans.hip).  Serves the 'kmeans' mode of the reference's
 * data_set_correspondences, shape_model/generate_corresponding_points.py:44-48, which pools the registered clouds of all
 * instances of one object and calls sklearn.cluster.k_means on the CPU, one object at a time.  B independent items:
 *   points (B, n, 3) fp32, centroids (B, K, 3) fp32, labels (B, n) int32, all DEVICE and contiguous; coordinates finite.
 *   1 <= K <= min(n, 4096), n <= 2^24, B <= 65535.  workspace: fsg_kmeans_workspace_bytes(B, n, K) bytes, 8-byte aligned; it
 *   carries a run (accumulators, scales, threshold, active flag, iteration count per item) from `prepare` through the steps.
 * prepare  once per run: the fixed-point scales of every item from its largest |coordinate| over points and centroids, the
 *   stopping threshold tol * (mean over the three axes of the variance of the item's points) (sklearn's rule), zeroed
 *   accumulators, every item active with iteration count 0.
 * step     one iteration, two launches, nothing read on the host.  Assign: label = argmin_k ((dx dx + dy dy) + dz dz) in fp32
 *   in that order, the lowest k on ties; coordinates and squared distances are summed per cluster as int64 fixed-point numbers
 *   (so the sums do not depend on any order, nor on the rest of the batch).  Finalize: centroid = sum / count in fp64 rounded
 *   to fp32, written over `centroids`; an empty cluster keeps its centroid (scipy.cluster.vq.kmeans2's rule, not sklearn's
 *   relocation); an item stops when no label differs from the `labels` it found (-1 everywhere before the first step) or when
 *   the summed squared centroid shift is <= its threshold.  A stopped item is frozen: later steps leave its centroids, labels,
 *   outputs and iteration count alone.
 * assign   labels, counts and inertia OF the given centroids for every item, frozen or not; centroids are not written.
 * Outputs of step and assign, each may be NULL: counts (B, K) int32; stats (B, 2) fp64 = inertia (the sum of the squared
 *   distances of this assignment), squared centroid shift; info (B, 4) int32 = labels changed, empty clusters, iterations
 *   run, active. */
#define FSG_KMEANS_MAX_K 4096           /* K: the accumulators of the clusters live in LDS */
#define FSG_KMEANS_MAX_POINTS (1 << 24) /* n: the index range of a point */
size_t fsg_kmeans_workspace_bytes(int B, int n, int K);
int fsg_kmeans_prepare_f32(const float *points, const float *centroids, int B, int n, int K, double tol, void *workspace,
                           size_t workspace_bytes, fsg_stream_t stream);
int fsg_kmeans_step_f32(const float *points, float *centroids, int32_t *labels, int B, int n, int K, void *workspace,
                        size_t workspace_bytes, int32_t *counts, double *stats, int32_t *info, fsg_stream_t stream);
int fsg_kmeans_assign_f32(const float *points, const float *centroids, int32_t *labels, int B, int n, int K, void *workspace,
                          size_t workspace_bytes, int32_t *counts, double *stats, int32_t *info, fsg_stream_t stream);

/* OPTICS reachability ordering (Ankerst et al., SIGMOD 1999) on 3-D points, batched and bit-reproducible (csrc/optics.hip).
 * Serves the 'cluster' mode of the reference's data_set_correspondences, shape_model/generate_corresponding_points.py:50-62,
 * which runs sklearn.cluster.OPTICS on the pooled clouds of one object at a time on the CPU.  B independent items:
 *   points (B, n, 3) fp32, max_eps (B) fp64 (each > 0 or +inf), ordering (B, n) int32, core2 / reach2 (B, n) fp64, pred (B, n)
 *   int32, all DEVICE and contiguous; coordinates finite (not checked: the loop count is n whatever the data, and every cell
 *   index is clamped into its table).  2 <= min_samples <= min(n, 64), n <= 262144, B <= 65535.  workspace:
 *   fsg_optics_workspace_bytes(B, n, min_samples) bytes (37120 + 44 n per item, rounded up to 16), 16-byte aligned.  NULL
 *   pointers, bad shapes and a short or misaligned workspace are FSG_ERR_ARG before any launch.
 * The rule (ours; sklearn's without its np.around(.., 15) and on squared distances):
 *   d2(i, j) = ((dx dx + dy dy) + dz dz) in fp64 in that order, dx = (double) x_i - (double) x_j; e2 = eps eps in fp64;
 *   N(i) = { j : d2(i, j) <= e2 }, i included; core2(i) = the min_samples-th smallest d2 over N(i) (i itself is the first, 0),
 *   +inf if N(i) is smaller.  reach2 = +inf, pred = -1; n times: p = the unprocessed point with the smallest (reach2, index),
 *   the LOWEST index on ties, +inf included; p is appended to `ordering`; if core2(p) < inf every unprocessed q in N(p) with
 *   v = max(core2(p), d2(p, q)) < reach2(q) gets reach2(q) = v, pred(q) = p.
 * core2, reach2 and pred are indexed by point; they are the SQUARES (no device square root takes part).  Three launches (cell
 * grid and stable sort; core distances; one workgroup per item for the ordering), no atomics, nothing read on the host,
 * capturable in a graph; the same inputs give the same bits on every run, alone or in a batch.  The cell grid only restricts
 * the pairs that are looked at; no result depends on it. */
#define FSG_OPTICS_MAX_POINTS 262144    /* n: 16 bytes of LDS per 64 points beside the 37 KiB cell table (static_assert) */
#define FSG_OPTICS_MAX_MIN_SAMPLES 64   /* the core distance takes min_samples passes over the neighbourhood; I // 16 <= 64 */
size_t fsg_optics_workspace_bytes(int B, int n, int min_samples);
int fsg_optics_f32(const float *points, const double *max_eps, int B, int n, int min_samples, int32_t *ordering, double *core2,
                   double *reach2, int32_t *pred, void *workspace, size_t workspace_bytes, fsg_stream_t stream);

/* Weighted sample elimination (Yuksel, "Sample Elimination for Generating Poisson Disk Sample Sets", 2015), batched and
 * bit-reproducible (csrc/poisson_disk.hip).  Serves TriangleMesh.sample_points_poisson_disk, which the reference takes from
 * open3d on the host, one mesh at a time (shape_model/point_cloud_registration.py:224, :338).  B independent items:
 *   points (B, M, 3) fp32, radii (B, 2) fp32 = (R, r_min) per item, keep (B, n_keep) int32, order (B, M - n_keep) int32 or
 *   NULL, all DEVICE and contiguous; coordinates finite.  1 <= n_keep <= M <= 16384 (FSG_ERR_UNSUPPORTED above: the weights of
 *   an item live in LDS), B <= 65535.  workspace: fsg_sample_elimination_workspace_bytes(B, M) bytes (8 M per item), 8-byte
 *   aligned.  NULL pointers, bad shapes and a short or misaligned workspace are FSG_ERR_ARG before any launch.
 * The rule (ours, not open3d's loop):
 *   pair    d2 = ((dx dx + dy dy) + dz dz) in fp32 in that order; samples i != j are neighbours iff R > 0 and d2 < R R (the
 *     fp32 product); d = fmaxf(sqrtf(d2), r_min), t = fmaxf(1 - d / R, 0), w = ((t t)^2)^2 (alpha = 8 by three fp32
 *     squarings), q = rintf(w 2^24) as an integer.  Exact duplicates are neighbours with d = r_min.  The clamp of t acts only
 *     for r_min > R.
 *   weight  of a sample = the int64 sum of q over its alive neighbours: no summation order, tiling or batch neighbour can
 *     change it, and the subtractions below are exact.
 *   round   M - n_keep times: remove the alive sample with the largest weight, the LOWEST index on ties, and subtract
 *     q(removed, j) from every alive neighbour j.  R <= 0 (or NaN), or no neighbours anywhere: all weights are 0 and the
 *     removal runs in index order; that is defined behaviour.
 * keep receives the surviving indices in ASCENDING order (survivors keep their sample order), order the removal sequence.
 * n_keep == M writes 0 .. M-1 and removes nothing.  Two launches (weights over (item, tile); one workgroup per item for the
 * rounds), no atomics, nothing read on the host, capturable in a graph; the same inputs give the same bits on every run,
 * alone or in a batch. */
#define FSG_SAMPLE_ELIMINATION_MAX_POINTS 16384 /* M: 14 index bits in the selection key, the weights of one item fill LDS */
size_t fsg_sample_elimination_workspace_bytes(int B, int M);
int fsg_sample_elimination_f32(const float *points, const float *radii, int B, int M, int n_keep, int32_t *keep, int32_t *order,
                               void *workspace, size_t workspace_bytes, fsg_stream_t stream);

/* Random-walker lobe filling and lobes-to-fissures (csrc/random_walk.hip).  Volumes are (B, D, H, W), DEVICE, contiguous.
 *
 * The graph of compute_laplace_matrix (data_processing/random_walk.py:15-77) is never a matrix: nodes are the voxels, edges
 *   the axis neighbours inside the volume (no wrap), w_ij = (im_i == im_j ? 1 : 0.01) for FSG_RW_BINARY (im: bytes) or
 *   exp(-(im_i - im_j)^2 / (2 * 8^2)) for FSG_RW_INTENSITY (im: fp32), L = diag(1e-5 + sum_j w_ij) - W.  The degree counts
 *   every in-volume neighbour, masked or seeded alike (:70-75).
 * The solve is random_walk (:80-116): seeded = label != 0 inside the mask (mask NULL: every voxel is inside), unknown = the
 *   rest of the mask, system k has the right-hand side b_i = sum of w_ij over seeded in-mask neighbours j of label k + 1.  A
 *   label outside 0..K seeds no system (it absorbs with value 0).  Instead of the reference's pyamg hierarchy (:309-321) the
 *   B K systems run Jacobi-preconditioned conjugate gradients together from x = 0: `prep` writes the state byte, the inverse
 *   diagonal, r = b and the first reductions (two launches); `iterate` enqueues `iterations` iterations numbered from
 *   `first_iteration` (the caller counts; three launches each: stencil, update, one workgroup per system for the scalars).
 *   A system stops once |r| <= tol |b| on the recurrence's r: stop_iter[b K + k] (DEVICE, int32) then holds the number of
 *   iterations it took (-1 while it runs, 0 for an all-zero right-hand side) and its x is final -- later iterations skip it,
 *   so its result does not depend on the rest of the batch.  relres (DEVICE, fp32, per system) = |r| / |b| after the last
 *   iteration the system took part in.  The host decides when to look (the wrapper does every 25 iterations).
 *   `finish` writes prob (B, D, H, W, K) fp32 (one-hot rows at seeds, x at unknowns, 0 outside the mask; may be NULL) and
 *   filled (bytes; may be NULL) = first-index argmax + 1 inside the mask, 0 outside: fill_lobes (data_processing/
 *   find_lobes.py:17-30), where a voxel whose probabilities are all 0 becomes label 1.
 * K is 1..8.  Reductions are fp64 partials summed in a fixed order, no atomics: the same input gives the same bits.
 * workspace: the query below, 8-byte aligned, owned by the caller from prep to finish; it holds five (B, K, D, H, W) fp32
 *   vectors, 5 bytes per voxel of state and the partial sums.  Too small a workspace is FSG_ERR_ARG.
 *
 * fsg_lobes_to_fissures_u8 is the tensor part of lobes_to_fissures (find_lobes.py:47-88) on labels, without the one-hot
 *   volume: a label counts as present at a voxel if the voxel or one of its six in-volume neighbours carries it; fissure 1
 *   where 3 and 4 are present, overwritten by 2 where 1 and 2 (n_lobes == 5: or 1 and 5) are, overwritten by 3 where 2 and 5
 *   are (n_lobes == 5 only).  n_lobes is the largest label of the volume, at least 4 (the reference fails on an index below).
 */
#define FSG_RW_BINARY 0
#define FSG_RW_INTENSITY 1
#define FSG_RW_MAX_LABELS 8 /* K */
size_t fsg_random_walk_workspace_bytes(int B, int K, int D, int H, int W);
int fsg_random_walk_prep(const void *im, int mode, const void *labels, int labels_are_i32, const uint8_t *mask, int B, int K, int D,
                         int H, int W, void *workspace, size_t workspace_bytes, int32_t *stop_iter, float *relres,
                         fsg_stream_t stream);
int fsg_random_walk_iterate(const void *im, int mode, int B, int K, int D, int H, int W, int first_iteration, int iterations,
                            float tol, void *workspace, size_t workspace_bytes, int32_t *stop_iter, float *relres,
                            fsg_stream_t stream);
int fsg_random_walk_finish(int B, int K, int D, int H, int W, const void *workspace, size_t workspace_bytes, float *prob,
                           uint8_t *filled, fsg_stream_t stream);
int fsg_lobes_to_fissures_u8(const uint8_t *lobes, int B, int D, int H, int W, int n_lobes, uint8_t *fissures,
                             fsg_stream_t stream);

/* Binary morphology with ball structuring elements, connected components and component statistics on bit planes
 * (csrc/morphology.hip).  Replaces the SimpleITK filters of find_lobes (data_processing/find_lobes.py:114-158: BinaryErode,
 * BinaryDilate, BinaryMorphologicalClosing, BinaryMorphologicalOpening, ConnectedComponentImageFilter,
 * RelabelComponentImageFilter, LabelShapeStatisticsImageFilter) and of multiple_objects_morphology (utils/image_ops.py:31-47:
 * DilateObjectMorphology, ErodeObjectMorphology).  Volumes are (B, D, H, W), DEVICE, contiguous.
 *
 * A bit plane of a binary volume is (B, D, H, WW) 64-bit words, WW = ceil(W / 64): bit i of word j of a row is voxel
 *   x = 64 j + i; the bits past W are always 0.  `pack` sets a bit where the byte is nonzero (value = -1) or equals `value`
 *   (0..255), `unpack` writes bytes 0 / 1.  `window` copies a box: out(z, y, x) = in(z + oz, y + oy, x + ox) where that lies
 *   inside `in` and 0 elsewhere -- negative offsets pad, positive ones crop; in and out must differ.
 * Ball dilation: the structuring element is the set of offsets o with sum_i (o_i / (r_i + 0.5))^2 <= 1, r = (rz, ry, rx), each
 *   0..8 (19, 81, 179, 389 voxels for isotropic r = 1..4); `border` (0 / 1) is the value outside the volume.  inv_in complements
 *   the input inside the volume before, inv_out the result after, so erosion with border b is inv_in = inv_out = 1 with
 *   border 1 - b.  One launch; in and out must differ.  Closing / opening are compositions of these.
 * Connected components of a bit plane, connectivity 6, 18 or 26 -> labels (B, D, H, W) int32, 0 = background, components
 *   numbered 1..n in raster order of their first voxel (scipy.ndimage.label's numbering), n (B) int32 DEVICE.  Union-find by
 *   smallest voxel index with atomicMin: the same input gives the same labels, an item's labels do not depend on the batch.
 *   workspace: the query below (4 bytes per voxel + 4 per 1024 voxels), 8-byte aligned.
 * Component statistics: stats (B, cap, 4) int64 = voxel count and the sums of the z, y, x indices of the labels 1..cap (a
 *   larger label is left out), zeroed by the call, integer atomics (exact).
 * Relabel: out[i] = lut[b][labels[i]] (0 for a label outside 0..lut_len-1); lut (B, lut_len) int32; out int32 or int64.
 * Bad arguments (a radius outside 0..8, a connectivity other than 6 / 18 / 26, a NULL pointer, a short workspace, 2^31 or more
 *   voxels) are FSG_ERR_ARG. */
#define FSG_MORPH_MAX_RADIUS 8 /* rz, ry, rx of fsg_ball_dilate_bits */
int fsg_bits_pack_u8(const uint8_t *vol, int B, int D, int H, int W, int value, uint64_t *bits, fsg_stream_t stream);
int fsg_bits_unpack_u8(const uint64_t *bits, int B, int D, int H, int W, uint8_t *vol, fsg_stream_t stream);
int fsg_bits_window(const uint64_t *in, int B, int Di, int Hi, int Wi, int oz, int oy, int ox, int Do, int Ho, int Wo,
                    uint64_t *out, fsg_stream_t stream);
int fsg_ball_dilate_bits(const uint64_t *in, int B, int D, int H, int W, int rz, int ry, int rx, int border, int inv_in,
                         int inv_out, uint64_t *out, fsg_stream_t stream);
size_t fsg_cc_workspace_bytes(int B, int D, int H, int W);
int fsg_cc_label_bits(const uint64_t *bits, int B, int D, int H, int W, int connectivity, int32_t *labels, int32_t *n,
                      void *workspace, size_t workspace_bytes, fsg_stream_t stream);
int fsg_component_stats_i32(const int32_t *labels, int B, int D, int H, int W, int cap, int64_t *stats, fsg_stream_t stream);
int fsg_relabel_lut_i32(const int32_t *labels, int B, int64_t n_per_item, const int32_t *lut, int lut_len, void *out,
                        int out_is_i64, fsg_stream_t stream);

/* Exact squared Euclidean distance transform of bit planes, optional feature transform, nearest of K planes (csrc/edt.hip).
 * Stands where data_processing/process_lung_mask.py:80-91 of the reference calls scipy.ndimage.distance_transform_edt, and
 * gives the nearest-neighbour distances between the voxel clouds of two label maps of metrics.py:79-93.  All pointers DEVICE.
 *
 * bits is a bit plane (B, D, H, WW) as above.  A SITE is a voxel whose bit is 0; out_d2 (B, D, H, W) is, at every voxel, the
 *   smallest (s0 dz)^2 + (s1 dy)^2 + (s2 dx)^2 to a site of the same item.  An item without a site gives +inf everywhere in
 *   the fp32 mode and INT32_MAX in the int32 mode (scipy returns garbage there; this rule is ours).
 * Three separable passes (W from the words of the row, then H, then D; see the head of csrc/edt.hip), each exact.  The int32
 *   mode (unit spacing) is exact in integers; every dimension is at most 16384 and D H W < 2^31.  The fp32 mode forms each
 *   term as fl(fl(s * delta)^2) and each sum with one rounding, no fused multiply-add; spacings are positive, at most 1e6.
 * out_idx (B, D, H, W) int32 or NULL: the linear index (z H + y) W + x, inside the item, of the site that won; -1 where
 *   there is none.  Ties: per pass the smaller |delta| wins, then the lower index along that axis -- not scipy's rule.
 * No atomics, no host read, everything on `stream`: the same input gives the same bits, an item does not depend on its batch.
 * workspace: the query below (4 bytes per voxel, 8 with indices), 8-byte aligned.
 * Nearest label: d2 is (K, V) int32 (is_f32 = 0) or fp32 distance planes, K <= 64; out[v] = cand[k] of the first plane k
 *   with the smallest value (cand ascending: the lowest label wins a tie, as np.argmin does at process_lung_mask.py:87), or 0
 *   where keep (V) uint8, if given, is 0 (process_lung_mask.py:88).
 * Bad arguments (a dimension above 16384, 2^31 voxels or more, a spacing that is not positive, a NULL pointer, a short
 *   workspace) are FSG_ERR_ARG. */
#define FSG_EDT_MAX_DIM 16384 /* D, H, W: 3 * 16383^2 fits an int32 */
#define FSG_EDT_MAX_LABELS 64 /* K of fsg_edt_nearest_label */
size_t fsg_edt_workspace_bytes(int B, int D, int H, int W, int with_indices);
int fsg_edt_sq_i32(const uint64_t *bits, int B, int D, int H, int W, int32_t *out_d2, int32_t *out_idx, void *workspace,
                   size_t workspace_bytes, fsg_stream_t stream);
int fsg_edt_sq_f32(const uint64_t *bits, int B, int D, int H, int W, float s0, float s1, float s2, float *out_d2,
                   int32_t *out_idx, void *workspace, size_t workspace_bytes, fsg_stream_t stream);
int fsg_edt_nearest_label(const void *d2, int is_f32, int K, int64_t V, const int32_t *cand, const uint8_t *keep, int32_t *out,
                          fsg_stream_t stream);

/* In-plane binary thinning of a bit plane (csrc/thinning.hip).  Stands where sitk.BinaryThinning stands in the reference's
 * poisson_reconstruction (data_processing/surface_fitting.py:109, called from train_segmentation_net.py:75-148 and
 * regularize_fissure_segmentations): the two-sub-iteration thinning of Gonzalez & Woods that ITK's BinaryThinningImageFilter
 * documents, applied in the (y, x) plane of every slice, neighbours outside a slice clamped to the nearest voxel inside it.  The
 * rule and its numpy oracle (tests/thinning_oracle.py) are the authority: parity with SimpleITK is unpinned.
 *
 * in / out: bit planes (B, D, H, ceil(W / 64)) as above (bits past W are 0 on the way out whatever came in); out may be in.
 * iterations (B, D) int32 or NULL: per slice, the number of odd + even step pairs that cleared a voxel.
 * One launch, one workgroup per (item, slice), the slice twice in LDS, the loop to convergence inside the launch (capped at
 *   H W + 1 pairs).  No atomics, no host read, everything on `stream`: the same input gives the same bits, a slice does not
 *   depend on its neighbours or its batch.
 * A slice holds at most fsg_thin_max_words() = 8192 words, H * ceil(W / 64) (512 x 1024 or 1024 x 512 voxels); a larger one, a
 *   NULL plane or a non-positive dimension is FSG_ERR_ARG. */
#define FSG_THIN_MAX_WORDS 8192 /* what fsg_thin_max_words() returns: 64 KiB of LDS per copy of the slice */
int fsg_thin_max_words(void);
int fsg_thin_bits(const uint64_t *in, int B, int D, int H, int W, uint64_t *out, int32_t *iterations, fsg_stream_t stream);

/* Voxel patch augmentation and resampling (csrc/spatial.hip).  Stands where ImageDataset.__getitem__ of the reference
 * (data.py:290-327) calls batchgenerators' SpatialTransform + MirrorTransform (augmentations.py:29-49), sitk.Resample
 * (utils/image_ops.py:12-28) and normalize_img (data.py:365-366).  All pointers DEVICE, everything fp32, no atomics, no host
 * read, everything on `stream`: the same input gives the same bits, an item does not depend on its batch.
 *
 * Prefilter, one axis: in is (outer, n, inner), out (outer, n + 2 FSG_BSPLINE_PAD, inner): every line of n samples extended
 *   by FSG_BSPLINE_PAD edge-replicated samples on both sides and turned into cubic B-spline coefficients as
 *   scipy.ndimage.spline_filter1d(order=3, mode='nearest') does (pole sqrt(3) - 2).  Three calls, one per axis, give the
 *   coefficients that fsg_spatial_resample_f32 reads at order 3.  in != out.
 * Gauss, one axis: in and out are (B, outer, n, inner), outer n inner < 2^31; out = gaussian_filter1d(in, sigma[b],
 *   mode='constant', cval=0, truncate=4) along the n axis with scipy's taps (radius int(4 sigma + 0.5), which may exceed n),
 *   times alpha[b] when alpha is not NULL.  sigma, alpha (B).  An item whose sigma is not in (0, 255] gives NaN.  in != out.
 * Resample: for output voxel o = (oz, oy, ox) of item b the source coordinate is
 *     x = M_b ((o - (patch - 1) / 2) + elastic_b(o)) + centre_b      voxel units, axes (D, H, W)
 *   with matrix (B, 3, 3) row-major, centre (B, 3), elastic (B, 3, pd, ph, pw) or NULL.
 *   src (B, C, D, H, W) is read at order_data 0 (nearest, floor(x + 0.5)) or 1 (trilinear), the coordinate clamped to
 *   [0, n - 1]; at order_data 3 src is the prefiltered (B, C, D + 2 PAD, H + 2 PAD, W + 2 PAD) read at x + PAD with the 4 tap
 *   indices per axis clamped to the padded array (scipy's map_coordinates(order=3, mode='nearest'): beyond the padding the
 *   value runs into the edge coefficient).  out_img
 *   (B, C, pd, ph, pw) = ia * value + ib.  src may be NULL.
 *   seg (B, Cs, D, H, W) of seg_kind FSG_LABEL_* (values must fit an int32), or NULL: order_seg 0 is the nearest label,
 *   order_seg 1 the largest label whose summed trilinear weight among the 8 corners is >= 0.5, else 0; for both a
 *   coordinate outside [0, n - 1] on any axis gives 0 (scipy's mode='constant', cval=0).  out_seg (B, Cs, pd, ph, pw) int64.
 *   mirror (B, 3) uint8 or NULL: a nonzero flag stores the item's output reversed along that axis.
 * Volumes (padded) and patches hold fewer than 2^31 voxels, B <= 65535.  Bad arguments are FSG_ERR_ARG. */
#define FSG_ELASTIC_MAX_SIGMA 255.0f /* sigma of fsg_gauss_axis_f32: its tap table lives in LDS */
#define FSG_BSPLINE_PAD 12
#define FSG_LABEL_U8 0
#define FSG_LABEL_I32 1
#define FSG_LABEL_I64 2
int fsg_bspline_prefilter_axis_f32(const float *in, int64_t outer, int n, int64_t inner, float *out, fsg_stream_t stream);
int fsg_gauss_axis_f32(const float *in, int B, int64_t outer, int n, int64_t inner, const float *sigma, const float *alpha,
                       float *out, fsg_stream_t stream);
int fsg_spatial_resample_f32(const float *src, int C, int order_data, const void *seg, int seg_kind, int Cs, int order_seg,
                             int B, int D, int H, int W, int pd, int ph, int pw, const float *matrix, const float *centre,
                             const float *elastic, const uint8_t *mirror, float ia, float ib, float *out_img,
                             int64_t *out_seg, fsg_stream_t stream);

/* Mesh regularisers and surface sampling for the PC-AE mesh loss (csrc/mesh.hip).  Replace pytorch3d's mesh_edge_loss,
 * mesh_normal_consistency, mesh_laplacian_smoothing(method="uniform") and sample_points_from_meshes as
 * losses/mesh_loss.py:28-57 and data_processing/surface_fitting_optimization.py call them.  All pointers DEVICE.
 *
 * A batch is N meshes over one packed vertex array verts (total_verts, 3) fp32.  Topology is built once per face list by the
 *   caller (fissure_segmentation_amd/mesh.py) and holds LOCAL vertex indices, so the meshes of a shared-face batch point at
 *   one copy.  desc (N, 8) int32 per mesh: first vertex, vertex count V, first entry of its V + 1 offsets in nbr_off and
 *   inc_off, first pair, edge count E, pair count P, two unused.  nbr_off[o + i] .. nbr_off[o + i + 1] delimit vertex i's
 *   neighbours in nbr (ascending, over the unique undirected edges); pairs (., 4) int32 = (v0, v1, a, b): an edge and the
 *   opposite vertices of two faces sharing it; inc_off likewise delimits vertex i's entries in inc, each 4 * (pair - first
 *   pair) + role (0..3 = v0, v1, a, b), ascending.
 * Per mesh, each a mean:  edge = mean over edges |va - vb|^2;  normal = mean over pairs 1 - cos(n0, n1), n0 = (v1 - v0) x
 *   (a - v0), n1 = -(v1 - v0) x (b - v0), cos = n0 / max(|n0|, 1e-8) . n1 / max(|n1|, 1e-8) (0 without pairs);  laplacian =
 *   mean over vertices |sum_j v_j / d_i - v_i| (degree 0: |v_i|; gradient 0 where the norm is 0).
 * -> terms (N, 3) fp32 (edge, normal, laplacian), mean (3) over the meshes, grads (3, total_verts, 3) = d terms[m, t] / d verts
 *   of mesh m (NULL: not written).  One launch plus a one-workgroup finalize.  Gradients are formed per vertex from the
 *   incidence lists in list order, sums are fp64 in a fixed order, no atomics: the same input gives the same bits and a mesh's
 *   numbers do not depend on the rest of the batch.  Any V; meshes of up to 4096 vertices are staged in LDS.
 * workspace: the query below, 8-byte aligned.  The topology arrays are NOT checked against V (the caller builds them).
 *
 * Sampling: sdesc (N, 4) int32 per mesh: first vertex, V, first face in faces (., 3) int32 (LOCAL indices), face count F > 0.
 *   u (N, n, 3) uniforms in [0, 1).  face = min{ j : C[j] > u0 C[F-1] }, C the inclusive fp64 prefix sum of the fp64 face
 *   areas in face order (a mesh without area: every face alike, C[j] = j + 1); weights (1 - sqrt u1, sqrt u1 (1 - u2),
 *   sqrt u1 u2) fp32 -> pts (N, n, 3) = sum_c w_c v[face_c], face (N, n) int32, w (N, n, 3).  Two launches.
 *   bwd: grad_verts (total_verts, 3) = sum over the mesh's samples, in sample order, of w_c g on the face corners that are the
 *   vertex (every vertex of every mesh is written); g (N, n, 3).  O(V n) compares per mesh, no sort, no atomics, one launch.
 * N <= 65535.  Bad shapes, NULL pointers, a short or misaligned workspace are FSG_ERR_ARG before any launch. */
size_t fsg_mesh_reg_workspace_bytes(int N, int max_V);
int fsg_mesh_reg_f32(const float *verts, int64_t total_verts, const int32_t *desc, int N, int max_V, const int32_t *nbr_off,
                     const int32_t *nbr, const int32_t *pairs, const int32_t *inc_off, const int32_t *inc, float *terms,
                     float *mean, float *grads, void *workspace, size_t workspace_bytes, fsg_stream_t stream);
size_t fsg_mesh_sample_workspace_bytes(int N, int max_F);
int fsg_mesh_sample_f32(const float *verts, const int32_t *faces, const int32_t *sdesc, int N, int max_F, const float *u, int n,
                        float *pts, int32_t *face, float *w, void *workspace, size_t workspace_bytes, fsg_stream_t stream);
int fsg_mesh_sample_bwd_f32(const float *g, const int32_t *face, const float *w, const int32_t *faces, const int32_t *sdesc,
                            int N, int max_V, int n, float *grad_verts, fsg_stream_t stream);

/* Point cloud <-> dense grid, and the spectral Poisson solve of DPSR (csrc/grid_points.hip).  Replace models/divroc.py:24-61
 * (DiVRoC: a splat obtained by differentiating grid_sample against a zero grid, and its backward), models/dpsr_utils.py:156-199
 * (grid_interp), :227-287 (point_rasterize with its (B N 8 C, 5) int64 scatter index) and models/dpsr_net.py:74-87
 * (spectral_PSR between rfftn and irfftn).  All pointers DEVICE, all floating point fp32, any D, H, W.
 *
 * mode FSG_GRID_TORCH: coords (B, N, 3) = (x -> W, y -> H, z -> D) in [-1, 1], grid_sample's align_corners=False
 *   unnormalisation t = ((x + 1) S - 1) / 2, trilinear, padding zeros: a corner outside the grid gives and receives nothing;
 *   any coordinate is legal: a point without a corner in the grid (far outside, infinite or NaN on an axis) reads 0, adds
 *   nothing and gets a zero gradient.  mode FSG_GRID_SAP: coords = (0 -> D, 1 -> H, 2 -> W) in [0, 1], cubesize =
 *   1 / (S - 1), lower corner floor(p / cubesize), upper corner fmod(ceil(p / cubesize), S), weights |p - opposite corner| /
 *   cubesize, every expression in fp32 in the reference's order (nodes, 0 and 1 reach the reference's voxels); every size >= 2;
 *   points outside [0, 1] are outside the contract, their out-of-grid corners are dropped, nothing outside the grid is touched.
 * Splat, values (B, C, N) -> grid (B, C, D, H, W) = sum of the trilinear contributions, in three steps:
 *   fsg_grid_corners_f32 writes keys (B, 8 N) int32 (destination voxel z H W + y W + x, D H W for a dropped corner) and
 *   w (B, 8 N), entry 8 n + corner;  the CALLER sorts every row of keys with a STABLE sort and keeps the permutation (int64,
 *   position before the sort);  fsg_grid_splat_sorted_f32 zeroes the grid and sums every voxel's run in row order, a run cut
 *   at every multiple of 64 row positions, the pieces added in position order.  No floating-point atomics: the same input gives
 *   the same bits and an item gives the same bits alone and inside a batch.  workspace: the query below, 4-byte aligned.
 * Sample: sampled (B, C, N) = trilinear reading of grid at coords (NULL: not written); with weights (B, C, N) also
 *   grad_coords (B, N, 3) = sum_c weights[c] d sampled[c] / d coords, indices held constant: TORCH mode is grid_sample's
 *   backward, SAP mode is autograd through grid_interp (torch's abs: 0 at 0).  weights and grad_coords are both NULL or both
 *   given.  One launch, the 8 C corners are read once.  Splat and sample are adjoint; together they give every gradient of both.
 * Spectral solve: in (B, 3, R0, R1, R2 / 2 + 1) complex64 = rfftn of the normal field -> out (B, R0, R1, R2 / 2 + 1) complex64,
 *   Phi = sum_d c_d in_d, c_d = -i omega_d G / (-|omega|^2 + 1e-6), omega = 2 pi fftfreq (fp32), G = exp(-0.5 (2 sig |f| /
 *   R0)^2) (fp64, rounded), Phi = 0 at the DC term.  adjoint = 1: in (B, R0, R1, R2 / 2 + 1) = grad Phi -> out (B, 3, ...) =
 *   conj(c_d) grad Phi.  No permutes; in and out must differ.
 * B <= 65535, N <= 2^27, D H W < 2^31 - 1.  Bad shapes, modes, NULL pointers or a short workspace are FSG_ERR_ARG before any
 *   launch. */
#define FSG_GRID_TORCH 0
#define FSG_GRID_SAP 1
int fsg_grid_corners_f32(const float *coords, int B, int N, int D, int H, int W, int mode, int32_t *keys, float *w,
                         fsg_stream_t stream);
size_t fsg_grid_splat_workspace_bytes(int B, int C, int N);
int fsg_grid_splat_sorted_f32(const float *values, const int32_t *keys_sorted, const int64_t *perm, const float *w, int B, int C,
                              int N, int D, int H, int W, float *grid, void *workspace, size_t workspace_bytes,
                              fsg_stream_t stream);
int fsg_grid_sample_f32(const float *grid, const float *coords, const float *weights, int B, int C, int N, int D, int H, int W,
                        int mode, float *sampled, float *grad_coords, fsg_stream_t stream);
int fsg_psr_spectral_f32(const float *in, int B, int R0, int R1, int R2, double sig, int adjoint, float *out,
                         fsg_stream_t stream);

/* Marching cubes on a dense grid (csrc/marching_cubes.hip; the case table csrc/mc_table.h is generated by tools/gen_mc_table.py).
 * Replace pytorch3d.ops.marching_cubes and Meshes.verts_normals_padded as DifferentiableMarchingCubes calls them
 * (models/dpsr_utils.py:60-64) and skimage.measure.marching_cubes of compute_surface_mesh_marching_cubes
 * (data_processing/find_lobes.py).  All pointers DEVICE.  Parity with those two libraries is unpinned (neither is available):
 * the table, the orders and the mask rule below are this library's own.
 *
 * field (B, D, H, W) fp32, every size >= 2, B D H W < 2^31, B <= 65535.  A node is inside iff value < isolevel (fp32; NaN is
 *   outside).  mask (uint8, nonzero = in; NULL = all) has mask_item_stride D H W (one per item) or 0 (shared); a cell emits
 *   triangles iff all 8 of its corner nodes are in the mask, a grid edge carries a vertex iff it crosses the isolevel and one of
 *   the <= 4 cells round it emits.  The labels form takes ONE int32 volume (D, H, W) for all items: item b is the object
 *   labels == first_label + b, cut as the field (labels != first_label + b) at 0.5, so normals point out of the object.
 * count: four launches -> workspace (the query below, 8-byte aligned; it must reach the emit call unchanged) and totals, int64
 *   (4 B + 1): [2 b] vertices and [2 b + 1] triangles of item b, [2 B] nonzero iff validate and a field value is not finite,
 *   [2 B + 1 + 2 b], [2 B + 2 + 2 b] the rows where item b starts in the packed outputs.  The caller reads totals (the one
 *   readback; the sizes depend on the data, so the pair cannot be captured into a graph) and must not emit when a per-item
 *   total exceeds 2^31 - 1.
 * emit: three launches -> verts (total_verts, 3) fp32 in (x, y, z) = index along (W, H, D), faces (total_faces, 3) int64 indices
 *   LOCAL to their item, normals (total_verts, 3) fp32.  Vertex order (item, z, y, x of the lower node of the edge, axis x < y < z),
 *   face order (item, cell, table order).  position = p_a + t (p_b - p_a), t = (isolevel - v_a) / (v_b - v_a), p the node
 *   coordinate: 2 i / (S - 1) - 1 with local_coords, else i * (sx, sy, sz).  normal = sum over the vertex's faces of
 *   (v1 - v0) x (v2 - v0) in output coordinates, in (cell z, y, x, table order) order, divided by max(|n|, 1e-6); it points
 *   toward increasing field values.  Rows at or past total_verts / total_faces are never written.
 * No floating-point atomics and none that decide an order: the same input gives the same bits, an item the same bits alone and
 *   inside a batch.  Bad shapes, NULL pointers, a short or misaligned workspace are FSG_ERR_ARG before any launch. */
size_t fsg_mc_workspace_bytes(int B, int D, int H, int W);
int fsg_mc_count_f32(const float *field, const uint8_t *mask, int64_t mask_item_stride, int B, int D, int H, int W, float isolevel,
                     int validate, void *workspace, size_t workspace_bytes, int64_t *totals, fsg_stream_t stream);
int fsg_mc_count_labels_i32(const int32_t *labels, const uint8_t *mask, int64_t mask_item_stride, int first_label, int B, int D,
                            int H, int W, void *workspace, size_t workspace_bytes, int64_t *totals, fsg_stream_t stream);
int fsg_mc_emit_f32(const float *field, int B, int D, int H, int W, float isolevel, int local_coords, float sx, float sy, float sz,
                    const void *workspace, size_t workspace_bytes, const int64_t *totals, int64_t total_verts, int64_t total_faces,
                    float *verts, int64_t *faces, float *normals, fsg_stream_t stream);
int fsg_mc_emit_labels_i32(const int32_t *labels, int first_label, int B, int D, int H, int W, int local_coords, float sx, float sy,
                           float sz, const void *workspace, size_t workspace_bytes, const int64_t *totals, int64_t total_verts,
                           int64_t total_faces, float *verts, int64_t *faces, float *normals, fsg_stream_t stream);

/* Point-cloud normal estimation on packed clouds (csrc/pcl_normals.hip).  Replaces pytorch3d.ops.estimate_pointcloud_normals and
 * estimate_pointcloud_local_coord_frames as models/dpsr_net.py:173-175 calls them; parity with pytorch3d is unpinned (the
 * library is not available), the semantics below are restated from its ops/points_normals.py.  All pointers DEVICE.
 *
 * xyz (n, 3) fp32 packed, offset (b) int32 cumulative segment ends (as fsg_knn_segment_f32 takes them; empty segments allowed),
 * idx (n, K) int32 neighbour lists in that kernel's layout: row q holds points of q's segment in ascending distance, q itself
 * first.  A point of a segment of n_s points uses k_s = max(1, min(K, n_s - 1)) neighbours (itself included) and reads only
 * the first k_s columns of its row; the columns beyond are never touched.  An index outside [0, n) is clamped into the cloud
 * (it cannot fault); that it lies in the right segment is the caller's business.
 *   C = mean_j (x_j - mean)(x_j - mean)^T over the k_s neighbours; curvatures (n, 3) = its eigenvalues ascending; normals (n, 3)
 *   = the unit eigenvector of the smallest, z = that of the largest.  With disambiguate != 0 a vector v is negated iff
 *   #{j : v . (x_j - p) > 0} < k_s / 2 (applied to the normal and to z; on a convex surface the normal then points INWARDS).
 *   frames (n, 3, 3) or NULL: columns (normal, y = z x normal, z).
 * Rank-deficient C (coincident, collinear, planar neighbours) gives finite orthonormal vectors.  A non-finite coordinate makes
 * the rows that list it non-finite and nothing else.  fp32, no atomics: the same input gives the same bits.
 * 2 <= K <= 64, b >= 1, n <= 2^28; bad shapes and NULL pointers are FSG_ERR_ARG before any launch. */
#define FSG_PCL_NORMALS_MAX_K 64 /* K: what fsg_knn_segment_f32 can deliver */
int fsg_pcl_normals_f32(const float *xyz, const int32_t *idx, const int32_t *offset, int b, int n, int K, int disambiguate,
                        float *normals, float *curvatures, float *frames, fsg_stream_t stream);

/* Surface fitting of labelled point clouds: consistent normal orientation and mesh clean-up (csrc/mesh_cleanup.hip; DESIGN.md
 * "Surface fitting").  All pointers DEVICE.  Only integer atomics whose result does not depend on their order are used: the
 * same input gives the same bits.  Bad shapes, NULL pointers, a short or misaligned workspace are FSG_ERR_ARG before any launch.
 *
 * fsg_orient_normals_f32 replaces pcd.orient_normals_consistent_tangent_plane(100) of data_processing/surface_fitting.py:62-64.
 *   xyz, normals (n, 3) fp32 packed (normals need not be unit), idx (n, K) int32 in fsg_knn_segment_f32's layout (self first;
 *   an index outside the row's segment is clamped into it), offset (b) int32 cumulative segment ends.  Per segment of n_s points
 *   the undirected graph {u, idx[u, j]}, 1 <= j < k_s = min(K, n_s - 1), with weights max(0, 1 - |n_u . n_v|); its minimum
 *   spanning forest under the key (fp32 bits of w >> 8, min(u, v), max(u, v)) by Boruvka rounds (64-bit atomic min per
 *   component), orientation carried as union-find with parity.  Per connected component of that graph: the member of largest
 *   z (lowest index on ties) ends with n_z >= 0, every other member follows by parity along the forest.  open3d adds Euclidean
 *   MST edges to connect the graph; this does not: every component is oriented on its own.
 *   out (n, 3) = normals with the sign bit flipped or not, signs (n) int8 = +1 / -1, comp (n) int32 = the smallest member of the
 *   point's component.  ceil(log2 n) + 1 rounds of four launches are always issued, rounds after the last merge return at once:
 *   no host read.  2 <= K <= 64, n <= 2^20 (20 bits per endpoint in the key), workspace 16-byte aligned.
 * fsg_face_union_i32 replaces mesh.cluster_connected_triangles() of utils/general_utils.py:177.  sorted_keys (3 F) int64: the
 *   keys min(a, b) * V + max(a, b) of the half-edges (3 f + e: edge e of face f) in ascending order, half_edge (3 F) int64 the
 *   permutation that sorts them.  Faces with an equal key are united (an edge with more than two faces links all of them):
 *   parent (F) int32 is scratch, root (F) int32 = the smallest face of every face's cluster.
 * fsg_cluster_stats_f64 replaces cluster_area and the np.unique / np.mean of utils/general_utils.py:177-195.  verts (V, 3),
 *   faces (F, 3) int32 into verts; sorted_clusters (F) int32 = the cluster (0 .. C - 1) of every face in ascending order and
 *   face_order (F) int64 the stable permutation that sorts them; sorted_vertex_keys (3 F) int64 = cluster * V + vertex of every
 *   face corner, ascending.  -> area (C) fp64 = sum of 0.5 |(v1 - v0) x (v2 - v0)|, num_verts (C) int64 and vert_sum (C, 3)
 *   fp64 over the DISTINCT vertices of the cluster's faces (a vertex of two clusters counts in both).  One launch, fixed order.
 * fsg_mesh_keep_flags_u8 replaces the flags of mask_out_verts_from_mesh (utils/general_utils.py:157-167) and of
 *   TriangleMesh.crop (data_processing/surface_fitting.py:71-74).  verts (V, 3) in (x, y, z), vert_offset (B + 1) int32 the first
 *   vertex of every mesh; keep = keep_in (NULL = all) AND lo <= v <= hi of boxes (B, 6) fp32 (NULL = no box; per mesh lo xyz,
 *   hi xyz) AND mask[iz, iy, ix] (NULL = no mask) of a (D, H, W) uint8 volume at i = floor(v / spacing), clamped from above as
 *   the reference does; a negative index (or NaN) is OUTSIDE, where the reference's indexing would wrap around.
 * fsg_mesh_face_flags_u8 / fsg_mesh_compact_f32 replace remove_vertices_by_mask, remove_triangles_by_mask and
 *   remove_unreferenced_vertices (utils/general_utils.py:168, :207-209).  A face survives iff its three vertices do and
 *   face_keep (NULL = all) is set; vert_used marks the vertices of surviving faces.  The caller scans the flags it wants to
 *   keep (exclusive prefix sums vert_new, face_new, int64); compact writes survivors in their old order, faces re-indexed and
 *   LOCAL to their mesh (int64), normals alongside when given. */
#define FSG_ORIENT_MAX_POINTS (1 << 20) /* n of fsg_orient_normals_f32: 20 bits per endpoint in the edge key */
size_t fsg_orient_normals_workspace_bytes(int n, int K);
int fsg_orient_normals_f32(const float *xyz, const float *normals, const int32_t *idx, const int32_t *offset, int b, int n, int K,
                           void *workspace, size_t workspace_bytes, float *out, int8_t *signs, int32_t *comp, fsg_stream_t stream);
int fsg_face_union_i32(const int64_t *sorted_keys, const int64_t *half_edge, int F, int32_t *parent, int32_t *root,
                       fsg_stream_t stream);
int fsg_cluster_stats_f64(const float *verts, const int32_t *faces, const int32_t *sorted_clusters, const int64_t *face_order,
                          const int64_t *sorted_vertex_keys, int V, int F, int C, double *area, int64_t *num_verts, double *vert_sum,
                          fsg_stream_t stream);
int fsg_mesh_keep_flags_u8(const float *verts, int V, const int32_t *vert_offset, int B, const uint8_t *keep_in, const float *boxes,
                           const uint8_t *mask, int D, int H, int W, float sx, float sy, float sz, uint8_t *keep, fsg_stream_t stream);
int fsg_mesh_face_flags_u8(const int32_t *faces, int V, int F, const uint8_t *vert_keep, const uint8_t *face_keep, uint8_t *face_out,
                           uint8_t *vert_used, fsg_stream_t stream);
int fsg_mesh_compact_f32(const float *verts, const float *normals, const int32_t *faces, int V, int F, const int32_t *vert_offset,
                         int B, const uint8_t *vert_flag, const int64_t *vert_new, const uint8_t *face_flag, const int64_t *face_new,
                         float *verts_out, float *normals_out, int64_t *faces_out, fsg_stream_t stream);

/* Dense Adam image registration (csrc/dense_reg.hip).  Replace the body of the optimisation loop of
 * shape_model/adam_registration.py:106-124: three avg_pool3d and their backward, a grid_sample of every feature channel with
 * its sampled (C, S0, S1, S2) tensor, three slice-difference regularisers.  All pointers DEVICE.  An iteration is four launches
 * of entry points and no host read: smooth3 of the parameter, objective, smooth3 of grad_disp, fsg_adam_flat_f32.
 *
 * fsg_reg_smooth3_f32: in (B, C, S0, S1, S2) fp32 -> out, the same shape = avg_pool3d(kernel 3, stride 1, padding 1,
 *   count_include_pad=True) applied three times (:110-111, :129-130).  Per axis that is T^3, T the tridiagonal 1/3 operator with
 *   zero neighbours outside the domain: the values outside are zero again after every pool, so within two cells of a border and
 *   on an axis shorter than 7 it is NOT the truncated [1 3 6 7 6 3 1] / 27.  The axes commute and T is symmetric: the operator
 *   is its own adjoint, the backward pass calls this entry with the gradient.  One launch (an LDS tile with a halo of 3).
 *   Every axis >= 3 (avg_pool3d refuses smaller ones), in != out, B C <= 65535.
 * fsg_reg_objective_f16: disp (B, 3, S0, S1, S2) fp32 = the smoothed field, channel c displaces along axis S_c in the
 *   reference's units; feat_fix, feat_mov (B, S0, S1, S2, Cp) fp16, channels last, 16-byte aligned, Cp a multiple of 8,
 *   C <= Cp <= 4096, channels C .. Cp - 1 are ignored.  Per node (:115-122): the identity coordinate of
 *   affine_grid(align_corners=False) plus disp[c] / ((S_c - 1) / 2) with the channel flip (channel 0 -> last grid coordinate
 *   <-> axis S0), grid_sample's align_corners=False unnormalisation -- together t_c = i_c + disp[c] S_c / (S_c - 1) --,
 *   trilinear weights, zero padding: a corner outside the volume gives nothing to the value and nothing to the gradient.
 *   cost = cost_scale / (C nodes) sum over nodes and channels of (sample - fix)^2, nodes = S0 S1 S2, per item.
 *   reg (:112-114) = lambda * sum over the axes a of the mean of the squared forward differences of disp along a, each mean
 *   over its own 3 (S_a - 1) S_b S_c elements; lambda == 0 skips it (reg = 0 whatever the field holds).
 *   -> grad_disp (B, 3, S0, S1, S2) = d (cost + reg) / d disp (one-sided differences at the borders), loss (B, 2) fp32 =
 *   { cost, reg } of every item.  Any disp is legal: a coordinate far outside, infinite or NaN reads 0, gets a zero data-term
 *   gradient and never indexes outside the volumes (fsg_grid_sample_f32's contract); the regulariser of a non-finite field is
 *   not finite.  Sums: fp32 per node, then fp64 per workgroup and per item in a fixed order (a finishing launch); no
 *   floating-point atomics: the same input gives the same bits, an item gives the same bits alone and inside a batch.
 *   workspace: the query below, 8-byte aligned.
 * B <= 65535, S0 S1 S2 < 2^31 (offsets into the volumes are 64-bit).  Bad shapes, NULL pointers, misaligned volumes or a short
 *   workspace are FSG_ERR_ARG before any launch. */
int fsg_reg_smooth3_f32(const float *in, int B, int C, int S0, int S1, int S2, float *out, fsg_stream_t stream);
size_t fsg_reg_objective_workspace_bytes(int B, int S0, int S1, int S2);
int fsg_reg_objective_f16(const float *disp, const void *feat_fix, const void *feat_mov, int B, int C, int Cp, int S0, int S1, int S2,
                          float lambda, float cost_scale, float *grad_disp, float *loss, void *workspace, size_t workspace_bytes,
                          fsg_stream_t stream);

/* Voxel CNN inference (csrc/seg_cnn.hip): the eval-mode backbone block of models/mobilenet.py and the tail of the patch loop of
 * models/seg_cnn.py:48-62.  All pointers DEVICE unless said otherwise; fp32.
 *
 * fsg_mbconv3d_fwd_f32: one inverted-residual block in one launch; the expanded tensor is never written to memory.
 *   x (B, D, H, W, Cin) -- the logical (B, Cin, D, H, W) tensor in channels-last memory -- -> y (B, Do, Ho, Wo, Cout), the same.
 *   expand: w1 (Cmid, Cin), the 1x1x1 product; with first != 0 the dense 3x3x3, stride-2, padding-1 convolution of ONE channel,
 *     w1 (Cmid, 27) with the taps in (kd, kh, kw) order, whose output has (n - 1) / 2 + 1 cells per axis.
 *   then v s1 + b1 (the folded BatchNorm, per channel), ReLU6; depthwise 3x3x3 wd (Cmid, 27), stride 1 | 2, padding 1 with zeros
 *     around the ACTIVATED tensor, (n - 1) / stride + 1 cells per axis; v s2 + b2, ReLU6; project w3 (Cout, Cmid); v s3 + b3, no
 *     activation; residual != 0 adds x (needs stride 1, Cin == Cout, first == 0).
 *   Limits: 1 <= Cin, Cout <= 64, Cmid a multiple of 16 in 16..384, B D H W >= 1, D H W < 2^31, x != y.  Anything else, or a NULL
 *   pointer, is FSG_ERR_ARG before the launch.  Products on the exact fp32 matrix instruction, sums in a fixed order, no atomics:
 *   the same bits on every run, and an item gives the same bits alone and inside a batch.
 *
 * fsg_patch_accumulate_f32: logits (P, K, pd/2, ph/2, pw/2), the half-resolution output of the head for P patches of
 *   pd x ph x pw voxels (even); starts: HOST (P, 4) int32 = { item, z, y, x }, the patch's corner in the volume.  Per patch:
 *   x2 trilinear up-sampling (align_corners = False), softmax over K, times wmap (pd, ph, pw), or 1 where wmap is NULL, cropped
 *   to the part of the patch inside the volume -- a patch that overhangs the volume was replicate-padded by
 *   ceil(r / 2) cells in front and floor(r / 2) behind, r the overhang -- and added into sum (B, K, D, H, W); the weight into
 *   wsum (B, 1, D, H, W).  One launch per patch in the order of `starts` on `stream`: overlapping patches add in that order.
 * fsg_patch_finalize_f32: out (B, K, D, H, W) = softmax over K of sum / wsum (the reference applies its activation to every
 *   patch AND to the normalised sum); out may be sum. */
#define FSG_MBCONV_MAX_CIN 64
#define FSG_MBCONV_MAX_CMID 384
#define FSG_MBCONV_MAX_COUT 64
int fsg_mbconv3d_fwd_f32(const float *x, const float *w1, const float *s1, const float *b1, const float *wd, const float *s2,
                         const float *b2, const float *w3, const float *s3, const float *b3, int B, int Cin, int Cmid, int Cout,
                         int D, int H, int W, int stride, int first, int residual, float *y, fsg_stream_t stream);
int fsg_patch_accumulate_f32(const float *logits, int P, int K, int pd, int ph, int pw, const int *starts, const float *wmap,
                             float *sum, float *wsum, int B, int D, int H, int W, fsg_stream_t stream);
int fsg_patch_finalize_f32(const float *sum, const float *wsum, int B, int K, int D, int H, int W, float *out, fsg_stream_t stream);

/* DSEG-AE: from a labelled cloud to the auto-encoder's inputs (csrc/dseg_ae.hip), for every (item, object) group of a batch at
 * once -- what dseg_ae_regularization.py:62-138 of the reference does per object of one cloud.  All pointers DEVICE.
 *
 * fsg_label_partition: stable split of B labelled clouds into packed segments.  labels (B, N) of label_kind FSG_LABEL_*;
 *   x (B, C, N) fp32 channel-major, C >= 3, of which channels 0..2 are read; objects first_label .. first_label + L - 1,
 *   1 <= L <= 16; any other label is dropped.  -> counts (B, L) int32; offset (B L) int32, the END of every segment, cumulative
 *   in (item, object) order; xyz (B N, 3) fp32 and src (B N) int32, of which the first offset[B L - 1] rows are written: a
 *   segment's points in ascending order of src, their index inside the item.  Two launches: per-tile counts from wave ballots,
 *   then every tile takes its base from the counts in a fixed order and scatters by ballot rank.  B N < 2^31.
 * fsg_segment_jitter_extend_f32: random_extend_points for G packed segments, one workgroup each.  xyz (n, 3) with offset (G);
 *   nn_d2 (n): squared distance of every point to the nearest OTHER point of its segment (column 1 of
 *   fsg_knn_segment_f32(nsample = 2) of the cloud against itself); new_offset (G): every segment at least as long as before,
 *   n_new = new_offset[G - 1]; the caller's draws over the P = n_new - n padded rows, packed in segment order: src_idx (P) int32,
 *   the source row inside the segment (clamped to it), direction (P, 3), z (P).  -> out (n_new, 3): the segment, then
 *   xyz[src] + direction / |direction| * (z * std + mean); stats (G, 2) = { mean, std } of sqrtf(nn_d2) over the segment, the
 *   unbiased deviation, from fp64 sums in a fixed order (two passes); both 0 for fewer than two points.  A zero direction
 *   gives NaN, as in the reference.
 * fsg_fps_start_f32: fsg_fps_f32 with a first sample: start (b) int32, the index INSIDE each segment (clamped to it), or NULL
 *   for 0.  One workgroup of 1024 threads per segment; up to 16 384 points a segment lives in registers, longer ones in
 *   global memory with tmp (n) fp32 as the running distances.  Same arithmetic and tie rule as fsg_fps_f32 (largest distance,
 *   then lowest index): with start NULL the same idx bit for bit.
 * No atomics: the same bits on every run, a group the same alone and in a batch.  Bad arguments are FSG_ERR_ARG. */
#define FSG_PARTITION_MAX_LABELS 16 /* L of fsg_label_partition */
size_t fsg_label_partition_workspace_bytes(int B, int N, int L);
int fsg_label_partition(const void *labels, int label_kind, const float *x, int B, int C, int N, int first_label, int L,
                        int32_t *counts, int32_t *offset, float *xyz, int32_t *src, void *workspace, size_t workspace_bytes,
                        fsg_stream_t stream);
int fsg_segment_jitter_extend_f32(const float *xyz, const int32_t *offset, const float *nn_d2, const int32_t *new_offset,
                                  const int32_t *src_idx, const float *direction, const float *z, int G, int n, int n_new, float *out,
                                  float *stats, fsg_stream_t stream);
int fsg_fps_start_f32(const float *xyz, const int32_t *offset, const int32_t *new_offset, const int32_t *start, int b, int n,
                      float *tmp, int32_t *idx, fsg_stream_t stream);

/* Thin-plate-spline interpolation of displacements (csrc/tps.hip).  Serves the 'tps' interpolation mode of the reference,
 * shape_model/point_cloud_registration.py:24-67 (class TPS), :70-89 (thin_plate_dense) and :119-133
 * (interpolate_displacements_tps), which fits on n control points, evaluates on a (D/4, H/4, W/4) lattice, upsamples to the
 * dense (D, H, W, 3) field and grid_samples Q points out of it.  u(r) = r^2 log(r + 1e-6).  B independent items, DEVICE
 * pointers, contiguous rows; control (B, n, 3) fp32; theta (B, n + 4, C) fp64 = n spline weights, then the affine rows
 * (1, x, y, z); 1 <= C <= 4; B <= 65535.
 * fsg_tps_system_f64: the matrix of TPS.fit (:32-44) -> A (B, n + 4, n + 4) fp64: u(|c_i - c_j|) off the diagonal, lambda ON it,
 *   then [1 | c], its transpose and a zero block.  Distances are sums of squared differences, in fp64 (NOT the reference's
 *   ra + rb - 2 ab in fp32): the matrix is symmetric bit for bit.  1 <= n <= 32764.  The solve is the caller's.
 * fsg_tps_eval_f32: TPS.z (:63-67) -> out (B, Q, C) fp32 = a0 + a1 x + a2 y + a3 z + sum_j w_j u(|q - c_j|).  query (B, Q, 3)
 *   fp32, or NULL for the nodes of an align_corners=True lattice (D1, H1, W1) with Q = D1 H1 W1 (thin_plate_dense's x2, :75):
 *   node q = (iz H1 + iy) W1 + ix lies at (x, y, z) = (c(ix, W1), c(iy, H1), c(iz, D1)), c(i, L) = -1 + 2 i / (L - 1) rounded to
 *   fp32, 0 for L = 1.  One lane per query; u and the sum over j (ascending) are fp64.
 * fsg_tps_grid_sample_f32: :86-87 and :131-132 without the lattice and without the field -> out (B, Q, C) fp32, what
 *   grid_sample(align_corners=False, zeros padding) at grid (B, Q, 3) fp32 (x, y, z in [-1, 1]; x runs along W) reads from the
 *   trilinear align_corners=True upsample to (D, H, W) of the spline on the lattice (D1, H1, W1) above.  Per axis the two fine
 *   taps and their two coarse nodes each fold into weights of at most 3 consecutive nodes (fp64); the spline is evaluated at
 *   those 27 nodes as in fsg_tps_eval_f32 and the products are added in node order (z slowest).  A sample whose taps all fall
 *   outside gives exactly 0.  1 <= coarse <= fine <= 2^24 per axis.
 * No atomics, no workspace, nothing read on the host: the same inputs give the same bits, an item's output does not depend on
 * the batch, and every entry can be captured in a graph.  Bad arguments are FSG_ERR_ARG. */
#define FSG_TPS_MAX_CHANNELS 4 /* C */
int fsg_tps_system_f64(const float *control, int B, int n, double lambd, double *A, fsg_stream_t stream);
int fsg_tps_eval_f32(const float *query, const float *control, const double *theta, int B, int Q, int n, int C, int D1, int H1,
                     int W1, float *out, fsg_stream_t stream);
int fsg_tps_grid_sample_f32(const float *grid, const float *control, const double *theta, int B, int Q, int n, int C, int D, int H,
                            int W, int D1, int H1, int W1, float *out, fsg_stream_t stream);

/* Batched fp64 Cholesky factorisation and solve, and the symmetric positive definite form of deformable CPD's M-step
 * (csrc/cholesky.hip).  Serves the M x M solve of pycpd's DeformableRegistration.update_transform behind the reference's
 * shape_model/point_cloud_registration.py:101-116.  B independent items, DEVICE pointers, row-major contiguous fp64.
 * fsg_cholesky_f64: A (B, n, n) -> L with A = L L^T, in place, lower: only the lower triangle is read and written, the strict
 *   upper triangle is left as it is.  info (B) int32 DEVICE: 0 = factored; j = the leading minor of order j is not positive
 *   (LAPACK potrf's convention, 1-based), tested as !(pivot > 0), so a NaN pivot is caught.  The kernels always run to the end:
 *   the contents of a failed item are unspecified from column j on, the other items do not see the failure.  A left-looking
 *   sweep over panels of FSG_CHOL_BLOCK columns on v_mfma_f64_16x16x4_f64, one launch per panel and one for the diagonal blocks
 *   (n / FSG_CHOL_BLOCK + 1 launches, rounded up), no workspace.
 * fsg_cholesky_solve_f64: L as written above (its strict upper triangle is not read), X (B, n, r) the right-hand sides on entry
 *   and the solutions of L L^T x = b on exit, 1 <= r <= FSG_CHOL_MAX_RHS.  One workgroup per item, blocked forward and back
 *   substitution.  An item whose info is not 0 yields unspecified values, never a fault.
 * fsg_cpd_spd_system_f64: G (B, M, M), P1 (B, M), PX (B, M, 3), Y (B, M, 3), sigma2 (B) DEVICE, alpha -> d (B, M) = sqrt(P1);
 *   S (B, M, M), lower triangle only: S_ij = (d_i G_ij) d_j + (i == j) alpha sigma2; rhs (B, M, 3):
 *   rhs_i = d_i > 0 ? (PX_i - P1_i Y_i) / d_i : 0.  With S V = rhs, W = d V solves (diag(P1) G + alpha sigma2 I) W = PX - P1 Y;
 *   a row with P1 = 0 has exactly alpha sigma2 on the diagonal of S, zeros beside it, and rhs 0.  1 <= M <= FSG_CHOL_MAX_N.
 * Fixed summation orders, no atomics, nothing read on the host: the same inputs give the same bits, alone or in a batch, and
 * every entry can be captured in a graph.  Bad arguments are FSG_ERR_ARG. */
#define FSG_CHOL_BLOCK 64       /* columns of a panel */
#define FSG_CHOL_MAX_N 8192     /* n, M */
#define FSG_CHOL_MAX_BATCH 65535 /* B */
#define FSG_CHOL_MAX_RHS 8      /* r */
int fsg_cholesky_f64(double *A, int B, int n, int32_t *info, fsg_stream_t stream);
int fsg_cholesky_solve_f64(const double *L, double *X, int B, int n, int r, fsg_stream_t stream);
int fsg_cpd_spd_system_f64(const double *G, const double *P1, const double *PX, const double *Y, const double *sigma2, double alpha,
                           int B, int M, double *S, double *rhs, double *d, fsg_stream_t stream);

/* The null-space Cholesky route of the thin-plate-spline fit (csrc/tps_nullspace.hip).  Stands in for the solve of TPS.fit,
 * shape_model/point_cloud_registration.py:32-52: the saddle point [[K, P], [P^T, 0]] [w; a] = [f; 0], K = u(|c_i - c_j|) +
 * lambda I exactly as fsg_tps_system_f64 writes it, P = [1 | c] (n x 4).  u is conditionally positive definite of order 2, so
 * with P = Q [R; 0] the block S = (Q^T K Q)[4:, 4:] of order m = n - 4 is symmetric positive definite for points that are
 * distinct (or lambda > 0) and not in one plane: w = Q [0; y] with S y = (Q^T f)[4:], and R a = (Q^T (f - K w))[:4].  ours, not
 * the reference's, which hands the indefinite system to an LU.  B independent items, DEVICE pointers, contiguous rows, fp64
 * but for control (B, n, 3) fp32; B <= 65535; n >= 1 and n - 4 <= FSG_CHOL_MAX_N; K is never stored.
 * fsg_tps_ns_system_f64: -> V (B, n, 4) the Householder vectors of P in LAPACK dgeqr2's convention (column k: zeros, a 1 at
 *   row k, the vector below; beta = -sign(alpha) |x|, tau = (beta - alpha) / beta, tau = 0 where nothing lies below alpha),
 *   tau (B, 4), R (B, 4, 4) upper triangular with zeros below, S (B, m, m) LOWER triangle only, the form fsg_cholesky_f64
 *   takes (not touched for n <= 4, where it may be NULL), and the rank status info (B) int32 DEVICE: 0, or -k (1-based) for the
 *   first |R_kk| that is not above n 2^-52 max_j |R_jj| (points in one plane, fewer than 4 points, a NaN).  The launches:
 *   the QR (one workgroup per item), X = K V with K on the fly, the dlatrd recurrence X -> W in place with
 *   Q^T K Q = K - V W^T - W V^T, and S_ij = K_(i+4)(j+4) - sum_k (V_(i+4)k W_(j+4)k + W_(i+4)k V_(j+4)k), one thread per entry.
 *   work: FSG_TPS_NS_SYSTEM_WORK_PER_POINT B n doubles (it holds W).
 * fsg_tps_ns_solve_f64: values (B, n, C) fp64, V, tau, R from above, L (B, m, m) the factor fsg_cholesky_f64 made of S (NULL
 *   allowed for n <= 4: no factorisation exists and fsg_cholesky_solve_f64 is not launched; w = 0) -> theta (B, n + 4, C): the
 *   n spline weights, then the affine rows.  1 <= C <= FSG_TPS_MAX_CHANNELS.  work: FSG_TPS_NS_SOLVE_WORK_PER_VALUE B n C
 *   doubles.  The theta of an item whose status or whose factorisation's status is not 0 is unspecified, never a fault; with
 *   fewer than 4 points its affine rows are NaN.
 * Fixed summation orders, no atomics, nothing read on the host: the same inputs give the same bits, alone or in a batch, and
 * both entries can be captured in a graph.  Bad arguments are FSG_ERR_ARG. */
#define FSG_TPS_NS_SYSTEM_WORK_PER_POINT 4 /* doubles of `work` per control point: W (n, 4) */
#define FSG_TPS_NS_SOLVE_WORK_PER_VALUE 2  /* doubles of `work` per value: Q^T f (n, C) and y (n - 4, C) */
int fsg_tps_ns_system_f64(const float *control, int B, int n, double lambd, double *V, double *tau, double *R, double *S,
                          int32_t *info, double *work, fsg_stream_t stream);
int fsg_tps_ns_solve_f64(const float *control, const double *values, const double *V, const double *tau, const double *R,
                         const double *L, int B, int n, int C, double lambd, double *work, double *theta, fsg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FSG_HIP_H */
