// Private interface of the kNN translation units (knn_dense.hip, knn_rows_mfma.hip, knn_split.hip, knn_mfma.hip,
// knn_experiments.hip) and of the two files that call into them (edgeconv.hip, pointops.hip): the debug bits of `flags`, the
// cross-file launch functions and the cycle-stamp helper.  Not part of the C ABI (include/fsg_hip.h).
#pragma once
#include "fsg_common.h"

// ---- debug / cross-check bits of `flags`, above the public FSG_KNN_FIX_DIAG 1, _DROP_FIRST 2, _FORCE_ROWS 4, _FORCE_MFMA 8.
// The values are the FSG_KNN_DBG_* defines of include/fsg_hip.h (tests, tools and bench.py pass the numbers: they are fixed).
enum : int {
    KNN_DBG_HALF_CHUNKS = FSG_KNN_DBG_HALF_CHUNKS,   // two-phase kernel: 512-candidate chunks (k + drop <= 32, > 16 channels)
    KNN_DBG_TWO_PHASE = FSG_KNN_DBG_TWO_PHASE,       // the two-phase kernel (knn_rows_mfma.hip) instead of the split kernel
    KNN_DBG_ALL_SLOW = FSG_KNN_DBG_ALL_SLOW,         // split kernel: every query through the slow exact path
    KNN_DBG_STATS = FSG_KNN_DBG_STATS,               // split kernel: nominee statistics (fsg_debug_knn_split_stats)
    KNN_DBG_STAMPS = FSG_KNN_DBG_STAMPS,             // split kernel: cycle stamps (fsg_debug_knn_split_stamps / _refine_stamps);
                                                     // forces the two-launch form unless KNN_DBG_ONE_LAUNCH is set too
    KNN_DBG_ONE_LAUNCH = FSG_KNN_DBG_ONE_LAUNCH,     // split kernel: the one-launch (monolithic) kernel
    KNN_DBG_BF16 = FSG_KNN_DBG_BF16,                 // split kernel: the bf16 three-product form above 4 channels
};
// every bit a public entry accepts; anything else is FSG_ERR_ARG (a stale tool fails loudly instead of timing the default path)
constexpr int KNN_FLAGS_ALL = FSG_KNN_FIX_DIAG | FSG_KNN_DROP_FIRST | FSG_KNN_FORCE_ROWS | FSG_KNN_FORCE_MFMA | KNN_DBG_HALF_CHUNKS |
                              KNN_DBG_TWO_PHASE | KNN_DBG_ALL_SLOW | KNN_DBG_STATS | KNN_DBG_STAMPS | KNN_DBG_ONE_LAUNCH | KNN_DBG_BF16;
// bits that keep fsg_knn_dense_ws_f32 / fsg_knn_dense_ws_pq_f32 away from the split kernel
constexpr int KNN_BYPASS_SPLIT = KNN_DBG_TWO_PHASE | FSG_KNN_FORCE_ROWS | FSG_KNN_FORCE_MFMA | KNN_DBG_HALF_CHUNKS;

#define FSG_KNN_REQUIRE_FLAGS(entry, flags) \
    FSG_REQUIRE(!((flags) & ~KNN_FLAGS_ALL), "%s: unknown flag bit(s) %u (a removed debug bit?)", entry, (unsigned)((flags) & ~KNN_FLAGS_ALL))

// ---- launch functions.  All return FSG_ERR_UNSUPPORTED when the shape is outside the kernel's envelope (the caller falls back).
// knn_rows_mfma.hip: the two-phase kernel, and the packed-segment query on the same selection machinery
int fsg_knn_rows_mfma_launch(const float *x, int B, int N, int64_t stride_b, int64_t stride_c, int c_knn, int k, int flags,
                             int32_t *idx_out, float *dist_out, float *xx_scratch, hipStream_t st);
int fsg_knn_segment_rows_launch(const float *xyz, const float *new_xyz, const int32_t *offset, const int32_t *new_offset,
                                int b, int n, int m, int nsample, int32_t *idx, float *dist2, hipStream_t st);
// knn_mfma.hip (libfsg_hip_experiments.so): the first matrix-core kernel
int fsg_knn_mfma_launch(const float *x, int B, int N, int64_t stride_b, int64_t stride_c, int c_knn, int k, int flags,
                        int32_t *idx_out, float *dist_out, float *xx_scratch, hipStream_t st);

// knn_split.hip: the split kernel (coarse sweep + exact refine)
struct KnnSplitOpts {
    // the workspace already holds the prep products (squared norms, centred norms, fp16 image, scale: written by the producer of
    // the points, ec1_apply_prep_kernel) and this is the point-major (B, N, c_knn) copy of the points (c_knn a multiple of 16,
    // N % 64 == 0): the prep launch is skipped and x is not read
    const float *prepared_xt = nullptr;
    // also wanted: pq_out (B, N, pq_rows) = x^T pq_w^T (c_knn <= 4).  *pq_fused tells whether the build's first launch wrote it
    // (the no-prep path); otherwise the caller launches fsg_knn_pq_rows_launch itself
    const float *pq_w = nullptr;
    int pq_rows = 0;
    float *pq_out = nullptr;
    bool *pq_fused = nullptr;
};
size_t fsg_knn_split_workspace_bytes(int B, int N, int c_knn);
int fsg_knn_split_launch(const float *x, int B, int N, int64_t stride_b, int64_t stride_c, int c_knn, int k, int flags,
                         int32_t *idx_out, float *dist_out, void *ws, size_t ws_bytes, hipStream_t st, const KnnSplitOpts &o = {});
int fsg_knn_pq_rows_launch(const float *x, int B, int N, int64_t stride_b, int64_t stride_c, int c_knn, const float *pq_w,
                           int pq_rows, float *pq_out, hipStream_t st);
// where the prep products live inside the workspace (fp16 form, for a producer that emits them itself: edgeconv.hip)
int fsg_knn_split_ws_pointers(void *ws, size_t ws_bytes, int B, int N, int c_knn, float **xx, float **xs, void **cand,
                              float **cscale);

#ifdef __HIPCC__
// Cycle stamp (KNN_DBG_STAMPS): slot i of this wave <- the shader clock.  buf = [WGS workgroups][WPG waves][SLOTS], workgroups
// beyond the first WGS of the grid write nothing.  `on` is wave-uniform, so a launch without the flag pays one scalar branch.
template <int WGS, int WPG, int SLOTS>
__device__ __forceinline__ void knn_stamp(unsigned long long *buf, bool on, int wave, int lane, int i) {
    if (on) {
        const unsigned wg = blockIdx.x + gridDim.x * blockIdx.y;
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        if (wg < WGS && lane == 0) buf[(wg * WPG + wave) * SLOTS + i] = t;
    }
}
#endif
