// Private interface between edgeconv.hip, which defines these launch functions, and the files that call them
// (edgeconv2.hip, bn_act.hip, chamfer.hip).  Not part of the C ABI (include/fsg_hip.h).
#pragma once
#include "fsg_common.h"

// ---- one-layer EdgeConv passes that the two-layer EdgeConv reuses
// statistics + per-point sums of layer 1 (ysel / arg untouched); it leaves fsg_ec_stats1_records(B, N) records in `partials`
int fsg_ec_stats1_records(int B, int N);
int fsg_ec_stats1_launch(const float *pq, const int32_t *idx, const float *gamma, int B, int N, int k, int Co,
                         float *ysel, uint8_t *arg, float *ssum, float *partials, hipStream_t st);
// BatchNorm + LeakyReLU on the selected values; _prep also emits the next graph build's prep products (and pq_next if w_next)
int fsg_ec_apply_launch(const float *ysel, const float *gamma, const float *beta, const float *mean, const float *invstd,
                        int B, int N, int Co, float slope, float *out, float *out_pm, hipStream_t st);
int fsg_ec_apply_prep_launch(const float *ysel, const float *gamma, const float *beta, const float *mean, const float *invstd,
                             int B, int N, int Co, float slope, float *out, float *out_pm, void *knn_ws, size_t knn_ws_bytes,
                             const float *w_next, float *pq_next, hipStream_t st);
// h = grad_out f'(u) on the selected edge, and dbeta / dgamma
int fsg_ec_bwd_point_launch(const float *gout, const float *gout_pm, long ld_pm, const float *gout_pm2, long ld_pm2,
                            const float *ysel, const float *gamma, const float *beta, const float *mean, const float *invstd,
                            int B, int N, int Co, float slope, float *h, float *partials, float *dbeta, float *dgamma,
                            hipStream_t st);

// ---- BatchNorm reductions, also behind bn_act.hip
// `partials` holds R records of 3*Co floats FOLLOWED by the fp64 stage area (fsg_ec_finalize_stage_floats(Co) floats)
size_t fsg_ec_finalize_stage_floats(int Co);
int fsg_ec_finalize_launch(const float *partials, int R, int Co, float eps, float momentum, float *mean, float *invstd,
                           float *running_mean, float *running_var, hipStream_t st);
// out0 (and out1 if nvec == 2) = the sum over R records of nvec vectors of L floats
int fsg_ec_sum_launch(const float *partials, int R, int L, int nvec, float *out0, float *out1, hipStream_t st);

// ---- reverse of a bipartite graph (NS sources x k slots -> N destinations), multi-workgroup builder; also behind chamfer.hip
int fsg_csr_bipartite_launch(const int32_t *idx, int B, int NS, int N, int k, int32_t *rowptr, int32_t *col, int32_t *cnt,
                             int32_t *tmp, hipStream_t st);
