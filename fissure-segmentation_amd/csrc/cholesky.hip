// Batched fp64 Cholesky factorisation and solve, and the symmetrised M-step system of deformable CPD -- include/fsg_hip.h:
// fsg_cholesky_f64, fsg_cholesky_solve_f64, fsg_cpd_spd_system_f64.
//
//   factor   a left-looking sweep over column panels of kNB = 64, one launch per panel, and one last launch for the diagonal
//            blocks.  In the launch of panel k the workgroup of row block i > k forms the stacked 128 x 64 block
//            [A_kk ; A_ik] - [L_k. ; L_i.] L_k.^T on v_mfma_f64_16x16x4_f64 (the rows L_k. are the B operand of both halves, so
//            recomputing the diagonal block costs matrix flops and no memory traffic), factors the diagonal half in LDS (unblocked,
//            left-looking: inner products from zero, one subtraction, a division by the root of the pivot), carries
//            its own half through the same column operations (that is A_ik L_kk^-T) and writes L_ik.  Nobody writes a diagonal
//            block while a launch may still read the matrix entries under it: the last launch, one workgroup per diagonal block,
//            recomputes every L_kk by the same instructions and writes it.  No workspace.
//   info     the pivot test is !(pivot > 0) on the value the root is taken of.  All workgroups of panel k see the same pivots;
//            the one of row block k + 1 records k0 + j (1-based) unless an earlier panel has, and the last launch does so for
//            the last block.  Plain stores ordered by the launches: no atomics.  Nothing returns early: a failed item runs
//            through its NaNs.
//   solve    one workgroup per item.  Forward L y = b left-looking, back L^T x = y likewise: a 64 x 64 block of L is staged in
//            LDS, thread (row | column, quarter) adds its 16 products for all right-hand sides, the four quarters are added in
//            order; the diagonal block is solved by one wave per right-hand side, lane = row, the pivot row's value handed
//            round by a wave shuffle.
//   system   one thread per entry of the lower triangle of S = D G D + alpha sigma^2 I, D = diag(sqrt(P1)).
// Summation orders are fixed by the shape alone, so an item has the same bits alone and in a batch.  Tails are predicated:
// rows and columns past n read as those of an identity and are never written.
#include <math.h>

#include "fsg_common.h"

namespace {

constexpr int kNB = FSG_CHOL_BLOCK;   // 64
constexpr int kThreads = 256;
constexpr int kKT = 32;               // columns of L staged per step of the panel product
constexpr int kKS = kKT + 1;          // their row stride in LDS
constexpr int kCS = kNB + 1;          // row stride of a staged 64-column block
constexpr int kMaxRhs = FSG_CHOL_MAX_RHS;
static_assert(kNB == 64 && kThreads == 4 * kNB, "the thread maps below are written for 64 x 64 blocks and four waves");

typedef double d4 __attribute__((ext_vector_type(4)));

// the staged block(s), row stride kCS, and the four partial sums per row of the in-block factorisation
constexpr size_t factor_lds_bytes(int MT) { return (size_t)MT * kNB * (kCS + 4) * sizeof(double); }

// MT = 2: panel launch, blockIdx.x -> row block i = k + 1 + blockIdx.x; writes L_ik.  MT = 1: diagonal launch, blockIdx.x -> k;
// writes L_kk.
template <int MT>
__global__ __launch_bounds__(kThreads) void chol_panel_kernel(double *__restrict__ Aall, int n, int kpanel, int nblk,
                                                              int *__restrict__ info) {
    extern __shared__ double lds[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.y;
    const int k = MT == 2 ? kpanel : (int)blockIdx.x;
    const int i = MT == 2 ? kpanel + 1 + (int)blockIdx.x : k;
    const int k0 = k * kNB, i0 = i * kNB;
    double *A = Aall + (size_t)b * n * n;

    // ---- S = [L_k. ; L_i.] L_k.^T over the columns [0, k0), wave w: row tiles w (diagonal half) and w + 4 (own half).  Every
    // staged step of kKT columns is summed from zero on the matrix pipe and then added to the running total: short sums of
    // small partial values keep the rounding of a long inner product near that of a pairwise sum.
    d4 tot[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) tot[m][ct] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int kt = 0; kt < k0; kt += kKT) {
        __syncthreads();
        {
            const int cc = t & 31, r0 = t >> 5;
#pragma unroll 4
            for (int p = 0; p < MT * kNB / 8; ++p) {
                const int row = r0 + 8 * p;
                const int grow = (row < kNB ? k0 : i0 - kNB) + row;
                lds[row * kKS + cc] = grow < n ? A[(size_t)grow * n + kt + cc] : 0.0;
            }
        }
        __syncthreads();
        d4 acc[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[m][ct] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < kKT / 4; ++kk) {
            const int off = (lane & 15) * kKS + kk * 4 + (lane >> 4);
            double bf[4], af[MT];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bf[ct] = lds[ct * 16 * kKS + off];
#pragma unroll
            for (int m = 0; m < MT; ++m) af[m] = lds[(w + 4 * m) * 16 * kKS + off];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (m == 0 && ct > w) continue;   // above the diagonal of the diagonal block (wave-uniform)
                    acc[m][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m], bf[ct], acc[m][ct], 0, 0, 0);
                }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) tot[m][ct] = tot[m][ct] + acc[m][ct];
    }
    __syncthreads();   // the staged columns are dead; the same LDS now holds the block itself, row stride kCS

    // ---- block = A - S (result layout of the fp64 instruction: col = lane & 15, row = (lane >> 4) + 4 reg)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            if (m == 0 && ct > w) continue;           // never read
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int rl = w * 16 + (lane >> 4) + 4 * reg, col = ct * 16 + (lane & 15);
                const int grow = (m == 0 ? k0 : i0) + rl;
                double v;
                if (m == 0) {
                    if (col > rl) v = 0.0;            // the strict upper triangle of A is not read
                    else if (grow < n) v = A[(size_t)grow * n + k0 + col] - tot[m][ct][reg];
                    else v = col == rl ? 1.0 : 0.0;   // past n: an identity, whose pivots pass
                } else {
                    v = grow < n ? A[(size_t)grow * n + k0 + col] - tot[m][ct][reg] : 0.0;
                }
                lds[(m * kNB + rl) * kCS + col] = v;
            }
        }

    // ---- factor the diagonal half, left-looking, and carry the own half along (that is A_ik L_kk^-T).  Column j: thread
    // (row r, wave w) sums the products of the columns k = w, w + 4, ... < j of its row(s) with row j, from zero; the four
    // partial sums are added in order and subtracted once; every thread forms the pivot itself (the same bits in all of them);
    // wave 0 divides the diagonal half's column by its root, wave 1 the own half's.  The root replaces the pivot one step
    // late: while column j is formed, the other threads still read the pivot.
    double *part = lds + MT * kNB * kCS;   // [4][MT * kNB]
    const int r = lane;
    int fail = 0;
    double root = 0.0;
    for (int j = 0; j < kNB; ++j) {
        __syncthreads();
        if (j > 0 && w == 0 && r == j - 1) lds[(j - 1) * kCS + j - 1] = root;
        double pD = 0.0, pR = 0.0;
        for (int k = w; k < j; k += 4) {
            const double lj = lds[j * kCS + k];
            if (r >= j) pD = fma(lds[r * kCS + k], lj, pD);
            if (MT == 2) pR = fma(lds[(kNB + r) * kCS + k], lj, pR);
        }
        part[w * MT * kNB + r] = pD;
        if (MT == 2) part[w * MT * kNB + kNB + r] = pR;
        __syncthreads();
        const double sj = ((part[j] + part[MT * kNB + j]) + part[2 * MT * kNB + j]) + part[3 * MT * kNB + j];
        const double p = lds[j * kCS + j] - sj;
        if (!(p > 0.0) && fail == 0) fail = j + 1;
        root = sqrt(p);
        if (w == 0 && r > j) {
            const double sr = ((part[r] + part[MT * kNB + r]) + part[2 * MT * kNB + r]) + part[3 * MT * kNB + r];
            lds[r * kCS + j] = (lds[r * kCS + j] - sr) / root;
        }
        if (MT == 2 && w == 1) {
            const int q = kNB + r;
            const double sr = ((part[q] + part[MT * kNB + q]) + part[2 * MT * kNB + q]) + part[3 * MT * kNB + q];
            lds[q * kCS + j] = (lds[q * kCS + j] - sr) / root;
        }
    }
    __syncthreads();
    if (w == 0 && r == kNB - 1) lds[r * kCS + r] = root;
    __syncthreads();

    // ---- out
    {
        const int col = lane;
        for (int rl = w; rl < kNB; rl += 4) {
            const int grow = i0 + rl;
            if (grow >= n) break;
            if (MT == 2) A[(size_t)grow * n + k0 + col] = lds[(kNB + rl) * kCS + col];
            else if (col <= rl) A[(size_t)grow * n + k0 + col] = lds[rl * kCS + col];
        }
    }
    const bool recorder = MT == 2 ? blockIdx.x == 0 : k == nblk - 1;
    if (recorder && t == 0) {
        if (k == 0) info[b] = fail;
        else if (fail != 0 && info[b] == 0) info[b] = k0 + fail;
    }
}

__device__ __forceinline__ double shfl_f64(double v, int src) { return __shfl(v, src, 64); }

__global__ __launch_bounds__(kThreads) void chol_solve_kernel(const double *__restrict__ Lall, double *__restrict__ Xall, int n,
                                                              int r) {
    __shared__ double tile[kNB * kCS];
    __shared__ double vec[kNB * kMaxRhs];             // the 64 solved values a block of L is multiplied with; 0 past r and n
    __shared__ double part[4 * kNB * kMaxRhs];
    const int t = threadIdx.x, lane = t & 63, q = t >> 6, b = blockIdx.x;
    const double *L = Lall + (size_t)b * n * n;
    double *X = Xall + (size_t)b * n * r;
    const int nblk = (n + kNB - 1) / kNB;

    for (int sweep = 0; sweep < 2; ++sweep) {         // 0: L y = b, blocks upward; 1: L^T x = y, blocks downward
        for (int step = 0; step < nblk; ++step) {
            const int k = sweep == 0 ? step : nblk - 1 - step, k0 = k * kNB;
            double acc[kMaxRhs];
#pragma unroll
            for (int rr = 0; rr < kMaxRhs; ++rr) acc[rr] = 0.0;
            for (int js = 0; js < step; ++js) {
                const int j = sweep == 0 ? js : nblk - 1 - js, j0 = j * kNB;
                // forward: the block L[k rows][j columns], thread = row of k; back: L[j rows][k columns], thread = column of k
                const int rb = sweep == 0 ? k0 : j0, cb = sweep == 0 ? j0 : k0;
                __syncthreads();
                for (int rl = q; rl < kNB; rl += 4)
                    tile[rl * kCS + lane] = (rb + rl < n && cb + lane < n) ? L[(size_t)(rb + rl) * n + cb + lane] : 0.0;
                for (int e = t; e < kNB * kMaxRhs; e += kThreads) {
                    const int row = e / kMaxRhs, rr = e % kMaxRhs;
                    vec[e] = (rr < r && j0 + row < n) ? X[(size_t)(j0 + row) * r + rr] : 0.0;
                }
                __syncthreads();
                for (int u = q * 16; u < q * 16 + 16; ++u) {
                    const double l = sweep == 0 ? tile[lane * kCS + u] : tile[u * kCS + lane];
#pragma unroll
                    for (int rr = 0; rr < kMaxRhs; ++rr) acc[rr] = fma(l, vec[u * kMaxRhs + rr], acc[rr]);
                }
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < kMaxRhs; ++rr) part[(q * kNB + lane) * kMaxRhs + rr] = acc[rr];
            for (int rl = q; rl < kNB; rl += 4) {     // the diagonal block; past n an identity
                const int gr = k0 + rl, gc = k0 + lane;
                tile[rl * kCS + lane] = (gr < n && lane <= rl) ? L[(size_t)gr * n + gc] : (lane == rl ? 1.0 : 0.0);
            }
            __syncthreads();
            for (int rr = q; rr < r; rr += 4) {       // one wave per right-hand side, lane = row
                const int gr = k0 + lane;
                double v = 0.0;
                if (gr < n) {
                    const double s = ((part[lane * kMaxRhs + rr] + part[(kNB + lane) * kMaxRhs + rr]) +
                                      part[(2 * kNB + lane) * kMaxRhs + rr]) + part[(3 * kNB + lane) * kMaxRhs + rr];
                    v = X[(size_t)gr * r + rr] - s;
                }
                if (sweep == 0) {
                    for (int j = 0; j < kNB; ++j) {
                        if (lane == j) v = v / tile[j * kCS + j];
                        const double vj = shfl_f64(v, j);
                        if (lane > j) v = fma(-tile[lane * kCS + j], vj, v);
                    }
                } else {
                    for (int j = kNB - 1; j >= 0; --j) {
                        if (lane == j) v = v / tile[j * kCS + j];
                        const double vj = shfl_f64(v, j);
                        if (lane < j) v = fma(-tile[j * kCS + lane], vj, v);
                    }
                }
                if (gr < n) X[(size_t)gr * r + rr] = v;
            }
            // (the barrier at the top of the next step orders these stores before the loads of `vec`)
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void cpd_spd_system_kernel(const double *__restrict__ G, const double *__restrict__ P1,
                                                                  const double *__restrict__ PX, const double *__restrict__ Y,
                                                                  const double *__restrict__ sigma2, double alpha, int M,
                                                                  double *__restrict__ S, double *__restrict__ rhs,
                                                                  double *__restrict__ d) {
    const int j = blockIdx.x * kThreads + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    if (j > i) return;
    const double *p1 = P1 + (size_t)b * M;
    const double pi = p1[i], di = sqrt(pi), dj = sqrt(p1[j]);
    const size_t e = ((size_t)b * M + i) * M + j;
    double v = (di * G[e]) * dj;
    if (i == j) v = v + alpha * sigma2[b];
    S[e] = v;
    if (j == 0) {
        const size_t row = ((size_t)b * M + i) * 3;
        d[(size_t)b * M + i] = di;
#pragma unroll
        for (int c = 0; c < 3; ++c) rhs[row + c] = di > 0.0 ? (PX[row + c] - pi * Y[row + c]) / di : 0.0;
    }
}

int check_shape(const char *who, int B, int n) {
    FSG_REQUIRE(B >= 0 && B <= FSG_CHOL_MAX_BATCH && n >= 1 && n <= FSG_CHOL_MAX_N, "%s: bad shape B=%d n=%d (1 <= n <= %d, B <= %d)",
                who, B, n, FSG_CHOL_MAX_N, FSG_CHOL_MAX_BATCH);
    return FSG_OK;
}

}  // namespace

extern "C" int fsg_cholesky_f64(double *A, int B, int n, int *info, fsg_stream_t stream) {
    int rc = check_shape("fsg_cholesky_f64", B, n);
    if (rc != FSG_OK) return rc;
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(A && info, "fsg_cholesky_f64: NULL pointer");
    FSG_GRANT_LDS("fsg_cholesky_f64", chol_panel_kernel<2>, factor_lds_bytes(2));
    const int nblk = fsg_cdiv(n, kNB);
    for (int k = 0; k + 1 < nblk; ++k)
        hipLaunchKernelGGL(chol_panel_kernel<2>, dim3(nblk - 1 - k, B), dim3(kThreads), factor_lds_bytes(2), (hipStream_t)stream, A, n,
                           k, nblk, info);
    hipLaunchKernelGGL(chol_panel_kernel<1>, dim3(nblk, B), dim3(kThreads), factor_lds_bytes(1), (hipStream_t)stream, A, n, 0, nblk,
                       info);
    FSG_CHECK_LAUNCH("fsg_cholesky_f64");
    return FSG_OK;
}

extern "C" int fsg_cholesky_solve_f64(const double *L, double *X, int B, int n, int r, fsg_stream_t stream) {
    int rc = check_shape("fsg_cholesky_solve_f64", B, n);
    if (rc != FSG_OK) return rc;
    FSG_REQUIRE(r >= 1 && r <= kMaxRhs, "fsg_cholesky_solve_f64: r=%d right-hand sides (1 <= r <= %d)", r, kMaxRhs);
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(L && X, "fsg_cholesky_solve_f64: NULL pointer");
    hipLaunchKernelGGL(chol_solve_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, L, X, n, r);
    FSG_CHECK_LAUNCH("fsg_cholesky_solve_f64");
    return FSG_OK;
}

extern "C" int fsg_cpd_spd_system_f64(const double *G, const double *P1, const double *PX, const double *Y, const double *sigma2,
                                      double alpha, int B, int M, double *S, double *rhs, double *d, fsg_stream_t stream) {
    int rc = check_shape("fsg_cpd_spd_system_f64", B, M);
    if (rc != FSG_OK) return rc;
    FSG_REQUIRE(alpha == alpha, "fsg_cpd_spd_system_f64: alpha is not a number");
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(G && P1 && PX && Y && sigma2 && S && rhs && d, "fsg_cpd_spd_system_f64: NULL pointer");
    hipLaunchKernelGGL(cpd_spd_system_kernel, dim3(fsg_cdiv(M, kThreads), M, B), dim3(kThreads), 0, (hipStream_t)stream, G, P1, PX, Y,
                       sigma2, alpha, M, S, rhs, d);
    FSG_CHECK_LAUNCH("fsg_cpd_spd_system_f64");
    return FSG_OK;
}
