// The null-space Cholesky route of the thin-plate-spline fit -- include/fsg_hip.h: fsg_tps_ns_system_f64, fsg_tps_ns_solve_f64.
//
// TPS.fit (shape_model/point_cloud_registration.py:32-52) solves the saddle point [[K, P], [P^T, 0]] [w; a] = [f; 0] with
// K = u(|c_i - c_j|) + lambda I and P = [1 | c] (n x 4).  u(r) = r^2 log r is conditionally positive definite of order 2, so K is
// positive definite on the null space of P^T.  With P = Q [R; 0], Q = H_0 H_1 H_2 H_3 (Householder, LAPACK dgeqr2's convention),
// P^T w = 0 means w = Q [0; y], the rows 4.. of Q^T K Q [0; y] + [R a; 0] = Q^T f are S y = g with S = (Q^T K Q)[4:, 4:]
// symmetric positive definite of order m = n - 4, and the rows 0..3 are R a = (Q^T (f - K w))[:4].
//   qr       one workgroup per item; thread t owns the rows t, t + 256, ... of the working copy of P, which lives in V.  Per
//            column: the squared norm below the pivot, beta = -sign(alpha) sqrt(alpha^2 + norm), tau = (beta - alpha) / beta,
//            v = x / (alpha - beta), then the reflector on the columns to the right.  tau = 0 where nothing lies below the pivot.
//   kblock   X = K B for a block B of NC <= 4 columns, K on the fly: one lane per row, the control points and the block's rows
//            staged through LDS kChunk at a time, the sum over j ascending, in runs of kSub products summed from zero and then
//            added to the running total (the rounding of a long sum stays near that of a pairwise one).
//   w        the dlatrd recurrence, one workgroup per item, X -> W in place: Q^T K Q = K - V W^T - W V^T.
//   reduced  one thread per entry of the lower triangle of S, u on the fly; the strict upper triangle is not written.
//   reflect  Q^T or Q on an (n, C) block, one workgroup per item, rows owned as in qr: g = (Q^T f)[4:]; w = Q [0; y];
//            a = R^-1 (Q^T (f - K w))[:4].
// K is the matrix of fsg_tps_system_f64 bit for bit: the same tps_u, the same difference form, lambda itself on the diagonal.
// Every sum over the points is a per-thread sum over the thread's rows in ascending order followed by a tree over the 256
// threads: fixed by n alone.  No atomics, no scratch, no host read; an item reads and writes only its own rows.
#include <math.h>

#include "fsg_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 512;        // control points staged at a time by kblock
constexpr int kSub = 16;           // products summed from zero before they join the running total
constexpr int kMaxC = FSG_TPS_MAX_CHANNELS;
static_assert(kMaxC <= 4 && FSG_TPS_NS_SYSTEM_WORK_PER_POINT == 4 && FSG_TPS_NS_SOLVE_WORK_PER_VALUE == 2,
              "kblock serves blocks of up to 4 columns; the work buffers are W (n, 4) and [T (n, C); Y (n - 4, C)]");

__device__ __forceinline__ double tps_u(double d2) {
    const double r = sqrt(d2);
    return (r * r) * log(r + 1e-6);
}

// entry (i, j) of K + lambda I as tps_system_kernel writes it; (xi, yi, zi) is row i's point
__device__ __forceinline__ double k_entry(bool diag, double xi, double yi, double zi, float4 cj, double lambd) {
    const double dx = xi - (double)cj.x, dy = yi - (double)cj.y, dz = zi - (double)cj.z;
    return diag ? lambd : tps_u((dx * dx + dy * dy) + dz * dz) + 0.0;
}

// v[c] <- the sum of v[c] over the workgroup, the same bits in every thread; red holds NV * kThreads doubles
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *red) {
    const int t = threadIdx.x;
    __syncthreads();   // (whoever still reads the last result)
#pragma unroll
    for (int c = 0; c < NV; ++c) red[c * kThreads + t] = v[c];
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < NV; ++c) red[c * kThreads + t] = red[c * kThreads + t] + red[c * kThreads + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = red[c * kThreads];
}

__global__ __launch_bounds__(kThreads) void ns_qr_kernel(const float *__restrict__ ctrl, int n, double *__restrict__ Vall,
                                                         double *__restrict__ tauall, double *__restrict__ Rall,
                                                         int *__restrict__ info) {
    __shared__ double red[4 * kThreads];
    __shared__ double piv[4][4];   // row k of the working matrix as step k found it
    const int t = threadIdx.x, b = blockIdx.x;
    const float *c = ctrl + (size_t)b * n * 3;
    double *V = Vall + (size_t)b * n * 4;
    for (int i = t; i < n; i += kThreads) {
        V[4 * i] = 1.0;
        V[4 * i + 1] = (double)c[3 * i], V[4 * i + 2] = (double)c[3 * i + 1], V[4 * i + 3] = (double)c[3 * i + 2];
    }
    double R[4][4], tau[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tau[k] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) R[k][j] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= n) continue;   // (uniform) no row left: R_kk = 0, H_k = I
        __syncthreads();
        if (t < 4) piv[k][t] = V[4 * k + t];   // (thread k wrote row k)
        double x2[1] = {0.0};
        for (int i = t; i < n; i += kThreads)
            if (i > k) x2[0] = x2[0] + V[4 * i + k] * V[4 * i + k];
        block_sum<1>(x2, red);
        const double alpha = piv[k][k];
        double beta = alpha, denom = 1.0;
        if (x2[0] != 0.0) {
            beta = -copysign(sqrt(alpha * alpha + x2[0]), alpha);
            tau[k] = (beta - alpha) / beta;
            denom = alpha - beta;
        }
        double d[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = t; i < n; i += kThreads)
            if (i > k) {
                const double v = x2[0] != 0.0 ? V[4 * i + k] / denom : 0.0;
                V[4 * i + k] = v;
#pragma unroll
                for (int j = k + 1; j < 4; ++j) d[j] = d[j] + v * V[4 * i + j];
            }
        block_sum<4>(d, red);
        R[k][k] = beta;
#pragma unroll
        for (int j = k + 1; j < 4; ++j) {
            d[j] = tau[k] * (piv[k][j] + d[j]);
            R[k][j] = piv[k][j] - d[j];
        }
        for (int i = t; i < n; i += kThreads)
            if (i > k) {
#pragma unroll
                for (int j = k + 1; j < 4; ++j) V[4 * i + j] = V[4 * i + j] - d[j] * V[4 * i + k];
            }
        if (t == k) {   // row k is final: v_{<k}[k], then 1, then zeros
            V[4 * k + k] = 1.0;
#pragma unroll
            for (int j = k + 1; j < 4; ++j) V[4 * k + j] = 0.0;
        }
    }
    if (t == 0) {
        double top = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) top = fmax(top, fabs(R[k][k]));   // (fmax passes over a NaN)
        const double thr = (double)n * 0x1p-52 * top;
        int st = 0;
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (!(fabs(R[k][k]) > thr)) st = -(k + 1);   // a NaN counts
        info[b] = st;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tauall[(size_t)b * 4 + k] = tau[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) Rall[(size_t)b * 16 + 4 * k + j] = R[k][j];
        }
    }
}

// out (n, NC) = (K + lambda I) blk, blk (n, NC) contiguous rows; both with their own item strides
template <int NC>
__global__ __launch_bounds__(kThreads) void ns_kblock_kernel(const float *__restrict__ ctrl, const double *__restrict__ blk,
                                                             size_t blk_stride, int n, double lambd, double *__restrict__ out,
                                                             size_t out_stride) {
    __shared__ float4 tile[kChunk];
    __shared__ double rows[kChunk * NC];
    const int t = threadIdx.x, b = blockIdx.y, i = blockIdx.x * kThreads + t;
    const float *c = ctrl + (size_t)b * n * 3;
    const double *bl = blk + (size_t)b * blk_stride;
    const bool ok = i < n;
    const double x = ok ? (double)c[3 * i] : 0.0, y = ok ? (double)c[3 * i + 1] : 0.0, z = ok ? (double)c[3 * i + 2] : 0.0;
    double tot[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) tot[cc] = 0.0;
    for (int j0 = 0; j0 < n; j0 += kChunk) {
        const int cnt = min(kChunk, n - j0);
        __syncthreads();
        for (int j = t; j < cnt; j += kThreads) {
            const float *r = c + 3 * (size_t)(j0 + j);
            tile[j] = make_float4(r[0], r[1], r[2], 0.0f);
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) rows[j * NC + cc] = bl[(size_t)(j0 + j) * NC + cc];
        }
        __syncthreads();
        for (int js = 0; js < cnt; js += kSub) {
            const int je = min(js + kSub, cnt);
            double acc[NC];
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) acc[cc] = 0.0;
            for (int j = js; j < je; ++j) {
                const double u = k_entry(j0 + j == i, x, y, z, tile[j], lambd);
#pragma unroll
                for (int cc = 0; cc < NC; ++cc) acc[cc] = acc[cc] + rows[j * NC + cc] * u;
            }
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) tot[cc] = tot[cc] + acc[cc];
        }
    }
    if (ok) {
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) out[(size_t)b * out_stride + (size_t)i * NC + cc] = tot[cc];
    }
}

// step K of the recurrence: p = tau_K (x_K - V_<K (W_<K^T v_K) - W_<K (V_<K^T v_K)), w_K = p - (tau_K / 2) (p^T v_K) v_K
template <int K>
__device__ __forceinline__ void w_step(const double *__restrict__ V, double *__restrict__ W, double tau, int n, double *red) {
    const int t = threadIdx.x;
    double d[2 * K + 1];   // W_<K^T v_K, then V_<K^T v_K (the last slot pads K = 0)
#pragma unroll
    for (int j = 0; j < 2 * K + 1; ++j) d[j] = 0.0;
    if (K > 0) {
        for (int i = t; i < n; i += kThreads) {
            const double v = V[4 * i + K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                d[j] = d[j] + W[4 * i + j] * v;
                d[K + j] = d[K + j] + V[4 * i + j] * v;
            }
        }
        block_sum<2 * K + 1>(d, red);
    }
    double s[1] = {0.0};
    for (int i = t; i < n; i += kThreads) {
        double p = W[4 * i + K];
#pragma unroll
        for (int j = 0; j < K; ++j) p = p - V[4 * i + j] * d[j];
#pragma unroll
        for (int j = 0; j < K; ++j) p = p - W[4 * i + j] * d[K + j];
        p = tau * p;
        W[4 * i + K] = p;
        s[0] = s[0] + p * V[4 * i + K];
    }
    block_sum<1>(s, red);
    const double h = (tau / 2.0) * s[0];
    for (int i = t; i < n; i += kThreads) W[4 * i + K] = W[4 * i + K] - h * V[4 * i + K];
}

__global__ __launch_bounds__(kThreads) void ns_w_kernel(const double *__restrict__ Vall, const double *__restrict__ tauall, int n,
                                                        double *__restrict__ Wall) {
    __shared__ double red[7 * kThreads];
    const int b = blockIdx.x;
    const double *V = Vall + (size_t)b * n * 4, *tau = tauall + (size_t)b * 4;
    double *W = Wall + (size_t)b * n * 4;
    w_step<0>(V, W, tau[0], n, red);
    w_step<1>(V, W, tau[1], n, red);
    w_step<2>(V, W, tau[2], n, red);
    w_step<3>(V, W, tau[3], n, red);
}

__global__ __launch_bounds__(kThreads) void ns_reduced_kernel(const float *__restrict__ ctrl, const double *__restrict__ Vall,
                                                              const double *__restrict__ Wall, int n, double lambd,
                                                              double *__restrict__ Sall) {
    const int m = n - 4;
    const int j = blockIdx.x * kThreads + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    if (j > i) return;   // (i < m by the grid)
    const float *c = ctrl + (size_t)b * n * 3, *ci = c + 3 * (i + 4), *cj = c + 3 * (j + 4);
    const double *Vi = Vall + ((size_t)b * n + i + 4) * 4, *Vj = Vall + ((size_t)b * n + j + 4) * 4;
    const double *Wi = Wall + ((size_t)b * n + i + 4) * 4, *Wj = Wall + ((size_t)b * n + j + 4) * 4;
    double s = k_entry(i == j, (double)ci[0], (double)ci[1], (double)ci[2], make_float4(cj[0], cj[1], cj[2], 0.0f), lambd);
#pragma unroll
    for (int k = 0; k < 4; ++k) s = s - (Vi[k] * Wj[k] + Wi[k] * Vj[k]);
    Sall[((size_t)b * m + i) * m + j] = s;
}

// mode 0: T = f, T <- Q^T T, Y = T[4:].  mode 1: theta[:n] = [0; Y], theta[:n] <- Q theta[:n].  mode 2: T = f - T, T <- Q^T T,
// theta[n:] = R^-1 T[:4].
template <int C>
__global__ __launch_bounds__(kThreads) void ns_reflect_kernel(int mode, const double *__restrict__ fall,
                                                              const double *__restrict__ Vall, const double *__restrict__ tauall,
                                                              const double *__restrict__ Rall, int n, double *__restrict__ Tall,
                                                              double *__restrict__ Yall, double *__restrict__ thall) {
    __shared__ double red[C * kThreads];
    const int t = threadIdx.x, b = blockIdx.x, m = n > 4 ? n - 4 : 0;
    const double *f = fall + (size_t)b * n * C, *V = Vall + (size_t)b * n * 4;
    double *Y = Yall + (size_t)b * m * C, *theta = thall + (size_t)b * (n + 4) * C;
    double *buf = mode == 1 ? theta : Tall + (size_t)b * n * C;
    for (int i = t; i < n; i += kThreads) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double v;
            if (mode == 0) v = f[(size_t)i * C + c];
            else if (mode == 1) v = i < 4 ? 0.0 : Y[(size_t)(i - 4) * C + c];
            else v = f[(size_t)i * C + c] - buf[(size_t)i * C + c];
            buf[(size_t)i * C + c] = v;
        }
    }
    for (int step = 0; step < 4; ++step) {
        const int k = mode == 1 ? 3 - step : step;
        if (k >= n) continue;   // (uniform)
        const double tau = tauall[(size_t)b * 4 + k];
        double d[C];
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = 0.0;
        for (int i = t; i < n; i += kThreads) {
            const double v = V[4 * i + k];
#pragma unroll
            for (int c = 0; c < C; ++c) d[c] = d[c] + v * buf[(size_t)i * C + c];
        }
        block_sum<C>(d, red);
        for (int i = t; i < n; i += kThreads) {
            const double v = V[4 * i + k];
#pragma unroll
            for (int c = 0; c < C; ++c) buf[(size_t)i * C + c] = buf[(size_t)i * C + c] - v * (tau * d[c]);
        }
    }
    if (mode == 0) {
        for (int i = t; i < n; i += kThreads)
            if (i >= 4) {
#pragma unroll
                for (int c = 0; c < C; ++c) Y[(size_t)(i - 4) * C + c] = buf[(size_t)i * C + c];
            }
    } else if (mode == 2) {
        __syncthreads();   // rows 0..3 belong to threads 0..3
        if (t < C) {
            const double *R = Rall + (size_t)b * 16;
            double a[4];
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                double s = k < n ? buf[(size_t)k * C + t] : __builtin_nan("");   // fewer than 4 points: no affine part
#pragma unroll
                for (int j = k + 1; j < 4; ++j) s = s - R[4 * k + j] * a[j];
                a[k] = s / R[4 * k + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) theta[(size_t)(n + k) * C + t] = a[k];
        }
    }
}

int check(const char *who, int B, int n, double lambd) {
    FSG_REQUIRE(B >= 0 && B <= 65535 && n >= 1 && n - 4 <= FSG_CHOL_MAX_N,
                "%s: bad shape B=%d n=%d (n >= 1, n - 4 <= %d, B <= 65535)", who, B, n, FSG_CHOL_MAX_N);
    FSG_REQUIRE(lambd == lambd, "%s: lambda is not a number", who);
    return FSG_OK;
}

template <int C>
int solve(const float *control, const double *values, const double *V, const double *tau, const double *R, const double *L, int B,
          int n, double lambd, double *work, double *theta, hipStream_t s) {
    const int m = n > 4 ? n - 4 : 0;
    double *T = work, *Y = work + (size_t)B * n * C;
    hipLaunchKernelGGL(ns_reflect_kernel<C>, dim3(B), dim3(kThreads), 0, s, 0, values, V, tau, R, n, T, Y, theta);
    if (m > 0) {
        const int rc = fsg_cholesky_solve_f64(L, Y, B, m, C, (fsg_stream_t)s);
        if (rc != FSG_OK) return rc;
    }
    hipLaunchKernelGGL(ns_reflect_kernel<C>, dim3(B), dim3(kThreads), 0, s, 1, values, V, tau, R, n, T, Y, theta);
    hipLaunchKernelGGL(ns_kblock_kernel<C>, dim3(fsg_cdiv(n, kThreads), B), dim3(kThreads), 0, s, control, (const double *)theta,
                       (size_t)(n + 4) * C, n, lambd, T, (size_t)n * C);
    hipLaunchKernelGGL(ns_reflect_kernel<C>, dim3(B), dim3(kThreads), 0, s, 2, values, V, tau, R, n, T, Y, theta);
    return FSG_OK;
}

}  // namespace

extern "C" int fsg_tps_ns_system_f64(const float *control, int B, int n, double lambd, double *V, double *tau, double *R, double *S,
                                     int32_t *info, double *work, fsg_stream_t stream) {
    int rc = check("fsg_tps_ns_system_f64", B, n, lambd);
    if (rc != FSG_OK) return rc;
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(control && V && tau && R && info && work && (S || n <= 4), "fsg_tps_ns_system_f64: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ns_qr_kernel, dim3(B), dim3(kThreads), 0, s, control, n, V, tau, R, info);
    hipLaunchKernelGGL(ns_kblock_kernel<4>, dim3(fsg_cdiv(n, kThreads), B), dim3(kThreads), 0, s, control, (const double *)V,
                       (size_t)n * 4, n, lambd, work, (size_t)n * 4);
    hipLaunchKernelGGL(ns_w_kernel, dim3(B), dim3(kThreads), 0, s, (const double *)V, (const double *)tau, n, work);
    if (n > 4)
        hipLaunchKernelGGL(ns_reduced_kernel, dim3(fsg_cdiv(n - 4, kThreads), n - 4, B), dim3(kThreads), 0, s, control,
                           (const double *)V, (const double *)work, n, lambd, S);
    FSG_CHECK_LAUNCH("fsg_tps_ns_system_f64");
    return FSG_OK;
}

extern "C" int fsg_tps_ns_solve_f64(const float *control, const double *values, const double *V, const double *tau, const double *R,
                                    const double *L, int B, int n, int C, double lambd, double *work, double *theta,
                                    fsg_stream_t stream) {
    int rc = check("fsg_tps_ns_solve_f64", B, n, lambd);
    if (rc != FSG_OK) return rc;
    FSG_REQUIRE(C >= 1 && C <= kMaxC, "fsg_tps_ns_solve_f64: C=%d channels (1 <= C <= %d)", C, kMaxC);
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(control && values && V && tau && R && work && theta && (L || n <= 4), "fsg_tps_ns_solve_f64: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: rc = solve<1>(control, values, V, tau, R, L, B, n, lambd, work, theta, s); break;
        case 2: rc = solve<2>(control, values, V, tau, R, L, B, n, lambd, work, theta, s); break;
        case 3: rc = solve<3>(control, values, V, tau, R, L, B, n, lambd, work, theta, s); break;
        default: rc = solve<4>(control, values, V, tau, R, L, B, n, lambd, work, theta, s); break;
    }
    if (rc != FSG_OK) return rc;
    FSG_CHECK_LAUNCH("fsg_tps_ns_solve_f64");
    return FSG_OK;
}
