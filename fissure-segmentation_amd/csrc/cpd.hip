// Coherent point drift, E-step (Myronenko & Song 2010, fig. 2 / eq. 6) -- include/fsg_hip.h: fsg_cpd_estep_f32.
//
// The reference registers its corresponding-point shapes with pycpd (shape_model/point_cloud_registration.py:101-116,231-232),
// whose E-step builds the dense (M, N) responsibility matrix P in numpy and reduces it three ways.  Here P is never stored:
//   columns  one thread per fixed point n walks the moving points: d_min[n] = min_m |x_n - ty_m|^2, then
//            S[n] = sum_m exp(-(d - d_min) / 2 sigma^2);  inv[n] = 1 / (S + c exp(d_min / 2 sigma^2)),  Pt1[n] = S inv
//   rows     one thread per moving point m walks the fixed points: p = exp(-(d - d_min[n]) / 2 sigma^2) inv[n],
//            P1[m] = sum_n p,  PX[m] = sum_n p x_n;  the first workgroup of an item also adds up Np
// with d_min and inv (fp64, 16 N bytes per item) as the only workspace.  Inputs, outputs and the exponentials are fp32; the
// distances, the exponent's argument, the sums and inv are carried in fp64 (a few multiply-adds per pair), so what is left of the
// error is the fp32 exponential's own rounding -- not the rounding of |x - y|^2, which at sigma^2 = 1 is multiplied by the
// size of the exponent, and not the order of summation.
//
// Distances are sums of squared differences -- never |x|^2 - 2 x.y + |y|^2, which cancels at millimetre coordinates.  The
// exponent is taken relative to the column's nearest moving point, so a column sum cannot underflow to 0 while the plain fp32
// formula loses whole columns once 2 sigma^2 is small against the squared distances.  Where exp(d_min / 2 sigma^2) overflows,
// the outlier term owns the column and its responsibilities are 0 -- the limit; with w = 0 there is no outlier term and every
// column sums to 1.
//
// A workgroup is 4 waves over 64 points: the lane is the point, the wave takes a quarter of every staged chunk of the other
// cloud (LDS, read as a broadcast).  Sums run in an order that depends on N and M only (4 interleaved accumulators per thread,
// the waves combined as (0 + 1) + (2 + 3)), there is no atomic, and a workgroup sees one item: the same inputs give the same
// bits, whatever else is in the batch.
#include <math.h>

#include "fsg_common.h"

namespace {

constexpr int kPoints = 64;                 // points a workgroup owns: one per lane
constexpr int kWaves = 4;                   // each takes a quarter of every staged chunk
constexpr int kThreads = kPoints * kWaves;
constexpr int kChunk = 1024;                // points of the other cloud staged in LDS at a time (16 KiB as float4)
constexpr int kAcc = 4;                     // interleaved accumulators per thread

// |a - q|^2 in fp64 from fp32 coordinates: the differences and squares are exact, the two additions round at 1e-16
__device__ __forceinline__ double dist2(float ax, float ay, float az, const float4 &q) {
    const double dx = (double)ax - (double)q.x, dy = (double)ay - (double)q.y, dz = (double)az - (double)q.z;
    return __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
}

// exp(arg), arg <= 0 in fp64, by the fp32 exponential: arg = hi + lo with hi its fp32 rounding, exp(arg) = exp(hi) (1 + lo) to
// first order (|lo| <= 2^-25 |arg|).  Rounding the argument alone would cost |arg| * 6e-8 of relative error -- at
// sigma^2 = 1 more than everything else in this file together.
__device__ __forceinline__ double exp_neg(double arg) {
    const float hi = (float)arg;
    const double e = (double)expf(hi);
    return __builtin_fma(e, arg - (double)hi, e);
}

// points [c0, c0 + kChunk) of src (count x 3) -> LDS as (x, y, z, 0); rows past `count` are not read by anyone
__device__ __forceinline__ void stage(const float *__restrict__ src, int c0, int count, float4 *tile) {
    for (int i = threadIdx.x; i < kChunk && c0 + i < count; i += kThreads) {
        const float *p = src + 3 * (size_t)(c0 + i);
        tile[i] = make_float4(p[0], p[1], p[2], 0.0f);
    }
}

// c = (2 pi sigma^2)^(3/2) w / (1 - w) M / N.  In fp64: it is evaluated once per column, and where the outlier term dominates
// the denominator (small clouds, large sigma^2) its rounding would be the rounding of every responsibility
__device__ __forceinline__ double outlier_constant(float s2, float w, int N, int M) {
    if (!(w > 0.0f)) return 0.0;
    const double v = 6.28318530717958647692 * (double)s2;
    return v * sqrt(v) * ((double)w / (1.0 - (double)w)) * ((double)M / (double)N);
}

__global__ __launch_bounds__(kThreads) void cpd_columns_kernel(const float *__restrict__ X, size_t x_stride,
                                                               const float *__restrict__ TY,
                                                               const float *__restrict__ sigma2, float w, int N, int M,
                                                               double *__restrict__ dmin_out, double *__restrict__ inv_out,
                                                               float *__restrict__ Pt1) {
    __shared__ float4 tile[kChunk];
    __shared__ double red[kWaves][kPoints];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * kPoints + lane;
    const bool ok = n < N;
    const float *x = X + b * x_stride + 3 * (size_t)(ok ? n : N - 1);
    const float *ty = TY + (size_t)b * M * 3;
    const float px = x[0], py = x[1], pz = x[2];
    const float s2 = sigma2[b];
    const double h = 0.5 / (double)s2;
    const bool one_chunk = M <= kChunk;

    double dmin = INFINITY;
    for (int c0 = 0; c0 < M; c0 += kChunk) {
        __syncthreads();
        stage(ty, c0, M, tile);
        __syncthreads();
        const int cnt = min(kChunk, M - c0), per = (cnt + kWaves - 1) / kWaves, lo = wave * per, hi = min(cnt, lo + per);
        for (int i = lo; i < hi; ++i) dmin = fmin(dmin, dist2(px, py, pz, tile[i]));
    }
    red[wave][lane] = dmin;
    __syncthreads();
    dmin = fmin(fmin(red[0][lane], red[1][lane]), fmin(red[2][lane], red[3][lane]));

    double acc[kAcc] = {};
    for (int c0 = 0; c0 < M; c0 += kChunk) {
        if (!one_chunk) {   // otherwise the tile of the first sweep is still there
            __syncthreads();
            stage(ty, c0, M, tile);
            __syncthreads();
        }
        const int cnt = min(kChunk, M - c0), per = (cnt + kWaves - 1) / kWaves, lo = wave * per, hi = min(cnt, lo + per);
        for (int i = lo; i < hi; i += kAcc) {
#pragma unroll
            for (int j = 0; j < kAcc; ++j) {
                if (i + j < hi) acc[j] += exp_neg((dmin - dist2(px, py, pz, tile[i + j])) * h);
            }
        }
    }
    __syncthreads();   // every wave has read the minima
    red[wave][lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (wave == 0 && ok) {
        const double S = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);   // >= 1: the nearest point adds exp(0)
        const double c = outlier_constant(s2, w, N, M);
        const double inv = 1.0 / (c > 0.0 ? S + c * exp(dmin * h) : S);   // exp overflows -> inv = 0
        const size_t o = (size_t)b * N + n;
        dmin_out[o] = dmin;
        inv_out[o] = inv;
        Pt1[o] = (float)(S * inv);
    }
}

__global__ __launch_bounds__(kThreads) void cpd_rows_kernel(const float *__restrict__ X, size_t x_stride,
                                                            const float *__restrict__ TY, const float *__restrict__ sigma2,
                                                            int N, int M, const double *__restrict__ dmin_in,
                                                            const double *__restrict__ inv_in, const float *__restrict__ Pt1,
                                                            float *__restrict__ P1, float *__restrict__ PX,
                                                            float *__restrict__ Np) {
    __shared__ float4 tile[kChunk];
    __shared__ double invs[kChunk], dmins[kChunk];
    __shared__ double red[kWaves][4][kPoints];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * kPoints + lane;
    const bool ok = m < M;
    const float *x = X + b * x_stride;
    const float *y = TY + ((size_t)b * M + (ok ? m : M - 1)) * 3;
    const double *dmin = dmin_in + (size_t)b * N, *inv = inv_in + (size_t)b * N;
    const float qx = y[0], qy = y[1], qz = y[2];
    const double h = 0.5 / (double)sigma2[b];

    double a1[kAcc] = {}, ax[kAcc] = {}, ay[kAcc] = {}, az[kAcc] = {};
    for (int c0 = 0; c0 < N; c0 += kChunk) {
        __syncthreads();
        stage(x, c0, N, tile);
        for (int i = threadIdx.x; i < kChunk && c0 + i < N; i += kThreads) {
            invs[i] = inv[c0 + i];
            dmins[i] = dmin[c0 + i];
        }
        __syncthreads();
        const int cnt = min(kChunk, N - c0), per = (cnt + kWaves - 1) / kWaves, lo = wave * per, hi = min(cnt, lo + per);
        for (int i = lo; i < hi; i += kAcc) {
#pragma unroll
            for (int j = 0; j < kAcc; ++j) {
                if (i + j < hi) {
                    const float4 q = tile[i + j];
                    const double p = exp_neg((dmins[i + j] - dist2(qx, qy, qz, q)) * h) * invs[i + j];
                    a1[j] += p;
                    ax[j] = __builtin_fma(p, (double)q.x, ax[j]);
                    ay[j] = __builtin_fma(p, (double)q.y, ay[j]);
                    az[j] = __builtin_fma(p, (double)q.z, az[j]);
                }
            }
        }
    }
    red[wave][0][lane] = (a1[0] + a1[1]) + (a1[2] + a1[3]);
    red[wave][1][lane] = (ax[0] + ax[1]) + (ax[2] + ax[3]);
    red[wave][2][lane] = (ay[0] + ay[1]) + (ay[2] + ay[3]);
    red[wave][3][lane] = (az[0] + az[1]) + (az[2] + az[3]);
    __syncthreads();
    if (wave == 0 && ok) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (float)((red[0][k][lane] + red[1][k][lane]) + (red[2][k][lane] + red[3][k][lane]));
        const size_t o = (size_t)b * M + m;
        P1[o] = r[0];
        PX[3 * o] = r[1];
        PX[3 * o + 1] = r[2];
        PX[3 * o + 2] = r[3];
    }
    if (blockIdx.x == 0) {   // Np = sum_mn P = sum_n Pt1[n]: the columns are complete (previous launch), so no workgroup waits
        double *s = &red[0][0][0];   // kThreads values
        __syncthreads();
        double acc = 0.0;
        for (int i = threadIdx.x; i < N; i += kThreads) acc += (double)Pt1[(size_t)b * N + i];
        s[threadIdx.x] = acc;
        __syncthreads();
        for (int step = kThreads / 2; step > 0; step >>= 1) {
            if ((int)threadIdx.x < step) s[threadIdx.x] += s[threadIdx.x + step];
            __syncthreads();
        }
        if (threadIdx.x == 0) Np[b] = (float)s[0];
    }
}

}  // namespace

extern "C" size_t fsg_cpd_estep_workspace_bytes(int B, int N, int M) {
    (void)M;
    if (B <= 0 || N <= 0) return 0;
    return (size_t)B * N * 2 * sizeof(double);
}

extern "C" int fsg_cpd_estep_f32(const float *X, int64_t x_batch_stride, const float *TY, const float *sigma2, float w, int B,
                                 int N, int M, float *P1, float *Pt1, float *PX, float *Np, void *workspace,
                                 size_t workspace_bytes, fsg_stream_t stream) {
    FSG_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && M >= 1 && N <= (1 << 24) && M <= (1 << 24),
                "fsg_cpd_estep_f32: bad shape B=%d N=%d M=%d", B, N, M);
    FSG_REQUIRE(w >= 0.0f && w < 1.0f, "fsg_cpd_estep_f32: outlier weight w=%g outside [0, 1)", (double)w);
    FSG_REQUIRE(x_batch_stride == 0 || x_batch_stride >= 3 * (int64_t)N,
                "fsg_cpd_estep_f32: x_batch_stride=%lld is neither 0 (one shared cloud) nor at least 3 N", (long long)x_batch_stride);
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(X && TY && sigma2 && P1 && Pt1 && PX && Np && workspace, "fsg_cpd_estep_f32: NULL pointer");
    FSG_REQUIRE(((uintptr_t)workspace & 7) == 0, "fsg_cpd_estep_f32: workspace must be 8-byte aligned");
    FSG_REQUIRE(workspace_bytes >= fsg_cpd_estep_workspace_bytes(B, N, M),
                "fsg_cpd_estep_f32: workspace of %zu bytes, %zu needed", workspace_bytes, fsg_cpd_estep_workspace_bytes(B, N, M));
    double *inv = (double *)workspace, *dmin = inv + (size_t)B * N;
    hipLaunchKernelGGL(cpd_columns_kernel, dim3(fsg_cdiv(N, kPoints), B), dim3(kThreads), 0, (hipStream_t)stream, X,
                       (size_t)x_batch_stride, TY, sigma2, w, N, M, dmin, inv, Pt1);
    FSG_CHECK_LAUNCH("fsg_cpd_estep_f32");
    hipLaunchKernelGGL(cpd_rows_kernel, dim3(fsg_cdiv(M, kPoints), B), dim3(kThreads), 0, (hipStream_t)stream, X,
                       (size_t)x_batch_stride, TY, sigma2, N, M, dmin, inv, Pt1, P1, PX, Np);
    FSG_CHECK_LAUNCH("fsg_cpd_estep_f32");
    return FSG_OK;
}
