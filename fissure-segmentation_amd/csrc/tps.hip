// Thin-plate-spline interpolation of 3-D displacements -- include/fsg_hip.h: fsg_tps_system_f64, fsg_tps_eval_f32,
// fsg_tps_grid_sample_f32.
//
// The reference (shape_model/point_cloud_registration.py:24-89,119-133) fits a spline u(r) = r^2 log(r + 1e-6) on n control
// points, evaluates it on a coarse lattice of (D/4, H/4, W/4) nodes, upsamples that trilinearly to the full image and reads Q
// samples out of the dense field with grid_sample.  Both interpolations are linear, so one sample depends on at most 3 coarse
// nodes per axis; `grid_sample` below evaluates the spline at those 27 nodes only and never builds a lattice or a field.
//   system       one thread per entry of the (n+4, n+4) fp64 matrix of TPS.fit.  |c_i - c_j|^2 = ((dx dx + dy dy) + dz dz) on
//                the differences (fp64, of fp32 coordinates): (a - b)^2 and (b - a)^2 are the same bits, so the matrix is
//                symmetric bit for bit.  The diagonal is written as lambda itself.
//   eval         one lane per query (given, or implied by an align_corners=True lattice).  Control points and weights are
//                staged through LDS kChunk at a time and read as a broadcast; the sum over the control points runs in fp64 in
//                ascending order, one accumulator per channel.  u is evaluated in fp64: the weights sum to zero and
//                sum |w_j u_j| is thousands of times the result, so the rounding of u is what the result keeps.
//   grid_sample  32 lanes per sample, 27 of them own one coarse node each: the lane evaluates the spline there (the same loop
//                as eval), scales it by the node's composite weight, and lane 0 of the sample adds the 27 products in node order.
// No atomics, no scratch, no host read; the launch shape does not depend on B, and an item reads only its own rows.
#include <math.h>

#include "fsg_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 512;        // control points staged at a time: 8 KiB of float4 + 16 KiB of weights
constexpr int kMaxC = FSG_TPS_MAX_CHANNELS;
constexpr int kSlots = 32;         // lanes per sample in grid_sample; 27 carry a node
constexpr int kSamples = kThreads / kSlots;

__device__ __forceinline__ double tps_u(double d2) {
    const double r = sqrt(d2);
    return (r * r) * log(r + 1e-6);
}

// coordinate i of an align_corners=True lattice of L nodes over [-1, 1], rounded to fp32 (one node: 0, as affine_grid has it)
__device__ __forceinline__ float lattice_coord(int i, int L) {
    return L > 1 ? (float)(-1.0 + (2.0 * (double)i) / (double)(L - 1)) : 0.0f;
}

// a0 + a1 x + a2 y + a3 z + sum_j w_j u(|p - c_j|) for the lane's point p, every lane of the workgroup taking part in the
// staging.  tile / wts are the workgroup's LDS.
template <int C>
__device__ __forceinline__ void spline_at(float px, float py, float pz, const float *__restrict__ ctrl,
                                          const double *__restrict__ theta, int n, float4 *tile, double *wts, double (&out)[C]) {
    const int t = threadIdx.x;
    const double x = (double)px, y = (double)py, z = (double)pz;
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int j0 = 0; j0 < n; j0 += kChunk) {
        const int cnt = min(kChunk, n - j0);
        __syncthreads();
        for (int j = t; j < cnt; j += kThreads) {
            const float *r = ctrl + 3 * (size_t)(j0 + j);
            tile[j] = make_float4(r[0], r[1], r[2], 0.0f);
#pragma unroll
            for (int c = 0; c < C; ++c) wts[j * C + c] = theta[(size_t)(j0 + j) * C + c];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float4 r = tile[j];
            const double dx = x - (double)r.x, dy = y - (double)r.y, dz = z - (double)r.z;
            const double u = tps_u((dx * dx + dy * dy) + dz * dz);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + wts[j * C + c] * u;
        }
    }
    const double *a = theta + (size_t)n * C;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = (((a[c] + a[C + c] * x) + a[2 * C + c] * y) + a[3 * C + c] * z) + acc[c];
}

__global__ __launch_bounds__(kThreads) void tps_system_kernel(const float *__restrict__ ctrl, int n, double lambd,
                                                              double *__restrict__ A) {
    const int m = n + 4;
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (i >= m || j >= m) return;
    const float *c = ctrl + (size_t)b * n * 3;
    double v;
    if (i < n && j < n) {
        if (i == j) {
            v = lambd;
        } else {
            const double dx = (double)c[3 * i] - (double)c[3 * j], dy = (double)c[3 * i + 1] - (double)c[3 * j + 1],
                         dz = (double)c[3 * i + 2] - (double)c[3 * j + 2];
            v = tps_u((dx * dx + dy * dy) + dz * dz) + 0.0;   // (+ 0.0: the -0.0 of coincident points becomes the reference's 0.0)
        }
    } else if (i >= n && j >= n) {
        v = 0.0;
    } else {   // the [1 | c] border and its transpose
        const int p = i < n ? i : j, k = (i < n ? j : i) - n;
        v = k == 0 ? 1.0 : (double)c[3 * p + k - 1];
    }
    A[((size_t)b * m + i) * m + j] = v;
}

template <int C>
__global__ __launch_bounds__(kThreads) void tps_eval_kernel(const float *__restrict__ query, const float *__restrict__ ctrl,
                                                            const double *__restrict__ theta, int Q, int n, int H1, int W1,
                                                            int D1, float *__restrict__ out) {
    __shared__ float4 tile[kChunk];
    __shared__ double wts[kChunk * C];
    const int b = blockIdx.y, q = blockIdx.x * kThreads + threadIdx.x;
    const bool ok = q < Q;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (ok) {
        if (query) {
            const float *p = query + ((size_t)b * Q + q) * 3;
            px = p[0], py = p[1], pz = p[2];
        } else {
            const int ix = q % W1, iy = (q / W1) % H1, iz = q / (W1 * H1);
            px = lattice_coord(ix, W1), py = lattice_coord(iy, H1), pz = lattice_coord(iz, D1);
        }
    }
    double val[C];
    spline_at<C>(px, py, pz, ctrl + (size_t)b * n * 3, theta + (size_t)b * (n + 4) * C, n, tile, wts, val);
    if (ok) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[((size_t)b * Q + q) * C + c] = (float)val[c];
    }
}

// One axis of grid_sample(align_corners=False, zeros) on L fine voxels followed by the align_corners=True upsample from L1
// coarse nodes: normalised coordinate g -> first coarse node jb and the weights of jb, jb + 1, jb + 2.  A fine tap outside
// [0, L) is the zero padding and adds nothing; with both outside, every weight is 0 and jb = 0.
__device__ __forceinline__ void axis_weights(double g, int L, int L1, int &jb, double (&w)[3]) {
    w[0] = w[1] = w[2] = 0.0;
    jb = -1;
    const double pix = ((g + 1.0) * (double)L - 1.0) / 2.0;
    if (pix > -1.0 && pix < (double)L) {   // (false for a NaN as well)
        const double fl = floor(pix);
        const int i0 = (int)fl;
        const double f = pix - fl;
        const double scale = L > 1 ? (double)(L1 - 1) / (double)(L - 1) : 0.0;
#pragma unroll
        for (int tap = 0; tap < 2; ++tap) {
            const int i = i0 + tap;
            const double tw = tap ? f : 1.0 - f;
            if (i < 0 || i >= L) continue;
            const double src = scale * (double)i;
            const int j0 = min((int)src, L1 - 1);
            const int j1 = j0 + (j0 < L1 - 1 ? 1 : 0);
            const double lam = src - (double)j0;
            if (jb < 0) jb = j0;
            const int s0 = min(j0 - jb, 2), s1 = min(j1 - jb, 2);   // 0..1 and 0..2: consecutive fine voxels are < 1 node apart
            w[s0] = w[s0] + tw * (1.0 - lam);
            w[s1] = w[s1] + tw * lam;
        }
    }
    if (jb < 0) jb = 0;
}

template <int C>
__global__ __launch_bounds__(kThreads) void tps_grid_sample_kernel(const float *__restrict__ grid, const float *__restrict__ ctrl,
                                                                   const double *__restrict__ theta, int Q, int n, int D, int H,
                                                                   int W, int D1, int H1, int W1, float *__restrict__ out) {
    __shared__ float4 tile[kChunk];
    __shared__ double wts[kChunk * C];
    __shared__ double part[kSamples][kSlots][C];
    const int b = blockIdx.y, t = threadIdx.x, slot = t % kSlots, ls = t / kSlots;
    const int q = blockIdx.x * kSamples + ls;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    double wn = 0.0;
    if (q < Q && slot < 27) {
        const float *g = grid + ((size_t)b * Q + q) * 3;
        const int kx = slot % 3, ky = (slot / 3) % 3, kz = slot / 9;
        int jx, jy, jz;
        double wx[3], wy[3], wz[3];
        axis_weights((double)g[0], W, W1, jx, wx);
        axis_weights((double)g[1], H, H1, jy, wy);
        axis_weights((double)g[2], D, D1, jz, wz);
        wn = (wz[kz] * wy[ky]) * wx[kx];
        if (wn != 0.0) {   // (a node with a weight lies inside the lattice)
            px = lattice_coord(jx + kx, W1), py = lattice_coord(jy + ky, H1), pz = lattice_coord(jz + kz, D1);
        }
    }
    double val[C];
    spline_at<C>(px, py, pz, ctrl + (size_t)b * n * 3, theta + (size_t)b * (n + 4) * C, n, tile, wts, val);
#pragma unroll
    for (int c = 0; c < C; ++c) part[ls][slot][c] = wn != 0.0 ? wn * val[c] : 0.0;
    __syncthreads();
    if (q < Q && slot < C) {   // lane c of the sample adds channel c over the 27 nodes, in node order
        double s = 0.0;
        for (int k = 0; k < 27; ++k) s = s + part[ls][k][slot];
        out[((size_t)b * Q + q) * C + slot] = (float)s;
    }
}

int check(const char *who, int B, int Q, int n, int C) {
    FSG_REQUIRE(B >= 0 && B <= 65535 && Q >= 1 && n >= 1 && n <= (1 << 24) && C >= 1 && C <= kMaxC,
                "%s: bad shape B=%d Q=%d n=%d C=%d (Q, n >= 1, n <= 2^24, 1 <= C <= %d, B <= 65535)", who, B, Q, n, C, kMaxC);
    return FSG_OK;
}

}  // namespace

extern "C" int fsg_tps_system_f64(const float *control, int B, int n, double lambd, double *A, fsg_stream_t stream) {
    FSG_REQUIRE(B >= 0 && B <= 65535 && n >= 1 && n <= 32764, "fsg_tps_system_f64: bad shape B=%d n=%d (1 <= n <= 32764, B <= 65535)",
                B, n);
    FSG_REQUIRE(lambd == lambd, "fsg_tps_system_f64: lambda is not a number");
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(control && A, "fsg_tps_system_f64: NULL pointer");
    const int m = n + 4;
    hipLaunchKernelGGL(tps_system_kernel, dim3(fsg_cdiv(m, 64), fsg_cdiv(m, 4), B), dim3(kThreads), 0, (hipStream_t)stream, control,
                       n, lambd, A);
    FSG_CHECK_LAUNCH("fsg_tps_system_f64");
    return FSG_OK;
}

extern "C" int fsg_tps_eval_f32(const float *query, const float *control, const double *theta, int B, int Q, int n, int C, int D1,
                                int H1, int W1, float *out, fsg_stream_t stream) {
    int rc = check("fsg_tps_eval_f32", B, Q, n, C);
    if (rc != FSG_OK) return rc;
    if (!query)
        FSG_REQUIRE(D1 >= 1 && H1 >= 1 && W1 >= 1 && (long long)D1 * H1 * W1 == (long long)Q,
                    "fsg_tps_eval_f32: a lattice (%d, %d, %d) does not hold Q=%d queries", D1, H1, W1, Q);
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(control && theta && out, "fsg_tps_eval_f32: NULL pointer");
    const dim3 g(fsg_cdiv(Q, kThreads), B), blk(kThreads);
#define FSG_TPS_EVAL(CC)                                                                                                      \
    case CC:                                                                                                                  \
        hipLaunchKernelGGL(tps_eval_kernel<CC>, g, blk, 0, (hipStream_t)stream, query, control, theta, Q, n, H1, W1, D1, out); \
        break;
    switch (C) {
        FSG_TPS_EVAL(1)
        FSG_TPS_EVAL(2)
        FSG_TPS_EVAL(3)
        FSG_TPS_EVAL(4)
    }
#undef FSG_TPS_EVAL
    FSG_CHECK_LAUNCH("fsg_tps_eval_f32");
    return FSG_OK;
}

extern "C" int fsg_tps_grid_sample_f32(const float *grid, const float *control, const double *theta, int B, int Q, int n, int C,
                                       int D, int H, int W, int D1, int H1, int W1, float *out, fsg_stream_t stream) {
    int rc = check("fsg_tps_grid_sample_f32", B, Q, n, C);
    if (rc != FSG_OK) return rc;
    FSG_REQUIRE(D1 >= 1 && H1 >= 1 && W1 >= 1 && D1 <= D && H1 <= H && W1 <= W && D <= (1 << 24) && H <= (1 << 24) && W <= (1 << 24),
                "fsg_tps_grid_sample_f32: a coarse lattice (%d, %d, %d) under a fine grid (%d, %d, %d): need 1 <= coarse <= fine <= 2^24",
                D1, H1, W1, D, H, W);
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(grid && control && theta && out, "fsg_tps_grid_sample_f32: NULL pointer");
    const dim3 g(fsg_cdiv(Q, kSamples), B), blk(kThreads);
#define FSG_TPS_GS(CC)                                                                                                       \
    case CC:                                                                                                                 \
        hipLaunchKernelGGL(tps_grid_sample_kernel<CC>, g, blk, 0, (hipStream_t)stream, grid, control, theta, Q, n, D, H, W, D1, \
                           H1, W1, out);                                                                                     \
        break;
    switch (C) {
        FSG_TPS_GS(1)
        FSG_TPS_GS(2)
        FSG_TPS_GS(3)
        FSG_TPS_GS(4)
    }
#undef FSG_TPS_GS
    FSG_CHECK_LAUNCH("fsg_tps_grid_sample_f32");
    return FSG_OK;
}
