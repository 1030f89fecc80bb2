// Point-cloud normal estimation on packed clouds -- include/fsg_hip.h: fsg_pcl_normals_f32.
// Replaces pytorch3d.ops.estimate_pointcloud_normals / estimate_pointcloud_local_coord_frames as models/dpsr_net.py:173-175
// calls them: per point the covariance of its k nearest neighbours (itself included), the eigenvectors of that 3 x 3 matrix,
// and the majority rule that orients them.  The neighbour lists come from fsg_knn_segment_f32 (csrc/pointops.hip).
//
// Lane mapping: G adjacent lanes per point (4 for K <= 32, 8 above).  Lane l of a group takes neighbours l, l + G, ... and
// keeps their offsets d = x_j - p in registers (NPL = 4 or 8 per lane: at most 24 VGPRs, where one lane per point would need
// 192; 16 per lane spilled), so the cloud is gathered ONCE, all loads of a lane in flight together, and the centred moments
// and the sign pass read registers.  Sums over the group are xor shuffles (a butterfly: a + b and b + a are the same bits, so
// all lanes of a group hold identical sums), the 3 x 3 eigenproblem runs redundantly on all of them, lane 0 writes.  One lane
// per point would leave the workload (8 x 2048 points) at 256 waves for 1024 SIMDs, each walking 30 gathers; four lanes give
// 1024 waves.
//
// The covariance is taken in two steps from the registers: the mean of d, then C = mean of (d - mean)(d - mean)^T.  (Moments
// about p corrected by the mean afterwards lose digits when the neighbourhood is the whole cloud, k = n - 1: there |mean d|
// is as large as the spread.)  The eigensolver is cyclic Jacobi with a fixed number of sweeps: no data dependent trip count
// (no divergence between lanes), rotations with a zero off-diagonal are the identity, and the vectors are a product of
// rotations, so a rank-deficient C (coincident, collinear or exactly planar neighbours) still gives an orthonormal finite
// frame.  fp32 throughout, no atomics, fixed summation order: the same input gives the same bits.
#include "fsg_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int SWEEPS = 6;      // cyclic Jacobi converges quadratically; a 3 x 3 fp32 matrix is diagonal to rounding after 4-5

// the sum over the G lanes of a group, the same bits in every lane
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// one Jacobi rotation in the (P, Q) plane: A <- J^T A J, V <- V J.  t is the smaller root of t^2 + 2 theta t - 1 = 0.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(float (&A)[3][3], float (&V)[3][3]) {
    constexpr int R = 3 - P - Q;
    const float apq = A[P][Q], app = A[P][P], aqq = A[Q][Q];
    const float theta = (aqq - app) / (2.f * apq);       // apq == 0: inf or NaN, unused; |theta| huge: t rounds to 0
    float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    t = apq != 0.f ? t : 0.f;
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
    A[P][P] = app - t * apq;
    A[Q][Q] = aqq + t * apq;
    A[P][Q] = A[Q][P] = 0.f;
    const float arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float vp = V[i][P], vq = V[i][Q];
        V[i][P] = c * vp - s * vq;
        V[i][Q] = s * vp + c * vq;
    }
}

// order columns a < b of (w, V) so that w[a] <= w[b]; selects, not branches
template <int a, int b>
__device__ __forceinline__ void order_pair(float (&w)[3], float (&V)[3][3]) {
    const bool sw = w[b] < w[a];
    const float wa = w[a], wb = w[b];
    w[a] = sw ? wb : wa;
    w[b] = sw ? wa : wb;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float va = V[i][a], vb = V[i][b];
        V[i][a] = sw ? vb : va;
        V[i][b] = sw ? va : vb;
    }
}

template <int G, int NPL>
__global__ __launch_bounds__(BLOCK) void pcl_normals_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ idx,
                                                             const int32_t *__restrict__ offset, int b, int n, int K,
                                                             int disambiguate, float *__restrict__ normals,
                                                             float *__restrict__ curvatures, float *__restrict__ frames) {
    const int q = (int)(((long)blockIdx.x * BLOCK + threadIdx.x) / G);
    const int l = threadIdx.x & (G - 1);
    if (q >= n) return;                                   // whole groups leave together: the shuffles stay inside a group
    // the segment of q: the first s with offset[s] > q (empty segments repeat an offset and are stepped over)
    int lo = 0, hi = b - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offset[mid] > q) hi = mid;
        else lo = mid + 1;
    }
    const int st = lo ? offset[lo - 1] : 0, en = offset[lo];
    int k = en - st - 1;                                  // k_s = min(K, n_s - 1), at least the point itself
    k = k < K ? k : K;
    k = k > 1 ? k : 1;
    const int32_t *row = idx + (long)q * K;               // only columns < k are read: knn_segment pads the rest
    const float px = xyz[3L * q], py = xyz[3L * q + 1], pz = xyz[3L * q + 2];

    float dx[NPL], dy[NPL], dz[NPL];                      // this lane's neighbours relative to p; 0 where it has none
#pragma unroll
    for (int t = 0; t < NPL; ++t) {
        const int j = l + t * G;
        dx[t] = dy[t] = dz[t] = 0.f;
        if (j < k) {
            int i = row[j];
            i = i < 0 ? 0 : (i < n ? i : n - 1);          // a bad index reads a wrong point, never outside the cloud
            dx[t] = xyz[3L * i] - px;
            dy[t] = xyz[3L * i + 1] - py;
            dz[t] = xyz[3L * i + 2] - pz;
        }
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NPL; ++t) {
        s0 += dx[t]; s1 += dy[t]; s2 += dz[t];
    }
    const float inv = 1.f / (float)k;
    const float mx = group_sum<G>(s0) * inv, my = group_sum<G>(s1) * inv, mz = group_sum<G>(s2) * inv;
    float m00 = 0.f, m01 = 0.f, m02 = 0.f, m11 = 0.f, m12 = 0.f, m22 = 0.f;
#pragma unroll
    for (int t = 0; t < NPL; ++t) {
        const bool has = l + t * G < k;
        const float ex = has ? dx[t] - mx : 0.f, ey = has ? dy[t] - my : 0.f, ez = has ? dz[t] - mz : 0.f;
        m00 += ex * ex; m01 += ex * ey; m02 += ex * ez;
        m11 += ey * ey; m12 += ey * ez; m22 += ez * ez;
    }
    float A[3][3], V[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
    A[0][0] = group_sum<G>(m00) * inv;
    A[1][1] = group_sum<G>(m11) * inv;
    A[2][2] = group_sum<G>(m22) * inv;
    A[0][1] = A[1][0] = group_sum<G>(m01) * inv;
    A[0][2] = A[2][0] = group_sum<G>(m02) * inv;
    A[1][2] = A[2][1] = group_sum<G>(m12) * inv;
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        jacobi_rotate<0, 1>(A, V);
        jacobi_rotate<0, 2>(A, V);
        jacobi_rotate<1, 2>(A, V);
    }
    float w[3] = {A[0][0], A[1][1], A[2][2]};
    order_pair<0, 1>(w, V);
    order_pair<1, 2>(w, V);
    order_pair<0, 1>(w, V);

    float nx = V[0][0], ny = V[1][0], nz = V[2][0];       // smallest eigenvalue: the normal
    float zx = V[0][2], zy = V[1][2], zz = V[2][2];       // largest
    if (disambiguate) {
        // the majority rule: v keeps its sign iff at least half of the k neighbours lie on its positive side (the point itself
        // has d = 0 and counts as "not positive"; so do a lane's empty slots, which add nothing to either count)
        int pos_n = 0, pos_z = 0;
#pragma unroll
        for (int t = 0; t < NPL; ++t) {
            pos_n += (nx * dx[t] + ny * dy[t] + nz * dz[t]) > 0.f;
            pos_z += (zx * dx[t] + zy * dy[t] + zz * dz[t]) > 0.f;
        }
        pos_n = group_sum<G>(pos_n);
        pos_z = group_sum<G>(pos_z);
        const float fn = 2 * pos_n < k ? -1.f : 1.f, fz = 2 * pos_z < k ? -1.f : 1.f;
        nx *= fn; ny *= fn; nz *= fn;
        zx *= fz; zy *= fz; zz *= fz;
    }
    if (l != 0) return;
    normals[3L * q] = nx; normals[3L * q + 1] = ny; normals[3L * q + 2] = nz;
    curvatures[3L * q] = w[0]; curvatures[3L * q + 1] = w[1]; curvatures[3L * q + 2] = w[2];
    if (frames) {                                         // columns (n, y = z x n, z)
        const float yx = zy * nz - zz * ny, yy = zz * nx - zx * nz, yz = zx * ny - zy * nx;
        float *f = frames + 9L * q;
        f[0] = nx; f[1] = yx; f[2] = zx;
        f[3] = ny; f[4] = yy; f[5] = zy;
        f[6] = nz; f[7] = yz; f[8] = zz;
    }
}

}  // namespace

extern "C" int fsg_pcl_normals_f32(const float *xyz, const int32_t *idx, const int32_t *offset, int b, int n, int K,
                                   int disambiguate, float *normals, float *curvatures, float *frames, fsg_stream_t stream) {
    FSG_REQUIRE(xyz && idx && offset && normals && curvatures, "fsg_pcl_normals_f32: NULL pointer");
    FSG_REQUIRE(b > 0 && n >= 0 && n <= (1 << 28) && K >= 2 && K <= FSG_PCL_NORMALS_MAX_K, "fsg_pcl_normals_f32: bad shape b=%d n=%d K=%d", b, n, K);
    if (n == 0) return FSG_OK;
    const int lanes = K <= 32 ? 4 : 8;
    const dim3 grid(fsg_cdiv((long)n * lanes, BLOCK)), block(BLOCK);
#define FSG_PCLN(G, NPL)                                                                                                   \
    hipLaunchKernelGGL((pcl_normals_kernel<G, NPL>), grid, block, 0, (hipStream_t)stream, xyz, idx, offset, b, n, K,       \
                       disambiguate ? 1 : 0, normals, curvatures, frames)
    if (K <= 16) FSG_PCLN(4, 4);
    else if (K <= 32) FSG_PCLN(4, 8);
    else FSG_PCLN(8, 8);
#undef FSG_PCLN
    FSG_CHECK_LAUNCH("fsg_pcl_normals_f32");
    return FSG_OK;
}
