// Triangle meshes -> voxel label maps -- include/fsg_hip.h: fsg_mesh_labelmap_dist_f32, fsg_mesh_labelmap_cover_f32.
// Replaces mesh2labelmap_dist (data_processing/surface_fitting_optimization.py:332-358: the distance of every voxel to every
// mesh through open3d on the CPU) and the sampling of o3d_mesh_to_labelmap / mesh2labelmap_sampling
// (data_processing/surface_fitting.py:144-169, :19-39: 10^7 random surface samples per mesh, scattered).
//
// Both are scatters over the triangles: a face can only label the few voxels next to it, so the work is distributed over
// the faces of ALL meshes of a call (packed, one label per face), one wave per face.  The wave computes the face's bounding
// box in voxel indices -- in float, clipped to the volume BEFORE anything becomes an integer, so that no index is ever
// formed from a coordinate outside the volume (a vertex at 1e30 or Inf clips like any other; a NaN makes the box empty) --
// and its lanes walk the voxels of the box in row-major order, last axis fastest, 64 at a time.  Box limits are widened by
// 1e-3 of a voxel before rounding so that the division by the spacing cannot lose a voxel; the exact test below decides.
//
// distance band: box grown by the threshold; the squared distance from the voxel centre (i0 s0, i1 s1, i2 s2) to the face
//   is point_face of point_face.h, the arithmetic of point_mesh.hip; where it is <= threshold^2 the lane issues ONE 64-bit
//   unsigned atomic min of (float bits of d^2 << 32) | mesh into the key volume (d^2 >= +0, so the bit pattern orders like the
//   value; equal d^2: the lower mesh).  A second kernel turns keys into labels 1 + mesh (0 where no key was written or
//   the mask is clear).  Min commutes, so the result does not depend on the order of arrival: bitwise reproducible.
// coverage: box not grown; cell (i0, i1, i2) is [i s, (i + 1) s) per axis and is tested against the triangle by separating
//   axes: the 3 box axes (half-open: a triangle lying in the upper face of a cell belongs to the next cell, as floor() puts
//   it), the face normal and the 9 cross products of a box axis and an edge (closed).  A face without area needs no case of
//   its own: its normal is 0 and says nothing, the projections of the triangle are those of its longest edge, and the nine
//   cross products are then the segment-box axes (a point: only the box axes are left).  A hit is one 64-bit atomic max of
//   1 + mesh straight into the int64 output (zeroed before), so later meshes win like the reference's overwriting.
//
// Cost: a wave spends ceil(box voxels / 64) steps of ~120 (band) / ~260 (coverage) VALU issues on its face.  Fissure meshes
// have boxes of 30-400 voxels.  A face whose box is the whole volume is handled by the same loop, by ONE wave: 128^3 voxels
// are 32 768 steps.  Nothing is allocated here: the key volume comes from the caller.
#include "point_face.h"

namespace {

constexpr int WAVES = 4;             // faces per workgroup
constexpr float SLACK = 1e-3f;       // voxels by which a box limit is widened before it is rounded to an index

struct Box {
    int lo0, lo1, lo2;               // first voxel per axis
    uint32_t m1, m2, count;          // extent along axes 1 and 2, number of voxels (0: nothing to do)
};

// [lo, hi] in world units -> index range [first, last] of one axis, clipped to [0, n - 1] in float; false if empty.
// `cells`: indices are floor(x / s) (coverage) instead of the voxel centres i s inside [lo, hi] (band).
__device__ __forceinline__ bool axis_range(float lo, float hi, float s, int n, bool cells, int &first, int &last) {
    if (!(lo <= hi)) return false;                                        // NaN
    const float qlo = lo / s - SLACK, qhi = hi / s + SLACK;
    const float flo = fmaxf(cells ? floorf(qlo) : ceilf(qlo), 0.f);
    const float fhi = fminf(floorf(qhi), fminf((float)(n - 1), 2147483520.f));   // the largest float that fits an int
    if (!(flo <= fhi)) return false;                                      // outside the volume (or NaN from Inf / Inf)
    first = min((int)flo, n - 1);                                         // (float)(n - 1) may have rounded up
    last = min((int)fhi, n - 1);
    return true;
}

__device__ __forceinline__ Box face_box(const float *__restrict__ verts, const int32_t *__restrict__ f, int n0, int n1, int n2,
                                        float s0, float s1, float s2, float grow, bool cells) {
    const float *pa = verts + (long)f[0] * 3, *pb = verts + (long)f[1] * 3, *pc = verts + (long)f[2] * 3;
    Box b = {0, 0, 0, 0u, 0u, 0u};
    int hi0, hi1, hi2;
    if (!axis_range(fminf(fminf(pa[0], pb[0]), pc[0]) - grow, fmaxf(fmaxf(pa[0], pb[0]), pc[0]) + grow, s0, n0, cells, b.lo0, hi0) ||
        !axis_range(fminf(fminf(pa[1], pb[1]), pc[1]) - grow, fmaxf(fmaxf(pa[1], pb[1]), pc[1]) + grow, s1, n1, cells, b.lo1, hi1) ||
        !axis_range(fminf(fminf(pa[2], pb[2]), pc[2]) - grow, fmaxf(fmaxf(pa[2], pb[2]), pc[2]) + grow, s2, n2, cells, b.lo2, hi2))
        return b;
    // fminf / fmaxf drop a NaN operand: a face with one NaN vertex would get the box of the others
    if (!(pa[0] == pa[0] && pa[1] == pa[1] && pa[2] == pa[2] && pb[0] == pb[0] && pb[1] == pb[1] && pb[2] == pb[2] &&
          pc[0] == pc[0] && pc[1] == pc[1] && pc[2] == pc[2]))
        return b;
    b.m1 = (uint32_t)(hi1 - b.lo1 + 1);
    b.m2 = (uint32_t)(hi2 - b.lo2 + 1);
    b.count = (uint32_t)(hi0 - b.lo0 + 1) * b.m1 * b.m2;                  // <= n0 n1 n2 < 2^31
    return b;
}

// the l-th voxel of the box, row-major
__device__ __forceinline__ void box_voxel(const Box &b, uint32_t l, int &i0, int &i1, int &i2) {
    const uint32_t t = l / b.m2;
    i2 = b.lo2 + (int)(l - t * b.m2);
    const uint32_t u = t / b.m1;
    i1 = b.lo1 + (int)(t - u * b.m1);
    i0 = b.lo0 + (int)u;
}

__global__ __launch_bounds__(WAVES * 64) void labelmap_dist_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                    const int32_t *__restrict__ labels, int F, int n0, int n1,
                                                                    int n2, float s0, float s1, float s2, float thr, float thr2,
                                                                    unsigned long long *__restrict__ keys) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int face = blockIdx.x * WAVES + wave;
    if (face >= F) return;
    const int32_t *f = faces + (long)face * 3;
    const Box b = face_box(verts, f, n0, n1, n2, s0, s1, s2, thr, false);
    if (b.count == 0u) return;
    float4 r[REC];
    face_record(verts, f, r);
    const unsigned long long label = (unsigned long long)(uint32_t)labels[face];
    for (uint32_t l = lane; l < b.count; l += 64) {
        int i0, i1, i2;
        box_voxel(b, l, i0, i1, i2);
        float s, t;
        const float d = point_face((float)i0 * s0, (float)i1 * s1, (float)i2 * s2, r, s, t);
        if (d <= thr2)
            __hip_atomic_fetch_min(keys + ((long)i0 * n1 + i1) * n2 + i2,
                                   ((unsigned long long)__builtin_bit_cast(uint32_t, d) << 32) | label, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void labelmap_decode_kernel(const unsigned long long *__restrict__ keys,
                                                               const uint8_t *__restrict__ mask, long n, int64_t *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    out[i] = (k != ~0ull && (!mask || mask[i])) ? 1 + (int64_t)(uint32_t)k : 0;
}

// does the axis (ax, ay, az) separate the triangle u, v, w (relative to the box centre) from the box of half sizes h?
__device__ __forceinline__ bool separates(float ax, float ay, float az, const float *u, const float *v, const float *w, float h0,
                                          float h1, float h2) {
    const float pu = dot3(ax, ay, az, u[0], u[1], u[2]), pv = dot3(ax, ay, az, v[0], v[1], v[2]);
    const float pw = dot3(ax, ay, az, w[0], w[1], w[2]);
    const float rad = __builtin_fmaf(h2, fabsf(az), __builtin_fmaf(h1, fabsf(ay), h0 * fabsf(ax)));
    return fminf(fminf(pu, pv), pw) > rad || fmaxf(fmaxf(pu, pv), pw) < -rad;
}

__global__ __launch_bounds__(WAVES * 64) void labelmap_cover_kernel(const float *__restrict__ verts,
                                                                     const int32_t *__restrict__ faces,
                                                                     const int32_t *__restrict__ labels, int F, int n0, int n1,
                                                                     int n2, float s0, float s1, float s2,
                                                                     unsigned long long *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int face = blockIdx.x * WAVES + wave;
    if (face >= F) return;
    const int32_t *f = faces + (long)face * 3;
    const Box b = face_box(verts, f, n0, n1, n2, s0, s1, s2, 0.f, true);
    if (b.count == 0u) return;
    const float *pa = verts + (long)f[0] * 3, *pb = verts + (long)f[1] * 3, *pc = verts + (long)f[2] * 3;
    const float e[3][3] = {{pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]}, {pc[0] - pb[0], pc[1] - pb[1], pc[2] - pb[2]},
                           {pa[0] - pc[0], pa[1] - pc[1], pa[2] - pc[2]}};
    const float nx = __builtin_fmaf(e[0][1], e[1][2], -(e[0][2] * e[1][1])), ny = __builtin_fmaf(e[0][2], e[1][0], -(e[0][0] * e[1][2]));
    const float nz = __builtin_fmaf(e[0][0], e[1][1], -(e[0][1] * e[1][0]));
    const float lo[3] = {fminf(fminf(pa[0], pb[0]), pc[0]), fminf(fminf(pa[1], pb[1]), pc[1]), fminf(fminf(pa[2], pb[2]), pc[2])};
    const float hi[3] = {fmaxf(fmaxf(pa[0], pb[0]), pc[0]), fmaxf(fmaxf(pa[1], pb[1]), pc[1]), fmaxf(fmaxf(pa[2], pb[2]), pc[2])};
    const float h0 = 0.5f * s0, h1 = 0.5f * s1, h2 = 0.5f * s2;
    const unsigned long long label = 1ull + (uint32_t)labels[face];
    for (uint32_t l = lane; l < b.count; l += 64) {
        int i0, i1, i2;
        box_voxel(b, l, i0, i1, i2);
        // the box axes, half-open: the triangle has to reach below the cell's upper limit and to its lower limit or above
        const float c0 = (float)i0 * s0, c1 = (float)i1 * s1, c2 = (float)i2 * s2;
        if (!(lo[0] < c0 + s0 && hi[0] >= c0 && lo[1] < c1 + s1 && hi[1] >= c1 && lo[2] < c2 + s2 && hi[2] >= c2)) continue;
        const float m0 = c0 + h0, m1 = c1 + h1, m2 = c2 + h2;
        const float u[3] = {pa[0] - m0, pa[1] - m1, pa[2] - m2}, v[3] = {pb[0] - m0, pb[1] - m1, pb[2] - m2};
        const float w[3] = {pc[0] - m0, pc[1] - m1, pc[2] - m2};
        bool apart = separates(nx, ny, nz, u, v, w, h0, h1, h2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                     // (1,0,0) x e, (0,1,0) x e, (0,0,1) x e
            apart = apart || separates(0.f, -e[k][2], e[k][1], u, v, w, h0, h1, h2) ||
                    separates(e[k][2], 0.f, -e[k][0], u, v, w, h0, h1, h2) || separates(-e[k][1], e[k][0], 0.f, u, v, w, h0, h1, h2);
        }
        if (!apart)
            __hip_atomic_fetch_max(out + ((long)i0 * n1 + i1) * n2 + i2, label, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the checks both entry points share; n: the number of voxels
int check_volume(const char *who, const void *verts, const void *faces, const void *labels, const void *out, int V, int F, int d0,
                 int d1, int d2, float s0, float s1, float s2, long *n) {
    FSG_REQUIRE(verts && faces && labels && out, "%s: NULL pointer", who);
    FSG_REQUIRE(V > 0 && F > 0 && d0 > 0 && d1 > 0 && d2 > 0, "%s: bad shape V=%d F=%d volume %d x %d x %d", who, V, F, d0, d1, d2);
    FSG_REQUIRE(s0 > 0.f && s1 > 0.f && s2 > 0.f && s0 < INFINITY && s1 < INFINITY && s2 < INFINITY,
                "%s: spacing (%g, %g, %g) must be positive and finite", who, s0, s1, s2);
    *n = (long)d0 * d1 * d2;
    FSG_REQUIRE(*n < (1L << 31), "%s: volume %d x %d x %d has 2^31 voxels or more", who, d0, d1, d2);
    return FSG_OK;
}

}  // namespace

extern "C" int fsg_mesh_labelmap_dist_f32(const float *verts, const int32_t *faces, const int32_t *labels, int V, int F, int d0,
                                          int d1, int d2, float s0, float s1, float s2, float dist_threshold,
                                          const uint8_t *mask, uint64_t *keys, int64_t *out, fsg_stream_t stream) {
    long n = 0;
    if (int rc = check_volume("fsg_mesh_labelmap_dist_f32", verts, faces, labels, out, V, F, d0, d1, d2, s0, s1, s2, &n)) return rc;
    FSG_REQUIRE(keys, "fsg_mesh_labelmap_dist_f32: NULL pointer (key volume)");
    FSG_REQUIRE(dist_threshold >= 0.f, "fsg_mesh_labelmap_dist_f32: threshold %g is negative or NaN", dist_threshold);
    if (hipMemsetAsync(keys, 0xff, (size_t)n * 8, (hipStream_t)stream) != hipSuccess) {
        fsg_set_error("fsg_mesh_labelmap_dist_f32: cannot initialise the key volume");
        return FSG_ERR_HIP;
    }
    hipLaunchKernelGGL(labelmap_dist_kernel, dim3(fsg_cdiv(F, WAVES)), dim3(WAVES * 64), 0, (hipStream_t)stream, verts, faces, labels,
                       F, d0, d1, d2, s0, s1, s2, dist_threshold, dist_threshold * dist_threshold, (unsigned long long *)keys);
    FSG_CHECK_LAUNCH("fsg_mesh_labelmap_dist_f32");
    hipLaunchKernelGGL(labelmap_decode_kernel, dim3(fsg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long *)keys, mask, n, out);
    FSG_CHECK_LAUNCH("fsg_mesh_labelmap_dist_f32");
    return FSG_OK;
}

extern "C" int fsg_mesh_labelmap_cover_f32(const float *verts, const int32_t *faces, const int32_t *labels, int V, int F, int d0,
                                           int d1, int d2, float s0, float s1, float s2, int64_t *out, fsg_stream_t stream) {
    long n = 0;
    if (int rc = check_volume("fsg_mesh_labelmap_cover_f32", verts, faces, labels, out, V, F, d0, d1, d2, s0, s1, s2, &n)) return rc;
    if (hipMemsetAsync(out, 0, (size_t)n * 8, (hipStream_t)stream) != hipSuccess) {
        fsg_set_error("fsg_mesh_labelmap_cover_f32: cannot clear the output");
        return FSG_ERR_HIP;
    }
    hipLaunchKernelGGL(labelmap_cover_kernel, dim3(fsg_cdiv(F, WAVES)), dim3(WAVES * 64), 0, (hipStream_t)stream, verts, faces, labels,
                       F, d0, d1, d2, s0, s1, s2, (unsigned long long *)out);
    FSG_CHECK_LAUNCH("fsg_mesh_labelmap_cover_f32");
    return FSG_OK;
}
