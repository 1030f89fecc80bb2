// The project's point-triangle arithmetic, shared by point_mesh.hip (distance of query points to a mesh) and voxelize.hip
// (distance band of a mesh on a voxel grid): every file that includes this evaluates a (point, face) pair with the same
// instructions in the same order, so their distances agree bit for bit.
//
// The pair evaluation has no case split.  With p = q - a the closest point is a + s ab + t ac for one of four candidate
// (s, t), each of which is a point OF the triangle whatever the rounding:
//   edge AB (clamp(p.ab / |ab|^2), 0)      edge AC (0, clamp(p.ac / |ac|^2))      edge BC (1 - u, u), u = clamp(bp.bc / |bc|^2)
//   plane   (v, w) = (clamp(p.m1, 0, 1), clamp(p.m2, 0, 1 - v)),  m1 = ac x n / |n|^2, m2 = n x ab / |n|^2, n = ab x ac
// and the distance is the smallest |p - s ab - t ac|^2, evaluated as a difference (never through the expanded quadratic,
// whose cancellation costs 1e-3 in the distance next to the surface).  If the projection falls inside, the plane candidate
// is it; if not, the closest point is on the boundary, i.e. on one of the three segments -- so the minimum over the four is
// exact, and a candidate that rounding moved can only be an upper bound of it.  A face without area (|n|^2 <= 1e-10 |ab|^2
// |ac|^2, sin < 1e-5) gets m1 = m2 = 0, whose candidate is the vertex a, and a collapsed edge gets the reciprocal 0, whose
// candidate is its end point: such faces yield the distance to their longest edge / to the point, never NaN or Inf.
#pragma once
#include "fsg_common.h"

namespace {

constexpr int REC = 5;               // float4 per face record
constexpr float NO_AREA = 1e-10f;    // |n|^2 <= NO_AREA |ab|^2 |ac|^2: no plane candidate
constexpr float TINY = 1e-30f;       // squared lengths at or below this count as zero (their reciprocal would overflow)

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

__device__ __forceinline__ float clamp01(float x, float hi) { return __builtin_amdgcn_fmed3f(x, 0.f, hi); }

// 1 / e, rounded so that e * result >= 1 (0 for no length): a query that IS the far end of an edge then has the parameter
// d / e = e / e clamped to exactly 1, its residual is exactly 0, and a mesh is at distance 0 from its own vertices
__device__ __forceinline__ float recip_up(float e) {
    if (!(e > TINY)) return 0.f;
    const float inv = 1.0f / e;
    return e * inv < 1.0f ? __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, inv) + 1u) : inv;
}

// r[0] = (a, 1/|ab|^2)  r[1] = (ab, 1/|ac|^2)  r[2] = (ac, 1/|bc|^2)  r[3] = (m1, |ab|^2 - ab.ac)  r[4] = (m2, 0)
__device__ __forceinline__ void face_record(const float *__restrict__ verts, const int32_t *__restrict__ f, float4 *r) {
    const float *pa = verts + (long)f[0] * 3, *pb = verts + (long)f[1] * 3, *pc = verts + (long)f[2] * 3;
    const float ax = pa[0], ay = pa[1], az = pa[2];
    const float abx = pb[0] - ax, aby = pb[1] - ay, abz = pb[2] - az;
    const float acx = pc[0] - ax, acy = pc[1] - ay, acz = pc[2] - az;
    const float bcx = acx - abx, bcy = acy - aby, bcz = acz - abz;
    const float e00 = dot3(abx, aby, abz, abx, aby, abz), e01 = dot3(abx, aby, abz, acx, acy, acz);
    const float e11 = dot3(acx, acy, acz, acx, acy, acz), ebc = dot3(bcx, bcy, bcz, bcx, bcy, bcz);
    const float nx = __builtin_fmaf(aby, acz, -(abz * acy)), ny = __builtin_fmaf(abz, acx, -(abx * acz));
    const float nz = __builtin_fmaf(abx, acy, -(aby * acx));
    const float nn = dot3(nx, ny, nz, nx, ny, nz);
    const float inv = (nn > TINY && nn > NO_AREA * (e00 * e11)) ? 1.0f / nn : 0.f;
    r[0] = make_float4(ax, ay, az, recip_up(e00));
    r[1] = make_float4(abx, aby, abz, recip_up(e11));
    r[2] = make_float4(acx, acy, acz, recip_up(ebc));
    r[3] = make_float4(__builtin_fmaf(acy, nz, -(acz * ny)) * inv, __builtin_fmaf(acz, nx, -(acx * nz)) * inv,
                       __builtin_fmaf(acx, ny, -(acy * nx)) * inv, e00 - e01);
    r[4] = make_float4(__builtin_fmaf(ny, abz, -(nz * aby)) * inv, __builtin_fmaf(nz, abx, -(nx * abz)) * inv,
                       __builtin_fmaf(nx, aby, -(ny * abx)) * inv, 0.f);
}

// |p - s ab - t ac|^2
__device__ __forceinline__ float resid2(float px, float py, float pz, float s, float t, const float4 &ab, const float4 &ac) {
    const float rx = __builtin_fmaf(-t, ac.x, __builtin_fmaf(-s, ab.x, px));
    const float ry = __builtin_fmaf(-t, ac.y, __builtin_fmaf(-s, ab.y, py));
    const float rz = __builtin_fmaf(-t, ac.z, __builtin_fmaf(-s, ab.z, pz));
    return dot3(rx, ry, rz, rx, ry, rz);
}

// squared distance from q to the face of record r; (s, t): the closest point is a + s ab + t ac
__device__ __forceinline__ float point_face(float qx, float qy, float qz, const float4 *r, float &s, float &t) {
    const float4 a = r[0], ab = r[1], ac = r[2], m1 = r[3], m2 = r[4];
    const float px = qx - a.x, py = qy - a.y, pz = qz - a.z;
    const float d1 = dot3(px, py, pz, ab.x, ab.y, ab.z), d2 = dot3(px, py, pz, ac.x, ac.y, ac.z);
    const float v = clamp01(dot3(px, py, pz, m1.x, m1.y, m1.z), 1.f);
    const float w = clamp01(dot3(px, py, pz, m2.x, m2.y, m2.z), 1.f - v);
    const float tab = clamp01(d1 * a.w, 1.f), tac = clamp01(d2 * ab.w, 1.f), tbc = clamp01(((d2 - d1) + m1.w) * ac.w, 1.f);
    float d = resid2(px, py, pz, v, w, ab, ac);
    s = v; t = w;
    const float dab = resid2(px, py, pz, tab, 0.f, ab, ac);
    if (dab < d) { d = dab; s = tab; t = 0.f; }
    const float dac = resid2(px, py, pz, 0.f, tac, ab, ac);
    if (dac < d) { d = dac; s = 0.f; t = tac; }
    const float dbc = resid2(px, py, pz, 1.f - tbc, tbc, ab, ac);
    if (dbc < d) { d = dbc; s = 1.f - tbc; t = tbc; }
    return d;
}

}  // namespace
