// Unsigned point-to-triangle-mesh distance -- include/fsg_hip.h: fsg_point_mesh_dist_f32.
// Replaces the open3d RaycastingScene.compute_distance call of metrics.py:20-24 (the primitive under assd / batch_assd /
// pseudo_symmetric_point_to_mesh_distance).
//
// Brute force and VALU-bound like chamfer.hip (B*P*F pair evaluations, ~65 VALU issues each; inputs are a few hundred KB):
// one or two query points per lane in registers, the faces streamed through LDS in 512-face tiles that the eight waves of
// a workgroup split between them, a per-wave (distance, face) minimum merged at the end.  While staging, every thread turns
// one face into a 20-float record -- a, ab, ac, the reciprocals and the two barycentric gradients, nothing that depends on
// the query -- which every lane then reads by LDS broadcast; there is no prep launch and no per-face workspace.
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
//
// Tried and dropped: skipping a face whose bounding sphere is farther from every query of the wave than their running best
// (|q - c|^2 > 2 (R^2 + best), no square root).  The queries of a wave are not neighbours in space, so a wave seldom agrees
// to skip, and the test costs 9 VALU issues per query and face: 10.84 ms with it against 9.88 ms without at 100 000 points
// x 49 928 faces, 523 against 454 us at 20 000 x 7938.
#include "fsg_common.h"

namespace {

constexpr int WAVES = 8;             // 512 threads
constexpr int TILE = 512;            // faces staged in LDS per sweep step: one record per thread; each wave scans TILE / WAVES
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

// One workgroup = 64 * QPL query points (QPL per lane, so a record read from LDS serves QPL evaluations) x eight waves that
// split every 512-face tile between them; the eight partial (distance, face) minima of a query are merged at the end (lower
// face index on equal distance, like a sequential scan).
template <int QPL>
__global__ __launch_bounds__(WAVES * 64) void point_mesh_kernel(const float *__restrict__ pts, const float *__restrict__ verts,
                                                                 const int32_t *__restrict__ faces, int P, int V, int F,
                                                                 int per_mesh_faces, float *__restrict__ dist2,
                                                                 int32_t *__restrict__ face, float *__restrict__ closest) {
    constexpr int QW = 64 * QPL;
    __shared__ float4 rec[TILE][REC];
    __shared__ float pd[WAVES][QW];
    __shared__ int pj[WAVES][QW];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *vb = verts + (long)b * V * 3;
    const int32_t *fb = faces + (per_mesh_faces ? (long)b * F * 3 : 0L);
    float qx[QPL], qy[QPL], qz[QPL], best[QPL];
    int jb[QPL];
    bool act[QPL];
#pragma unroll
    for (int u = 0; u < QPL; ++u) {
        const int i = blockIdx.x * QW + lane + 64 * u;
        act[u] = i < P;
        qx[u] = qy[u] = qz[u] = 0.f;
        if (act[u]) { const float *p = pts + ((long)b * P + i) * 3; qx[u] = p[0]; qy[u] = p[1]; qz[u] = p[2]; }
        best[u] = INFINITY;
        jb[u] = 0;
    }
    constexpr int PER = TILE / WAVES;
    for (int t0 = 0; t0 < F; t0 += TILE) {
        const int cnt = min(TILE, F - t0);
        __syncthreads();
        for (int t = tid; t < cnt; t += WAVES * 64) face_record(vb, fb + (long)(t0 + t) * 3, rec[t]);
        __syncthreads();
        const int lo = wave * PER, hi = min(cnt, lo + PER);
        for (int j = lo; j < hi; ++j) {
            float4 r[REC];
#pragma unroll
            for (int k = 0; k < REC; ++k) r[k] = rec[j][k];   // same address in every lane: LDS broadcast
#pragma unroll
            for (int u = 0; u < QPL; ++u) {
                float s, t;
                const float d = point_face(qx[u], qy[u], qz[u], r, s, t);
                if (d < best[u]) { best[u] = d; jb[u] = t0 + j; }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < QPL; ++u) { pd[wave][lane + 64 * u] = best[u]; pj[wave][lane + 64 * u] = jb[u]; }
    __syncthreads();
    if (tid < QW) {
        float bd = pd[0][tid];
        int bj = pj[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const float d = pd[w][tid];
            const int j = pj[w][tid];
            if (d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
        }
        const int i = blockIdx.x * QW + tid;
        if (i < P) {
            const long o = (long)b * P + i;
            dist2[o] = bd;
            if (face) face[o] = bj;
            if (closest) {   // the winning face once more, this time for (s, t)
                float4 r[REC];
                face_record(vb, fb + (long)bj * 3, r);
                const float *p = pts + o * 3;
                float s, t;
                point_face(p[0], p[1], p[2], r, s, t);
                closest[o * 3] = __builtin_fmaf(t, r[2].x, __builtin_fmaf(s, r[1].x, r[0].x));
                closest[o * 3 + 1] = __builtin_fmaf(t, r[2].y, __builtin_fmaf(s, r[1].y, r[0].y));
                closest[o * 3 + 2] = __builtin_fmaf(t, r[2].z, __builtin_fmaf(s, r[1].z, r[0].z));
            }
        }
    }
}

}  // namespace

extern "C" int fsg_point_mesh_dist_f32(const float *pts, const float *verts, const int32_t *faces, int B, int P, int V, int F,
                                       int Bf, float *dist2, int32_t *face, float *closest, fsg_stream_t stream) {
    FSG_REQUIRE(pts && verts && faces && dist2, "fsg_point_mesh_dist_f32: NULL pointer");
    FSG_REQUIRE(B >= 0 && P > 0 && V > 0 && F > 0 && B <= 65535, "fsg_point_mesh_dist_f32: bad shape B=%d P=%d V=%d F=%d", B, P,
                V, F);
    FSG_REQUIRE(Bf == 1 || Bf == B, "fsg_point_mesh_dist_f32: faces of %d meshes for a batch of %d (1 = shared, or one each)", Bf,
                B);
    if (B == 0) return FSG_OK;
    // two queries per lane halve the LDS reads per evaluation, one per lane doubles the workgroups: the latter until the
    // former would put two workgroups on every CU
    if ((long)fsg_cdiv(P, 128) * B >= 512)
        hipLaunchKernelGGL(point_mesh_kernel<2>, dim3(fsg_cdiv(P, 128), B), dim3(WAVES * 64), 0, (hipStream_t)stream, pts, verts,
                           faces, P, V, F, Bf == B && B > 1, dist2, face, closest);
    else
        hipLaunchKernelGGL(point_mesh_kernel<1>, dim3(fsg_cdiv(P, 64), B), dim3(WAVES * 64), 0, (hipStream_t)stream, pts, verts,
                           faces, P, V, F, Bf == B && B > 1, dist2, face, closest);
    FSG_CHECK_LAUNCH("fsg_point_mesh_dist_f32");
    return FSG_OK;
}
