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
// The pair evaluation itself (exact four-candidate form, faces without area legal) is face_record / point_face of
// point_face.h, shared with voxelize.hip.
//
// Tried and dropped: skipping a face whose bounding sphere is farther from every query of the wave than their running best
// (|q - c|^2 > 2 (R^2 + best), no square root).  The queries of a wave are not neighbours in space, so a wave seldom agrees
// to skip, and the test costs 9 VALU issues per query and face: 10.84 ms with it against 9.88 ms without at 100 000 points
// x 49 928 faces, 523 against 454 us at 20 000 x 7938.
#include "point_face.h"

namespace {

constexpr int WAVES = 8;             // 512 threads
constexpr int TILE = 512;            // faces staged in LDS per sweep step: one record per thread; each wave scans TILE / WAVES

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
