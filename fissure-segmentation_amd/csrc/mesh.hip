// Mesh regularisers and surface sampling for the PC-AE mesh loss -- include/fsg_hip.h: fsg_mesh_reg_f32,
// fsg_mesh_sample_f32, fsg_mesh_sample_bwd_f32.
// Replaces pytorch3d's mesh_edge_loss, mesh_normal_consistency, mesh_laplacian_smoothing(method="uniform") and
// sample_points_from_meshes as losses/mesh_loss.py:28-57 of the reference calls them.
//
// Regularisers.  The three terms and their vertex gradients come out of ONE launch (plus a one-workgroup finalize): the loss is
// the last node of the training step, so the pass that evaluates it hands back d term / d vertex and autograd only scales.
// Work is cut into chunks of 256 vertices of one mesh, one thread per vertex, one workgroup per chunk (the training batch, 32
// meshes of 2025 vertices, is 256 workgroups: one per CU).  A thread forms the whole gradient of its vertex from the
// topology's incidence lists in list order -- nothing is scattered, there are no floating-point atomics:
//   edge      g_k = 2/E sum_{j in N(k)} (v_k - v_j);              value: the edges (k, j) with j > k
//   Laplacian L_i = 1/d_i sum_{j in N(i)} v_j - v_i (degree 0: -v_i), u_i = L_i / |L_i| (0 at |L_i| = 0),
//             g_k = 1/V (sum_{i in N(k)} u_i / d_i - u_k);        value: |L_k|.  u_i of the neighbours is RECOMPUTED from the
//             two-ring (d^2 ~ 36 reads) instead of exchanged: no pass boundary, so chunks of a mesh need no synchronisation
//   normal    per pair (v0, v1, a, b): e = v1 - v0, n0 = e x (a - v0), n1 = -(e x (b - v0)), x_i = n_i / max(|n_i|, 1e-8),
//             term 1 - x0.x1; d/dn0 = -(x1 - (x0.x1) n0/|n0|) / max(|n0|, 1e-8) (n0/|n0| := 0 at 0: the clamp has no
//             gradient, the norm has torch's).  A vertex re-evaluates every pair it is part of (~11 at the training shape)
//             and keeps the gradient of its role; the pair's value is counted where the vertex is v0.
// The mesh's vertices are staged in LDS when they fit (V <= 4096, 48 KB; 24 KB at the training size), else every read is a
// global gather -- the same code on another pointer.  Arithmetic is fp64 on the fp32 vertices (the kernel waits for gathers,
// not for the VALU), the per-chunk sums are fp64 in a fixed tree, and finalize adds a mesh's chunk records in chunk order:
// the same input gives the same bits, and a mesh's result does not depend on the rest of the batch.
//
// Sampler.  `cdf` (one workgroup per mesh) writes the inclusive fp64 prefix sum of the fp64 face areas; `sample` (one thread
// per sample) picks the face by bisection, min{ j : C[j] > u0 C[F-1] }, and writes fp32 barycentric weights and the point.
// The backward has every vertex scan the samples of its mesh in sample order (face corners broadcast from LDS, a hit is
// rare): O(V n) compares, ~12 M per mesh at the training shape, no sort, no atomics, one launch.
#include "fsg_common.h"

namespace {

constexpr int CHUNK = 256;            // vertices per workgroup, one per thread
constexpr int LDS_MAX_V = 4096;       // a mesh of up to this many vertices is staged in LDS (12 bytes each)
constexpr double COS_EPS = 1e-8;      // torch.nn.functional.cosine_similarity's eps

struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ D3 operator/(D3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// vertex i of the mesh: from the LDS copy or from global memory
template <bool LDS>
__device__ __forceinline__ D3 vert(const float *sv, const float *__restrict__ gv, int i) {
    if constexpr (LDS) {
        return {(double)sv[3 * i], (double)sv[3 * i + 1], (double)sv[3 * i + 2]};
    } else {
        const float *p = gv + 3 * (long)i;
        return {(double)p[0], (double)p[1], (double)p[2]};
    }
}

// mesh descriptor, 8 int32: first vertex in `verts`, vertex count, first entry of the mesh's V + 1 offsets in nbr_off /
// inc_off, first pair in `pairs`, edge count, pair count, 2 unused
struct MeshDesc {
    int vbase, V, obase, pbase, E, P;
};
__device__ __forceinline__ MeshDesc load_desc(const int32_t *__restrict__ desc, int m) {
    const int32_t *d = desc + 8 * (long)m;
    return {d[0], d[1], d[2], d[3], d[4], d[5]};
}

struct RegOut {
    double val[3];   // this vertex's share of the three sums
    D3 g[3];         // d term / d vertex, already divided by E, P, V
};

template <bool LDS>
__device__ __forceinline__ void reg_vertex(const float *sv, const float *__restrict__ gv, const MeshDesc &md, int k,
                                           const int32_t *__restrict__ nbr_off, const int32_t *__restrict__ nbr,
                                           const int32_t *__restrict__ pairs, const int32_t *__restrict__ inc_off,
                                           const int32_t *__restrict__ inc, RegOut &o) {
    const D3 vk = vert<LDS>(sv, gv, k);
    // ---- edge length and uniform Laplacian: the neighbours, and the neighbours' neighbours for u_i
    const int n0 = nbr_off[md.obase + k], n1 = nbr_off[md.obase + k + 1], dk = n1 - n0;
    D3 s = {0, 0, 0}, acc = {0, 0, 0};
    double e_val = 0;
    for (int t = n0; t < n1; ++t) {
        const int j = nbr[t];
        const D3 vj = vert<LDS>(sv, gv, j);
        s = s + vj;
        if (j > k) {
            const D3 d = vk - vj;
            e_val += dot(d, d);
        }
        const int m0 = nbr_off[md.obase + j], m1 = nbr_off[md.obase + j + 1];
        D3 sj = {0, 0, 0};
        for (int q = m0; q < m1; ++q) sj = sj + vert<LDS>(sv, gv, nbr[q]);
        const double dj = (double)(m1 - m0);   // >= 1: k is among them
        const D3 Lj = sj / dj - vj;   // a true division: exactly 0 where the neighbours' sum is exactly dj vj
        const double nj = sqrt(dot(Lj, Lj));
        if (nj > 0) acc = acc + Lj * (1.0 / (nj * dj));
    }
    const D3 Lk = dk > 0 ? s / (double)dk - vk : vk * -1.0;
    const double nk = sqrt(dot(Lk, Lk));
    const D3 uk = nk > 0 ? Lk * (1.0 / nk) : D3{0, 0, 0};
    o.val[0] = e_val;
    o.g[0] = md.E > 0 ? (vk * (double)dk - s) * (2.0 / (double)md.E) : D3{0, 0, 0};
    o.val[2] = nk;
    o.g[2] = (acc - uk) * (1.0 / (double)md.V);
    // ---- normal consistency: every pair this vertex takes part in
    const int i0 = inc_off[md.obase + k], i1 = inc_off[md.obase + k + 1];
    D3 gn = {0, 0, 0};
    double n_val = 0;
    for (int t = i0; t < i1; ++t) {
        const int code = inc[t], role = code & 3;
        const int32_t *pr = pairs + 4 * ((long)md.pbase + (code >> 2));
        const D3 v0 = vert<LDS>(sv, gv, pr[0]);
        const D3 e = vert<LDS>(sv, gv, pr[1]) - v0, pa = vert<LDS>(sv, gv, pr[2]) - v0, qb = vert<LDS>(sv, gv, pr[3]) - v0;
        const D3 na = cross(e, pa), nb = cross(qb, e);
        const double ra = sqrt(dot(na, na)), rb = sqrt(dot(nb, nb));
        // unit normals by true division (parallel normals give cos = 1 and a zero gradient EXACTLY, as torch's do); x is the
        // unit normal unless the norm is below eps
        const D3 ua = ra > 0 ? na / ra : D3{0, 0, 0}, ub = rb > 0 ? nb / rb : D3{0, 0, 0};
        const double ca = fmax(ra, COS_EPS), cb = fmax(rb, COS_EPS);
        const D3 xa = ra >= COS_EPS ? ua : na / ca, xb = rb >= COS_EPS ? ub : nb / cb;
        const double c = dot(xa, xb);
        if (role == 0) n_val += 1.0 - c;
        // d (1 - cos) / d na and / d nb
        const D3 Ga = (ua * c - xb) / ca, Gb = (ub * c - xa) / cb;
        // na = e x pa, nb = qb x e
        const D3 ge = cross(pa, Ga) + cross(Gb, qb), gp = cross(Ga, e), gq = cross(e, Gb);
        const D3 g = role == 1 ? ge : role == 2 ? gp : role == 3 ? gq : (ge + gp + gq) * -1.0;
        gn = gn + g;
    }
    o.val[1] = n_val;
    o.g[1] = md.P > 0 ? gn * (1.0 / (double)md.P) : D3{0, 0, 0};
}

// grid (max chunks per mesh, N).  rec: 3 doubles per (mesh, chunk); grads: three (total_verts, 3) planes or NULL
__global__ __launch_bounds__(CHUNK) void mesh_reg_kernel(const float *__restrict__ verts, const int32_t *__restrict__ desc,
                                                         const int32_t *__restrict__ nbr_off, const int32_t *__restrict__ nbr,
                                                         const int32_t *__restrict__ pairs,
                                                         const int32_t *__restrict__ inc_off, const int32_t *__restrict__ inc,
                                                         double *__restrict__ rec, float *__restrict__ grads,
                                                         long total_verts) {
    __shared__ float sv[LDS_MAX_V * 3];
    __shared__ double part[CHUNK / 64][3];
    const int m = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const MeshDesc md = load_desc(desc, m);
    if (chunk * CHUNK >= md.V) return;   // a smaller mesh of a mixed batch (uniform over the workgroup)
    const float *gv = verts + 3 * (long)md.vbase;
    const int k = chunk * CHUNK + tid;
    const bool act = k < md.V;
    RegOut o;
#pragma unroll
    for (int t = 0; t < 3; ++t) { o.val[t] = 0; o.g[t] = {0, 0, 0}; }
    if (md.V <= LDS_MAX_V) {
        for (int i = tid; i < 3 * md.V; i += CHUNK) sv[i] = gv[i];
        __syncthreads();
        if (act) reg_vertex<true>(sv, gv, md, k, nbr_off, nbr, pairs, inc_off, inc, o);
    } else if (act) {
        reg_vertex<false>(sv, gv, md, k, nbr_off, nbr, pairs, inc_off, inc, o);
    }
    if (grads && act) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            float *g = grads + ((long)t * total_verts + md.vbase + k) * 3;
            g[0] = (float)o.g[t].x; g[1] = (float)o.g[t].y; g[2] = (float)o.g[t].z;
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const double v = wave_sum_lane0(o.val[t]);
        if (lane == 0) part[wave][t] = v;
    }
    __syncthreads();
    if (tid < 3) {
        double v = 0;
        for (int w = 0; w < CHUNK / 64; ++w) v += part[w][tid];
        rec[((long)m * gridDim.x + chunk) * 3 + tid] = v;
    }
}

// one workgroup: terms (N, 3) = the chunk records of a mesh added in chunk order, over E / P / V; mean (3) over the meshes
__global__ __launch_bounds__(256) void mesh_reg_finalize_kernel(const int32_t *__restrict__ desc, const double *__restrict__ rec,
                                                                int N, int max_chunks, float *__restrict__ terms,
                                                                float *__restrict__ mean) {
    for (int idx = threadIdx.x; idx < 3 * N; idx += 256) {
        const int m = idx / 3, t = idx - 3 * m;
        const MeshDesc md = load_desc(desc, m);
        const int nc = (md.V + CHUNK - 1) / CHUNK;
        double s = 0;
        for (int c = 0; c < nc; ++c) s += rec[((long)m * max_chunks + c) * 3 + t];
        const int den = t == 0 ? md.E : t == 1 ? md.P : md.V;
        terms[idx] = den > 0 ? (float)(s / (double)den) : 0.f;
    }
    __syncthreads();   // the terms this workgroup wrote are visible to it
    if (threadIdx.x < 3) {
        double s = 0;
        for (int m = 0; m < N; ++m) s += (double)terms[3 * m + threadIdx.x];
        mean[threadIdx.x] = (float)(s / (double)N);
    }
}

// ------------------------------------------------------------------------------------------------------------- sampler
// sampler descriptor, 4 int32: first vertex in `verts`, vertex count, first face in `faces`, face count
struct SampDesc {
    int vbase, V, fbase, F;
};
__device__ __forceinline__ SampDesc load_sdesc(const int32_t *__restrict__ sdesc, int m) {
    const int32_t *d = sdesc + 4 * (long)m;
    return {d[0], d[1], d[2], d[3]};
}

__device__ __forceinline__ double face_area(const float *__restrict__ gv, const int32_t *__restrict__ f) {
    const D3 a = vert<false>(nullptr, gv, f[0]);
    const D3 n = cross(vert<false>(nullptr, gv, f[1]) - a, vert<false>(nullptr, gv, f[2]) - a);
    return 0.5 * sqrt(dot(n, n));
}

// one workgroup per mesh: C[j] = area_0 + ... + area_j in fp64 (thread t owns a run of consecutive faces; the run totals are
// added in thread order).  A mesh without area gets C[j] = j + 1: every face alike.
__global__ __launch_bounds__(256) void mesh_cdf_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                       const int32_t *__restrict__ sdesc, int max_F, double *__restrict__ cdf) {
    __shared__ double tot[256];
    const int m = blockIdx.x, tid = threadIdx.x;
    const SampDesc sd = load_sdesc(sdesc, m);
    const float *gv = verts + 3 * (long)sd.vbase;
    const int32_t *fm = faces + 3 * (long)sd.fbase;
    double *C = cdf + (long)m * max_F;
    const int run = (sd.F + 255) / 256, j0 = min(sd.F, tid * run), j1 = min(sd.F, j0 + run);
    double s = 0;
    for (int j = j0; j < j1; ++j) s += face_area(gv, fm + 3 * (long)j);
    tot[tid] = s;
    __syncthreads();
    double before = 0, all = 0;
    for (int t = 0; t < 256; ++t) {
        if (t == tid) before = all;
        all += tot[t];
    }
    if (all > 0) {
        s = before;
        for (int j = j0; j < j1; ++j) {
            s += face_area(gv, fm + 3 * (long)j);
            C[j] = s;
        }
    } else {
        for (int j = j0; j < j1; ++j) C[j] = (double)(j + 1);
    }
}

// grid (ceil(n / 256), N), one thread per sample
__global__ __launch_bounds__(256) void mesh_sample_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                          const int32_t *__restrict__ sdesc, int max_F,
                                                          const double *__restrict__ cdf, const float *__restrict__ u, int n,
                                                          float *__restrict__ pts, int32_t *__restrict__ face,
                                                          float *__restrict__ w) {
    const int m = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const SampDesc sd = load_sdesc(sdesc, m);
    const double *C = cdf + (long)m * max_F;
    const long o = (long)m * n + s;
    const float u0 = u[3 * o], u1 = u[3 * o + 1], u2 = u[3 * o + 2];
    const double t = (double)u0 * C[sd.F - 1];
    int lo = 0, hi = sd.F - 1;   // the last face if no C[j] exceeds t (u0 = 1)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (C[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int32_t *f = faces + 3 * ((long)sd.fbase + lo);
    const float *gv = verts + 3 * (long)sd.vbase;
    const float *a = gv + 3 * (long)f[0], *b = gv + 3 * (long)f[1], *c = gv + 3 * (long)f[2];
    const float r = sqrtf(u1);
    const float w0 = 1.0f - r, w1 = r * (1.0f - u2), w2 = r * u2;
    face[o] = lo;
    w[3 * o] = w0; w[3 * o + 1] = w1; w[3 * o + 2] = w2;
#pragma unroll
    for (int d = 0; d < 3; ++d) pts[3 * o + d] = w0 * a[d] + w1 * b[d] + w2 * c[d];
}

// grid (ceil(max_V / 256), N), one thread per vertex: grad_v = sum over the samples, in sample order, of w_corner g where the
// sample's face has the vertex at that corner.  The corner ids of 256 samples at a time are staged in LDS and read by broadcast.
// The samples' g and w are staged with the ids, so a hit reads LDS only.  Measured 243 us at the training shape and for one
// mesh alike (latency-bound: four waves per workgroup, each walking all n samples); one sample per step and global reads in
// the hit branch measured the same, 231 and 272 us.  Untried: the sample range of a chunk split over more waves.
__global__ __launch_bounds__(256) void mesh_sample_bwd_kernel(const float *__restrict__ g, const int32_t *__restrict__ face,
                                                              const float *__restrict__ w, const int32_t *__restrict__ faces,
                                                              const int32_t *__restrict__ sdesc, int n,
                                                              float *__restrict__ grad_verts) {
    __shared__ int4 ids[256];   // the three corners of a sample's face; -1 behind the last sample
    __shared__ float sg[256][3], sw[256][3];   // its upstream gradient and weights: a hit must not wait for global memory
    const int m = blockIdx.y, tid = threadIdx.x;
    const SampDesc sd = load_sdesc(sdesc, m);
    if (blockIdx.x * 256 >= sd.V) return;   // uniform over the workgroup
    const int k = blockIdx.x * 256 + tid;
    const int32_t *fm = faces + 3 * (long)sd.fbase;
    D3 acc = {0, 0, 0};
    for (int s0 = 0; s0 < n; s0 += 256) {
        const int cnt = min(256, n - s0);
        __syncthreads();
        int4 mine = make_int4(-1, -1, -1, -1);
        if (tid < cnt) {
            const int32_t *f = fm + 3 * (long)face[(long)m * n + s0 + tid];
            mine = make_int4(f[0], f[1], f[2], -1);
            const long o = 3 * ((long)m * n + s0 + tid);
#pragma unroll
            for (int d = 0; d < 3; ++d) { sg[tid][d] = g[o + d]; sw[tid][d] = w[o + d]; }
        }
        ids[tid] = mine;
        __syncthreads();
        // eight samples per step: the reads go out together, a hit (rare: ~6 of a mesh's faces touch a vertex) is handled
        // after them, in sample order
        for (int j0 = 0; j0 < cnt; j0 += 8) {
            unsigned hit = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int4 q = ids[j0 + r];
                hit |= (q.x == k || q.y == k || q.z == k) ? 1u << r : 0u;
            }
            while (hit) {
                const int j = j0 + __ffs(hit) - 1;
                hit &= hit - 1;
                const int4 q = ids[j];
                const D3 gs = {(double)sg[j][0], (double)sg[j][1], (double)sg[j][2]};
                if (q.x == k) acc = acc + gs * (double)sw[j][0];
                if (q.y == k) acc = acc + gs * (double)sw[j][1];
                if (q.z == k) acc = acc + gs * (double)sw[j][2];
            }
        }
    }
    if (k < sd.V) {
        float *gv = grad_verts + 3 * ((long)sd.vbase + k);
        gv[0] = (float)acc.x; gv[1] = (float)acc.y; gv[2] = (float)acc.z;
    }
}

}  // namespace

extern "C" size_t fsg_mesh_reg_workspace_bytes(int N, int max_V) {
    if (N <= 0 || max_V <= 0) return 0;
    return (size_t)N * (size_t)fsg_cdiv(max_V, CHUNK) * 3 * sizeof(double);
}

extern "C" int fsg_mesh_reg_f32(const float *verts, int64_t total_verts, const int32_t *desc, int N, int max_V,
                                const int32_t *nbr_off, const int32_t *nbr, const int32_t *pairs, const int32_t *inc_off,
                                const int32_t *inc, float *terms, float *mean, float *grads, void *workspace,
                                size_t workspace_bytes, fsg_stream_t stream) {
    FSG_REQUIRE(verts && desc && nbr_off && nbr && pairs && inc_off && inc && terms && mean && workspace,
                "fsg_mesh_reg_f32: NULL pointer");
    FSG_REQUIRE(N > 0 && N <= 65535 && max_V > 0 && total_verts >= max_V && total_verts < (1LL << 31) / 3,
                "fsg_mesh_reg_f32: bad shape N=%d max_V=%d total_verts=%lld (N <= 65535, max_V <= total_verts < 2^31 / 3)", N,
                max_V, (long long)total_verts);
    FSG_REQUIRE(((uintptr_t)workspace & 7) == 0, "fsg_mesh_reg_f32: workspace must be 8-byte aligned");
    FSG_REQUIRE(workspace_bytes >= fsg_mesh_reg_workspace_bytes(N, max_V), "fsg_mesh_reg_f32: workspace of %zu bytes, need %zu",
                workspace_bytes, fsg_mesh_reg_workspace_bytes(N, max_V));
    const int chunks = fsg_cdiv(max_V, CHUNK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_reg_kernel, dim3(chunks, N), dim3(CHUNK), 0, st, verts, desc, nbr_off, nbr, pairs, inc_off, inc,
                       (double *)workspace, grads, (long)total_verts);
    hipLaunchKernelGGL(mesh_reg_finalize_kernel, dim3(1), dim3(256), 0, st, desc, (const double *)workspace, N, chunks, terms,
                       mean);
    FSG_CHECK_LAUNCH("fsg_mesh_reg_f32");
    return FSG_OK;
}

extern "C" size_t fsg_mesh_sample_workspace_bytes(int N, int max_F) {
    if (N <= 0 || max_F <= 0) return 0;
    return (size_t)N * (size_t)max_F * sizeof(double);
}

extern "C" int fsg_mesh_sample_f32(const float *verts, const int32_t *faces, const int32_t *sdesc, int N, int max_F,
                                   const float *u, int n, float *pts, int32_t *face, float *w, void *workspace,
                                   size_t workspace_bytes, fsg_stream_t stream) {
    FSG_REQUIRE(verts && faces && sdesc && u && pts && face && w && workspace, "fsg_mesh_sample_f32: NULL pointer");
    FSG_REQUIRE(N > 0 && N <= 65535 && max_F > 0 && n > 0 && (int64_t)N * n < (1LL << 31) / 3,
                "fsg_mesh_sample_f32: bad shape N=%d max_F=%d n=%d (N <= 65535, N n < 2^31 / 3)", N, max_F, n);
    FSG_REQUIRE(((uintptr_t)workspace & 7) == 0, "fsg_mesh_sample_f32: workspace must be 8-byte aligned");
    FSG_REQUIRE(workspace_bytes >= fsg_mesh_sample_workspace_bytes(N, max_F),
                "fsg_mesh_sample_f32: workspace of %zu bytes, need %zu", workspace_bytes,
                fsg_mesh_sample_workspace_bytes(N, max_F));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_cdf_kernel, dim3(N), dim3(256), 0, st, verts, faces, sdesc, max_F, (double *)workspace);
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(fsg_cdiv(n, 256), N), dim3(256), 0, st, verts, faces, sdesc, max_F,
                       (const double *)workspace, u, n, pts, face, w);
    FSG_CHECK_LAUNCH("fsg_mesh_sample_f32");
    return FSG_OK;
}

extern "C" int fsg_mesh_sample_bwd_f32(const float *g, const int32_t *face, const float *w, const int32_t *faces,
                                       const int32_t *sdesc, int N, int max_V, int n, float *grad_verts,
                                       fsg_stream_t stream) {
    FSG_REQUIRE(g && face && w && faces && sdesc && grad_verts, "fsg_mesh_sample_bwd_f32: NULL pointer");
    FSG_REQUIRE(N > 0 && N <= 65535 && max_V > 0 && n > 0 && (int64_t)N * n < (1LL << 31) / 3,
                "fsg_mesh_sample_bwd_f32: bad shape N=%d max_V=%d n=%d (N <= 65535, N n < 2^31 / 3)", N, max_V, n);
    hipLaunchKernelGGL(mesh_sample_bwd_kernel, dim3(fsg_cdiv(max_V, 256), N), dim3(256), 0, (hipStream_t)stream, g, face, w,
                       faces, sdesc, n, grad_verts);
    FSG_CHECK_LAUNCH("fsg_mesh_sample_bwd_f32");
    return FSG_OK;
}
