// Surface fitting of labelled point clouds: consistent normal orientation and mesh clean-up -- include/fsg_hip.h:
// fsg_orient_normals_f32, fsg_face_union_i32, fsg_cluster_stats_f64, fsg_mesh_keep_flags_u8, fsg_mesh_face_flags_u8,
// fsg_mesh_compact_f32.  Replaces, on the device, what data_processing/surface_fitting.py:62-64 takes from open3d
// (orient_normals_consistent_tangent_plane) and utils/general_utils.py:157-209 (remove_vertices_by_mask,
// cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices).  DESIGN.md has the definitions.
//
// ORIENTATION.  The graph of a segment: edges {u, idx[u, j]}, 1 <= j < k_s = min(K, n_s - 1), weight w = max(0, 1 - |n_u . n_v|)
// (the dot product summed x, y, z without fma: the same bits from either end).  The minimum spanning forest under the key
//     (fp32 bits of w >> 8) << 40 | min(u, v) << 20 | max(u, v)          (u, v local to the segment: n_s <= 2^20)
// is unique because the key names its edge.  Boruvka rounds of four launches each:
//   compress  every point walks to its root, XORing the parities on the way, and stores (root << 1 | parity) both into its link
//             and into a snapshot that the next two kernels read (they never read a link that another lane is writing).
//             Walkers may meet links that other walkers have just shortened: a link always holds an ancestor and the parity
//             relative to it, old or new, and roots do not change in this launch, so every interleaving ends with the same word.
//   min edge  one lane per (u, j): an edge between two components offers its key to both roots by a 64-bit atomic min, after a
//             plain look that skips offers which cannot win, and combined over the lanes of a wave that name the same root
//             (atomics on ONE address serialise).  Two launches: first every edge offers to the root of its OWN point u -- a wave
//             holds the edges of one or two points, so that is about one atomic per wave --, then to the root of the neighbour
//             v, where the look now sees that root's own minimum and turns most offers away (in one launch the first round
//             issues an atomic per edge to scattered addresses, 1.26e6 at 20 000 x 63; the split is reasoned, its gain was not
//             measured apart from the flag store below).  Min commutes: the winner does not depend on arrival.
//   hook      a root R whose winning edge (a, b) leads to the component O links under O with parity
//             par(a) ^ par(b) ^ [n_a . n_b < 0]; when O chose the same edge, only the higher of the two roots hooks.  With a strict
//             total order the chosen edges hold no cycle but these pairs.
// A round that finds an edge between components raises its flag (one lane per wave, and only while the flag still reads 0:
// 20 000 waves storing to ONE word serialised and were 3.5 of the call's 4.1 ms); the kernels of later rounds see a missing
// flag and return (ceil(log2 n) + 1 rounds are always LAUNCHED: no host read).  Afterwards, per component: the smallest member
// (atomic min) is its id, the member of largest z, lowest index on ties (atomic max of f2o(z) << 32 | ~index), gets n_z >= 0, and
// every other member the sign that its parity relative to that member dictates.  Only integer atomics whose result does not
// depend on their order: the same input gives the same bits, a segment the same bits alone and inside a batch.
//
// FACE CLUSTERS.  The caller sorts the 3F keys min(a, b) * V + max(a, b) of the half-edges (torch.sort: plumbing); equal
// neighbours in that order share an edge, and a run of c equal keys chains its c faces.  Union: find the two roots, hook the
// LARGER under the smaller by atomic min, go on with whatever the min displaced.  Parents only ever decrease, so there is no
// cycle and the root of a cluster is its smallest face.  Finds shorten the path they walk (atomic min with the grandparent).
//
// STATISTICS.  One workgroup per cluster over two sorted lists of the caller (faces by cluster; (cluster, vertex) keys): fp64
// area, and the count and fp64 coordinate sum of the DISTINCT vertices (a key that differs from its predecessor).  A lane adds
// its elements in ascending order, the lanes are added by the shuffle tree, the eight waves in order: a fixed order.
#include "fsg_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr unsigned long long NOKEY = ~0ull;
constexpr int ORIENT_MAX_N = FSG_ORIENT_MAX_POINTS;     // 20 bits per endpoint in the key

__device__ __forceinline__ int ld32(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st32(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One atomic min / max per (wave, destination) where lanes share destinations: up to AGG_TRIES times the lanes that name the
// first live lane's destination combine their values over the wave (xor butterfly) and that lane issues ONE atomic; whoever is
// left issues its own.  Measured need: 20 000 same-address 64-bit atomics serialise at ~17 ns each (336 us for the root pass of one
// component).  Min and max commute, so the result is the one of per-lane atomics.  EVERY lane of the wave must call (live or not).
constexpr int AGG_TRIES = 4;
template <bool IS_MIN, typename T>
__device__ __forceinline__ void wave_agg_atomic(T *base, int dest, T value, bool live) {
    const int lane = threadIdx.x & 63;
    const T identity = IS_MIN ? ~(T)0 : (T)0;
#pragma unroll 1
    for (int t = 0; t < AGG_TRIES; ++t) {
        const unsigned long long m = __ballot(live);
        if (m == 0ull) return;
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int d0 = __shfl(dest, leader);
        const bool mine = live && dest == d0;
        T v = mine ? value : identity;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const T o = __shfl_xor(v, off);
            v = IS_MIN ? (o < v ? o : v) : (o > v ? o : v);
        }
        if (lane == leader) {
            if (IS_MIN) __hip_atomic_fetch_min(base + d0, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else __hip_atomic_fetch_max(base + d0, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        live = live && !mine;
    }
    if (live) {
        if (IS_MIN) __hip_atomic_fetch_min(base + dest, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_fetch_max(base + dest, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the carve of the orientation workspace; every array has n entries but the flags
struct OrientWs {
    unsigned long long *best, *zkey;      // per root: the round's winning edge key; the key of the member of largest z
    int *link, *snap, *seg_st, *seg_en, *cmin, *flags;
};

__host__ __device__ inline size_t orient_round16(size_t x) { return (x + 15) & ~(size_t)15; }

inline int orient_rounds(int n) {
    int r = 0;
    while ((1L << r) < n) ++r;
    return r + 1;
}

inline size_t orient_ws_bytes(int n) {
    return 2 * orient_round16((size_t)n * 8) + 5 * orient_round16((size_t)n * 4) + orient_round16((size_t)(orient_rounds(n) + 1) * 4);
}

inline OrientWs orient_carve(void *ws, int n) {
    char *p = (char *)ws;
    OrientWs w;
    w.flags = (int *)p;                   // first: the memset of every call clears exactly this block
    p += orient_round16((size_t)(orient_rounds(n) + 1) * 4);
    w.best = (unsigned long long *)p;
    p += orient_round16((size_t)n * 8);
    w.zkey = (unsigned long long *)p;
    p += orient_round16((size_t)n * 8);
    w.link = (int *)p;
    p += orient_round16((size_t)n * 4);
    w.snap = (int *)p;
    p += orient_round16((size_t)n * 4);
    w.seg_st = (int *)p;
    p += orient_round16((size_t)n * 4);
    w.seg_en = (int *)p;
    p += orient_round16((size_t)n * 4);
    w.cmin = (int *)p;
    return w;
}

// n_u . n_v, summed x, y, z (the file is built with -ffp-contract=off): the same bits for (u, v) and (v, u)
__device__ __forceinline__ float edge_dot(const float *__restrict__ nrm, int u, int v) {
    const float *a = nrm + 3L * u, *b = nrm + 3L * v;
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__global__ __launch_bounds__(BLOCK) void orient_init_kernel(const int32_t *__restrict__ offset, int b, int n, OrientWs w) {
    const int u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= n) return;
    int lo = 0, hi = b - 1;               // the first segment whose end lies beyond u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offset[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    int st = lo ? offset[lo - 1] : 0, en = offset[lo];
    st = st < 0 ? 0 : (st > u ? u : st);  // offsets that do not cover u: a segment of its own, never an index outside the cloud
    en = en > n ? n : (en <= u ? u + 1 : en);
    w.seg_st[u] = st;
    w.seg_en[u] = en;
    w.link[u] = u << 1;
    w.zkey[u] = 0ull;
    w.cmin[u] = 0x7fffffff;
}

// round: -1 = the final pass (always runs); otherwise the pass returns when the round before found nothing to merge
__global__ __launch_bounds__(BLOCK) void orient_compress_kernel(int n, int round, OrientWs w) {
    if (round > 0 && w.flags[round - 1] == 0) return;
    const int u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= n) return;
    int cur = u, par = 0;
    for (int step = 0; step < n; ++step) {            // a path has fewer than n links
        const int l = ld32(w.link + cur), p = l >> 1;
        if (p == cur) break;
        par ^= l & 1;
        cur = p;
    }
    const int v = (cur << 1) | par;
    st32(w.link + u, v);
    w.snap[u] = v;
    w.best[u] = NOKEY;
}

__global__ __launch_bounds__(BLOCK) void orient_min_edge_kernel(const float *__restrict__ nrm, const int32_t *__restrict__ idx, int n,
                                                                 int K, int round, int far_side, OrientWs w) {
    if (round > 0 && w.flags[round - 1] == 0) return;             // uniform over the grid
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    bool live = i < (long)n * (K - 1);                             // no lane leaves before the wave-wide offers below
    int ru = 0, rv = 0;
    unsigned long long key = NOKEY;
    if (live) {
        const int u = (int)(i / (K - 1)), j = 1 + (int)(i - (long)u * (K - 1));
        const int st = w.seg_st[u], en = w.seg_en[u];
        int ks = en - st - 1;
        ks = ks < K ? ks : K;
        live = j < ks;
        if (live) {
            int v = idx[(long)u * K + j];
            v = v < st ? st : (v >= en ? en - 1 : v);             // a bad index names a wrong point of the segment, never one outside it
            ru = w.snap[u] >> 1;
            rv = w.snap[v] >> 1;
            live = ru != rv;
            if (live) {
                const float wgt = fmaxf(1.f - fabsf(edge_dot(nrm, u, v)), 0.f);
                const unsigned lu = (unsigned)(u - st), lv = (unsigned)(v - st);
                key = ((unsigned long long)(__float_as_uint(wgt) >> 8) << 40) | ((unsigned long long)(lu < lv ? lu : lv) << 20) |
                      (unsigned long long)(lu < lv ? lv : lu);
            }
        }
    }
    if (__ballot(live) == 0ull) return;
    // the look only saves atomics: a stale value is larger than the current one, so no winning offer is skipped
    const int r = far_side ? rv : ru;
    wave_agg_atomic<true>(w.best, r, key, live && key < __hip_atomic_load(w.best + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    // the round's flag (see the head of the file)
    if (!far_side && (threadIdx.x & 63) == 0 && ld32(w.flags + round) == 0) st32(w.flags + round, 1);
}

__global__ __launch_bounds__(BLOCK) void orient_hook_kernel(const float *__restrict__ nrm, int n, int round, OrientWs w) {
    if (w.flags[round] == 0) return;
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n || (w.snap[r] >> 1) != r) return;
    const unsigned long long key = w.best[r];
    if (key == NOKEY) return;
    const int st = w.seg_st[r];
    const int a = st + (int)((key >> 20) & 0xFFFFFu), b = st + (int)(key & 0xFFFFFu);
    const int sa = w.snap[a], sb = w.snap[b];
    const bool a_mine = (sa >> 1) == r;
    const int o = a_mine ? sb >> 1 : sa >> 1;
    if (w.best[o] == key && r < o) return;            // both chose this edge: the lower root stays
    const int flip = edge_dot(nrm, a, b) < 0.f ? 1 : 0;
    st32(w.link + r, (o << 1) | (((sa ^ sb) & 1) ^ flip));
}

__global__ __launch_bounds__(BLOCK) void orient_roots_kernel(const float *__restrict__ xyz, int n, OrientWs w) {
    const int u = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = u < n;
    const int r = live ? w.snap[u] >> 1 : 0;
    const unsigned long long zk = live ? ((unsigned long long)f2o(xyz[3L * u + 2]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)u)
                                       : 0ull;
    wave_agg_atomic<true>((unsigned *)w.cmin, r, (unsigned)u, live);     // indices are non-negative: unsigned order = int order
    wave_agg_atomic<false>(w.zkey, r, zk, live);
}

__global__ __launch_bounds__(BLOCK) void orient_sign_kernel(const float *__restrict__ nrm, int n, OrientWs w, float *__restrict__ out,
                                                             int8_t *__restrict__ signs, int32_t *__restrict__ comp) {
    const int u = blockIdx.x * BLOCK + threadIdx.x;
    if (u >= n) return;
    const int s = w.snap[u], r = s >> 1;
    int t = (int)(0xFFFFFFFFu - (unsigned)(w.zkey[r] & 0xFFFFFFFFull));
    t = t < 0 || t >= n ? u : t;                      // cannot happen: every member offered its own index
    const int flip = ((nrm[3L * t + 2] < 0.f ? 1 : 0) ^ w.snap[t] ^ s) & 1;
    const unsigned m = (unsigned)flip << 31;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3L * u + c] = __uint_as_float(__float_as_uint(nrm[3L * u + c]) ^ m);
    signs[u] = flip ? -1 : 1;
    comp[u] = w.cmin[r];
}

// ---------------------------------------------------------------------------------------------------- face clusters
__global__ __launch_bounds__(BLOCK) void iota_kernel(int n, int32_t *__restrict__ p) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) p[i] = i;
}

__device__ __forceinline__ int face_find(int *parent, int x) {
    for (;;) {
        const int p = ld32(parent + x);
        if (p == x) return x;
        const int g = ld32(parent + p);
        if (g != p) atomicMin(parent + x, g);         // halve the path; parents only decrease
        x = p;
    }
}

__global__ __launch_bounds__(BLOCK) void face_union_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ half_edge,
                                                            long n3, int F, int *__restrict__ parent) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x + 1;
    if (i >= n3 || keys[i] != keys[i - 1]) return;
    long ha = half_edge[i] / 3, hb = half_edge[i - 1] / 3;
    if (ha < 0 || ha >= F || hb < 0 || hb >= F) return;   // not a permutation of the half-edges: nothing is linked
    int a = face_find(parent, (int)ha), b = face_find(parent, (int)hb);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);     // a was a root when found; if it still is, it hangs under b now
        if (old == a) break;
        a = face_find(parent, old);                   // somebody hooked a meanwhile: what the min displaced still needs b
        b = face_find(parent, b);
    }
}

__global__ __launch_bounds__(BLOCK) void face_root_kernel(int F, const int *__restrict__ parent, int32_t *__restrict__ root) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int x = f, p;
    while ((p = parent[x]) != x) x = p;
    root[f] = x;
}

// ------------------------------------------------------------------------------------------------ cluster statistics
constexpr int STATS_BLOCK = 512;    // one workgroup per cluster (1024 lanes would cap the unrolled gathers at 128 VGPRs: scratch)

template <typename T>
__device__ __forceinline__ long lower_bound(const T *__restrict__ a, long n, T key) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// every thread's v -> the workgroup's sum in thread 0 (lanes by the shuffle tree, then the waves in order)
__device__ __forceinline__ double block_sum_thread0(double v, double *red) {
    v = wave_sum_lane0(v);
    __syncthreads();                                  // red may still be read from the sum before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < STATS_BLOCK / 64; ++k) s += red[k];
    return s;
}

__global__ __launch_bounds__(STATS_BLOCK) void cluster_stats_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                               const int32_t *__restrict__ cl_sorted,
                                                               const int64_t *__restrict__ face_order,
                                                               const int64_t *__restrict__ vkeys, int V, int F,
                                                               double *__restrict__ area, int64_t *__restrict__ nvert,
                                                               double *__restrict__ vsum) {
    __shared__ double red[STATS_BLOCK / 64];
    const int g = blockIdx.x;
    const long f0 = lower_bound<int32_t>(cl_sorted, F, g), f1 = lower_bound<int32_t>(cl_sorted, F, g + 1);
    double a = 0.;
    for (long i = f0 + threadIdx.x; i < f1; i += STATS_BLOCK) {
        const long f = face_order[i];
        if (f < 0 || f >= F) continue;
        const int32_t *t = faces + 3 * f;
        const float *p0 = verts + 3L * clampi(t[0], V - 1), *p1 = verts + 3L * clampi(t[1], V - 1), *p2 = verts + 3L * clampi(t[2], V - 1);
        const double ux = (double)p1[0] - p0[0], uy = (double)p1[1] - p0[1], uz = (double)p1[2] - p0[2];
        const double vx = (double)p2[0] - p0[0], vy = (double)p2[1] - p0[1], vz = (double)p2[2] - p0[2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        a += 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
    }
    const int64_t k0 = (int64_t)g * V;
    const long v0 = lower_bound<int64_t>(vkeys, 3L * F, k0), v1 = lower_bound<int64_t>(vkeys, 3L * F, k0 + V);
    double sx = 0., sy = 0., sz = 0., cnt = 0.;
    for (long i = v0 + threadIdx.x; i < v1; i += STATS_BLOCK) {
        const int64_t k = vkeys[i];
        if (i > v0 && vkeys[i - 1] == k) continue;    // seen: the list is sorted
        const float *p = verts + 3 * (k - k0);
        sx += p[0];
        sy += p[1];
        sz += p[2];
        cnt += 1.;
    }
    a = block_sum_thread0(a, red);
    sx = block_sum_thread0(sx, red);
    sy = block_sum_thread0(sy, red);
    sz = block_sum_thread0(sz, red);
    cnt = block_sum_thread0(cnt, red);                // exact: whole numbers below 2^53
    if (threadIdx.x == 0) {
        area[g] = a;
        nvert[g] = (int64_t)cnt;
        vsum[3L * g] = sx;
        vsum[3L * g + 1] = sy;
        vsum[3L * g + 2] = sz;
    }
}

// ------------------------------------------------------------------------------------------- keep flags, compaction
// the mesh of a packed vertex: the last m with voff[m] <= v (voff has B + 1 entries, empty meshes repeat one)
__device__ __forceinline__ int mesh_of(const int32_t *__restrict__ voff, int B, int v) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (voff[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// floor(x / s) as an index of an axis of n cells, clamped from above; -1 when it is negative or x is NaN
__device__ __forceinline__ int cell_index(float x, float s, int n) {
    const float q = floorf(x / s);
    if (!(q >= 0.f)) return -1;
    return (int)fminf(q, (float)(n - 1));
}

__global__ __launch_bounds__(BLOCK) void keep_flags_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ voff,
                                                            int B, const uint8_t *__restrict__ keep_in, const float *__restrict__ boxes,
                                                            const uint8_t *__restrict__ mask, int D, int H, int W, float sx, float sy,
                                                            float sz, uint8_t *__restrict__ keep) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const float x = verts[3L * v], y = verts[3L * v + 1], z = verts[3L * v + 2];
    bool k = keep_in ? keep_in[v] != 0 : true;
    if (boxes) {
        const float *bx = boxes + 6L * mesh_of(voff, B, v);           // (lo x, y, z, hi x, y, z), inclusive
        k = k && x >= bx[0] && y >= bx[1] && z >= bx[2] && x <= bx[3] && y <= bx[4] && z <= bx[5];
    }
    if (mask) {
        const int ix = cell_index(x, sx, W), iy = cell_index(y, sy, H), iz = cell_index(z, sz, D);
        k = k && ix >= 0 && iy >= 0 && iz >= 0 && mask[((long)iz * H + iy) * W + ix] != 0;
    }
    keep[v] = k ? 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void face_flags_kernel(const int32_t *__restrict__ faces, int V, int F,
                                                            const uint8_t *__restrict__ vkeep, const uint8_t *__restrict__ face_keep,
                                                            uint8_t *__restrict__ fkeep, uint8_t *__restrict__ used) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3L * f], b = faces[3L * f + 1], c = faces[3L * f + 2];
    bool k = (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;   // a bad index drops the face
    k = k && vkeep[a] && vkeep[b] && vkeep[c] && (!face_keep || face_keep[f]);
    fkeep[f] = k ? 1 : 0;
    if (k) used[a] = used[b] = used[c] = 1;           // every writer writes 1
}

__global__ __launch_bounds__(BLOCK) void compact_kernel(const float *__restrict__ verts, const float *__restrict__ normals,
                                                         const int32_t *__restrict__ faces, int V, int F,
                                                         const int32_t *__restrict__ voff, int B, const uint8_t *__restrict__ vflag,
                                                         const int64_t *__restrict__ vnew, const uint8_t *__restrict__ fflag,
                                                         const int64_t *__restrict__ fnew, float *__restrict__ verts_out,
                                                         float *__restrict__ normals_out, int64_t *__restrict__ faces_out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < V && vflag[i]) {
        const long o = vnew[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            verts_out[3 * o + c] = verts[3L * i + c];
            if (normals) normals_out[3 * o + c] = normals[3L * i + c];
        }
    }
    if (i < F && fflag[i]) {
        const int a = faces[3L * i], b = faces[3L * i + 1], c = faces[3L * i + 2];
        if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return;
        const long base = vnew[clampi(voff[mesh_of(voff, B, a)], V - 1)];   // the first new vertex of the face's mesh
        const long o = fnew[i];
        faces_out[3 * o] = vnew[a] - base;
        faces_out[3 * o + 1] = vnew[b] - base;
        faces_out[3 * o + 2] = vnew[c] - base;
    }
}

}  // namespace

extern "C" size_t fsg_orient_normals_workspace_bytes(int n, int K) {
    (void)K;
    return n > 0 && n <= ORIENT_MAX_N ? orient_ws_bytes(n) : 0;
}

extern "C" int fsg_orient_normals_f32(const float *xyz, const float *normals, const int32_t *idx, const int32_t *offset, int b, int n,
                                      int K, void *workspace, size_t workspace_bytes, float *out, int8_t *signs, int32_t *comp,
                                      fsg_stream_t stream) {
    FSG_REQUIRE(xyz && normals && idx && offset && out && signs && comp, "fsg_orient_normals_f32: NULL pointer");
    FSG_REQUIRE(b > 0 && n >= 0 && K >= 2 && K <= 64, "fsg_orient_normals_f32: bad shape b=%d n=%d K=%d", b, n, K);
    FSG_REQUIRE(n <= ORIENT_MAX_N, "fsg_orient_normals_f32: n=%d points, the edge key holds 20 bits per endpoint (n <= %d)", n,
                ORIENT_MAX_N);
    if (n == 0) return FSG_OK;
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= orient_ws_bytes(n),
                "fsg_orient_normals_f32: workspace NULL, not 16-byte aligned or shorter than %zu bytes", orient_ws_bytes(n));
    const hipStream_t s = (hipStream_t)stream;
    const OrientWs w = orient_carve(workspace, n);
    const int rounds = orient_rounds(n);
    if (hipMemsetAsync(w.flags, 0, orient_round16((size_t)(rounds + 1) * 4), s) != hipSuccess) {
        fsg_set_error("fsg_orient_normals_f32: cannot clear the round flags");
        return FSG_ERR_HIP;
    }
    const dim3 block(BLOCK), pts(fsg_cdiv(n, BLOCK)), edges(fsg_cdiv((long)n * (K - 1), BLOCK));
    hipLaunchKernelGGL(orient_init_kernel, pts, block, 0, s, offset, b, n, w);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(orient_compress_kernel, pts, block, 0, s, n, r, w);
        hipLaunchKernelGGL(orient_min_edge_kernel, edges, block, 0, s, normals, idx, n, K, r, 0, w);
        hipLaunchKernelGGL(orient_min_edge_kernel, edges, block, 0, s, normals, idx, n, K, r, 1, w);
        hipLaunchKernelGGL(orient_hook_kernel, pts, block, 0, s, normals, n, r, w);
    }
    hipLaunchKernelGGL(orient_compress_kernel, pts, block, 0, s, n, -1, w);
    hipLaunchKernelGGL(orient_roots_kernel, pts, block, 0, s, xyz, n, w);
    hipLaunchKernelGGL(orient_sign_kernel, pts, block, 0, s, normals, n, w, out, signs, comp);
    FSG_CHECK_LAUNCH("fsg_orient_normals_f32");
    return FSG_OK;
}

extern "C" int fsg_face_union_i32(const int64_t *sorted_keys, const int64_t *half_edge, int F, int32_t *parent, int32_t *root,
                                  fsg_stream_t stream) {
    FSG_REQUIRE(sorted_keys && half_edge && parent && root, "fsg_face_union_i32: NULL pointer");
    FSG_REQUIRE(F >= 0 && F <= 0x7fffffff / 3, "fsg_face_union_i32: bad shape F=%d", F);
    if (F == 0) return FSG_OK;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(iota_kernel, dim3(fsg_cdiv(F, BLOCK)), dim3(BLOCK), 0, s, F, parent);
    hipLaunchKernelGGL(face_union_kernel, dim3(fsg_cdiv(3L * F, BLOCK)), dim3(BLOCK), 0, s, sorted_keys, half_edge, 3L * F, F, parent);
    hipLaunchKernelGGL(face_root_kernel, dim3(fsg_cdiv(F, BLOCK)), dim3(BLOCK), 0, s, F, parent, root);
    FSG_CHECK_LAUNCH("fsg_face_union_i32");
    return FSG_OK;
}

extern "C" int fsg_cluster_stats_f64(const float *verts, const int32_t *faces, const int32_t *sorted_clusters, const int64_t *face_order,
                                     const int64_t *sorted_vertex_keys, int V, int F, int C, double *area, int64_t *num_verts,
                                     double *vert_sum, fsg_stream_t stream) {
    FSG_REQUIRE(verts && faces && sorted_clusters && face_order && sorted_vertex_keys && area && num_verts && vert_sum,
                "fsg_cluster_stats_f64: NULL pointer");
    FSG_REQUIRE(V > 0 && F > 0 && F <= 0x7fffffff / 3 && C >= 0 && C <= F, "fsg_cluster_stats_f64: bad shape V=%d F=%d C=%d", V, F, C);
    if (C == 0) return FSG_OK;
    hipLaunchKernelGGL(cluster_stats_kernel, dim3(C), dim3(STATS_BLOCK), 0, (hipStream_t)stream, verts, faces, sorted_clusters, face_order,
                       sorted_vertex_keys, V, F, area, num_verts, vert_sum);
    FSG_CHECK_LAUNCH("fsg_cluster_stats_f64");
    return FSG_OK;
}

extern "C" int fsg_mesh_keep_flags_u8(const float *verts, int V, const int32_t *vert_offset, int B, const uint8_t *keep_in,
                                      const float *boxes, const uint8_t *mask, int D, int H, int W, float sx, float sy, float sz,
                                      uint8_t *keep, fsg_stream_t stream) {
    FSG_REQUIRE(verts && vert_offset && keep, "fsg_mesh_keep_flags_u8: NULL pointer");
    FSG_REQUIRE(V >= 0 && B > 0, "fsg_mesh_keep_flags_u8: bad shape V=%d B=%d", V, B);
    if (mask) {
        FSG_REQUIRE(D > 0 && H > 0 && W > 0 && (long)D * H * W < (1L << 31), "fsg_mesh_keep_flags_u8: bad mask volume %d x %d x %d", D,
                    H, W);
        FSG_REQUIRE(sx > 0.f && sy > 0.f && sz > 0.f && sx < INFINITY && sy < INFINITY && sz < INFINITY,
                    "fsg_mesh_keep_flags_u8: spacing (%g, %g, %g) must be positive and finite", sx, sy, sz);
    }
    if (V == 0) return FSG_OK;
    hipLaunchKernelGGL(keep_flags_kernel, dim3(fsg_cdiv(V, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, verts, V, vert_offset, B,
                       keep_in, boxes, mask, D, H, W, sx, sy, sz, keep);
    FSG_CHECK_LAUNCH("fsg_mesh_keep_flags_u8");
    return FSG_OK;
}

extern "C" int fsg_mesh_face_flags_u8(const int32_t *faces, int V, int F, const uint8_t *vert_keep, const uint8_t *face_keep,
                                      uint8_t *face_out, uint8_t *vert_used, fsg_stream_t stream) {
    FSG_REQUIRE(faces && vert_keep && face_out && vert_used, "fsg_mesh_face_flags_u8: NULL pointer");
    FSG_REQUIRE(V > 0 && F >= 0, "fsg_mesh_face_flags_u8: bad shape V=%d F=%d", V, F);
    if (hipMemsetAsync(vert_used, 0, (size_t)V, (hipStream_t)stream) != hipSuccess) {
        fsg_set_error("fsg_mesh_face_flags_u8: cannot clear the vertex flags");
        return FSG_ERR_HIP;
    }
    if (F == 0) return FSG_OK;
    hipLaunchKernelGGL(face_flags_kernel, dim3(fsg_cdiv(F, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, faces, V, F, vert_keep,
                       face_keep, face_out, vert_used);
    FSG_CHECK_LAUNCH("fsg_mesh_face_flags_u8");
    return FSG_OK;
}

extern "C" int fsg_mesh_compact_f32(const float *verts, const float *normals, const int32_t *faces, int V, int F,
                                    const int32_t *vert_offset, int B, const uint8_t *vert_flag, const int64_t *vert_new,
                                    const uint8_t *face_flag, const int64_t *face_new, float *verts_out, float *normals_out,
                                    int64_t *faces_out, fsg_stream_t stream) {
    FSG_REQUIRE(verts && faces && vert_offset && vert_flag && vert_new && face_flag && face_new && verts_out && faces_out,
                "fsg_mesh_compact_f32: NULL pointer");
    FSG_REQUIRE(!normals == !normals_out, "fsg_mesh_compact_f32: NULL pointer (normals in and out go together)");
    FSG_REQUIRE(V > 0 && F >= 0 && B > 0, "fsg_mesh_compact_f32: bad shape V=%d F=%d B=%d", V, F, B);
    hipLaunchKernelGGL(compact_kernel, dim3(fsg_cdiv(V > F ? V : F, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, verts, normals, faces,
                       V, F, vert_offset, B, vert_flag, vert_new, face_flag, face_new, verts_out, normals_out, faces_out);
    FSG_CHECK_LAUNCH("fsg_mesh_compact_f32");
    return FSG_OK;
}
