// Lloyd's k-means on 3-D points, batched, bit-reproducible -- include/fsg_hip.h: fsg_kmeans_prepare_f32, fsg_kmeans_step_f32,
// fsg_kmeans_assign_f32.
//
// The reference pools the registered clouds of all instances of one object and clusters them with sklearn.cluster.k_means on
// the CPU, one object at a time (shape_model/generate_corresponding_points.py:44-48).  Here B items of n points and K centres
// run together; one iteration is two launches and nothing is read on the host:
//   assign    one lane owns one point.  The centres are staged in LDS (kChunk at a time, read as a broadcast; the running
//             minimum is carried across chunks), d = ((dx dx + dy dy) + dz dz) in fp32 in exactly that order (the build has
//             -ffp-contract=off), strict `<` over ascending centre index: the lowest index wins a tie.  The label goes out as
//             int32; the point's coordinates, a count and the distance are added to LDS accumulators of the workgroup, which
//             end in the item's global accumulators, one atomic per touched cluster and component.
//   finalize  one workgroup per item: new centre = sum / count in fp64, rounded to fp32; an empty cluster keeps its centre
//             (scipy.cluster.vq.kmeans2's rule); the squared centre shift, the stopping rule and the freeze; the accumulators
//             are left zeroed for the next assign.
//
// Reproducibility: every sum that crosses lanes is an INTEGER sum.  A coordinate x becomes llrint(x * 2^s) (round half to
// even, in fp64, where x * 2^s is exact), a squared distance llrint(d * 2^si), with
//   e = frexp exponent of the item's largest |coordinate| over points and initial centres (M < 2^e; M = 0: e = 0),
//   L = ceil(log2 n),   s = 62 - L - e,   si = 62 - L - (2 e + 4)
// so that |x 2^s| < 2^(62 - L) and d 2^si < 2^(62 - L) (d <= 3 (2 M)^2 < 2^(2 e + 4)) and n of them cannot leave int64.  Integer
// addition is associative: the order in which lanes, workgroups and atomics arrive does not matter, and an item sees only its
// own scale.  The two fp64 reductions (variance in prepare, centre shift in finalize) run in the fixed order of block_sum.
//
// Coordinates must be finite.  K <= kMaxK = 4096 (28 K bytes of LDS accumulators beside the 16 KiB centre tile), n <= 2^24.
#include <math.h>

#include "fsg_common.h"

namespace {

constexpr int kThreads = 256;   // assign: points of one tile, one per lane
constexpr int kChunk = 1024;    // centres staged at a time (16 KiB as float4)
constexpr int kMaxK = FSG_KMEANS_MAX_K;
constexpr int kRed = 1024;      // threads of the per-item kernels (prepare, finalize)
constexpr int kBlocksTarget = 2048;   // workgroups of one assign launch the tiles are spread over (about 8 per CU)

struct ItemState {   // per item, in the workspace
    unsigned long long inertia_fix;   // sum of llrint(d 2^si) of the running assign
    double threshold;                 // tol * mean over the axes of the variance of the points
    int s, si;                        // the two fixed-point exponents
    int active, n_iter;
    unsigned n_changed;
    int pad;
};
static_assert(sizeof(ItemState) == 40, "ItemState layout");

__host__ __device__ inline size_t item_bytes(int K) { return (size_t)K * 24 + (size_t)((K + 1) & ~1) * 4 + 48; }

struct ItemView {
    unsigned long long *sums;   // (K, 3)
    unsigned *counts;           // (K)
    ItemState *st;
};
__device__ __forceinline__ ItemView view(char *ws, int b, int K) {
    char *base = ws + (size_t)b * item_bytes(K);
    return {(unsigned long long *)base, (unsigned *)(base + (size_t)K * 24), (ItemState *)(base + item_bytes(K) - 48)};
}

// sum of v over the kRed threads of the workgroup in a fixed order: the halving tree over thread indices.  Every thread gets it.
__device__ __forceinline__ double block_sum(double v, double *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int step = kRed / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + step];
        __syncthreads();
    }
    return red[0];
}

// Once per run, one workgroup per item: scales, the stopping threshold, zeroed accumulators, active = 1, n_iter = 0.
__global__ __launch_bounds__(kRed) void kmeans_prepare_kernel(const float *__restrict__ pts, const float *__restrict__ cen, int n,
                                                              int K, double tol, char *ws) {
    __shared__ double red[kRed];
    __shared__ float redf[kRed];
    const int b = blockIdx.x, t = threadIdx.x;
    const float *p = pts + (size_t)b * n * 3, *c = cen + (size_t)b * K * 3;
    ItemView v = view(ws, b, K);
    for (int i = t; i < 3 * K; i += kRed) v.sums[i] = 0;
    for (int i = t; i < K; i += kRed) v.counts[i] = 0;

    float m = 0.0f;
    for (size_t i = t; i < (size_t)3 * n; i += kRed) m = fmaxf(m, fabsf(p[i]));
    for (int i = t; i < 3 * K; i += kRed) m = fmaxf(m, fabsf(c[i]));
    redf[t] = m;
    __syncthreads();
    for (int step = kRed / 2; step > 0; step >>= 1) {
        if (t < step) redf[t] = fmaxf(redf[t], redf[t + step]);
        __syncthreads();
    }
    m = redf[0];

    // variance per axis, two passes in fp64: thread t adds rows t, t + kRed, ... in that order, then the tree
    double var[3];
    for (int a = 0; a < 3; ++a) {
        double acc = 0.0;
        for (int i = t; i < n; i += kRed) acc = acc + (double)p[3 * (size_t)i + a];
        const double mean = block_sum(acc, red) / (double)n;
        acc = 0.0;
        for (int i = t; i < n; i += kRed) {
            const double d = (double)p[3 * (size_t)i + a] - mean;
            acc = acc + d * d;
        }
        var[a] = block_sum(acc, red) / (double)n;
    }
    if (t == 0) {
        int e = 0;
        if (m > 0.0f) (void)frexpf(m, &e);
        int L = 0;
        while (((long long)1 << L) < (long long)n) ++L;
        ItemState *st = v.st;
        st->inertia_fix = 0;
        st->threshold = tol * (((var[0] + var[1]) + var[2]) / 3.0);
        st->s = 62 - L - e;
        st->si = 62 - L - (2 * e + 4);
        st->active = 1;
        st->n_iter = 0;
        st->n_changed = 0;
        st->pad = 0;
    }
}

// LDS: float4 tile[kChunk] | u64 sums[3 K] | u32 counts[K]
__global__ __launch_bounds__(kThreads) void kmeans_assign_kernel(const float *__restrict__ pts, const float *__restrict__ cen,
                                                                 int32_t *__restrict__ labels, int n, int K, int tiles_per_block,
                                                                 char *ws, int force) {
    extern __shared__ __align__(16) char smem[];
    __shared__ unsigned long long blk_inertia;
    __shared__ unsigned blk_changed;
    float4 *tile = (float4 *)smem;
    unsigned long long *lsum = (unsigned long long *)(smem + (size_t)kChunk * sizeof(float4));
    unsigned *lcnt = (unsigned *)(lsum + 3 * (size_t)K);

    const int b = blockIdx.y, t = threadIdx.x;
    ItemView v = view(ws, b, K);
    if (!force && !v.st->active) return;   // a frozen item: nothing of it changes (uniform over the workgroup)
    const int s = v.st->s, si = v.st->si;
    const float *p = pts + (size_t)b * n * 3, *c = cen + (size_t)b * K * 3;
    int32_t *lab = labels + (size_t)b * n;

    for (int i = t; i < 3 * K; i += kThreads) lsum[i] = 0;
    for (int i = t; i < K; i += kThreads) lcnt[i] = 0;
    if (t == 0) {
        blk_inertia = 0;
        blk_changed = 0;
    }
    const int ntiles = (n + kThreads - 1) / kThreads;
    const int t0 = blockIdx.x * tiles_per_block, t1 = min(ntiles, t0 + tiles_per_block);
    const bool one_chunk = K <= kChunk;
    bool staged = false;
    unsigned long long my_inertia = 0;
    unsigned my_changed = 0;

    for (int tl = t0; tl < t1; ++tl) {
        const int i = tl * kThreads + t;
        const bool ok = i < n;
        const float *q = p + 3 * (size_t)(ok ? i : n - 1);
        const float px = q[0], py = q[1], pz = q[2];
        float best = INFINITY;
        int arg = 0;
        for (int c0 = 0; c0 < K; c0 += kChunk) {
            const int cnt = min(kChunk, K - c0);
            if (!(one_chunk && staged)) {   // K <= kChunk: the tile of the first pass stays
                __syncthreads();
                for (int j = t; j < cnt; j += kThreads) {
                    const float *r = c + 3 * (size_t)(c0 + j);
                    tile[j] = make_float4(r[0], r[1], r[2], 0.0f);
                }
                __syncthreads();
                staged = true;
            }
#pragma unroll 4
            for (int j = 0; j < cnt; ++j) {
                const float4 r = tile[j];
                const float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
                const float d = ((dx * dx + dy * dy) + dz * dz);
                if (d < best) {
                    best = d;
                    arg = c0 + j;
                }
            }
        }
        if (ok) {
            my_changed += lab[i] != arg;
            lab[i] = arg;
            atomicAdd(&lsum[3 * arg + 0], (unsigned long long)llrint(ldexp((double)px, s)));
            atomicAdd(&lsum[3 * arg + 1], (unsigned long long)llrint(ldexp((double)py, s)));
            atomicAdd(&lsum[3 * arg + 2], (unsigned long long)llrint(ldexp((double)pz, s)));
            atomicAdd(&lcnt[arg], 1u);
            my_inertia += (unsigned long long)llrint(ldexp((double)best, si));
        }
    }
    atomicAdd(&blk_inertia, my_inertia);
    if (my_changed) atomicAdd(&blk_changed, my_changed);
    __syncthreads();
    for (int k = t; k < K; k += kThreads) {
        const unsigned cnt = lcnt[k];
        if (cnt) {
            atomicAdd(&v.counts[k], cnt);
            atomicAdd(&v.sums[3 * k + 0], lsum[3 * k + 0]);
            atomicAdd(&v.sums[3 * k + 1], lsum[3 * k + 1]);
            atomicAdd(&v.sums[3 * k + 2], lsum[3 * k + 2]);
        }
    }
    if (t == 0) {
        atomicAdd(&v.st->inertia_fix, blk_inertia);
        if (blk_changed) atomicAdd(&v.st->n_changed, blk_changed);
    }
}

// One workgroup per item.  update = 1: the second launch of an iteration (new centres, stopping rule); update = 0: report the
// accumulators of a plain assign.  Either way they are zero afterwards.  A frozen item is skipped unless `force`.
__global__ __launch_bounds__(kRed) void kmeans_finalize_kernel(float *__restrict__ cen, int K, char *ws, int update, int force,
                                                               int32_t *__restrict__ counts_out, double *__restrict__ stats,
                                                               int32_t *__restrict__ info) {
    __shared__ double red[kRed];
    __shared__ unsigned empties;
    const int b = blockIdx.x, t = threadIdx.x;
    ItemView v = view(ws, b, K);
    ItemState *st = v.st;
    if (!force && !st->active) return;
    const int s = st->s;
    float *c = cen + (size_t)b * K * 3;
    if (t == 0) empties = 0;
    __syncthreads();
    double shift = 0.0;
    unsigned my_empty = 0;
    for (int k = t; k < K; k += kRed) {
        const unsigned cnt = v.counts[k];
        if (counts_out) counts_out[(size_t)b * K + k] = (int32_t)cnt;
        v.counts[k] = 0;
        double d[3];
        for (int a = 0; a < 3; ++a) {
            const long long sum = (long long)v.sums[3 * k + a];
            v.sums[3 * k + a] = 0;
            const float old = c[3 * k + a];
            float neu = old;
            if (cnt) neu = (float)ldexp((double)sum / (double)cnt, -s);
            d[a] = (double)neu - (double)old;
            if (update) c[3 * k + a] = neu;
        }
        my_empty += cnt == 0;
        shift = shift + ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    }
    if (my_empty) atomicAdd(&empties, my_empty);
    shift = block_sum(shift, red);   // (its barriers also publish `empties`)
    if (t == 0) {
        const unsigned changed = st->n_changed;
        const double inertia = ldexp((double)(long long)st->inertia_fix, -st->si);
        st->inertia_fix = 0;
        st->n_changed = 0;
        if (update) {
            st->n_iter += 1;
            if (changed == 0 || shift <= st->threshold) st->active = 0;
        }
        if (stats) {
            stats[2 * b] = inertia;
            stats[2 * b + 1] = shift;
        }
        if (info) {
            info[4 * b] = (int32_t)changed;
            info[4 * b + 1] = (int32_t)empties;
            info[4 * b + 2] = st->n_iter;
            info[4 * b + 3] = st->active;
        }
    }
}

int check(const char *who, int B, int n, int K) {
    FSG_REQUIRE(B >= 0 && B <= 65535 && n >= 1 && n <= FSG_KMEANS_MAX_POINTS && K >= 1 && K <= kMaxK && K <= n,
                "%s: bad shape B=%d n=%d K=%d (1 <= K <= min(n, %d), n <= 2^24, B <= 65535)", who, B, n, K, kMaxK);
    return FSG_OK;
}

int check_workspace(const char *who, int B, int n, int K, const void *workspace, size_t workspace_bytes) {
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: workspace must be non-NULL and 8-byte aligned", who);
    FSG_REQUIRE(workspace_bytes >= fsg_kmeans_workspace_bytes(B, n, K), "%s: workspace of %zu bytes, %zu needed", who,
                workspace_bytes, fsg_kmeans_workspace_bytes(B, n, K));
    return FSG_OK;
}

int run(const char *who, const float *points, float *centroids, int32_t *labels, int B, int n, int K, void *workspace,
        size_t workspace_bytes, int update, int32_t *counts, double *stats, int32_t *info, fsg_stream_t stream) {
    int rc = check(who, B, n, K);
    if (rc != FSG_OK) return rc;
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(points && centroids && labels, "%s: NULL pointer", who);
    rc = check_workspace(who, B, n, K, workspace, workspace_bytes);
    if (rc != FSG_OK) return rc;
    const size_t lds = (size_t)kChunk * sizeof(float4) + (size_t)K * 28;
    FSG_GRANT_LDS(who, kmeans_assign_kernel, lds);
    const int ntiles = fsg_cdiv(n, kThreads);
    const int per_item = kBlocksTarget / B > 0 ? kBlocksTarget / B : 1;
    const int tiles_per_block = fsg_cdiv(ntiles, per_item);
    const int force = update ? 0 : 1;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(fsg_cdiv(ntiles, tiles_per_block), B), dim3(kThreads), lds, (hipStream_t)stream,
                       points, (const float *)centroids, labels, n, K, tiles_per_block, (char *)workspace, force);
    FSG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(kmeans_finalize_kernel, dim3(B), dim3(kRed), 0, (hipStream_t)stream, centroids, K, (char *)workspace, update,
                       force, counts, stats, info);
    FSG_CHECK_LAUNCH(who);
    return FSG_OK;
}

}  // namespace

extern "C" size_t fsg_kmeans_workspace_bytes(int B, int n, int K) {
    (void)n;
    if (B <= 0 || K <= 0) return 0;
    return (size_t)B * item_bytes(K);
}

extern "C" int fsg_kmeans_prepare_f32(const float *points, const float *centroids, int B, int n, int K, double tol,
                                      void *workspace, size_t workspace_bytes, fsg_stream_t stream) {
    int rc = check("fsg_kmeans_prepare_f32", B, n, K);
    if (rc != FSG_OK) return rc;
    FSG_REQUIRE(tol >= 0.0, "fsg_kmeans_prepare_f32: tol=%g must not be negative", tol);
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(points && centroids, "fsg_kmeans_prepare_f32: NULL pointer");
    rc = check_workspace("fsg_kmeans_prepare_f32", B, n, K, workspace, workspace_bytes);
    if (rc != FSG_OK) return rc;
    hipLaunchKernelGGL(kmeans_prepare_kernel, dim3(B), dim3(kRed), 0, (hipStream_t)stream, points, centroids, n, K, tol,
                       (char *)workspace);
    FSG_CHECK_LAUNCH("fsg_kmeans_prepare_f32");
    return FSG_OK;
}

extern "C" int fsg_kmeans_step_f32(const float *points, float *centroids, int32_t *labels, int B, int n, int K, void *workspace,
                                   size_t workspace_bytes, int32_t *counts, double *stats, int32_t *info, fsg_stream_t stream) {
    return run("fsg_kmeans_step_f32", points, centroids, labels, B, n, K, workspace, workspace_bytes, 1, counts, stats, info,
               stream);
}

extern "C" int fsg_kmeans_assign_f32(const float *points, const float *centroids, int32_t *labels, int B, int n, int K,
                                     void *workspace, size_t workspace_bytes, int32_t *counts, double *stats, int32_t *info,
                                     fsg_stream_t stream) {
    return run("fsg_kmeans_assign_f32", points, (float *)centroids, labels, B, n, K, workspace, workspace_bytes, 0, counts, stats,
               info, stream);
}
