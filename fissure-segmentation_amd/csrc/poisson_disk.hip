// Weighted sample elimination (Yuksel, "Sample Elimination for Generating Poisson Disk Sample Sets", CGF 2015), batched and
// bit-reproducible -- include/fsg_hip.h: fsg_sample_elimination_f32.
//
// The reference thins init_factor x N uniform surface samples of one mesh down to N with open3d's
// TriangleMesh.sample_points_poisson_disk (shape_model/point_cloud_registration.py:224 and :338): a heap and a KD-tree on the
// host, one mesh at a time.  Here B items of M samples run together, one workgroup per item, and nothing is read on the host.
//
// The rule (ours; restated bit for bit in tests/poisson_disk_oracle.py):
//   pair     d2 = ((dx dx + dy dy) + dz dz) in fp32 in that order (the build has -ffp-contract=off); i != j are neighbours iff
//            R > 0 and d2 < R R (the fp32 product); d = fmaxf(sqrtf(d2), r_min), t = fmaxf(1 - d / R, 0), w = ((t t)^2)^2
//            (alpha = 8 by three fp32 squarings), q = (int64) rintf(w 2^24).  d2 does not depend on the order of the pair, so
//            q(i, j) = q(j, i).  The clamp of t only matters for r_min > R, where it keeps w inside [0, 1].
//   weight   of a sample: the sum of q over its alive neighbours, an int64 (at most 16383 terms of at most 2^24).  Integer
//            addition is associative: how the initial sum is tiled over lanes and workgroups does not matter, the later
//            subtractions are exact, and an item sees only its own samples.
//   round    remove the alive sample with the largest weight, the lowest index on ties, and subtract q(removed, j) from every
//            alive neighbour j.  M - n_keep rounds.  Without neighbours every weight is 0 and removal runs in index order.
//
// Launches:
//   weights      grid (ceil(M / 256), B), one lane per sample: the sample's row of the pair matrix, 256 columns staged in LDS
//                at a time and read as a broadcast, summed in a register -> workspace (B, M) int64.
//   eliminate    one workgroup per item, min(1024, M rounded up to a wave) threads; lane t owns samples t, t + nt, ...
//                LDS: int64 weight[M] (-1 = removed: the alive flag is the sign) | fp32 x[M] | y[M] | z[M].  The coordinates
//                are staged while 20 M bytes fit beside the cross-wave slots (M <= kCoordLdsMax = 8128); above that the
//                weights alone take 8 M bytes (128 KiB at M = 16384) and the coordinates of the removed sample, three
//                floats a round, are read from global memory (the item's 192 KiB stay in L2).  The staged coordinates
//                serve that one broadcast read only: a lane's own samples (at most 16) sit in its registers.
//                A round is ONE pass of a lane over its samples -- mark the sample removed last round, subtract its pair
//                weight from the lane's alive neighbours, and take the lane's maximum of the key
//                (weight << 14 | 16383 - index) + 1 on the way -- then the DPP wave maximum, one slot per wave in LDS, ONE
//                barrier, and the DPP maximum over the slots, one slot per lane (the slots are double-buffered, so the next
//                round's writes cannot overtake this round's reads).  A lane touches only its own weights: they need no
//                barrier.  After the last round the survivors are compacted in ascending order by a workgroup prefix sum.
//                Measured (MI355X, N = 1024 of M = 5120, 4096 rounds): 7.95 ms for 1 and for 8 items, 10.2 ms for 256 (one
//                per CU), 1.8 us a round beside the weights launch (0.58 ms, 2.7 ms at B = 256);
//                profiles/poisson_disk_bench.jsonl.  With every thread reading all the slots in a loop after the barrier
//                the call took 12.3 ms.  The round is bound by the VALU issue of ONE CU: about 20 instructions per sample
//                (the distance, two 64-bit compares, the key) for M samples on 4 SIMDs.  Untried: a cell grid of side R, so
//                that a round visits the 27 cells around the removed sample instead of every sample, with the arg-max kept
//                per cell.
// No atomics, no scratch; `order` and `keep` are the only global writes of the elimination.
#include <math.h>

#include "fsg_common.h"

namespace {

constexpr int kMaxM = FSG_SAMPLE_ELIMINATION_MAX_POINTS;          // 14 index bits of the key; 8 kMaxM bytes of weights are 128 KiB of LDS
constexpr int kCoordLdsMax = 8128;    // 20 M bytes of weights and coordinates + the static slots <= 160 KiB
constexpr int kMaxThreads = 1024;
constexpr int kMaxWaves = kMaxThreads / 64;
constexpr int kTile = 256;            // weights launch: samples of one workgroup, columns staged at a time
static_assert((size_t)kCoordLdsMax * 20 <= FSG_LDS_WHOLE_CU && (size_t)kMaxM * 8 <= FSG_LDS_WHOLE_CU, "LDS budget");

__device__ __forceinline__ float sqdist_ordered(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the quantised pair weight of two neighbours at squared distance d2
__device__ __forceinline__ long long pair_q(float d2, float R, float r_min) {
    const float d = fmaxf(sqrtf(d2), r_min);
    float t = fmaxf(1.0f - d / R, 0.0f);
    t = t * t;
    t = t * t;
    t = t * t;
    return (long long)rintf(t * 16777216.0f);
}

__global__ __launch_bounds__(kTile) void se_weights_kernel(const float *__restrict__ pts, const float *__restrict__ radii, int M,
                                                           long long *__restrict__ weights) {
    __shared__ float tx[kTile], ty[kTile], tz[kTile];
    const int b = blockIdx.y, t = threadIdx.x, i = blockIdx.x * kTile + t;
    const float *p = pts + (size_t)b * M * 3;
    const float R = radii[2 * b], r_min = radii[2 * b + 1], R2 = R * R;
    const bool ok = i < M;
    if (!(R > 0.0f)) {   // uniform over the workgroup: nobody has a neighbour
        if (ok) weights[(size_t)b * M + i] = 0;
        return;
    }
    const float *q = p + 3 * (size_t)(ok ? i : M - 1);
    const float px = q[0], py = q[1], pz = q[2];
    long long sum = 0;
    for (int j0 = 0; j0 < M; j0 += kTile) {
        const int cnt = min(kTile, M - j0);
        __syncthreads();
        if (t < cnt) {
            const float *r = p + 3 * (size_t)(j0 + t);
            tx[t] = r[0];
            ty[t] = r[1];
            tz[t] = r[2];
        }
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
            const float d2 = sqdist_ordered(px, py, pz, tx[jj], ty[jj], tz[jj]);
            if (d2 < R2 && j0 + jj != i) sum += pair_q(d2, R, r_min);
        }
    }
    if (ok) weights[(size_t)b * M + i] = sum;
}

// CL: the coordinates are staged in LDS (M <= kCoordLdsMax).  PPL: samples per lane, a power of two >= ceil(M / blockDim.x)
template <bool CL, int PPL>
__global__ __launch_bounds__(kMaxThreads) void se_eliminate_kernel(const float *__restrict__ pts, const float *__restrict__ radii,
                                                                   int M, int n_keep, const long long *__restrict__ weights,
                                                                   int32_t *__restrict__ keep, int32_t *__restrict__ order) {
    extern __shared__ __align__(16) char smem[];
    __shared__ u64 wkey[2 * kMaxWaves];
    __shared__ int wcnt[kMaxWaves];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const float *p = pts + (size_t)b * M * 3;
    int32_t *kp = keep + (size_t)b * n_keep;
    const int n_remove = M - n_keep;
    if (n_remove == 0) {   // nothing to remove: the weights were not formed
        for (int j = tid; j < M; j += nt) kp[j] = j;
        return;
    }
    int32_t *ord = order ? order + (size_t)b * n_remove : nullptr;
    long long *wt = (long long *)smem;
    float *cx = (float *)(wt + M), *cy = cx + M, *cz = cy + M;   // (CL only)
    constexpr int WB = PPL < 8 ? PPL : 8;   // weights read from LDS at a time (16 at once would spill)
    float px[PPL], py[PPL], pz[PPL];   // the lane's own samples stay in registers; LDS serves the removed sample's broadcast
#pragma unroll
    for (int r = 0; r < PPL; ++r) {
        const int j = tid + r * nt;
        const bool ok = j < M;
        px[r] = ok ? p[3 * (size_t)j] : 0.f;
        py[r] = ok ? p[3 * (size_t)j + 1] : 0.f;
        pz[r] = ok ? p[3 * (size_t)j + 2] : 0.f;
        if (ok) {
            wt[j] = weights[(size_t)b * M + j];
            if (CL) {
                cx[j] = px[r];
                cy[j] = py[r];
                cz[j] = pz[r];
            }
        }
    }
    const float R = radii[2 * b], r_min = radii[2 * b + 1], R2 = R * R;
    const bool has_r = R > 0.0f;
    if (CL) __syncthreads();   // the removed sample's coordinates are another lane's

    int cur = -1;
    for (int t = 0; t < n_remove; ++t) {
        const bool upd = has_r && cur >= 0;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (upd) {
            qx = CL ? cx[cur] : p[3 * (size_t)cur];
            qy = CL ? cy[cur] : p[3 * (size_t)cur + 1];
            qz = CL ? cz[cur] : p[3 * (size_t)cur + 2];
        }
        u64 best = 0;
#pragma unroll
        for (int r0 = 0; r0 < PPL; r0 += WB) {
            long long w[WB];
#pragma unroll
            for (int r = 0; r < WB; ++r) {   // the reads of a group first: one LDS latency for all of them
                const int j = tid + (r0 + r) * nt;
                w[r] = j < M ? wt[j] : -1;
            }
#pragma unroll
            for (int r = 0; r < WB; ++r) {
                const int j = tid + (r0 + r) * nt;
                if (w[r] < 0) continue;
                if (j == cur) {
                    wt[j] = -1;
                    continue;
                }
                if (upd) {
                    const float d2 = sqdist_ordered(px[r0 + r], py[r0 + r], pz[r0 + r], qx, qy, qz);
                    if (d2 < R2) {
                        w[r] -= pair_q(d2, R, r_min);
                        wt[j] = w[r];
                    }
                }
                const u64 key = (((u64)w[r] << 14) | (u64)(kMaxM - 1 - j)) + 1;
                best = key > best ? key : best;
            }
        }
        best = wave_max_u64_bcast(best);
        const int slot = (t & 1) * kMaxWaves;
        if (lane == 0) wkey[slot + wave] = best;
        __syncthreads();
        best = wave_max_u64_bcast(lane < nw ? wkey[slot + lane] : 0);   // one slot per lane: cheaper than nw reads per thread
        cur = kMaxM - 1 - (int)((best - 1) & (u64)(kMaxM - 1));   // n_keep >= 1: somebody was alive, best > 0
        if (tid == 0 && ord) ord[t] = cur;
    }
    if (cur % nt == tid) wt[cur] = -1;   // the last removal, by its owner

    // survivors in ascending order: samples j0 .. j0 + nt - 1 of a pass are one per thread, in thread order
    int base = 0;
    for (int j0 = 0; j0 < M; j0 += nt) {
        const int j = j0 + tid;
        const int flag = j < M && wt[j] >= 0;
        const int incl = wave_incl_scan(flag);
        __syncthreads();   // (the previous pass has read wcnt)
        if (lane == 63) wcnt[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < nw; ++w) {
            const int c = wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (flag) kp[base + before + incl - 1] = j;
        base += total;
    }
}

}  // namespace

extern "C" size_t fsg_sample_elimination_workspace_bytes(int B, int M) {
    if (B <= 0 || M <= 0) return 0;
    return (size_t)B * (size_t)M * sizeof(long long);
}

extern "C" int fsg_sample_elimination_f32(const float *points, const float *radii, int B, int M, int n_keep, int32_t *keep,
                                          int32_t *order, void *workspace, size_t workspace_bytes, fsg_stream_t stream) {
    const char *who = "fsg_sample_elimination_f32";
    FSG_REQUIRE(B >= 0 && B <= 65535 && M >= 1 && n_keep >= 1 && n_keep <= M,
                "%s: bad shape B=%d M=%d n_keep=%d (1 <= n_keep <= M, B <= 65535)", who, B, M, n_keep);
    if (M > kMaxM) {
        fsg_set_error("%s: M=%d samples per item, the kernel keeps at most %d weights in LDS", who, M, kMaxM);
        return FSG_ERR_UNSUPPORTED;
    }
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(points && radii && keep, "%s: NULL pointer", who);
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: workspace must be non-NULL and 8-byte aligned", who);
    FSG_REQUIRE(workspace_bytes >= fsg_sample_elimination_workspace_bytes(B, M), "%s: workspace of %zu bytes, %zu needed", who,
                workspace_bytes, fsg_sample_elimination_workspace_bytes(B, M));
    long long *weights = (long long *)workspace;
    const bool cl = M <= kCoordLdsMax;
    const size_t lds = (size_t)M * (cl ? 20 : 8);
    const int nt = M >= kMaxThreads ? kMaxThreads : 64 * fsg_cdiv(M, 64);
    const int per_lane = fsg_cdiv(M, nt);
#define SE_LAUNCH(CL, PPL)                                                                                                    \
    do {                                                                                                                      \
        FSG_GRANT_LDS(who, (se_eliminate_kernel<CL, PPL>), lds);                                                              \
        if (n_keep < M) {                                                                                                     \
            hipLaunchKernelGGL(se_weights_kernel, dim3(fsg_cdiv(M, kTile), B), dim3(kTile), 0, (hipStream_t)stream, points,   \
                               radii, M, weights);                                                                            \
            FSG_CHECK_LAUNCH(who);                                                                                            \
        }                                                                                                                     \
        hipLaunchKernelGGL((se_eliminate_kernel<CL, PPL>), dim3(B), dim3(nt), lds, (hipStream_t)stream, points, radii, M,     \
                           n_keep, (const long long *)weights, keep, order);                                                  \
    } while (0)
    if (!cl) SE_LAUNCH(false, 16);
    else if (per_lane > 4) SE_LAUNCH(true, 8);
    else if (per_lane > 2) SE_LAUNCH(true, 4);
    else if (per_lane > 1) SE_LAUNCH(true, 2);
    else SE_LAUNCH(true, 1);
#undef SE_LAUNCH
    FSG_CHECK_LAUNCH(who);
    return FSG_OK;
}
