// DSEG-AE glue between the segmentation network and the point-cloud auto-encoder -- include/fsg_hip.h: fsg_label_partition,
// fsg_segment_jitter_extend_f32, fsg_fps_start_f32.  Replace, for all (item, object) groups of a batch at once, what
// dseg_ae_regularization.py:62-138 of the reference does once per object of one cloud: the boolean-mask gather of an object's
// points, random_extend_points and the pure-torch farthest point sampling loop with its random start.
//
// No atomics, no scratch, fixed summation orders: the same bits on every run, for a group alone or inside a batch.
#include "fsg_common.h"

namespace {

// ------------------------------------------------------------------------------------------------- stable label partition
constexpr int PT = 256;               // threads of a partition workgroup
constexpr int PTILE = 1024;           // points of a tile
constexpr int PR = PTILE / PT;        // rounds of a tile: point j = t PTILE + r PT + tid
constexpr int PW = PT / 64;           // waves
constexpr int PSLOT = PR * PW;        // (round, wave) slots of a tile, in ascending point order
constexpr int MAXL = FSG_PARTITION_MAX_LABELS;

// the label of point i relative to first_label, or -1 outside [0, L)
__device__ __forceinline__ int rel_label(const void *__restrict__ lab, int kind, long i, int first, int L) {
    const long v = kind == FSG_LABEL_U8 ? (long)((const uint8_t *)lab)[i]
                 : kind == FSG_LABEL_I32 ? (long)((const int32_t *)lab)[i] : (long)((const int64_t *)lab)[i];
    const long r = v - first;
    return r >= 0 && r < L ? (int)r : -1;
}

// one wave ballot per (round, object): wcnt[slot][l] = points of object l in the slot, rank[r] = how many of them lie before
// this lane's point (its place inside the slot when it carries that label)
__device__ __forceinline__ void tile_ballots(const void *__restrict__ lab, int kind, long item0, int N, int t, int first, int L,
                                             int (&rel)[PR], int (&rank)[PR], int *wcnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        const int j = t * PTILE + r * PT + tid;
        rel[r] = j < N ? rel_label(lab, kind, item0 + j, first, L) : -1;
        rank[r] = 0;
        for (int l = 0; l < L; ++l) {
            const unsigned long long m = __ballot(rel[r] == l);
            const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (rel[r] == l) rank[r] = below;
            if (lane == 0) wcnt[(r * PW + wave) * MAXL + l] = __popcll(m);
        }
    }
}

__global__ __launch_bounds__(PT) void partition_hist_kernel(const void *__restrict__ lab, int kind, int N, int T, int first, int L,
                                                             int32_t *__restrict__ hist) {
    __shared__ int wcnt[PSLOT * MAXL];
    const int b = blockIdx.x / T, t = blockIdx.x - b * T;
    int rel[PR], rank[PR];
    tile_ballots(lab, kind, (long)b * N, N, t, first, L, rel, rank, wcnt);
    __syncthreads();
    if ((int)threadIdx.x < L) {
        int s = 0;
#pragma unroll
        for (int q = 0; q < PSLOT; ++q) s += wcnt[q * MAXL + threadIdx.x];
        hist[(long)blockIdx.x * L + threadIdx.x] = s;
    }
}

// tile (b, t): the place of its first point of object l is [groups before (b, l) in (item, object) order] + [object l in the
// tiles of item b before t]; both come from the tile counts, walked 16 rows of (item, tile) at a time and summed in row order
__global__ __launch_bounds__(PT) void partition_scatter_kernel(const void *__restrict__ lab, int kind, const float *__restrict__ x,
                                                                int C, int N, int T, int first, int L,
                                                                const int32_t *__restrict__ hist, int32_t *__restrict__ counts,
                                                                int32_t *__restrict__ offset, float *__restrict__ xyz,
                                                                int32_t *__restrict__ src) {
    __shared__ int wcnt[PSLOT * MAXL];
    __shared__ int red[3][16][MAXL];
    __shared__ int tot[3][MAXL];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int b = blockIdx.x / T, t = blockIdx.x - b * T;
    int rel[PR], rank[PR];
    tile_ballots(lab, kind, (long)b * N, N, t, first, L, rel, rank, wcnt);

    const int row0 = tid >> 4, lp = tid & 15;
    int sA = 0, sB = 0, sC = 0;   // object lp: in the items before b; in item b; in item b's tiles before t
    if (lp < L)
        for (int row = row0; row < (b + 1) * T; row += 16) {
            const int h = hist[(long)row * L + lp];
            if (row < b * T) sA += h;
            else {
                sB += h;
                if (row < b * T + t) sC += h;
            }
        }
    red[0][row0][lp] = sA;
    red[1][row0][lp] = sB;
    red[2][row0][lp] = sC;
    __syncthreads();
    if (tid < 3 * MAXL) {
        const int w = tid >> 4, l = tid & 15;
        int s = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += red[w][q][l];
        tot[w][l] = s;
    }
    __syncthreads();
    if (tid < L) {
        int before = 0;
        for (int l = 0; l < L; ++l) before += tot[0][l] + (l < tid ? tot[1][l] : 0);
        if (t == 0) {
            counts[b * L + tid] = tot[1][tid];
            offset[b * L + tid] = before + tot[1][tid];
        }
        int run = before + tot[2][tid];
#pragma unroll
        for (int q = 0; q < PSLOT; ++q) {
            const int c = wcnt[q * MAXL + tid];
            wcnt[q * MAXL + tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        if (rel[r] < 0) continue;
        const int j = t * PTILE + r * PT + tid;
        const long dst = wcnt[(r * PW + wave) * MAXL + rel[r]] + rank[r];
        const float *xb = x + (long)b * C * N + j;
        xyz[3 * dst] = xb[0];
        xyz[3 * dst + 1] = xb[N];
        xyz[3 * dst + 2] = xb[2L * N];
        src[dst] = j;
    }
}

// ---------------------------------------------------------------------------------------- jittered extension of segments
constexpr int JT = 256;

// sum of one double per thread over the workgroup, to every thread: strided partial sums, the wave tree, the waves in order
__device__ __forceinline__ double block_sum_f64(double v, double *red) {
    v = wave_sum_lane0(v);
    __syncthreads();   // (the previous use of red is over)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < JT / 64; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(JT) void jitter_extend_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ offset,
                                                            const float *__restrict__ nn_d2, const int32_t *__restrict__ new_offset,
                                                            const int32_t *__restrict__ src_idx, const float *__restrict__ direction,
                                                            const float *__restrict__ z, float *__restrict__ out,
                                                            float *__restrict__ stats) {
    __shared__ double red[JT / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int st = g ? offset[g - 1] : 0, len = offset[g] - st;
    const int ns = g ? new_offset[g - 1] : 0, nlen = new_offset[g] - ns;
    const int ps = ns - st;   // this segment's first padded row: the segments before it grew by that much
    float mean = 0.f, sd = 0.f;
    if (len >= 2) {   // (wave-uniform)
        double s = 0.0;
        for (int j = tid; j < len; j += JT) s += (double)sqrtf(nn_d2[st + j]);
        const double mu = block_sum_f64(s, red) / len;
        double q = 0.0;
        for (int j = tid; j < len; j += JT) {
            const double d = (double)sqrtf(nn_d2[st + j]) - mu;
            q += d * d;
        }
        mean = (float)mu;
        sd = (float)sqrt(block_sum_f64(q, red) / (len - 1));
    }
    if (tid == 0) {
        stats[2 * g] = mean;
        stats[2 * g + 1] = sd;
    }
    const int keep = len < nlen ? len : nlen;
    for (int e = tid; e < 3 * keep; e += JT) out[3L * ns + e] = xyz[3L * st + e];
    for (int p = tid; p < nlen - keep; p += JT) {
        float ox = 0.f, oy = 0.f, oz = 0.f;
        if (len > 0) {
            const long row = ps + p;
            const long s = st + clampi(src_idx[row], len - 1);
            const float dx = direction[3 * row], dy = direction[3 * row + 1], dz = direction[3 * row + 2];
            const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
            const float mag = z[row] * sd + mean;
            ox = xyz[3 * s] + dx / nrm * mag;
            oy = xyz[3 * s + 1] + dy / nrm * mag;
            oz = xyz[3 * s + 2] + dz / nrm * mag;
        }
        out[3L * (ns + keep + p)] = ox;
        out[3L * (ns + keep + p) + 1] = oy;
        out[3L * (ns + keep + p) + 2] = oz;
    }
}

// ------------------------------------------------------------------------------- farthest point sampling with a start index
// One workgroup of 16 waves per segment.  Up to 16 384 points the segment's coordinates and running minima live in registers
// (PPL per lane, point j = tid + 1024 r); the arithmetic and the tie rule are fps_multi_wave's (pointops.hip): sqdist3, fminf,
// largest distance, then lowest index.  The coordinates cannot all live in LDS as they do there, so each lane carries the
// coordinates of its best candidate and a wave's winner puts them next to its key: the next pivot is an LDS broadcast, not a
// dependent global load.
constexpr int FT = 1024, FWAVES = FT / 64, FMAX_PPL = 16;

struct FpsSlot {
    u64 key;
    float x, y, z, pad;
};

// the workgroup's arg-max from each lane's candidate (bv, bj) with coordinates (bx, by, bz): -> the winning index, and the
// winner's coordinates in (cx, cy, cz).  slots: the half of the double buffer that belongs to this iteration.
__device__ __forceinline__ int fps_block_pick(float bv, int bj, float bx, float by, float bz, FpsSlot *slots, float &cx, float &cy,
                                              float &cz) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 k = bv >= 0.f ? (((u64)__float_as_uint(bv) << 32) | (unsigned)(0x7fffffff - bj)) : 0ull;
    const u64 wk = wave_max_u64_bcast(k);
    if (wk == 0ull) {
        if (lane == 0) slots[wave].key = 0ull;
    } else if (k == wk) {   // one lane: indices are unique
        slots[wave].key = wk;
        slots[wave].x = bx;
        slots[wave].y = by;
        slots[wave].z = bz;
    }
    __syncthreads();
    u64 best = slots[lane & (FWAVES - 1)].key;   // every row of 16 lanes holds the 16 waves' keys
#pragma unroll
    for (int s = 0; s < 4; ++s) best = dpp_max_step(best, s);   // butterfly inside the rows: every lane has the maximum
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)best);
    const int cur = 0x7fffffff - (int)lo;
    const FpsSlot *w = slots + ((cur >> 6) & (FWAVES - 1));   // the winner's wave, for both index layouts below
    cx = w->x;
    cy = w->y;
    cz = w->z;
    return cur;
}

template <int PPL>
__device__ __forceinline__ void fps_registers(const float *__restrict__ xyz, int st, int len, int cur, int qs, int qe,
                                              int32_t *__restrict__ idx, FpsSlot *slots) {
    const int tid = threadIdx.x;
    float px[PPL], py[PPL], pz[PPL], md[PPL];
#pragma unroll
    for (int r = 0; r < PPL; ++r) {
        const int j = tid + FT * r;
        const bool ok = j < len;
        px[r] = ok ? xyz[3L * (st + j)] : 0.f;
        py[r] = ok ? xyz[3L * (st + j) + 1] : 0.f;
        pz[r] = ok ? xyz[3L * (st + j) + 2] : 0.f;
        md[r] = 1e10f;
    }
    float cx = xyz[3L * (st + cur)], cy = xyz[3L * (st + cur) + 1], cz = xyz[3L * (st + cur) + 2];
    if (tid == 0) idx[qs] = st + cur;
    for (int t = qs + 1; t < qe; ++t) {
        float bv = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bj = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < PPL; ++r) {
            const int j = tid + FT * r;
            const float d = sqdist3(px[r], py[r], pz[r], cx, cy, cz);
            const float v = fminf(d, md[r]);
            md[r] = v;
            if (j < len && v > bv) { bv = v; bj = j; bx = px[r]; by = py[r]; bz = pz[r]; }
        }
        cur = fps_block_pick(bv, bj, bx, by, bz, slots + (t & 1) * FWAVES, cx, cy, cz);
        if (tid == 0) idx[t] = st + cur;
    }
}

// segments of more than 16 384 points: coordinates and running minima from global memory (md: the caller's scratch, this
// segment's rows of it), same workgroup, same arg-max.  The winner's wave is (j mod 1024) / 64 here too.
__device__ __forceinline__ void fps_global(const float *__restrict__ xyz, int st, int len, int cur, int qs, int qe,
                                           float *__restrict__ md, int32_t *__restrict__ idx, FpsSlot *slots) {
    const int tid = threadIdx.x;
    for (int j = tid; j < len; j += FT) md[st + j] = 1e10f;
    float cx = xyz[3L * (st + cur)], cy = xyz[3L * (st + cur) + 1], cz = xyz[3L * (st + cur) + 2];
    if (tid == 0) idx[qs] = st + cur;
    for (int t = qs + 1; t < qe; ++t) {
        float bv = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bj = 0x7fffffff;
        for (int j = tid; j < len; j += FT) {
            const float x = xyz[3L * (st + j)], y = xyz[3L * (st + j) + 1], zc = xyz[3L * (st + j) + 2];
            const float v = fminf(sqdist3(x, y, zc, cx, cy, cz), md[st + j]);
            md[st + j] = v;
            if (v > bv) { bv = v; bj = j; bx = x; by = y; bz = zc; }
        }
        cur = fps_block_pick(bv, bj, bx, by, bz, slots + (t & 1) * FWAVES, cx, cy, cz);
        if (tid == 0) idx[t] = st + cur;
    }
}

__global__ __launch_bounds__(FT) void fps_start_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ offset,
                                                        const int32_t *__restrict__ new_offset, const int32_t *__restrict__ start,
                                                        float *__restrict__ md, int32_t *__restrict__ idx) {
    __shared__ FpsSlot slots[2 * FWAVES];
    const int s = blockIdx.x;
    const int st = s ? offset[s - 1] : 0, len = offset[s] - st;
    const int qs = s ? new_offset[s - 1] : 0, qe = new_offset[s];
    if (qe <= qs) return;
    if (len <= 0) {   // samples asked of an empty segment: index 0, as fsg_fps_f32 answers
        for (int t = qs + (int)threadIdx.x; t < qe; t += FT) idx[t] = 0;
        return;
    }
    const int cur = start ? clampi(start[s], len - 1) : 0;
    if (len <= 4 * FT) fps_registers<4>(xyz, st, len, cur, qs, qe, idx, slots);
    else if (len <= 8 * FT) fps_registers<8>(xyz, st, len, cur, qs, qe, idx, slots);
    else if (len <= FMAX_PPL * FT) fps_registers<FMAX_PPL>(xyz, st, len, cur, qs, qe, idx, slots);
    else fps_global(xyz, st, len, cur, qs, qe, md, idx, slots);
}

}  // namespace

extern "C" size_t fsg_label_partition_workspace_bytes(int B, int N, int L) {
    if (B <= 0 || N <= 0 || L <= 0) return 0;
    return (size_t)B * (size_t)fsg_cdiv(N, PTILE) * (size_t)L * sizeof(int32_t);
}

extern "C" int fsg_label_partition(const void *labels, int label_kind, const float *x, int B, int C, int N, int first_label, int L,
                                   int32_t *counts, int32_t *offset, float *xyz, int32_t *src, void *workspace,
                                   size_t workspace_bytes, fsg_stream_t stream) {
    FSG_REQUIRE(labels && x && counts && offset && xyz && src && workspace, "fsg_label_partition: NULL pointer");
    FSG_REQUIRE(label_kind == FSG_LABEL_U8 || label_kind == FSG_LABEL_I32 || label_kind == FSG_LABEL_I64,
                "fsg_label_partition: label_kind %d", label_kind);
    FSG_REQUIRE(B > 0 && N > 0 && C >= 3 && L >= 1 && L <= MAXL && (long)B * N < (1L << 31) && (long)B * C * N < (1L << 40),
                "fsg_label_partition: bad shape B=%d C=%d N=%d L=%d (1 <= L <= %d, B N < 2^31)", B, C, N, L, MAXL);
    FSG_REQUIRE(workspace_bytes >= fsg_label_partition_workspace_bytes(B, N, L), "fsg_label_partition: workspace of %zu bytes",
                workspace_bytes);
    const int T = fsg_cdiv(N, PTILE);
    hipStream_t st = (hipStream_t)stream;
    int32_t *hist = (int32_t *)workspace;
    hipLaunchKernelGGL(partition_hist_kernel, dim3(B * T), dim3(PT), 0, st, labels, label_kind, N, T, first_label, L, hist);
    FSG_CHECK_LAUNCH("fsg_label_partition/hist");
    hipLaunchKernelGGL(partition_scatter_kernel, dim3(B * T), dim3(PT), 0, st, labels, label_kind, x, C, N, T, first_label, L, hist,
                       counts, offset, xyz, src);
    FSG_CHECK_LAUNCH("fsg_label_partition/scatter");
    return FSG_OK;
}

extern "C" int fsg_segment_jitter_extend_f32(const float *xyz, const int32_t *offset, const float *nn_d2, const int32_t *new_offset,
                                             const int32_t *src_idx, const float *direction, const float *z, int G, int n, int n_new,
                                             float *out, float *stats, fsg_stream_t stream) {
    FSG_REQUIRE(xyz && offset && nn_d2 && new_offset && out && stats, "fsg_segment_jitter_extend_f32: NULL pointer");
    FSG_REQUIRE(G > 0 && n > 0 && n_new >= n, "fsg_segment_jitter_extend_f32: bad shape G=%d n=%d n_new=%d", G, n, n_new);
    FSG_REQUIRE(n_new == n || (src_idx && direction && z), "fsg_segment_jitter_extend_f32: %d padded rows without draws", n_new - n);
    hipLaunchKernelGGL(jitter_extend_kernel, dim3(G), dim3(JT), 0, (hipStream_t)stream, xyz, offset, nn_d2, new_offset, src_idx,
                       direction, z, out, stats);
    FSG_CHECK_LAUNCH("fsg_segment_jitter_extend_f32");
    return FSG_OK;
}

extern "C" int fsg_fps_start_f32(const float *xyz, const int32_t *offset, const int32_t *new_offset, const int32_t *start, int b, int n,
                                 float *tmp, int32_t *idx, fsg_stream_t stream) {
    FSG_REQUIRE(xyz && offset && new_offset && tmp && idx, "fsg_fps_start_f32: NULL pointer");
    FSG_REQUIRE(b > 0 && n > 0, "fsg_fps_start_f32: bad shape b=%d n=%d", b, n);
    hipLaunchKernelGGL(fps_start_kernel, dim3(b), dim3(FT), 0, (hipStream_t)stream, xyz, offset, new_offset, start, tmp, idx);
    FSG_CHECK_LAUNCH("fsg_fps_start_f32");
    return FSG_OK;
}
