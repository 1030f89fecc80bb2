// OPTICS reachability ordering on 3-D points (Ankerst, Breunig, Kriegel, Sander, "OPTICS: Ordering Points To Identify the
// Clustering Structure", SIGMOD 1999), batched and bit-reproducible -- include/fsg_hip.h: fsg_optics_f32.
//
// The reference pools the registered clouds of all instances of one object and runs sklearn.cluster.OPTICS on the CPU, one
// object at a time (shape_model/generate_corresponding_points.py:50-62); sklearn's loop is O(n^2) in Python.  Here B items of n
// points run together and nothing is read on the host.
//
// The rule (ours; restated bit for bit in tests/optics_oracle.py):
//   pair     d2(i, j) = ((dx dx + dy dy) + dz dz) in fp64 in that order (the build has -ffp-contract=off), dx = (double) x_i -
//            (double) x_j: symmetric bit for bit.  e2 = eps eps (the fp64 product; inf stays inf).  N(i) = { j : d2 <= e2 }, i
//            included.
//   core2    of i: the k-th smallest d2(i, j) over N(i), multiplicities counted, i itself the first with 0; +inf if |N(i)| < k.
//   order    reach2 = +inf, pred = -1, nobody processed.  n times: p = the unprocessed point with the smallest (reach2, index),
//            the LOWEST index on ties, +inf included; p is processed and appended; if core2(p) < inf, every unprocessed q in
//            N(p) with v = max(core2(p), d2(p, q)) < reach2(q) gets reach2(q) = v, pred(q) = p.
//   The squares go out; no square root is taken here.  Not sklearn's: no np.around(.., 15), comparisons on squares.
//
// A cell grid restricts which pairs are LOOKED AT; the exact d2 <= e2 decides, so no result depends on the grid.  Per axis the
// side is max(eps (1 + 2^-20), extent / kG): two points within eps are at most one cell apart (|dx| <= eps (1 + 2^-52) follows
// from d2 <= e2 because the rounded sums are monotone; the quotient (x - lo) / side carries a relative error of 2^-51 at values
// of at most 21, far below the 2^-20 slack).  eps = inf is one cell.  Every cell index is clamped into the grid.
//
// Launches (workspace: the item's grid, cell start table, then per SLOT -- position in cell order -- float4 (x, y, z, original
// index), core2, reach2, pred and two index buffers of the sort):
//   cells    one workgroup of 512 per item: bounding box (min / max are exact, any order), the grid, a STABLE sort of the points
//            by cell as three counting-sort passes (x, y, z digit, at most kG = 21 values): thread t owns a contiguous run of
//            points and a column of the (digit, thread) histogram in LDS, one workgroup prefix sum turns it into offsets.  No
//            atomics: slot order inside a cell is ascending original index.
//   core     one lane per slot: at most k passes over the 27 cells around the point, each taking the smallest d2 above the last
//            one and how often it occurs, until k are counted.  No list is kept: a few registers whatever k is.  k passes of
//            |27 cells| pairs: with eps = inf that is k n^2 pair evaluations per item.
//   order    one workgroup of 1024 per item.  LDS: per block of 64 consecutive slots the best (key, tag) of its unprocessed
//            slots, key = ~bits(reach2) (reach2 >= 0: the bit pattern orders like the value; 0 = nobody left), tag =
//            (2^32 - 1 - original index) << 32 | slot, so that the maximum of (key, tag) is the arg-min with ties to the lowest
//            ORIGINAL index; and the cell start table.  A step: every thread takes the best of its blocks, the DPP wave maximum,
//            one LDS slot per wave (double-buffered), a barrier, the maximum over the slots -> p.  Then the blocks that the 27
//            cells around p overlap are dealt to the waves, one wave a block: a lane tests and updates its slot, the wave
//            re-reduces the block into the table.  A block has one owner in a step, so no update races.  A barrier.  The
//            processed flag of a slot is the sign bit of its reach2 in the workspace (cleared on the way out).
// No atomics, no scratch; the loop count is n whatever the data.
#include <math.h>

#include "fsg_common.h"

namespace {

constexpr int kG = 21;                      // cells per axis at most: the reference's eps = 5 % of the range gives 21
constexpr int kCells = kG * kG * kG;
constexpr int kCellsPad = 9264;             // entries of the start table: kCells + 1, rounded up to 16 bytes
constexpr int kMaxN = FSG_OPTICS_MAX_POINTS;
constexpr int kMaxK = FSG_OPTICS_MAX_MIN_SAMPLES;
constexpr int kSortThreads = 512;           // 21 x 512 histogram words are 42 KiB of LDS
constexpr int kCoreThreads = 256;
constexpr int kOrdThreads = 1024;
constexpr int kOrdWaves = kOrdThreads / 64;
constexpr size_t kOrdLdsFixed = (size_t)kCellsPad * 4 + 4 * kOrdWaves * 8;   // start table + double-buffered wave slots
static_assert(kCells + 1 <= kCellsPad && kCellsPad % 4 == 0, "start table");
static_assert((size_t)(kMaxN / 64) * 16 + kOrdLdsFixed <= FSG_LDS_WHOLE_CU, "LDS budget of the ordering kernel");
static_assert(kMaxN % 64 == 0 && kMaxN / kSortThreads <= 65535, "cap");

struct Grid {
    double lo[3], side[3];
    int g[3], ncells;
};
static_assert(sizeof(Grid) == 64, "Grid layout");

__host__ __device__ inline size_t item_bytes(int n) {
    return sizeof(Grid) + (size_t)kCellsPad * 4 + (((size_t)n * 44 + 15) & ~(size_t)15);
}

struct Item {
    Grid *grid;
    int *cell_start;    // (ncells + 1) first slot of every cell, n at the end
    float4 *pts;        // (n) by slot: x, y, z, the bits of the original index
    double *core2;      // (n) by slot
    double *reach2;     // (n) by slot; sign bit = processed
    int *pred;          // (n) by slot: ORIGINAL index of the predecessor
    int *tmp_a, *tmp_b; // (n) each: the index permutation between the passes of the sort
};
__device__ __forceinline__ Item view(char *ws, int b, int n) {
    char *base = ws + (size_t)b * item_bytes(n);
    Item it;
    it.grid = (Grid *)base;
    it.cell_start = (int *)(base + sizeof(Grid));
    it.pts = (float4 *)(base + sizeof(Grid) + (size_t)kCellsPad * 4);
    it.core2 = (double *)(it.pts + n);
    it.reach2 = it.core2 + n;
    it.pred = (int *)(it.reach2 + n);
    it.tmp_a = it.pred + n;
    it.tmp_b = it.tmp_a + n;
    return it;
}

__device__ __forceinline__ double sqdist64(float ax, float ay, float az, float bx, float by, float bz) {
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// cell coordinate on one axis, clamped into the grid (a NaN quotient is cell 0)
__device__ __forceinline__ int cell_axis(double lo, double side, int g, float x) {
    const double q = fmin(fmax(((double)x - lo) / side, 0.0), (double)kG);
    return clampi((int)q, g - 1);
}

// ------------------------------------------------------------------------------------------------------------- cells
__global__ __launch_bounds__(kSortThreads) void optics_cells_kernel(const float *__restrict__ points,
                                                                    const double *__restrict__ max_eps, int n, char *ws) {
    constexpr int T = kSortThreads;
    __shared__ int hist[kG * T];
    __shared__ int red[T / 64];
    __shared__ Grid sg;
    const int b = blockIdx.x, t = threadIdx.x;
    const float *p = points + (size_t)b * n * 3;
    const Item it = view(ws, b, n);

    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = t; i < n; i += T) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = p[3 * (size_t)i + a];
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
    }
    float *redf = (float *)hist;   // 6 T floats
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        redf[a * T + t] = mn[a];
        redf[(3 + a) * T + t] = mx[a];
    }
    __syncthreads();
    for (int step = T / 2; step > 0; step >>= 1) {
        if (t < step) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                redf[a * T + t] = fminf(redf[a * T + t], redf[a * T + t + step]);
                redf[(3 + a) * T + t] = fmaxf(redf[(3 + a) * T + t], redf[(3 + a) * T + t + step]);
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const double eps = max_eps[b];
        int cells = 1;
        for (int a = 0; a < 3; ++a) {
            const double lo = (double)redf[a * T], extent = (double)redf[(3 + a) * T] - lo;
            const double side = fmax(eps * (1.0 + 0x1p-20), extent / (double)kG);
            sg.lo[a] = lo;
            sg.side[a] = side;
            sg.g[a] = (int)fmin(fmax(floor(extent / side), 0.0), (double)(kG - 1)) + 1;
            cells *= sg.g[a];
        }
        sg.ncells = cells;
        *it.grid = sg;
    }
    __syncthreads();

    // stable counting sort by the cell coordinate of one axis per pass, x first: the final order is (z, y, x) cell order
    const int chunk = (n + T - 1) / T;
    const int j0 = min(n, t * chunk), j1 = min(n, j0 + chunk);
    for (int pass = 0; pass < 3; ++pass) {
        const int *src = pass == 0 ? nullptr : (pass == 1 ? it.tmp_a : it.tmp_b);
        int *dst = pass == 1 ? it.tmp_b : it.tmp_a;
        const double lo = sg.lo[pass], side = sg.side[pass];
        const int g = sg.g[pass];
        for (int d = 0; d < kG; ++d) hist[d * T + t] = 0;
        for (int j = j0; j < j1; ++j) {
            const int i = src ? src[j] : j;
            hist[cell_axis(lo, side, g, p[3 * (size_t)i + pass]) * T + t] += 1;
        }
        __syncthreads();
        int sum = 0;   // the flattened (digit, thread) table in runs of kG: thread t scans entries t kG .. t kG + kG - 1
        for (int e = 0; e < kG; ++e) sum += hist[t * kG + e];
        int total;
        int base = block_excl_scan<T>(sum, red, total);
        for (int e = 0; e < kG; ++e) {
            const int c = hist[t * kG + e];
            hist[t * kG + e] = base;
            base += c;
        }
        __syncthreads();
        for (int j = j0; j < j1; ++j) {
            const int i = src ? src[j] : j;
            const int d = cell_axis(lo, side, g, p[3 * (size_t)i + pass]);
            const int at = hist[d * T + t];
            hist[d * T + t] = at + 1;
            dst[at] = i;
        }
        __syncthreads();
    }

    const int gx = sg.g[0], gy = sg.g[1];
    auto cell_of = [&](int i) {
        const float *q = p + 3 * (size_t)i;
        const int cx = cell_axis(sg.lo[0], sg.side[0], sg.g[0], q[0]);
        const int cy = cell_axis(sg.lo[1], sg.side[1], sg.g[1], q[1]);
        const int cz = cell_axis(sg.lo[2], sg.side[2], sg.g[2], q[2]);
        return (cz * gy + cy) * gx + cx;
    };
    for (int s = t; s < n; s += T) {
        const int i = it.tmp_a[s];
        const float *q = p + 3 * (size_t)i;
        it.pts[s] = make_float4(q[0], q[1], q[2], __int_as_float(i));
        const int c = cell_of(i), cprev = s > 0 ? cell_of(it.tmp_a[s - 1]) : -1;
        for (int cc = cprev + 1; cc <= c; ++cc) it.cell_start[cc] = s;   // every entry has one writer
        if (s == n - 1)
            for (int cc = c + 1; cc <= sg.ncells; ++cc) it.cell_start[cc] = n;
    }
}

// the slot ranges of the 27 cells around a point: for every (z, y) row the three x cells are consecutive slots
struct Around {
    int z0, z1, y0, y1, x0, x1, gx, gy;
    __device__ __forceinline__ Around(const Grid &g, float x, float y, float z) {
        const int cx = cell_axis(g.lo[0], g.side[0], g.g[0], x), cy = cell_axis(g.lo[1], g.side[1], g.g[1], y);
        const int cz = cell_axis(g.lo[2], g.side[2], g.g[2], z);
        gx = g.g[0];
        gy = g.g[1];
        x0 = max(cx - 1, 0), x1 = min(cx + 1, g.g[0] - 1);
        y0 = max(cy - 1, 0), y1 = min(cy + 1, g.g[1] - 1);
        z0 = max(cz - 1, 0), z1 = min(cz + 1, g.g[2] - 1);
    }
};

// -------------------------------------------------------------------------------------------------------------- core
__global__ __launch_bounds__(kCoreThreads) void optics_core_kernel(const double *__restrict__ max_eps, int n, int k, char *ws,
                                                                   double *__restrict__ core2_out) {
    const int b = blockIdx.y, s = blockIdx.x * kCoreThreads + threadIdx.x;
    if (s >= n) return;
    const Item it = view(ws, b, n);
    const Grid g = *it.grid;
    const double eps = max_eps[b], e2 = eps * eps;
    const float4 me = it.pts[s];
    const Around ar(g, me.x, me.y, me.z);
    double last = -1.0, core = INFINITY;
    int have = 0;
    for (int pass = 0; pass < k; ++pass) {   // the smallest d2 above `last` and how often it occurs
        double m = INFINITY;
        int cnt = 0;
        for (int zz = ar.z0; zz <= ar.z1; ++zz) {
            for (int yy = ar.y0; yy <= ar.y1; ++yy) {
                const int row = (zz * ar.gy + yy) * ar.gx;
                const int q0 = it.cell_start[row + ar.x0], q1 = it.cell_start[row + ar.x1 + 1];
                for (int q = q0; q < q1; ++q) {
                    const float4 o = it.pts[q];
                    const double d2 = sqdist64(me.x, me.y, me.z, o.x, o.y, o.z);
                    if (d2 <= e2 && d2 > last) {
                        if (d2 < m) {
                            m = d2;
                            cnt = 1;
                        } else if (d2 == m) {
                            cnt += 1;
                        }
                    }
                }
            }
        }
        if (cnt == 0) break;   // fewer than k neighbours
        have += cnt;
        if (have >= k) {
            core = m;
            break;
        }
        last = m;
    }
    it.core2[s] = core;
    core2_out[(size_t)b * n + __float_as_int(me.w)] = core;
}

// ------------------------------------------------------------------------------------------------------------- order
// the best (key, tag) over the 64 lanes, to every lane: the largest key, among equal keys the largest tag
__device__ __forceinline__ void wave_best(u64 &key, u64 &tag) {
    const u64 k = wave_max_u64_bcast(key);
    tag = wave_max_u64_bcast(key == k ? tag : 0);
    key = k;
}

__global__ __launch_bounds__(kOrdThreads) void optics_order_kernel(const double *__restrict__ max_eps, int n, char *ws,
                                                                   int32_t *__restrict__ ordering, double *__restrict__ reach2_out,
                                                                   int32_t *__restrict__ pred_out) {
    extern __shared__ __align__(16) char smem[];
    const int nblk = (n + 63) >> 6;
    u64 *wkey = (u64 *)smem;                  // 2 x kOrdWaves
    u64 *wtag = wkey + 2 * kOrdWaves;         // 2 x kOrdWaves
    int *cstart = (int *)(wtag + 2 * kOrdWaves);
    u64 *bkey = (u64 *)(cstart + kCellsPad);  // nblk
    u64 *btag = bkey + nblk;                  // nblk
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Item it = view(ws, b, n);
    const Grid g = *it.grid;
    const double eps = max_eps[b], e2 = eps * eps;
    const float4 *pts = it.pts;
    const double *core2 = it.core2;
    double *reach2 = it.reach2;
    int *pred = it.pred;
    constexpr u64 kSign = (u64)1 << 63;

    // one wave, one block of 64 slots.  INIT: reach2 = inf, pred = -1.  Otherwise: slot ps becomes processed, and with `upd`
    // the unprocessed slots within eps of P take v = max(core_p, d2) if that lowers their reach2.  Then the block's best.
    auto process = [&](int blk, bool init, int ps, int pi, bool upd, float4 P, double core_p) {
        const int s = blk * 64 + lane;
        u64 key = 0, tag = 0;
        if (s < n) {
            const float4 o = pts[s];
            u64 bits;
            if (init) {
                bits = (u64)__double_as_longlong(INFINITY);
                reach2[s] = INFINITY;
                pred[s] = -1;
            } else {
                bits = (u64)__double_as_longlong(reach2[s]);
                if (s == ps) {
                    bits |= kSign;
                    reach2[s] = __longlong_as_double((long long)bits);
                } else if (upd && !(bits >> 63)) {
                    const double d2 = sqdist64(P.x, P.y, P.z, o.x, o.y, o.z);
                    if (d2 <= e2) {
                        const double v = fmax(core_p, d2);
                        if (v < __longlong_as_double((long long)bits)) {
                            bits = (u64)__double_as_longlong(v);
                            reach2[s] = v;
                            pred[s] = pi;
                        }
                    }
                }
            }
            if (!(bits >> 63)) {
                key = ~bits;
                tag = ((u64)(0xFFFFFFFFu - (unsigned)__float_as_int(o.w)) << 32) | (unsigned)s;
            }
        }
        wave_best(key, tag);
        if (lane == 0) {
            bkey[blk] = key;
            btag[blk] = tag;
        }
    };

    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int blk = wave; blk < nblk; blk += kOrdWaves) process(blk, true, -1, -1, false, none, 0.0);
    for (int c = tid; c <= g.ncells; c += kOrdThreads) cstart[c] = it.cell_start[c];
    __syncthreads();

    for (int step = 0; step < n; ++step) {
        u64 key = 0, tag = 0;
        for (int blk = tid; blk < nblk; blk += kOrdThreads) {
            const u64 k2 = bkey[blk], t2 = btag[blk];
            if (k2 > key || (k2 == key && t2 > tag)) {
                key = k2;
                tag = t2;
            }
        }
        wave_best(key, tag);
        const int buf = (step & 1) * kOrdWaves;
        if (lane == 0) {
            wkey[buf + wave] = key;
            wtag[buf + wave] = tag;
        }
        __syncthreads();
        key = lane < kOrdWaves ? wkey[buf + lane] : 0;
        tag = lane < kOrdWaves ? wtag[buf + lane] : 0;
        wave_best(key, tag);
        const int ps = (int)(unsigned)(tag & 0xFFFFFFFFu);
        const int pi = (int)(0xFFFFFFFFu - (unsigned)(tag >> 32));
        if (tid == 0) ordering[(size_t)b * n + step] = pi;
        if (step == n - 1) break;

        const float4 P = pts[ps];
        const double core_p = core2[ps];
        if (core_p < INFINITY) {
            // the blocks the 27 cells overlap, each once, dealt round-robin to the waves (the rows ascend in slot order)
            const Around ar(g, P.x, P.y, P.z);
            int next_free = 0, li = 0;
            for (int zz = ar.z0; zz <= ar.z1; ++zz) {
                for (int yy = ar.y0; yy <= ar.y1; ++yy) {
                    const int row = (zz * ar.gy + yy) * ar.gx;
                    const int q0 = cstart[row + ar.x0], q1 = cstart[row + ar.x1 + 1];
                    if (q0 >= q1) continue;
                    const int b0 = max(q0 >> 6, next_free), b1 = (q1 - 1) >> 6;
                    if (b0 > b1) continue;
                    for (int blk = b0 + ((wave - li) & (kOrdWaves - 1)); blk <= b1; blk += kOrdWaves)
                        process(blk, false, ps, pi, true, P, core_p);
                    li += b1 - b0 + 1;
                    next_free = b1 + 1;
                }
            }
        } else if (wave == 0) {
            process(ps >> 6, false, ps, pi, false, P, core_p);
        }
        __syncthreads();
    }

    __syncthreads();
    for (int s = tid; s < n; s += kOrdThreads) {
        const size_t at = (size_t)b * n + __float_as_int(pts[s].w);
        reach2_out[at] = __longlong_as_double(__double_as_longlong(reach2[s]) & (long long)~kSign);
        pred_out[at] = pred[s];
    }
}

}  // namespace

extern "C" size_t fsg_optics_workspace_bytes(int B, int n, int k) {
    (void)k;
    if (B <= 0 || n <= 0) return 0;
    return (size_t)B * item_bytes(n);
}

extern "C" int fsg_optics_f32(const float *points, const double *max_eps, int B, int n, int k, int32_t *ordering, double *core2,
                              double *reach2, int32_t *pred, void *workspace, size_t workspace_bytes, fsg_stream_t stream) {
    const char *who = "fsg_optics_f32";
    FSG_REQUIRE(B >= 0 && B <= 65535 && n >= 2 && n <= kMaxN && k >= 2 && k <= kMaxK && k <= n,
                "%s: bad shape B=%d n=%d min_samples=%d (2 <= min_samples <= min(n, %d), n <= %d, B <= 65535)", who, B, n, k, kMaxK,
                kMaxN);
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(points && max_eps && ordering && core2 && reach2 && pred, "%s: NULL pointer", who);
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: workspace must be non-NULL and 16-byte aligned", who);
    FSG_REQUIRE(workspace_bytes >= fsg_optics_workspace_bytes(B, n, k), "%s: workspace of %zu bytes, %zu needed", who,
                workspace_bytes, fsg_optics_workspace_bytes(B, n, k));
    const size_t lds = kOrdLdsFixed + (size_t)fsg_cdiv(n, 64) * 16;
    FSG_GRANT_LDS(who, optics_order_kernel, lds);
    hipLaunchKernelGGL(optics_cells_kernel, dim3(B), dim3(kSortThreads), 0, (hipStream_t)stream, points, max_eps, n,
                       (char *)workspace);
    FSG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(optics_core_kernel, dim3(fsg_cdiv(n, kCoreThreads), B), dim3(kCoreThreads), 0, (hipStream_t)stream, max_eps,
                       n, k, (char *)workspace, core2);
    FSG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(optics_order_kernel, dim3(B), dim3(kOrdThreads), lds, (hipStream_t)stream, max_eps, n, (char *)workspace,
                       ordering, reach2, pred);
    FSG_CHECK_LAUNCH(who);
    return FSG_OK;
}
