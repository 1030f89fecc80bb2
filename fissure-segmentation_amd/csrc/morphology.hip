// 3-D binary morphology with ball structuring elements, connected components and component statistics on bit planes --
// include/fsg_hip.h: fsg_bits_pack_u8, fsg_bits_unpack_u8, fsg_bits_window, fsg_ball_dilate_bits, fsg_cc_workspace_bytes,
// fsg_cc_label_bits, fsg_component_stats_i32, fsg_relabel_lut_i32.
// Replaces the SimpleITK filters of find_lobes (data_processing/find_lobes.py:114-158: BinaryErode, BinaryDilate,
// BinaryMorphologicalClosing / Opening, ConnectedComponentImageFilter, RelabelComponentImageFilter,
// LabelShapeStatisticsImageFilter) and of multiple_objects_morphology (utils/image_ops.py:31-47).
//
// Bit planes.  A binary volume (B, D, H, W) is held as (B, D, H, WW) 64-bit words, WW = ceil(W / 64): bit i of word j of a
// row is voxel x = 64 j + i.  The bits past W in the last word of a row are ALWAYS 0: every kernel that writes a plane masks
// them, every kernel that reads one may rely on it.
//
// Ball dilation.  The structuring element is { o : sum_i (o_i / (r_i + 0.5))^2 <= 1 }, r_i in 0..8 per axis, decided in
// integers (4 sum_i o_i^2 prod_{j != i} m_j^2 <= prod_j m_j^2 with m = 2 r + 1; the two sides have different parity, so the
// boundary is never met).  For each (dz, dy) of the ball the x extent is a half-width h(dz, dy), so
//   out(z, y) = OR over (dz, dy) of D_h(dz,dy)( in(z + dz, y + dy) ),   D_h = the run-dilation of a row by h voxels.
// D_h distributes over OR and D_h = D_1 D_(h-1), so a thread that owns one output word ORs the rows of each half-width
// class into a running word and widens it by one voxel between classes, the widest class first (Horner):
//   acc = A_rx;  for h = rx - 1 .. 0: acc = D_1(acc) | A_h,        A_h = OR of the rows whose half-width is exactly h.
// That is one LDS read of three words per (dz, dy) -- 69 for the radius-4 ball of 389 voxels -- and rx widenings of a few
// shifts, not a tap per voxel of the ball.  The running word travels with its two neighbour words (l, c, r); only the 8 bits
// of each that face c can reach c in at most 8 widenings, and what c would hand to a neighbour and get back it already holds,
// so the neighbours are widened on their own.  The rows of a tile (with their halo of rz slabs, ry rows, one word) are
// staged in LDS once; a row or word outside the volume reads as the border value, as do the bits past W.
// inv_in / inv_out complement the input on the way into LDS and the result on the way out: erosion with border b is
// inv_in = inv_out = 1 with border !b (the ball is symmetric), and a chain keeps its NOTs inside the launches.
//
// Connected components: union-find by minimum linear index (Playne & Hawick style).  parent[v] <= v always, parents only
// ever decrease, a root is a voxel with parent[v] == v, and a union hangs the larger root under the smaller, so the root of
// a finished component is its first voxel in raster order whatever order the atomics land in.  Launches:
//   local    tile 4 x 4 x 64 voxels in LDS: union with the backward neighbours inside the tile, flatten, write parents as
//            volume indices (-1: background)
//   merge    every voxel with a backward neighbour in another tile: union on global memory with atomicMin
//   flatten  root[v] = find(v) into the label array, and the number of roots in each chunk of 1024 voxels
//   scan     one workgroup per item: exclusive sums of the chunk counts, n
//   number   roots get 1 + their rank in raster order (into parent[root])
//   final    label[v] = parent[root[v]], background 0
// No workgroup waits on another; every loop of find and union is bounded because the indices it follows strictly decrease.
#include "fsg_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXR = FSG_MORPH_MAX_RADIUS;
constexpr int MAX_TAPS = (2 * MAXR + 1) * (2 * MAXR + 1);
constexpr int MAX_BLOCKS = 4096;   // grid-strided launches

struct Dims {
    int B, D, H, W, WW;
    long V;      // voxels of one item
    long rows;   // B D H
};

int check_dims(const char *name, int B, int D, int H, int W, Dims &d) {
    FSG_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535, "%s: bad shape B=%d D=%d H=%d W=%d", name, B, D, H, W);
    FSG_REQUIRE((long)B * D * H * W < (1L << 31), "%s: B D H W = %d %d %d %d exceeds 2^31 voxels", name, B, D, H, W);
    d.B = B; d.D = D; d.H = H; d.W = W;
    d.WW = (W + 63) / 64;
    d.V = (long)D * H * W;
    d.rows = (long)B * D * H;
    return FSG_OK;
}

inline int grid_for(long items, int per_block) {
    const long n = (items + per_block - 1) / per_block;
    return (int)(n < 1 ? 1 : (n > MAX_BLOCKS ? MAX_BLOCKS : n));
}

// the bits of the last word of a row that are voxels
__device__ __forceinline__ u64 tail_mask(int W, int WW, int j) {
    const int rem = W & 63;
    return (j == WW - 1 && rem) ? ((1ull << rem) - 1ull) : ~0ull;
}

// ------------------------------------------------------------------------------------------------ pack / unpack / window
// a wave per word: 64 bytes -> one ballot.  value < 0: voxel != 0, otherwise voxel == value
__global__ __launch_bounds__(NT) void pack_kernel(Dims d, const uint8_t *__restrict__ src, int value, u64 *__restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const long nwords = d.rows * d.WW, nwaves = (long)gridDim.x * (NT / 64);
    for (long w = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); w < nwords; w += nwaves) {   // (uniform over the wave)
        const long row = w / d.WW;
        const int j = (int)(w - row * d.WW), x = j * 64 + lane;
        bool on = false;
        if (x < d.W) {
            const uint8_t v = src[row * d.W + x];
            on = value < 0 ? v != 0 : v == (uint8_t)value;
        }
        const u64 word = __ballot(on);
        if (lane == 0) bits[w] = word;
    }
}

__global__ __launch_bounds__(NT) void unpack_kernel(Dims d, const u64 *__restrict__ bits, uint8_t *__restrict__ out) {
    const long n = d.rows * d.W;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long row = i / d.W;
        const int x = (int)(i - row * d.W);
        out[i] = (uint8_t)((bits[row * d.WW + (x >> 6)] >> (x & 63)) & 1ull);
    }
}

// out(z, y, x) = in(z + oz, y + oy, x + ox) where that lies inside `in`, 0 elsewhere: pads (negative offsets) and crops
__global__ __launch_bounds__(NT) void window_kernel(Dims di, Dims dout, int oz, int oy, int ox, const u64 *__restrict__ in,
                                                    u64 *__restrict__ out) {
    const long n = dout.rows * dout.WW;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const int j = (int)(i % dout.WW);
        long t = i / dout.WW;
        const int y = (int)(t % dout.H);
        t /= dout.H;
        const int z = (int)(t % dout.D), b = (int)(t / dout.D);
        const int zi = z + oz, yi = y + oy;
        u64 v = 0;
        if (zi >= 0 && zi < di.D && yi >= 0 && yi < di.H) {
            const u64 *row = in + (((long)b * di.D + zi) * di.H + yi) * di.WW;
            const int s = j * 64 + ox;                       // the source voxel of bit 0 (may be negative)
            const int q = s >> 6, sh = s & 63;               // (arithmetic shift: floor)
            const u64 lo = (q >= 0 && q < di.WW) ? row[q] : 0ull;
            const u64 hi = (q + 1 >= 0 && q + 1 < di.WW) ? row[q + 1] : 0ull;
            v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;    // (the source's bits past its W are 0)
        }
        out[i] = v & tail_mask(dout.W, dout.WW, j);
    }
}

// ------------------------------------------------------------------------------------------------------- ball dilation
// the (dz, dy) of the ball grouped by half-width: class h is taps[start[h]] .. taps[start[h + 1]] - 1
struct Taps {
    short start[MAXR + 2];
    signed char dz[MAX_TAPS], dy[MAX_TAPS];
};

struct Tile {
    int TZ, TY, XW;     // output rows and words of a workgroup: TZ * TY * XW <= NT
    int SZ, SY, SX;     // staged: TZ + 2 rz, TY + 2 ry, XW + 2
    int tiles_x;        // word chunks per row
};

__device__ __forceinline__ void widen1(u64 &l, u64 &c, u64 &r) {
    const u64 nc = c | (c << 1) | (c >> 1) | (l >> 63) | (r << 63);
    l = l | (l << 1) | (l >> 1);
    r = r | (r << 1) | (r >> 1);
    c = nc;
}

__global__ __launch_bounds__(NT) void dilate_kernel(Dims d, Tile t, Taps taps, int rz, int ry, int rx, int border, int inv_in,
                                                    int inv_out, const u64 *__restrict__ in, u64 *__restrict__ out) {
    extern __shared__ u64 stage[];   // [SZ][SY][SX]
    const int b = blockIdx.z;
    const int j0 = (blockIdx.x % t.tiles_x) * t.XW, y0 = (blockIdx.x / t.tiles_x) * t.TY, z0 = blockIdx.y * t.TZ;
    const u64 fill = border ? ~0ull : 0ull, flip = inv_in ? ~0ull : 0ull;
    const u64 *vol = in + (long)b * d.D * d.H * d.WW;
    const int S = t.SZ * t.SY * t.SX;
    for (int i = threadIdx.x; i < S; i += NT) {
        const int sj = i % t.SX, sy = (i / t.SX) % t.SY, sz = i / (t.SX * t.SY);
        const int z = z0 - rz + sz, y = y0 - ry + sy, j = j0 - 1 + sj;
        u64 v = fill;
        if (z >= 0 && z < d.D && y >= 0 && y < d.H && j >= 0 && j < d.WW) {
            const u64 m = tail_mask(d.W, d.WW, j);
            v = ((vol[((long)z * d.H + y) * d.WW + j] ^ flip) & m) | (fill & ~m);   // the bits past W read as the border
        }
        stage[i] = v;
    }
    __syncthreads();
    const int tj = threadIdx.x % t.XW, ty = (threadIdx.x / t.XW) % t.TY, tz = threadIdx.x / (t.XW * t.TY);
    const int z = z0 + tz, y = y0 + ty, j = j0 + tj;
    if (tz >= t.TZ || z >= d.D || y >= d.H || j >= d.WW) return;
    const u64 *centre = stage + ((tz + rz) * t.SY + (ty + ry)) * t.SX + tj + 1;
    u64 l = 0, c = 0, r = 0;
    for (int h = rx; h >= 0; --h) {
        if (h < rx) widen1(l, c, r);
        for (int k = taps.start[h]; k < taps.start[h + 1]; ++k) {   // (uniform bounds, scalar loads of the tap table)
            const u64 *p = centre + ((int)taps.dz[k] * t.SY + (int)taps.dy[k]) * t.SX;
            l |= p[-1];
            c |= p[0];
            r |= p[1];
        }
    }
    if (inv_out) c = ~c;
    out[(((long)b * d.D + z) * d.H + y) * d.WW + j] = c & tail_mask(d.W, d.WW, j);
}

// half-width of the ball's row at (dz, dy), -1 if the row is empty; all in integers (see the head of the file)
int half_width(int dz, int dy, int rz, int ry, int rx) {
    const long mz = 2 * rz + 1, my = 2 * ry + 1, mx = 2 * rx + 1;
    const long full = mz * mz * my * my * mx * mx;
    int h = -1;
    for (int dx = 0; dx <= rx; ++dx) {
        const long s = 4 * ((long)dz * dz * my * my * mx * mx + (long)dy * dy * mz * mz * mx * mx + (long)dx * dx * mz * mz * my * my);
        if (s <= full) h = dx;
    }
    return h;
}

// ------------------------------------------------------------------------------------------------ connected components
constexpr int CT_Z = 4, CT_Y = 4, CT_X = 64;            // the tile of the local pass: one word wide
constexpr int CT_N = CT_Z * CT_Y * CT_X;
constexpr int CHUNK = 1024;                              // voxels per workgroup of the numbering passes (4 per thread)

// is (dz, dy, dx) a backward neighbour (earlier in raster order) of the connectivity with at most maxd non-zero axes?
__device__ __forceinline__ bool backward(int dz, int dy, int dx, int maxd) {
    if (dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0)))) return false;
    return (dz != 0) + (dy != 0) + (dx != 0) <= maxd;
}

// LDS: follow parents to the root.  lab[a] <= a and a step is taken only while lab[a] != a, so a strictly decreases: at most
// CT_N steps.  A value read while another lane lowers it is an older parent: still an ancestor of the same set.
__device__ __forceinline__ int lds_find(volatile int *lab, int a) {
    int p = lab[a];
    while (p != a) {
        a = p;
        p = lab[a];
    }
    return a;
}

// LDS: unite the sets of a and b.  Every pass either returns or replaces the larger of the two roots by a strictly smaller
// index (the value atomicMin found there), both stay >= 0: at most a + b passes.  When atomicMin finds hi already hung
// under `old`, hi now points at min(old, lo) and the pass goes on to unite old with lo, so no link is lost.
__device__ __forceinline__ void lds_union(int *lab, int a, int b) {
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(&lab[hi], lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

__device__ __forceinline__ int g_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// global memory: the same two loops on agent-scope accesses.  parent[a] <= a, steps strictly decrease: at most a steps.  A
// stale parent is an older ancestor; the atomicMin of the union is what decides.
__device__ __forceinline__ int g_find(int *parent, int a) {
    int p = g_load(parent + a);
    while (p != a) {
        a = p;
        p = g_load(parent + a);
    }
    return a;
}

// at most a + b passes (see lds_union); no pass waits for another workgroup
__device__ __forceinline__ void g_union(int *parent, int a, int b) {
    for (;;) {
        a = g_find(parent, a);
        b = g_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

__global__ __launch_bounds__(NT) void cc_local_kernel(Dims d, int tiles_x, int maxd, const u64 *__restrict__ bits,
                                                      int *__restrict__ parent) {
    __shared__ int lab[CT_N];
    const int b = blockIdx.z;
    const int tx = blockIdx.x % tiles_x, x0 = tx * CT_X, y0 = (blockIdx.x / tiles_x) * CT_Y, z0 = blockIdx.y * CT_Z;
    const int lx = threadIdx.x & 63;
    bits += (long)b * d.D * d.H * d.WW;
    parent += (long)b * d.V;
#pragma unroll
    for (int k = 0; k < CT_N / NT; ++k) {
        const int row = (threadIdx.x >> 6) + k * (NT / 64), lz = row / CT_Y, ly = row % CT_Y;
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        const bool fg = z < d.D && y < d.H && x < d.W && ((bits[((long)z * d.H + y) * d.WW + tx] >> lx) & 1ull);
        lab[row * CT_X + lx] = fg ? row * CT_X + lx : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CT_N / NT; ++k) {
        const int row = (threadIdx.x >> 6) + k * (NT / 64), lz = row / CT_Y, ly = row % CT_Y, i = row * CT_X + lx;
        if (((volatile int *)lab)[i] < 0) continue;
        for (int dz = -1; dz <= 0; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!backward(dz, dy, dx, maxd)) continue;
                    const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
                    if (nz < 0 || ny < 0 || ny >= CT_Y || nx < 0 || nx >= CT_X) continue;
                    const int jn = (nz * CT_Y + ny) * CT_X + nx;
                    if (((volatile int *)lab)[jn] >= 0) lds_union(lab, i, jn);
                }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CT_N / NT; ++k) {
        const int row = (threadIdx.x >> 6) + k * (NT / 64), lz = row / CT_Y, ly = row % CT_Y, i = row * CT_X + lx;
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        if (z >= d.D || y >= d.H || x >= d.W) continue;
        int p = -1;
        if (lab[i] >= 0) {   // the order of a tile's voxels is the raster order of the volume: the tile root is its first voxel
            const int rt = lds_find(lab, i), rrow = rt / CT_X;
            p = (int)(((long)(z0 + rrow / CT_Y) * d.H + (y0 + rrow % CT_Y)) * d.W + x0 + (rt % CT_X));
        }
        parent[((long)z * d.H + y) * d.W + x] = p;
    }
}

__global__ __launch_bounds__(NT) void cc_merge_kernel(Dims d, int maxd, int *__restrict__ parent_all) {
    const int b = blockIdx.y;
    int *parent = parent_all + (long)b * d.V;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < d.V; v += (long)gridDim.x * NT) {
        const int x = (int)(v % d.W), y = (int)((v / d.W) % d.H), z = (int)(v / ((long)d.W * d.H));
        // only voxels on a face of their tile have a backward neighbour in another tile
        if ((z % CT_Z) && (y % CT_Y) && (y % CT_Y) != CT_Y - 1 && (x % CT_X) && (x % CT_X) != CT_X - 1) continue;
        if (g_load(parent + v) < 0) continue;
        for (int dz = -1; dz <= 0; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!backward(dz, dy, dx, maxd)) continue;
                    const int nz = z + dz, ny = y + dy, nx = x + dx;
                    if (nz < 0 || ny < 0 || ny >= d.H || nx < 0 || nx >= d.W) continue;
                    if (nz / CT_Z == z / CT_Z && ny / CT_Y == y / CT_Y && nx / CT_X == x / CT_X) continue;   // the local pass did it
                    const long nv = ((long)nz * d.H + ny) * d.W + nx;
                    if (g_load(parent + nv) >= 0) g_union(parent, (int)v, (int)nv);
                }
    }
}

// root[v] = find(v) (parents are final: plain loads), and the roots of each chunk are counted
__global__ __launch_bounds__(NT) void cc_flatten_kernel(Dims d, int nchunks, const int *__restrict__ parent_all,
                                                        int *__restrict__ root_all, int *__restrict__ counts) {
    __shared__ int red[NT / 64];
    const int b = blockIdx.y;
    const int *parent = parent_all + (long)b * d.V;
    int *root = root_all + (long)b * d.V;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {   // (uniform)
        int c = 0;
#pragma unroll
        for (int k = 0; k < CHUNK / NT; ++k) {
            const long v = (long)ch * CHUNK + threadIdx.x * (CHUNK / NT) + k;
            if (v >= d.V) continue;
            int a = parent[v];
            if (a >= 0) {
                int p = a;          // parent[a] <= a, followed only while it differs: strictly decreasing, at most v steps
                a = (int)v;
                while (p != a) {
                    a = p;
                    p = parent[a];
                }
                c += a == (int)v;
            }
            root[v] = a;
        }
        int total;
        block_excl_scan<NT>(c, red, total);
        if (threadIdx.x == 0) counts[(long)b * nchunks + ch] = total;
    }
}

// one workgroup per item: counts -> exclusive sums in place, n
__global__ __launch_bounds__(NT) void cc_scan_kernel(int nchunks, int *__restrict__ counts, int *__restrict__ n_out) {
    __shared__ int red[NT / 64];
    int *cnt = counts + (long)blockIdx.x * nchunks;
    int carry = 0;
    for (int base = 0; base < nchunks; base += NT) {   // (uniform)
        const int i = base + threadIdx.x;
        const int c = i < nchunks ? cnt[i] : 0;
        int total;
        const int ex = block_excl_scan<NT>(c, red, total);
        if (i < nchunks) cnt[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) n_out[blockIdx.x] = carry;
}

// roots, in raster order, get the labels 1..n: written into parent[root], which nothing follows any more
__global__ __launch_bounds__(NT) void cc_number_kernel(Dims d, int nchunks, const int *__restrict__ root_all,
                                                       const int *__restrict__ counts, int *__restrict__ parent_all) {
    __shared__ int red[NT / 64];
    const int b = blockIdx.y;
    const int *root = root_all + (long)b * d.V;
    int *parent = parent_all + (long)b * d.V;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {   // (uniform)
        const long v0 = (long)ch * CHUNK + threadIdx.x * (CHUNK / NT);
        bool is_root[CHUNK / NT];
        int c = 0;
#pragma unroll
        for (int k = 0; k < CHUNK / NT; ++k) {
            is_root[k] = v0 + k < d.V && root[v0 + k] == (int)(v0 + k);
            c += is_root[k];
        }
        int total;
        int rank = counts[(long)b * nchunks + ch] + block_excl_scan<NT>(c, red, total);
#pragma unroll
        for (int k = 0; k < CHUNK / NT; ++k)
            if (is_root[k]) parent[v0 + k] = ++rank;
    }
}

__global__ __launch_bounds__(NT) void cc_final_kernel(Dims d, const int *__restrict__ parent_all, int *__restrict__ label_all) {
    const int b = blockIdx.y;
    const int *parent = parent_all + (long)b * d.V;
    int *label = label_all + (long)b * d.V;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < d.V; v += (long)gridDim.x * NT) {
        const int rt = label[v];
        label[v] = rt >= 0 ? parent[rt] : 0;
    }
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// ------------------------------------------------------------------------------------------------ statistics, relabel
// stats (B, cap, 4) int64: voxel count and the sums of z, y, x of labels 1..cap.  A wave takes 64 consecutive voxels and
// adds once per distinct label among them (integer atomics: exact, any order).  The loop retires at least the leader's lane
// per pass: at most 64 passes.
__global__ __launch_bounds__(NT) void stats_kernel(Dims d, const int *__restrict__ labels, int cap, u64 *__restrict__ stats) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    labels += (long)b * d.V;
    stats += (long)b * cap * 4;
    const long vround = (d.V + 63) & ~63L;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < vround; v += (long)gridDim.x * NT) {   // (whole waves stay together)
        int lab = 0, x = 0, y = 0, z = 0;
        if (v < d.V) {
            lab = labels[v];
            x = (int)(v % d.W);
            y = (int)((v / d.W) % d.H);
            z = (int)(v / ((long)d.W * d.H));
        }
        bool todo = lab >= 1 && lab <= cap;
        for (;;) {
            const u64 open = __ballot(todo);
            if (!open) break;
            const int leader = __builtin_ctzll(open);
            const int L = __shfl(lab, leader, 64);
            const bool mine = todo && lab == L;
            const u64 group = __ballot(mine);
            const long long sz = wave_sum_lane0((long long)(mine ? z : 0)), sy = wave_sum_lane0((long long)(mine ? y : 0)),
                            sx = wave_sum_lane0((long long)(mine ? x : 0));
            if (lane == 0) {
                u64 *s = stats + (long)(L - 1) * 4;
                atomicAdd(s + 0, (u64)__builtin_popcountll(group));
                atomicAdd(s + 1, (u64)sz);
                atomicAdd(s + 2, (u64)sy);
                atomicAdd(s + 3, (u64)sx);
            }
            todo = todo && !mine;
        }
    }
}

template <typename OT>
__global__ __launch_bounds__(NT) void lut_kernel(long n_per_item, const int *__restrict__ labels, const int *__restrict__ lut,
                                                 int lut_len, OT *__restrict__ out) {
    const int b = blockIdx.y;
    labels += (long)b * n_per_item;
    out += (long)b * n_per_item;
    lut += (long)b * lut_len;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < n_per_item; v += (long)gridDim.x * NT) {
        const int l = labels[v];
        out[v] = (OT)((l >= 0 && l < lut_len) ? lut[l] : 0);
    }
}

}  // namespace

extern "C" int fsg_bits_pack_u8(const uint8_t *vol, int B, int D, int H, int W, int value, uint64_t *bits, fsg_stream_t stream) {
    const char *name = "fsg_bits_pack_u8";
    Dims d;
    if (int rc = check_dims(name, B, D, H, W, d)) return rc;
    FSG_REQUIRE(value >= -1 && value <= 255, "%s: value %d (-1: nonzero, 0..255: equal to)", name, value);
    FSG_REQUIRE(vol && bits, "%s: NULL pointer", name);
    pack_kernel<<<grid_for(d.rows * d.WW, NT / 64), NT, 0, (hipStream_t)stream>>>(d, vol, value, (u64 *)bits);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_bits_unpack_u8(const uint64_t *bits, int B, int D, int H, int W, uint8_t *vol, fsg_stream_t stream) {
    const char *name = "fsg_bits_unpack_u8";
    Dims d;
    if (int rc = check_dims(name, B, D, H, W, d)) return rc;
    FSG_REQUIRE(vol && bits, "%s: NULL pointer", name);
    unpack_kernel<<<grid_for(d.rows * d.W, NT), NT, 0, (hipStream_t)stream>>>(d, (const u64 *)bits, vol);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_bits_window(const uint64_t *in, int B, int Di, int Hi, int Wi, int oz, int oy, int ox, int Do, int Ho, int Wo,
                               uint64_t *out, fsg_stream_t stream) {
    const char *name = "fsg_bits_window";
    Dims di, dout;
    if (int rc = check_dims(name, B, Di, Hi, Wi, di)) return rc;
    if (int rc = check_dims(name, B, Do, Ho, Wo, dout)) return rc;
    const int lim = 1 << 20;
    FSG_REQUIRE(oz > -lim && oz < lim && oy > -lim && oy < lim && ox > -lim && ox < lim, "%s: offset (%d, %d, %d)", name, oz, oy, ox);
    FSG_REQUIRE(in && out && in != out, "%s: NULL pointer or in == out", name);
    window_kernel<<<grid_for(dout.rows * dout.WW, NT), NT, 0, (hipStream_t)stream>>>(di, dout, oz, oy, ox, (const u64 *)in, (u64 *)out);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_ball_dilate_bits(const uint64_t *in, int B, int D, int H, int W, int rz, int ry, int rx, int border, int inv_in,
                                    int inv_out, uint64_t *out, fsg_stream_t stream) {
    const char *name = "fsg_ball_dilate_bits";
    Dims d;
    if (int rc = check_dims(name, B, D, H, W, d)) return rc;
    FSG_REQUIRE(rz >= 0 && rz <= MAXR && ry >= 0 && ry <= MAXR && rx >= 0 && rx <= MAXR, "%s: radius (%d, %d, %d) outside 0..%d", name,
                rz, ry, rx, MAXR);
    FSG_REQUIRE((border == 0 || border == 1) && (inv_in == 0 || inv_in == 1) && (inv_out == 0 || inv_out == 1),
                "%s: border %d / inv_in %d / inv_out %d must be 0 or 1", name, border, inv_in, inv_out);
    FSG_REQUIRE(in && out && in != out, "%s: NULL pointer or in == out", name);
    Taps taps;
    int n = 0;
    for (int h = 0; h <= rx; ++h) {
        taps.start[h] = (short)n;
        for (int dz = -rz; dz <= rz; ++dz)
            for (int dy = -ry; dy <= ry; ++dy)
                if (half_width(dz, dy, rz, ry, rx) == h) {
                    taps.dz[n] = (signed char)dz;
                    taps.dy[n] = (signed char)dy;
                    ++n;
                }
    }
    for (int h = rx + 1; h <= MAXR + 1; ++h) taps.start[h] = (short)n;
    Tile t;
    t.XW = d.WW < 8 ? d.WW : 8;
    t.TY = 8;
    t.TZ = NT / (t.TY * t.XW);
    if (t.TZ > 8) t.TZ = 8;
    t.SZ = t.TZ + 2 * rz;
    t.SY = t.TY + 2 * ry;
    t.SX = t.XW + 2;
    t.tiles_x = fsg_cdiv(d.WW, t.XW);
    const long gx = (long)t.tiles_x * fsg_cdiv(H, t.TY);
    const int gy = fsg_cdiv(D, t.TZ);
    FSG_REQUIRE(gx < (1L << 31) && gy <= 65535, "%s: D=%d H=%d W=%d needs a grid of %ld x %d", name, D, H, W, gx, gy);
    const size_t lds = (size_t)t.SZ * t.SY * t.SX * sizeof(u64);   // at most 24 * 24 * 10 * 8 = 46080 bytes
    dilate_kernel<<<dim3((unsigned)gx, gy, B), NT, lds, (hipStream_t)stream>>>(d, t, taps, rz, ry, rx, border, inv_in, inv_out,
                                                                                 (const u64 *)in, (u64 *)out);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" size_t fsg_cc_workspace_bytes(int B, int D, int H, int W) {
    if (B < 1 || D < 1 || H < 1 || W < 1) return 0;
    const long V = (long)D * H * W;
    return align256((size_t)B * V * sizeof(int)) + align256((size_t)B * ((V + CHUNK - 1) / CHUNK) * sizeof(int));
}

extern "C" int fsg_cc_label_bits(const uint64_t *bits, int B, int D, int H, int W, int connectivity, int32_t *labels, int32_t *n,
                                 void *workspace, size_t workspace_bytes, fsg_stream_t stream) {
    const char *name = "fsg_cc_label_bits";
    Dims d;
    if (int rc = check_dims(name, B, D, H, W, d)) return rc;
    FSG_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "%s: connectivity %d (6, 18 or 26)", name, connectivity);
    const size_t need = fsg_cc_workspace_bytes(B, D, H, W);
    FSG_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: NULL or misaligned workspace", name);
    FSG_REQUIRE(bits && labels && n, "%s: NULL pointer", name);
    const int maxd = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
    const int nchunks = (int)((d.V + CHUNK - 1) / CHUNK);
    int *parent = (int *)workspace;
    int *counts = (int *)((char *)workspace + align256((size_t)B * d.V * sizeof(int)));
    const int tiles_x = fsg_cdiv(W, CT_X);
    const long gx = (long)tiles_x * fsg_cdiv(H, CT_Y);
    const int gy = fsg_cdiv(D, CT_Z);
    FSG_REQUIRE(gx < (1L << 31) && gy <= 65535, "%s: D=%d H=%d W=%d needs a grid of %ld x %d", name, D, H, W, gx, gy);
    hipStream_t s = (hipStream_t)stream;
    cc_local_kernel<<<dim3((unsigned)gx, gy, B), NT, 0, s>>>(d, tiles_x, maxd, (const u64 *)bits, parent);
    cc_merge_kernel<<<dim3(grid_for(d.V, NT), B), NT, 0, s>>>(d, maxd, parent);
    const dim3 cgrid(nchunks < MAX_BLOCKS ? nchunks : MAX_BLOCKS, B);
    cc_flatten_kernel<<<cgrid, NT, 0, s>>>(d, nchunks, parent, labels, counts);
    cc_scan_kernel<<<B, NT, 0, s>>>(nchunks, counts, n);
    cc_number_kernel<<<cgrid, NT, 0, s>>>(d, nchunks, labels, counts, parent);
    cc_final_kernel<<<dim3(grid_for(d.V, NT), B), NT, 0, s>>>(d, parent, labels);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_component_stats_i32(const int32_t *labels, int B, int D, int H, int W, int cap, int64_t *stats,
                                       fsg_stream_t stream) {
    const char *name = "fsg_component_stats_i32";
    Dims d;
    if (int rc = check_dims(name, B, D, H, W, d)) return rc;
    FSG_REQUIRE(cap >= 1 && (long)B * cap < (1L << 28), "%s: cap %d", name, cap);
    FSG_REQUIRE(labels && stats, "%s: NULL pointer", name);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, (size_t)B * cap * 4 * sizeof(int64_t), s) != hipSuccess) {
        fsg_set_error("%s: hipMemsetAsync failed", name);
        return FSG_ERR_HIP;
    }
    stats_kernel<<<dim3(grid_for(d.V, NT), B), NT, 0, s>>>(d, labels, cap, (u64 *)stats);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_relabel_lut_i32(const int32_t *labels, int B, int64_t n_per_item, const int32_t *lut, int lut_len, void *out,
                                   int out_is_i64, fsg_stream_t stream) {
    const char *name = "fsg_relabel_lut_i32";
    FSG_REQUIRE(B > 0 && B <= 65535 && n_per_item > 0 && (long)B * n_per_item < (1L << 31) && lut_len > 0, "%s: B=%d n=%ld lut_len=%d",
                name, B, (long)n_per_item, lut_len);
    FSG_REQUIRE(labels && lut && out, "%s: NULL pointer", name);
    const dim3 grid(grid_for(n_per_item, NT), B);
    if (out_is_i64) lut_kernel<int64_t><<<grid, NT, 0, (hipStream_t)stream>>>(n_per_item, labels, lut, lut_len, (int64_t *)out);
    else lut_kernel<int32_t><<<grid, NT, 0, (hipStream_t)stream>>>(n_per_item, labels, lut, lut_len, (int32_t *)out);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}
