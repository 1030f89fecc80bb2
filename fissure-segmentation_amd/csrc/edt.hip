// Exact separable squared Euclidean distance transform of bit planes, with the optional feature transform, and the
// nearest-of-K-planes compare -- include/fsg_hip.h: fsg_edt_workspace_bytes, fsg_edt_sq_i32, fsg_edt_sq_f32,
// fsg_edt_nearest_label.  Stands where the reference calls scipy.ndimage.distance_transform_edt
// (data_processing/process_lung_mask.py:80-91) and where it measures nearest-neighbour distances between the voxel clouds of
// two label maps (metrics.py:79-93).
//
// Definitions.  The input is a bit plane (csrc/morphology.hip: 64 voxels per word along W, the bits past W are 0) of a batch
// of volumes (B, D, H, W).  A SITE is a voxel whose bit is 0.  The result at a voxel p is
//   d2(p) = min over the sites q of the same item of  (s0 (pz - qz))^2 + (s1 (py - qy))^2 + (s2 (px - qx))^2,
// +inf when the item has no site (INT32_MAX in the int32 mode).  Three passes, each exact for its axis:
//   W   f0(z, y, x) = (s2 dx)^2 to the nearest site of the row, from count-leading / trailing-zero operations on the words of
//       the row; a row without a site gives +inf
//   H   f1(z, y, x) = min_i f0(z, i, x) + (s1 (y - i))^2
//   D   d2(z, y, x) = min_i f1(i, y, x) + (s0 (z - i))^2
// H and D: a lane owns one output voxel j of a line and walks outward, delta = 0, 1, 2, ... (j - delta before j + delta),
// replacing its best only by a strictly smaller value, and stops at the first delta with (s delta)^2 >= best: every term is
// non-negative and (s delta)^2 does not decrease with delta (also as rounded fp32), so nothing further out can be strictly
// smaller.  The tie rule follows: the smaller |delta| wins, then the lower index; in the W pass the left site wins a tie.  No
// stack, no atomics, no scratch: the same input gives the same bits, and an item does not depend on the rest of its batch.
// Bound: a line of length n costs at most n steps per voxel (one site in a corner of a set volume: O(n^2) per line).
// The lanes of a wave are 64 neighbours along the contiguous axis (W for the H pass, H W for the D pass), so every load and
// store of the walk is one coalesced row segment; the four waves of a workgroup own four consecutive positions of the same
// lines and so walk over the same segments one step apart (vector-cache reuse).  No LDS: no dimension is limited by it.
//
// Arithmetic.  int32 mode (unit spacing): delta^2 and sums in int32, exact; every dimension <= 16384, so 3 * 16383^2 fits.
// fp32 mode: t = fl(fl(s * float(delta))^2), value = fl(f + t), with -ffp-contract=off (no fused multiply-add).
//
// Feature transform (optional): the winning site travels with the value.  W pass: its x; H pass: y W + x; D pass: the linear
// index (z H + y) W + x inside the item, int32; -1 where the value is +inf.
#include <limits.h>

#include "fsg_common.h"

namespace {

constexpr int NT = 256;
constexpr int TJ = NT / 64;          // line positions per workgroup (one per wave)
constexpr int MAX_DIM = FSG_EDT_MAX_DIM;
constexpr int MAX_GRID = 1 << 20;    // grid-strided launches
constexpr int MAX_PLANES = FSG_EDT_MAX_LABELS;

template <typename T>
struct Arith;
template <>
struct Arith<int> {
    static __device__ __forceinline__ int inf() { return INT_MAX; }
    static __device__ __forceinline__ int sq(int delta, float) { return delta * delta; }
    static __device__ __forceinline__ int add(int f, int t) { return f == INT_MAX ? INT_MAX : f + t; }
};
template <>
struct Arith<float> {
    static __device__ __forceinline__ float inf() { return __builtin_huge_valf(); }
    static __device__ __forceinline__ float sq(int delta, float s) {
        const float d = s * (float)delta;
        return d * d;
    }
    static __device__ __forceinline__ float add(float f, float t) { return f + t; }
};

// the bits of word j of a row that are sites: the complement, without the bits past W
__device__ __forceinline__ u64 site_word(const u64 *__restrict__ row, int W, int WW, int j) {
    const int rem = W & 63;
    const u64 m = (j == WW - 1 && rem) ? ((1ull << rem) - 1ull) : ~0ull;
    return ~row[j] & m;
}

// W pass: a thread per voxel.  The searches over the words of the row end at the first word with a site: at most WW steps.
template <typename T, bool IDX>
__global__ __launch_bounds__(NT) void edt_row_kernel(long n, int W, int WW, float s, const u64 *__restrict__ bits,
                                                     T *__restrict__ f, int *__restrict__ site) {
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < n; v += (long)gridDim.x * NT) {
        const long r = v / W;
        const int x = (int)(v - r * W), j = x >> 6, bit = x & 63;
        const u64 *row = bits + r * WW;
        const u64 here = site_word(row, W, WW, j);
        int left = -1, right = -1;
        u64 m = here & (~0ull >> (63 - bit));            // sites at or before x
        if (m) left = j * 64 + 63 - __builtin_clzll(m);
        else
            for (int k = j - 1; k >= 0; --k) {
                const u64 w = ~row[k];                   // (not the last word, or the loop would not be here: no tail)
                if (w) {
                    left = k * 64 + 63 - __builtin_clzll(w);
                    break;
                }
            }
        m = here & (~0ull << bit);                       // sites at or after x
        if (m) right = j * 64 + __builtin_ctzll(m);
        else
            for (int k = j + 1; k < WW; ++k) {
                const u64 w = site_word(row, W, WW, k);
                if (w) {
                    right = k * 64 + __builtin_ctzll(w);
                    break;
                }
            }
        int q = -1, delta = 0;
        if (left >= 0 && (right < 0 || x - left <= right - x)) {   // a tie goes to the lower index
            q = left;
            delta = x - left;
        } else if (right >= 0) {
            q = right;
            delta = right - x;
        }
        f[v] = q >= 0 ? Arith<T>::sq(delta, s) : Arith<T>::inf();
        if (IDX) site[v] = q;
    }
}

// H and D passes.  The volume is (outer, L, S): lines of L values, S apart; a tile is TJ line positions x 64 neighbours.
// site_in holds the winner so far inside its (S-sized) slab, site_out = winner's line position * S + that.
template <typename T, bool IDX>
__global__ __launch_bounds__(NT) void edt_line_kernel(long outer, int L, long S, float s, const T *__restrict__ f,
                                                      const int *__restrict__ site_in, T *__restrict__ out,
                                                      int *__restrict__ site_out) {
    const int lane = threadIdx.x & 63, wj = threadIdx.x >> 6;
    const long tiles_i = (S + 63) / 64;
    const int tiles_j = (L + TJ - 1) / TJ;
    const long ntiles = outer * tiles_j * tiles_i;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long ti = t % tiles_i, rest = t / tiles_i;
        const int tj = (int)(rest % tiles_j);
        const long o = rest / tiles_j;
        const long i = ti * 64 + lane;
        const int j = tj * TJ + wj;
        if (i >= S || j >= L) continue;
        const long base = o * L * S + i;
        const T *line = f + base;
        T best = line[(long)j * S];
        int arg = j;
        const int dmax = j > L - 1 - j ? j : L - 1 - j;
        for (int d = 1; d <= dmax; ++d) {
            const T t2 = Arith<T>::sq(d, s);
            if (t2 >= best) break;
            if (j - d >= 0) {
                const T c = Arith<T>::add(line[(long)(j - d) * S], t2);
                if (c < best) {
                    best = c;
                    arg = j - d;
                }
            }
            if (j + d < L) {
                const T c = Arith<T>::add(line[(long)(j + d) * S], t2);
                if (c < best) {
                    best = c;
                    arg = j + d;
                }
            }
        }
        out[base + (long)j * S] = best;
        if (IDX) site_out[base + (long)j * S] = best == Arith<T>::inf() ? -1 : (int)(arg * S) + site_in[base + (long)arg * S];
    }
}

// out[v] = cand[k*], k* the first plane with the smallest value (strictly smaller replaces: planes in ascending label order
// give the tie to the lowest label); 0 where keep is given and 0 there
template <typename T>
__global__ __launch_bounds__(NT) void nearest_kernel(long V, int K, const T *__restrict__ d2, const int *__restrict__ cand,
                                                     const uint8_t *__restrict__ keep, int *__restrict__ out) {
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < V; v += (long)gridDim.x * NT) {
        T best = d2[v];
        int k = 0;
        for (int p = 1; p < K; ++p) {   // (uniform bound)
            const T c = d2[(long)p * V + v];
            if (c < best) {
                best = c;
                k = p;
            }
        }
        out[v] = (keep && !keep[v]) ? 0 : cand[k];
    }
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

inline int grid_for(long items, long per_block) {
    const long n = (items + per_block - 1) / per_block;
    return (int)(n < 1 ? 1 : (n > MAX_GRID ? MAX_GRID : n));
}

int check_shape(const char *name, int B, int D, int H, int W) {
    FSG_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535, "%s: bad shape B=%d D=%d H=%d W=%d", name, B, D, H, W);
    FSG_REQUIRE(D <= MAX_DIM && H <= MAX_DIM && W <= MAX_DIM, "%s: D=%d H=%d W=%d: a dimension exceeds %d", name, D, H, W, MAX_DIM);
    FSG_REQUIRE((long)D * H * W < (1L << 31), "%s: D H W = %d %d %d is 2^31 voxels or more", name, D, H, W);
    return FSG_OK;
}

template <typename T>
int run_edt(const char *name, const uint64_t *bits, int B, int D, int H, int W, float s0, float s1, float s2, T *out_d2,
            int32_t *out_idx, void *workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = check_shape(name, B, D, H, W)) return rc;
    const size_t need = fsg_edt_workspace_bytes(B, D, H, W, out_idx != nullptr);
    FSG_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: NULL or misaligned workspace", name);
    FSG_REQUIRE(bits && out_d2, "%s: NULL pointer", name);
    const long V = (long)D * H * W, n = (long)B * V;
    const int WW = (W + 63) / 64;
    T *tmp = (T *)workspace;
    int *tmp_idx = (int *)((char *)workspace + align256((size_t)n * sizeof(T)));
    const long tiles_h = (long)B * D * fsg_cdiv(H, TJ) * fsg_cdiv(W, 64);
    const long tiles_d = (long)B * fsg_cdiv(D, TJ) * (((long)H * W + 63) / 64);
    if (out_idx) {
        edt_row_kernel<T, true><<<grid_for(n, NT), NT, 0, st>>>(n, W, WW, s2, (const u64 *)bits, out_d2, out_idx);
        edt_line_kernel<T, true><<<grid_for(tiles_h, 1), NT, 0, st>>>((long)B * D, H, (long)W, s1, out_d2, out_idx, tmp, tmp_idx);
        edt_line_kernel<T, true><<<grid_for(tiles_d, 1), NT, 0, st>>>((long)B, D, (long)H * W, s0, tmp, tmp_idx, out_d2, out_idx);
    } else {
        edt_row_kernel<T, false><<<grid_for(n, NT), NT, 0, st>>>(n, W, WW, s2, (const u64 *)bits, out_d2, nullptr);
        edt_line_kernel<T, false><<<grid_for(tiles_h, 1), NT, 0, st>>>((long)B * D, H, (long)W, s1, out_d2, nullptr, tmp, nullptr);
        edt_line_kernel<T, false><<<grid_for(tiles_d, 1), NT, 0, st>>>((long)B, D, (long)H * W, s0, tmp, nullptr, out_d2, nullptr);
    }
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

}  // namespace

extern "C" size_t fsg_edt_workspace_bytes(int B, int D, int H, int W, int with_indices) {
    if (B < 1 || D < 1 || H < 1 || W < 1) return 0;
    const size_t plane = align256((size_t)B * D * H * W * 4);
    return with_indices ? 2 * plane : plane;
}

extern "C" int fsg_edt_sq_i32(const uint64_t *bits, int B, int D, int H, int W, int32_t *out_d2, int32_t *out_idx, void *workspace,
                              size_t workspace_bytes, fsg_stream_t stream) {
    return run_edt<int>("fsg_edt_sq_i32", bits, B, D, H, W, 1.f, 1.f, 1.f, out_d2, out_idx, workspace, workspace_bytes,
                        (hipStream_t)stream);
}

extern "C" int fsg_edt_sq_f32(const uint64_t *bits, int B, int D, int H, int W, float s0, float s1, float s2, float *out_d2,
                              int32_t *out_idx, void *workspace, size_t workspace_bytes, fsg_stream_t stream) {
    const char *name = "fsg_edt_sq_f32";
    FSG_REQUIRE(s0 > 0.f && s1 > 0.f && s2 > 0.f && s0 <= 1e6f && s1 <= 1e6f && s2 <= 1e6f,
                "%s: spacing (%g, %g, %g) must be positive and at most 1e6", name, (double)s0, (double)s1, (double)s2);
    return run_edt<float>(name, bits, B, D, H, W, s0, s1, s2, out_d2, out_idx, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int fsg_edt_nearest_label(const void *d2, int is_f32, int K, int64_t V, const int32_t *cand, const uint8_t *keep,
                                     int32_t *out, fsg_stream_t stream) {
    const char *name = "fsg_edt_nearest_label";
    FSG_REQUIRE(K >= 1 && K <= MAX_PLANES && V > 0 && V < (1L << 31), "%s: K=%d (1..%d) V=%ld", name, K, MAX_PLANES, (long)V);
    FSG_REQUIRE(d2 && cand && out, "%s: NULL pointer", name);
    const int grid = grid_for(V, NT);
    if (is_f32) nearest_kernel<float><<<grid, NT, 0, (hipStream_t)stream>>>(V, K, (const float *)d2, cand, keep, out);
    else nearest_kernel<int><<<grid, NT, 0, (hipStream_t)stream>>>(V, K, (const int *)d2, cand, keep, out);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}
