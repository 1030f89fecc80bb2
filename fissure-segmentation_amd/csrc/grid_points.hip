// The bridge between a point cloud and a dense grid, and the spectral Poisson solve of DPSR -- include/fsg_hip.h:
// fsg_grid_corners_f32, fsg_grid_splat_sorted_f32, fsg_grid_sample_f32, fsg_psr_spectral_f32.
// Replaces models/divroc.py:24-61 (splat by differentiating grid_sample against a zero grid), models/dpsr_utils.py:156-287
// (grid_interp, point_rasterize) and models/dpsr_net.py:74-87 (spectral_PSR between the two FFTs) of the reference.
//
// Two coordinate conventions, one set of kernels.  Per memory axis (D, H, W) a point has a lower and an upper index, their two
// weights and the derivatives of the weights with respect to the point's coordinate on that axis (`Axis`):
//   TORCH  grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False): coordinate (x -> W, y -> H, z -> D) in
//          [-1, 1], t = ((x + 1) S - 1) / 2, lower = floor t, upper = lower + 1, weights (lower + 1) - t and t - lower,
//          derivatives -S/2 and +S/2.  A corner outside the grid is dropped (gives and receives nothing).
//   SAP    point_rasterize / grid_interp: coordinate (0 -> D, 1 -> H, 2 -> W) in [0, 1], cs = 1 / (S - 1) in fp32, t = p / cs,
//          lower = floor t, upper = fmod(ceil t, S), weights |p - (lower + 1) cs| / cs and |p - lower cs| / cs, derivatives
//          sign(.) / cs with sign(0) = 0 (torch's abs).  Every expression is the reference's, in fp32, in its order, so a point
//          on a node (lower = upper, both corners land on one voxel) and the points 0 and 1 reach the reference's voxels.
//          Points outside [0, 1] are outside the contract; their out-of-grid corners are dropped, nothing is written outside.
// The weight of corner (a, b, c) is the product of three axis weights, multiplied in the reference's order.
//
// Splat (values (B, C, N) -> grid (B, C, D, H, W)) is store-and-sum, without floating-point atomics:
//   1. `corners`: one thread per point writes the 8 destination voxels (int32 key, D H W for a dropped corner) and the 8 weights
//      at positions 8 n + corner of the item's row.
//   2. the caller orders every row by key with a STABLE sort (torch.sort): a voxel's contributions become one run, in point order.
//   3. `splat_chunks`: a run is cut where the key changes and at every multiple of 64 positions of the row; the first thread of
//      a piece adds its <= 64 contributions in order, all channels in one pass over the piece (8 accumulators per pass), and
//      stores the sum -- into the grid when the piece is the whole run, else into the partial buffer at its own position.
//   4. `splat_runs`: the first thread of a run that was cut adds the run's partials in position order and stores the voxel.
//   The order of every sum is fixed by the item's own sorted row: the same input gives the same bits, an item gives the same
//   bits alone and inside a batch, and 2048 points in one cell cost 32 pieces of 64 per voxel instead of one thread's 2048.
// Sample (grid, coords -> sampled (B, C, N)) is one gather kernel, one thread per point: indices and weights once, then the
// channel loop reads the 8 corners of each channel once and forms the value and -- when `weights` (B, C, N) is given --
// grad_coords (B, N, 3) = sum_c weights_c d sample_c / d coord.  With the splat this serves all four autograd relations.
//
// Spectral solve: one thread per frequency of the half spectrum (B, R0, R1, R2/2 + 1) reads the three components of the
// transformed normal field in place (no permute), builds G (fp64, rounded to fp32 as the reference's buffer is), omega =
// 2 pi fftfreq in fp32 and Lap = -|omega|^2, and writes Phi = sum_d (-i omega_d G N_d) / (Lap + 1e-6), 0 at the DC term.
// With `adjoint` it writes grad N_d = conj(c_d) grad Phi instead, c_d = -i omega_d G / (Lap + 1e-6).
#include "fsg_common.h"

namespace {

constexpr int RUN_CHUNK = 64;   // a run of one voxel's contributions is cut at every multiple of this many row positions
constexpr int CH_BLOCK = 8;     // channels summed in one pass over a piece
constexpr int THREADS = 256;

struct Axis {
    int i0, i1;        // lower and upper index (either may lie outside 0..S-1: that corner is dropped)
    float w0, w1;      // their weights
    float d0, d1;      // d weight / d coordinate
};

__device__ __forceinline__ Axis axis_torch(float x, int S) {
    const float t = ((x + 1.f) * (float)S - 1.f) / 2.f;
    // the index comes from t clamped to [-2, S + 1] (NaN -> -2): there both corners are outside, so the clamp changes no result
    const float f = floorf(fminf(fmaxf(t, -2.f), (float)S + 1.f));
    Axis a;
    a.i0 = (int)f;
    a.i1 = a.i0 + 1;
    a.w0 = (f + 1.f) - t;
    a.w1 = t - f;
    a.d0 = -0.5f * (float)S;
    a.d1 = 0.5f * (float)S;
    return a;
}

__device__ __forceinline__ float sign0(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ Axis axis_sap(float p, int S) {
    const float size = (float)S, cs = 1.0f / (size - 1.0f);
    const float t = fminf(fmaxf(p / cs, -2.f), size + 1.f);   // inside [0, 1] the clamp is the identity
    const float f0 = floorf(t), f1 = fmodf(ceilf(t), size);
    const float e0 = p - (f0 + 1.f) * cs, e1 = p - f0 * cs;
    Axis a;
    a.i0 = (int)f0;
    a.i1 = (int)f1;
    a.w0 = fabsf(e0) / cs;
    a.w1 = fabsf(e1) / cs;
    a.d0 = sign0(e0) / cs;
    a.d1 = sign0(e1) / cs;
    return a;
}

// the three axes of point (b, n) in memory order D, H, W; comp[m] = which coordinate component belongs to memory axis m
__device__ __forceinline__ void point_axes(const float *__restrict__ coords, long pn, int D, int H, int W, int mode, Axis &aD,
                                           Axis &aH, Axis &aW) {
    const float c0 = coords[3 * pn], c1 = coords[3 * pn + 1], c2 = coords[3 * pn + 2];
    if (mode == FSG_GRID_TORCH) {
        aD = axis_torch(c2, D);
        aH = axis_torch(c1, H);
        aW = axis_torch(c0, W);
    } else {
        aD = axis_sap(c0, D);
        aH = axis_sap(c1, H);
        aW = axis_sap(c2, W);
    }
}

__device__ __forceinline__ bool inside(int i, int S) { return i >= 0 && i < S; }

// corner k = 4 a + 2 b + c takes the upper index on D / H / W where a / b / c is set
#define GP_CORNER(k, aD, aH, aW, iD, iH, iW, wD, wH, wW, dD, dH, dW)          \
    const int iD = (k & 4) ? aD.i1 : aD.i0, iH = (k & 2) ? aH.i1 : aH.i0, iW = (k & 1) ? aW.i1 : aW.i0;  \
    const float wD = (k & 4) ? aD.w1 : aD.w0, wH = (k & 2) ? aH.w1 : aH.w0, wW = (k & 1) ? aW.w1 : aW.w0; \
    const float dD = (k & 4) ? aD.d1 : aD.d0, dH = (k & 2) ? aH.d1 : aH.d0, dW = (k & 1) ? aW.d1 : aW.d0;

__global__ __launch_bounds__(THREADS) void corners_kernel(const float *__restrict__ coords, int N, int D, int H, int W, int mode,
                                                          int32_t *__restrict__ keys, float *__restrict__ w) {
    const int n = blockIdx.x * THREADS + threadIdx.x;
    if (n >= N) return;
    const long pn = (long)blockIdx.y * N + n;
    Axis aD, aH, aW;
    point_axes(coords, pn, D, H, W, mode, aD, aH, aW);
    const int DHW = D * H * W;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        GP_CORNER(k, aD, aH, aW, iD, iH, iW, wD, wH, wW, dD, dH, dW)
        (void)dD, (void)dH, (void)dW;
        const bool ok = inside(iD, D) && inside(iH, H) && inside(iW, W);
        keys[8 * pn + k] = ok ? (iD * H + iH) * W + iW : DHW;
        w[8 * pn + k] = mode == FSG_GRID_TORCH ? (wW * wH) * wD : (wD * wH) * wW;
    }
}

// keys / perm: the item's row after the stable sort (perm = position before the sort = 8 n + corner)
__global__ __launch_bounds__(THREADS) void splat_chunks_kernel(const float *__restrict__ values, const int32_t *__restrict__ keys,
                                                               const int64_t *__restrict__ perm, const float *__restrict__ w,
                                                               int C, int N, int DHW, float *__restrict__ grid,
                                                               float *__restrict__ part) {
    const int n8 = 8 * N, j = blockIdx.x * THREADS + threadIdx.x, b = blockIdx.y;
    if (j >= n8) return;
    const int32_t *k = keys + (long)b * n8;
    const int32_t key = k[j];
    if (key < 0 || key >= DHW) return;                         // a dropped corner (sorted behind every voxel)
    const bool run_start = j == 0 || k[j - 1] != key;
    if (!run_start && j % RUN_CHUNK != 0) return;
    const int end = min(n8, (j / RUN_CHUNK + 1) * RUN_CHUNK);
    int e = j + 1;
    while (e < end && k[e] == key) ++e;
    const bool whole = run_start && (e == n8 || k[e] != key);
    const int64_t *pm = perm + (long)b * n8;
    const float *wb = w + (long)b * n8;
    for (int c0 = 0; c0 < C; c0 += CH_BLOCK) {
        float acc[CH_BLOCK];
#pragma unroll
        for (int u = 0; u < CH_BLOCK; ++u) acc[u] = 0.f;
        for (int q = j; q < e; ++q) {
            const int p = (int)pm[q];
            const float wt = wb[p];
            const float *v = values + ((long)b * C + c0) * N + (p >> 3);
#pragma unroll
            for (int u = 0; u < CH_BLOCK; ++u)
                if (c0 + u < C) acc[u] += wt * v[(long)u * N];
        }
#pragma unroll
        for (int u = 0; u < CH_BLOCK; ++u)
            if (c0 + u < C) {
                const long bc = (long)b * C + c0 + u;
                if (whole)
                    grid[bc * DHW + key] = acc[u];
                else
                    part[bc * n8 + j] = acc[u];
            }
    }
}

__global__ __launch_bounds__(THREADS) void splat_runs_kernel(const int32_t *__restrict__ keys, int C, int N, int DHW,
                                                             const float *__restrict__ part, float *__restrict__ grid) {
    const int n8 = 8 * N, j = blockIdx.x * THREADS + threadIdx.x, b = blockIdx.y;
    if (j >= n8) return;
    const int32_t *k = keys + (long)b * n8;
    const int32_t key = k[j];
    if (key < 0 || key >= DHW) return;
    if (j != 0 && k[j - 1] == key) return;                     // not the first of its run
    const int end = (j / RUN_CHUNK + 1) * RUN_CHUNK;
    if (end >= n8 || k[end] != key) return;                    // the run was one piece: already stored (the row is sorted)
    for (int c = 0; c < C; ++c) {
        const float *pc = part + ((long)b * C + c) * n8;
        float tot = pc[j];
        for (int q = end; q < n8 && k[q] == key; q += RUN_CHUNK) tot += pc[q];
        grid[((long)b * C + c) * DHW + key] = tot;
    }
}

__global__ __launch_bounds__(THREADS) void sample_kernel(const float *__restrict__ grid, const float *__restrict__ coords,
                                                         const float *__restrict__ weights, int C, int N, int D, int H, int W,
                                                         int mode, float *__restrict__ sampled, float *__restrict__ gcoords) {
    const int n = blockIdx.x * THREADS + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    const long pn = (long)b * N + n;
    Axis aD, aH, aW;
    point_axes(coords, pn, D, H, W, mode, aD, aH, aW);
    int idx[8];
    float wt[8], gD[8], gH[8], gW[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        GP_CORNER(k, aD, aH, aW, iD, iH, iW, wD, wH, wW, dD, dH, dW)
        const bool ok = inside(iD, D) && inside(iH, H) && inside(iW, W);
        // a dropped corner takes no part at all: its weight may be inf or NaN (a coordinate far outside, or not finite)
        idx[k] = ok ? (iD * H + iH) * W + iW : -1;
        wt[k] = !ok ? 0.f : (mode == FSG_GRID_TORCH ? (wW * wH) * wD : (wD * wH) * wW);
        gD[k] = ok ? dD * (wH * wW) : 0.f;
        gH[k] = ok ? dH * (wD * wW) : 0.f;
        gW[k] = ok ? dW * (wD * wH) : 0.f;
    }
    const long DHW = (long)D * H * W;
    float tD = 0.f, tH = 0.f, tW = 0.f;
    for (int c = 0; c < C; ++c) {
        const float *g = grid + ((long)b * C + c) * DHW;
        float s = 0.f, sD = 0.f, sH = 0.f, sW = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = idx[k] >= 0 ? g[idx[k]] : 0.f;
            s += wt[k] * v;
            sD += gD[k] * v;
            sH += gH[k] * v;
            sW += gW[k] * v;
        }
        const long o = ((long)b * C + c) * N + n;
        if (sampled) sampled[o] = s;
        if (weights) {
            const float wc = weights[o];
            tD += wc * sD;
            tH += wc * sH;
            tW += wc * sW;
        }
    }
    if (gcoords) {
        const bool t = mode == FSG_GRID_TORCH;
        gcoords[3 * pn] = t ? tW : tD;
        gcoords[3 * pn + 1] = tH;
        gcoords[3 * pn + 2] = t ? tD : tW;
    }
}

// numpy's fftfreq(R, d = 1 / R): 0 .. (R - 1) / 2, then -(R / 2) .. -1
__device__ __forceinline__ int fft_freq(int i, int R) { return i <= (R - 1) / 2 ? i : i - R; }

__global__ __launch_bounds__(THREADS) void psr_spectral_kernel(const float2 *__restrict__ in, int R0, int R1, int R2h, double sig,
                                                               int adjoint, float2 *__restrict__ out) {
    const long per = (long)R0 * R1 * R2h, e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= per) return;
    const int b = blockIdx.y;
    const int k = (int)(e % R2h), j = (int)((e / R2h) % R1), i = (int)(e / ((long)R2h * R1));
    const int f0 = fft_freq(i, R0), f1 = fft_freq(j, R1), f2 = k;
    const double dis = sqrt((double)f0 * f0 + (double)f1 * f1 + (double)f2 * f2);
    const double a = sig * 2.0 * dis / (double)R0;
    const float G = (float)exp(-0.5 * (a * a));
    const float two_pi = 6.283185307179586f;
    const float o0 = (float)f0 * two_pi, o1 = (float)f1 * two_pi, o2 = (float)f2 * two_pi;
    const float den = -((o0 * o0 + o1 * o1) + o2 * o2) + 1e-6f;
    const bool dc = e == 0;
    if (!adjoint) {
        const float2 *p = in + (long)b * 3 * per + e;
        const float2 n0 = p[0], n1 = p[per], n2 = p[2 * per];
        float2 r;
        r.x = (((n0.y * G) * o0 + (n1.y * G) * o1) + (n2.y * G) * o2) / den;
        r.y = ((-(n0.x * G) * o0 + -(n1.x * G) * o1) + -(n2.x * G) * o2) / den;
        if (dc) r = make_float2(0.f, 0.f);
        out[(long)b * per + e] = r;
    } else {
        const float2 g = in[(long)b * per + e];
        const float s0 = dc ? 0.f : (G * o0) / den, s1 = dc ? 0.f : (G * o1) / den, s2 = dc ? 0.f : (G * o2) / den;
        float2 *q = out + (long)b * 3 * per + e;
        q[0] = make_float2(-(s0 * g.y), s0 * g.x);
        q[per] = make_float2(-(s1 * g.y), s1 * g.x);
        q[2 * per] = make_float2(-(s2 * g.y), s2 * g.x);
    }
}

// shapes shared by the three point-side entries
int check_shape(const char *entry, int B, int C, int N, int D, int H, int W, int mode) {
    FSG_REQUIRE(mode == FSG_GRID_TORCH || mode == FSG_GRID_SAP, "%s: bad mode %d (0 = TORCH, 1 = SAP)", entry, mode);
    FSG_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && N >= 1 && N <= (1 << 27) && D >= 1 && H >= 1 && W >= 1 &&
                    (long)D * H * W < 2147483647L,
                "%s: bad shape B=%d C=%d N=%d grid %dx%dx%d (B <= 65535, N <= 2^27, D H W < 2^31 - 1)", entry, B, C, N, D, H, W);
    FSG_REQUIRE(mode != FSG_GRID_SAP || (D >= 2 && H >= 2 && W >= 2),
                "%s: bad shape: SAP mode needs every grid size >= 2 (cubesize = 1 / (size - 1)), got %dx%dx%d", entry, D, H, W);
    return FSG_OK;
}

}   // namespace

extern "C" {

int fsg_grid_corners_f32(const float *coords, int B, int N, int D, int H, int W, int mode, int32_t *keys, float *w,
                         fsg_stream_t stream) {
    FSG_REQUIRE(coords && keys && w, "fsg_grid_corners_f32: NULL pointer");
    if (int rc = check_shape("fsg_grid_corners_f32", B, 1, N, D, H, W, mode)) return rc;
    corners_kernel<<<dim3(fsg_cdiv(N, THREADS), B), THREADS, 0, (hipStream_t)stream>>>(coords, N, D, H, W, mode, keys, w);
    FSG_CHECK_LAUNCH("fsg_grid_corners_f32");
    return FSG_OK;
}

size_t fsg_grid_splat_workspace_bytes(int B, int C, int N) {
    if (B < 1 || C < 1 || N < 1) return 0;
    return (size_t)B * C * 8 * N * sizeof(float);
}

int fsg_grid_splat_sorted_f32(const float *values, const int32_t *keys_sorted, const int64_t *perm, const float *w, int B, int C,
                              int N, int D, int H, int W, float *grid, void *workspace, size_t workspace_bytes,
                              fsg_stream_t stream) {
    FSG_REQUIRE(values && keys_sorted && perm && w && grid && workspace, "fsg_grid_splat_sorted_f32: NULL pointer");
    if (int rc = check_shape("fsg_grid_splat_sorted_f32", B, C, N, D, H, W, FSG_GRID_TORCH)) return rc;
    const size_t need = fsg_grid_splat_workspace_bytes(B, C, N);
    FSG_REQUIRE(workspace_bytes >= need, "fsg_grid_splat_sorted_f32: workspace of %zu bytes, need %zu", workspace_bytes, need);
    FSG_REQUIRE(((uintptr_t)workspace & 3) == 0, "fsg_grid_splat_sorted_f32: workspace must be 4-byte aligned");
    const int DHW = D * H * W;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(grid, 0, (size_t)B * C * DHW * sizeof(float), s) != hipSuccess) {
        fsg_set_error("fsg_grid_splat_sorted_f32: clearing the grid failed");
        return FSG_ERR_HIP;
    }
    const dim3 blocks(fsg_cdiv(8L * N, THREADS), B);
    splat_chunks_kernel<<<blocks, THREADS, 0, s>>>(values, keys_sorted, perm, w, C, N, DHW, grid, (float *)workspace);
    FSG_CHECK_LAUNCH("fsg_grid_splat_sorted_f32 (pieces)");
    splat_runs_kernel<<<blocks, THREADS, 0, s>>>(keys_sorted, C, N, DHW, (const float *)workspace, grid);
    FSG_CHECK_LAUNCH("fsg_grid_splat_sorted_f32 (runs)");
    return FSG_OK;
}

int fsg_grid_sample_f32(const float *grid, const float *coords, const float *weights, int B, int C, int N, int D, int H, int W,
                        int mode, float *sampled, float *grad_coords, fsg_stream_t stream) {
    FSG_REQUIRE(grid && coords && (sampled || grad_coords), "fsg_grid_sample_f32: NULL pointer");
    FSG_REQUIRE((weights != nullptr) == (grad_coords != nullptr),
                "fsg_grid_sample_f32: NULL pointer: weights and grad_coords come together");
    if (int rc = check_shape("fsg_grid_sample_f32", B, C, N, D, H, W, mode)) return rc;
    sample_kernel<<<dim3(fsg_cdiv(N, THREADS), B), THREADS, 0, (hipStream_t)stream>>>(grid, coords, weights, C, N, D, H, W, mode,
                                                                                      sampled, grad_coords);
    FSG_CHECK_LAUNCH("fsg_grid_sample_f32");
    return FSG_OK;
}

int fsg_psr_spectral_f32(const float *in, int B, int R0, int R1, int R2, double sig, int adjoint, float *out,
                         fsg_stream_t stream) {
    FSG_REQUIRE(in && out && in != out, "fsg_psr_spectral_f32: NULL pointer (or in == out)");
    FSG_REQUIRE(B >= 1 && B <= 65535 && R0 >= 1 && R1 >= 1 && R2 >= 1 && (long)R0 * R1 * (R2 / 2 + 1) < (1L << 31),
                "fsg_psr_spectral_f32: bad shape B=%d res %dx%dx%d", B, R0, R1, R2);
    FSG_REQUIRE(sig >= 0 && (adjoint == 0 || adjoint == 1), "fsg_psr_spectral_f32: bad sig %g or adjoint flag %d", sig, adjoint);
    const int R2h = R2 / 2 + 1;
    psr_spectral_kernel<<<dim3(fsg_cdiv((long)R0 * R1 * R2h, THREADS), B), THREADS, 0, (hipStream_t)stream>>>(
        (const float2 *)in, R0, R1, R2h, sig, adjoint, (float2 *)out);
    FSG_CHECK_LAUNCH("fsg_psr_spectral_f32");
    return FSG_OK;
}

}   // extern "C"
