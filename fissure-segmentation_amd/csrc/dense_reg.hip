// Dense Adam image registration -- include/fsg_hip.h: fsg_reg_smooth3_f32, fsg_reg_objective_workspace_bytes,
// fsg_reg_objective_f16.  Replaces the body of the optimisation loop of the reference's shape_model/adam_registration.py:106-124
// (three avg_pool3d forward and backward, a grid_sample of all feature channels with its sampled tensor, three slice-difference
// regularisers with their autograd graphs).
//
// smooth3: avg_pool3d(kernel 3, stride 1, padding 1, count_include_pad=True) applied three times.  One pool is the product over
// the axes of T, the tridiagonal 1/3 operator whose neighbours outside the domain are zero; the T of different axes commute, so
// three pools are T^3 per axis, and row i of T^3 is 1/27 times the number of 3-step walks (steps -1, 0, +1) from i that never
// leave 0 .. S - 1.  In the interior that is [1 3 6 7 6 3 1] / 27; within two cells of a border, and on an axis shorter than 7,
// the walks that would have left the domain are missing (the values outside are zero again after every pool).  Each thread
// counts the walks of its own position (walk_taps: three unrolled integer passes over seven registers), so the kernel is three
// separable 7-tap passes over an LDS tile with a halo of 3: along S2, along S1, along S0 into global memory.  T is symmetric and
// the axes commute: the operator is its own adjoint and the backward pass is the same launch.
//
// objective: one lane owns one node of the (S0, S1, S2) grid, lanes run along S2.  Per node: t_a = i_a + disp_a S_a / (S_a - 1)
// on each axis (the identity coordinate (2 i + 1) / S - 1 of affine_grid plus disp / ((S - 1) / 2), pushed through grid_sample's
// ((x + 1) S - 1) / 2 -- the node index drops out, so the fraction of t is formed from the displacement alone), the 8 corner
// offsets and the six per-axis weights; then a loop over chunks of 8 fp16 channels: one 16-byte load of the fixed features and
// one per corner of the moving ones, the sample and its three derivatives as a trilinear tree in registers (32 fewer registers
// than eight weights per output: four waves per SIMD instead of three), cost and the three gradient sums accumulated.
// Nothing per channel is stored; a corner outside the volume is never read and counts as the value 0.
// The regulariser reads the node's three displacement channels and their six neighbours.  Cost and regulariser leave the
// workgroup as one fp64 pair (wave shuffles, then LDS, a fixed order); a second launch adds an item's pairs in a fixed order.
// No floating-point atomics anywhere.
//
// Why one lane per node and not Cp / 8 lanes: Cp / 8 is 3 for the reference's 22 channels -- not a power of two, so a node's
// lanes would straddle waves or leave a quarter of each wave idle, and the four sums would need cross-lane adds.  With one lane
// per node the 16-byte chunks of neighbouring lanes lie Cp * 2 bytes apart, so a wave's load touches Cp / 8 times the lines it
// uses at once, but the next chunk iterations use the rest of exactly those lines while they are still in the vector cache.
#include "fsg_common.h"

namespace {

constexpr int THREADS = 256;

// ---------------------------------------------------------------------------------------------------------------- smooth3
constexpr int HALO = 3;
constexpr int T0 = 4, T1 = 8, T2 = 32;                                  // outputs per workgroup
constexpr int L0 = T0 + 2 * HALO, L1 = T1 + 2 * HALO, L2 = T2 + 2 * HALO;   // loaded tile 10 x 14 x 38
constexpr int TILE_IN = L0 * L1 * L2;                                   // 5320 floats; pass 2's 10 x 8 x 32 result reuses it
constexpr int TILE_A = L0 * L1 * T2;                                    // 4480 floats after the pass along S2 (39 200 bytes of LDS in all: four workgroups per CU)
static_assert(THREADS == T1 * T2, "passes 2 and 3 give one thread to every (y, x) of the tile");

// w[k] = number of 3-step walks from i to i + k - 3 inside 0 .. S - 1 (steps -1, 0, +1); 0 for a position outside the domain
__device__ __forceinline__ void walk_taps(int i, int S, float w[7]) {
    int c[7] = {0, 0, 0, 1, 0, 0, 0};
    if (i < 0 || i >= S) c[3] = 0;
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        int n[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int s = (k > 0 ? c[k - 1] : 0) + c[k] + (k < 6 ? c[k + 1] : 0);
            const int j = i + k - 3;
            n[k] = (j >= 0 && j < S) ? s : 0;
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) c[k] = n[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) w[k] = (float)c[k];
}

__global__ __launch_bounds__(THREADS) void reg_smooth3_kernel(const float *__restrict__ in, int S0, int S1, int S2, int n1, int n2,
                                                              float *__restrict__ out) {
    __shared__ float tin[TILE_IN];
    __shared__ float ta[TILE_A];
    const int tid = threadIdx.x;
    const int b2 = blockIdx.x % n2, b1 = (blockIdx.x / n2) % n1, b0 = blockIdx.x / (n2 * n1);
    const int o0 = b0 * T0, o1 = b1 * T1, o2 = b2 * T2;   // first output of the tile
    const long vol = (long)S0 * S1 * S2;
    const float *src = in + (long)blockIdx.y * vol;
    float *dst = out + (long)blockIdx.y * vol;

    for (int e = tid; e < TILE_IN; e += THREADS) {
        const int x = e % L2, y = (e / L2) % L1, z = e / (L2 * L1);
        const int g0 = o0 + z - HALO, g1 = o1 + y - HALO, g2 = o2 + x - HALO;
        const bool ok = g0 >= 0 && g0 < S0 && g1 >= 0 && g1 < S1 && g2 >= 0 && g2 < S2;
        tin[e] = ok ? src[((long)g0 * S1 + g1) * S2 + g2] : 0.f;
    }
    __syncthreads();

    const float third3 = 1.f / 27.f;
    {   // along S2: thread = (row group, x), rows are the 10 x 14 (z, y) pairs
        const int x = tid % T2, r0 = tid / T2;
        float w[7];
        walk_taps(o2 + x, S2, w);
        for (int r = r0; r < L0 * L1; r += THREADS / T2) {
            const float *p = tin + r * L2 + x;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 7; ++k) s += w[k] * p[k];
            ta[r * T2 + x] = s * third3;
        }
    }
    __syncthreads();
    {   // along S1: thread = (y, x), loop over the 10 planes; the result (10 x 8 x 32) goes where the loaded tile was
        const int x = tid % T2, y = tid / T2;
        float w[7];
        walk_taps(o1 + y, S1, w);
        for (int z = 0; z < L0; ++z) {
            const float *p = ta + (z * L1 + y) * T2 + x;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 7; ++k) s += w[k] * p[k * T2];
            tin[(z * T1 + y) * T2 + x] = s * third3;
        }
    }
    __syncthreads();
    {   // along S0: thread = (y, x), loop over the tile's planes, straight to global memory
        const int x = tid % T2, y = tid / T2;
        const int g1 = o1 + y, g2 = o2 + x;
        if (g1 < S1 && g2 < S2) {
            for (int z = 0; z < T0 && o0 + z < S0; ++z) {
                float w[7];
                walk_taps(o0 + z, S0, w);
                const float *p = tin + (z * T1 + y) * T2 + x;
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < 7; ++k) s += w[k] * p[k * T1 * T2];
                dst[((long)(o0 + z) * S1 + g1) * S2 + g2] = s * third3;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- objective
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

struct RegAxis {
    int i0;          // lower corner index; the upper one is i0 + 1 (either may lie outside 0 .. S - 1: that corner is dropped)
    float w0, w1;    // their weights; d weight / d t is -1 and +1
};

// t = i + u, u = disp * S / (S - 1).  The index comes from u clamped to +-(S + 2) (NaN -> the lower bound): wherever the clamp
// acts both corners are outside the volume, so it changes no result and no index leaves the int range.
__device__ __forceinline__ RegAxis reg_axis(int i, float d, int S, float unit) {
    const float lim = (float)(S + 2);
    const float u = fminf(fmaxf(d * unit, -lim), lim);
    const float f = floorf(u);
    RegAxis a;
    a.i0 = i + (int)f;
    a.w1 = u - f;
    a.w0 = 1.f - a.w1;
    return a;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = FSG_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, FSG_WAVE);
    return v;
}

struct RegParams {
    int C, Cp, S0, S1, S2, nblocks;
    float unit0, unit1, unit2;      // S_a / (S_a - 1): d t_a / d disp_a
    float gscale;                   // 2 cost_scale / (C nodes)
    double cscale;                  // cost_scale / (C nodes)
    double lam0, lam1, lam2;        // lambda / (3 (S_a - 1) S_b S_c); all three 0 when lambda == 0 (regulariser skipped)
};

__global__ __launch_bounds__(THREADS) void reg_objective_kernel(const float *__restrict__ disp, const _Float16 *__restrict__ ffix,
                                                                const _Float16 *__restrict__ fmov, RegParams P,
                                                                float *__restrict__ grad, double *__restrict__ partial) {
    __shared__ double red[2 * (THREADS / FSG_WAVE)];
    const int S0 = P.S0, S1 = P.S1, S2 = P.S2;
    const long nodes = (long)S0 * S1 * S2;
    const long n = (long)blockIdx.x * THREADS + threadIdx.x;
    const int b = blockIdx.y;
    float cost = 0.f;
    double reg = 0.0;
    if (n < nodes) {
        const int i2 = (int)(n % S2), i1 = (int)((n / S2) % S1), i0 = (int)(n / ((long)S2 * S1));
        const float *d = disp + (long)b * 3 * nodes + n;
        const float d0 = d[0], d1 = d[nodes], d2 = d[2 * nodes];
        const RegAxis a0 = reg_axis(i0, d0, S0, P.unit0), a1 = reg_axis(i1, d1, S1, P.unit1), a2 = reg_axis(i2, d2, S2, P.unit2);
        // corner k = 4 a + 2 b + c takes the upper index on S0 / S1 / S2 where a / b / c is set.  A dropped corner is never read
        // and its value is 0, so it gives nothing to the value or the gradient; the weights stay per axis (6 registers)
        long off[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j0 = a0.i0 + ((k >> 2) & 1), j1 = a1.i0 + ((k >> 1) & 1), j2 = a2.i0 + (k & 1);
            const bool ok = j0 >= 0 && j0 < S0 && j1 >= 0 && j1 < S1 && j2 >= 0 && j2 < S2;
            off[k] = ok ? (((long)j0 * S1 + j1) * S2 + j2) * P.Cp : -1;
        }
        const _Float16 *fx = ffix + ((long)b * nodes + n) * P.Cp;
        const _Float16 *mv = fmov + (long)b * nodes * P.Cp;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        for (int c0 = 0; c0 < P.Cp; c0 += 8) {
            const half8 f = *reinterpret_cast<const half8 *>(fx + c0);
            const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
            half8 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                v[k] = zero8;
                if (off[k] >= 0) v[k] = *reinterpret_cast<const half8 *>(mv + off[k] + c0);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // trilinear value and its three derivatives as a tree: along S2, then S1, then S0
                const float v0 = (float)v[0][j], v1 = (float)v[1][j], v2 = (float)v[2][j], v3 = (float)v[3][j];
                const float v4 = (float)v[4][j], v5 = (float)v[5][j], v6 = (float)v[6][j], v7 = (float)v[7][j];
                const float m00 = fmaf(a2.w1, v1, a2.w0 * v0), m01 = fmaf(a2.w1, v3, a2.w0 * v2);
                const float m10 = fmaf(a2.w1, v5, a2.w0 * v4), m11 = fmaf(a2.w1, v7, a2.w0 * v6);
                const float d00 = v1 - v0, d01 = v3 - v2, d10 = v5 - v4, d11 = v7 - v6;
                const float m0 = fmaf(a1.w1, m01, a1.w0 * m00), m1 = fmaf(a1.w1, m11, a1.w0 * m10);
                const float p0 = fmaf(a1.w1, d01, a1.w0 * d00), p1 = fmaf(a1.w1, d11, a1.w0 * d10);
                const float q0 = m01 - m00, q1 = m11 - m10;
                const float s = fmaf(a0.w1, m1, a0.w0 * m0);
                const float e0 = m1 - m0;
                const float e1 = fmaf(a0.w1, q1, a0.w0 * q0);
                const float e2 = fmaf(a0.w1, p1, a0.w0 * p0);
                const float diff = (c0 + j < P.C) ? s - (float)f[j] : 0.f;   // the pad channels are ignored
                cost = fmaf(diff, diff, cost);
                t0 = fmaf(diff, e0, t0);
                t1 = fmaf(diff, e1, t1);
                t2 = fmaf(diff, e2, t2);
            }
        }
        float gr0 = (P.gscale * P.unit0) * t0, gr1 = (P.gscale * P.unit1) * t1, gr2 = (P.gscale * P.unit2) * t2;

        if (P.lam0 != 0.0 || P.lam1 != 0.0 || P.lam2 != 0.0) {
            // forward differences belong to this node's share of the sum; the gradient needs the backward ones as well
            const float l0 = 2.f * (float)P.lam0, l1 = 2.f * (float)P.lam1, l2 = 2.f * (float)P.lam2;
            const long st0 = (long)S1 * S2, st1 = S2;
            float q0 = 0.f, q1 = 0.f, q2 = 0.f;
            auto channel = [&](const float *p, float c) -> float {
                const float f0 = i0 < S0 - 1 ? p[st0] - c : 0.f, r0 = i0 > 0 ? c - p[-st0] : 0.f;
                const float f1 = i1 < S1 - 1 ? p[st1] - c : 0.f, r1 = i1 > 0 ? c - p[-st1] : 0.f;
                const float f2 = i2 < S2 - 1 ? p[1] - c : 0.f, r2 = i2 > 0 ? c - p[-1] : 0.f;
                q0 = fmaf(f0, f0, q0);
                q1 = fmaf(f1, f1, q1);
                q2 = fmaf(f2, f2, q2);
                return (l0 * (r0 - f0) + l1 * (r1 - f1)) + l2 * (r2 - f2);
            };
            gr0 += channel(d, d0);
            gr1 += channel(d + nodes, d1);
            gr2 += channel(d + 2 * nodes, d2);
            reg = (P.lam0 * (double)q0 + P.lam1 * (double)q1) + P.lam2 * (double)q2;
        }
        float *g = grad + (long)b * 3 * nodes + n;
        g[0] = gr0;
        g[nodes] = gr1;
        g[2 * nodes] = gr2;
    }
    // the workgroup's pair: lanes in shuffle order, then the four waves in order
    const double cw = wave_sum_f64((double)cost), rw = wave_sum_f64(reg);
    const int wave = threadIdx.x / FSG_WAVE;
    if (threadIdx.x % FSG_WAVE == 0) {
        red[2 * wave] = cw;
        red[2 * wave + 1] = rw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0, r = 0.0;
        for (int w = 0; w < THREADS / FSG_WAVE; ++w) {
            c += red[2 * w];
            r += red[2 * w + 1];
        }
        double *o = partial + 2 * ((long)b * P.nblocks + blockIdx.x);
        o[0] = c;
        o[1] = r;
    }
}

// one workgroup per item: thread t adds the pairs t, t + 256, ... in order, then the 256 sums are added pairwise in LDS
__global__ __launch_bounds__(THREADS) void reg_objective_finish_kernel(const double *__restrict__ partial, int nblocks, double cscale,
                                                                       float *__restrict__ loss) {
    __shared__ double sc[THREADS], sr[THREADS];
    const double *p = partial + 2 * (long)blockIdx.x * nblocks;
    double c = 0.0, r = 0.0;
    for (int j = threadIdx.x; j < nblocks; j += THREADS) {
        c += p[2 * j];
        r += p[2 * j + 1];
    }
    sc[threadIdx.x] = c;
    sr[threadIdx.x] = r;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            sc[threadIdx.x] += sc[threadIdx.x + h];
            sr[threadIdx.x] += sr[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[2 * blockIdx.x] = (float)(cscale * sc[0]);
        loss[2 * blockIdx.x + 1] = (float)sr[0];
    }
}

int reg_check_grid(const char *entry, int B, int S0, int S1, int S2) {
    FSG_REQUIRE(B >= 1 && B <= 65535, "%s: bad shape: B=%d (1 .. 65535)", entry, B);
    FSG_REQUIRE(S0 >= 3 && S1 >= 3 && S2 >= 3, "%s: bad shape: grid %dx%dx%d, every axis must be >= 3 (avg_pool3d's own limit)", entry,
                S0, S1, S2);
    FSG_REQUIRE((long)S0 * S1 * S2 < (1L << 31), "%s: bad shape: grid %dx%dx%d, S0 S1 S2 must be < 2^31", entry, S0, S1, S2);
    return FSG_OK;
}

}   // namespace

extern "C" {

int fsg_reg_smooth3_f32(const float *in, int B, int C, int S0, int S1, int S2, float *out, fsg_stream_t stream) {
    FSG_REQUIRE(in && out, "fsg_reg_smooth3_f32: NULL pointer");
    FSG_REQUIRE(in != out, "fsg_reg_smooth3_f32: in and out must differ");
    if (int rc = reg_check_grid("fsg_reg_smooth3_f32", B, S0, S1, S2)) return rc;
    FSG_REQUIRE(C >= 1 && (long)B * C <= 65535, "fsg_reg_smooth3_f32: bad shape: B=%d C=%d (C >= 1, B C <= 65535)", B, C);
    const int n0 = fsg_cdiv(S0, T0), n1 = fsg_cdiv(S1, T1), n2 = fsg_cdiv(S2, T2);
    FSG_REQUIRE((long)n0 * n1 * n2 < (1L << 31), "fsg_reg_smooth3_f32: bad shape: too many tiles");
    reg_smooth3_kernel<<<dim3((unsigned)(n0 * n1 * n2), (unsigned)(B * C)), THREADS, 0, (hipStream_t)stream>>>(in, S0, S1, S2, n1, n2,
                                                                                                           out);
    FSG_CHECK_LAUNCH("fsg_reg_smooth3_f32");
    return FSG_OK;
}

size_t fsg_reg_objective_workspace_bytes(int B, int S0, int S1, int S2) {
    if (B < 1 || S0 < 1 || S1 < 1 || S2 < 1 || (long)S0 * S1 * S2 >= (1L << 31)) return 0;
    return (size_t)B * fsg_cdiv((long)S0 * S1 * S2, THREADS) * 2 * sizeof(double);
}

int fsg_reg_objective_f16(const float *disp, const void *feat_fix, const void *feat_mov, int B, int C, int Cp, int S0, int S1, int S2,
                          float lambda, float cost_scale, float *grad_disp, float *loss, void *workspace, size_t workspace_bytes,
                          fsg_stream_t stream) {
    FSG_REQUIRE(disp && feat_fix && feat_mov && grad_disp && loss && workspace, "fsg_reg_objective_f16: NULL pointer");
    if (int rc = reg_check_grid("fsg_reg_objective_f16", B, S0, S1, S2)) return rc;
    FSG_REQUIRE(C >= 1 && Cp >= C && Cp % 8 == 0 && Cp <= 4096,
                "fsg_reg_objective_f16: bad shape: C=%d Cp=%d (1 <= C <= Cp <= 4096, Cp a multiple of 8)", C, Cp);
    FSG_REQUIRE((((uintptr_t)feat_fix | (uintptr_t)feat_mov) & 15) == 0,
                "fsg_reg_objective_f16: the feature volumes must be 16-byte aligned");
    FSG_REQUIRE(((uintptr_t)workspace & 7) == 0, "fsg_reg_objective_f16: workspace must be 8-byte aligned");
    const size_t need = fsg_reg_objective_workspace_bytes(B, S0, S1, S2);
    FSG_REQUIRE(workspace_bytes >= need, "fsg_reg_objective_f16: workspace of %zu bytes, need %zu", workspace_bytes, need);
    const long nodes = (long)S0 * S1 * S2;
    RegParams P;
    P.C = C, P.Cp = Cp, P.S0 = S0, P.S1 = S1, P.S2 = S2;
    P.nblocks = fsg_cdiv(nodes, THREADS);
    P.unit0 = (float)((double)S0 / (S0 - 1)), P.unit1 = (float)((double)S1 / (S1 - 1)), P.unit2 = (float)((double)S2 / (S2 - 1));
    P.cscale = (double)cost_scale / ((double)C * (double)nodes);
    P.gscale = (float)(2.0 * P.cscale);
    const double lam = (double)lambda;   // lambda == 0: the regulariser is skipped, reg = 0 whatever the field holds
    P.lam0 = lambda == 0.f ? 0.0 : lam / (3.0 * (S0 - 1) * (double)S1 * S2);
    P.lam1 = lambda == 0.f ? 0.0 : lam / (3.0 * (S1 - 1) * (double)S0 * S2);
    P.lam2 = lambda == 0.f ? 0.0 : lam / (3.0 * (S2 - 1) * (double)S0 * S1);
    hipStream_t s = (hipStream_t)stream;
    reg_objective_kernel<<<dim3((unsigned)P.nblocks, (unsigned)B), THREADS, 0, s>>>(disp, (const _Float16 *)feat_fix,
                                                                                   (const _Float16 *)feat_mov, P, grad_disp,
                                                                                   (double *)workspace);
    FSG_CHECK_LAUNCH("fsg_reg_objective_f16");
    reg_objective_finish_kernel<<<dim3((unsigned)B), THREADS, 0, s>>>((const double *)workspace, P.nblocks, P.cscale, loss);
    FSG_CHECK_LAUNCH("fsg_reg_objective_f16 (finish)");
    return FSG_OK;
}

}   // extern "C"
