// Voxel patch augmentation and resampling -- include/fsg_hip.h: fsg_bspline_prefilter_axis_f32, fsg_gauss_axis_f32,
// fsg_spatial_resample_f32.  Stands where the reference's ImageDataset.__getitem__ (data.py:290-327) calls batchgenerators'
// SpatialTransform + MirrorTransform (augmentations.py:29-49: scipy's gaussian_filter for the elastic field, map_coordinates
// for the patch), sitk.Resample (utils/image_ops.py:12-28) and normalize_img (data.py:365-366).
//
// Three kernels, all fp32, one thread per line (prefilter), per four outputs of a line (Gauss) or per output voxel (resample),
// no atomics, no host read, sums in a fixed order: the same input gives the same bits, and an item does not depend on the rest of its batch.
//
// Cubic B-spline prefilter, one axis per launch.  A line of n samples is extended by PAD = 12 edge-replicated samples on both
//   sides (scipy's own padding for mode='nearest') and filtered as scipy.ndimage.spline_filter1d(order=3, mode='nearest')
//   filters it: gain 6, pole z = sqrt(3) - 2, the causal recursion c[j] += z c[j-1] from the whole-sample-symmetric start
//   c[0] += sum_i z^(i+1) c[i], the anticausal recursion c[j] = z (c[j+1] - c[j]) from c[last] *= z / (z - 1).  The start
//   sum stops after 32 terms (z^32 = 5e-19) and drops the z^n terms of the far end (n >= 25: below 5e-15).  The recursion
//   runs in the output line itself (a thread reads back only what it wrote).  Neighbouring threads own neighbouring lines, so
//   the H and D passes are coalesced; the W pass is not (64 rows per wave, one cache line each, reused for 32 steps).
//
// Gaussian smoothing of the elastic noise, one axis per launch, all items and components in it: the taps of
//   scipy.ndimage.gaussian_filter1d -- radius r = int(4 sigma + 0.5), exp(-0.5 k^2 / sigma^2) normalised by their sum --
//   are built per workgroup in LDS from the item's sigma (a device value); mode='constant', cval=0: taps outside the line
//   are skipped, so r may exceed the line.  An item whose sigma is not in (0, 255] gives NaN.
//
// Fused resample: for output voxel o of item b the source coordinate is M_b ((o - (patch - 1)/2) + elastic_b(o)) + centre_b in
//   voxel units, axes (D, H, W); the image patch (orders 0, 1, 3; edge-replicated), the label patch (orders 0, 1; 0 outside
//   [0, n-1]), the mirror flags (folded into the store index) and the intensity map a x + b (folded into the store) in one
//   launch.  Order 3 reads the coefficients above: 64 taps, separable weights, the coordinate moved by PAD, tap indices
//   clamped to the padded array (so beyond the padding the value runs into the edge coefficient within two samples) -- what
//   scipy's map_coordinates(order=3, mode='nearest') does.  Every coordinate is bounded before it becomes an index (a NaN
//   coordinate takes the lower bound) and every index is clamped, so no read leaves the arrays.
#include "fsg_common.h"

namespace {

constexpr int NT = 256;
constexpr int PAD = FSG_BSPLINE_PAD;
constexpr int MAX_GRID = 1 << 16;
constexpr int MAX_RADIUS = 1020;          // int(4 * 255 + 0.5)
constexpr float MAX_SIGMA = FSG_ELASTIC_MAX_SIGMA;
constexpr int GB = 4;                    // outputs per thread along the filtered axis
constexpr float POLE = -0.26794919243112270647f;   // sqrt(3) - 2

// ---------------------------------------------------------------------------------------------------- prefilter
__global__ __launch_bounds__(NT) void prefilter_axis_kernel(long lines, int n, long inner, const float *__restrict__ in,
                                                            float *__restrict__ out) {
    const int np = n + 2 * PAD;
    for (long t = (long)blockIdx.x * NT + threadIdx.x; t < lines; t += (long)gridDim.x * NT) {
        const long o = t / inner, s = t - o * inner;
        const float *src = in + o * n * inner + s;
        float *dst = out + o * np * inner + s;
        // the causal start: c0 + sum_{i < 32} z^(i+1) c[i]  (np >= 25, so every term exists up to i = 24; stop at np)
        const float first = 6.f * src[0];
        float zi = POLE, sum = 0.f;
        const int terms = np < 32 ? np : 32;
        for (int i = 0; i < terms; ++i) {
            const int j = clampi(i - PAD, n - 1);
            sum += zi * (6.f * src[(long)j * inner]);
            zi *= POLE;
        }
        float c = first + sum;
        dst[0] = c;
        for (int i = 1; i < np; ++i) {
            const int j = clampi(i - PAD, n - 1);
            c = 6.f * src[(long)j * inner] + POLE * c;
            dst[(long)i * inner] = c;
        }
        c *= POLE / (POLE - 1.f);
        dst[(long)(np - 1) * inner] = c;
        for (int i = np - 2; i >= 0; --i) {
            c = POLE * (c - dst[(long)i * inner]);
            dst[(long)i * inner] = c;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- elastic field
// in / out (B, outer, n, inner); grid (x, B).  A thread owns GB consecutive outputs of one line and walks once over the
// samples they touch: one load and one tap read per sample serve GB sums (the taps slide through registers).  Neighbouring
// threads own neighbouring lines (inner > 1: coalesced) or neighbouring output groups of a row (inner == 1: lanes GB apart).
// Each sum still adds its in-range samples in ascending order.  taps: 2 r + 1 floats of LDS between GB zeros.
__global__ __launch_bounds__(NT) void gauss_axis_kernel(long outer, int n, long inner, const float *__restrict__ sigma,
                                                        const float *__restrict__ alpha, const float *__restrict__ in,
                                                        float *__restrict__ out) {
    __shared__ float table[2 * MAX_RADIUS + 1 + 2 * GB];
    __shared__ float total;
    float *taps = table + GB;
    const int b = blockIdx.y;
    const float sg = sigma[b];
    const bool ok = sg > 0.f && sg <= MAX_SIGMA;
    const int r = ok ? (int)(4.0 * (double)sg + 0.5) : 0;
    const int ntaps = 2 * r + 1;
    const float f = -0.5f / (sg * sg);
    if (threadIdx.x < GB) table[threadIdx.x] = taps[ntaps + threadIdx.x] = 0.f;
    for (int k = threadIdx.x; k < ntaps; k += NT) {
        const float d = (float)(k - r);
        taps[k] = expf(f * (d * d));
    }
    __syncthreads();
    if (threadIdx.x < 64) {       // the normalising sum: lane l adds taps l, l + 64, ... in order, then the fixed ladder
        float part = 0.f;
        for (int k = threadIdx.x; k < ntaps; k += 64) part += taps[k];
        part = wave_sum_bcast_f(part);
        if (threadIdx.x == 0) total = part;
    }
    __syncthreads();
    const float tot = total;
    for (int k = threadIdx.x; k < ntaps; k += NT) taps[k] = taps[k] / tot;      // (each thread divides what it wrote)
    __syncthreads();
    const float scale = alpha ? alpha[b] : 1.f;
    const float bad = ok ? 0.f : __builtin_nanf("");
    const long per_item = outer * n * inner;
    const float *src = in + (long)b * per_item;
    float *dst = out + (long)b * per_item;
    const int groups = (n + GB - 1) / GB;
    const long work = outer * groups * inner;
    for (long e = (long)blockIdx.x * NT + threadIdx.x; e < work; e += (long)gridDim.x * NT) {
        const long s = e % inner, rest = e / inner;
        const int i0 = (int)(rest % groups) * GB;
        const long base = (rest / groups) * n * inner + s;
        const int jlo = i0 - r > 0 ? i0 - r : 0;
        const int jhi = i0 + GB - 1 + r < n - 1 ? i0 + GB - 1 + r : n - 1;
        float acc[GB], w[GB];
        int t = jlo - i0 + r;                      // the tap of sample j for output i0: j - i0 + r; for i0 + m: that - m
#pragma unroll
        for (int m = 0; m < GB; ++m) {
            acc[m] = bad;
            w[m] = taps[t - m];                    // t - m >= -(GB - 1): inside the zero border
        }
        for (int j = jlo; j <= jhi; ++j, ++t) {
            const float v = src[base + (long)j * inner];
#pragma unroll
            for (int m = 0; m < GB; ++m)
                acc[m] = (unsigned)(t - m) < (unsigned)ntaps ? fmaf(w[m], v, acc[m]) : acc[m];
#pragma unroll
            for (int m = GB - 1; m > 0; --m) w[m] = w[m - 1];
            w[0] = taps[t + 1];                    // t + 1 <= 2 r + GB: inside the zero border
        }
#pragma unroll
        for (int m = 0; m < GB; ++m)
            if (i0 + m < n) dst[base + (long)(i0 + m) * inner] = alpha ? scale * acc[m] : acc[m];
    }
}

// ---------------------------------------------------------------------------------------------------- fused resample
struct ResampleArgs {
    const float *src;      // (B, C, D + 2 pad, H + 2 pad, W + 2 pad), or NULL
    const void *seg;       // (B, Cs, D, H, W), or NULL
    const float *matrix;   // (B, 9)
    const float *centre;   // (B, 3)
    const float *elastic;  // (B, 3, P) or NULL
    const uint8_t *mirror; // (B, 3) or NULL
    float *out_img;        // (B, C, P)
    int64_t *out_seg;      // (B, Cs, P)
    int C, Cs, seg_kind, order_seg, pad;
    int D, H, W, pd, ph, pw;
    float ia, ib;
};

__device__ __forceinline__ int load_label(const void *p, int kind, long i) {
    if (kind == FSG_LABEL_U8) return ((const uint8_t *)p)[i];
    if (kind == FSG_LABEL_I32) return ((const int32_t *)p)[i];
    return (int)((const int64_t *)p)[i];
}

// a coordinate clamped to [0, hi] (NaN -> 0), its floor as an index and the fraction
__device__ __forceinline__ float clamp_coord(float x, int hi) { return fminf(fmaxf(x, 0.f), (float)hi); }

// a coordinate in the padded coefficient array, kept within two samples of it (NaN -> -2): further out every tap is the
// edge coefficient anyway
__device__ __forceinline__ float spline_coord(float x, int np) { return fminf(fmaxf(x + (float)PAD, -2.f), (float)(np + 1)); }

// scipy's cubic B-spline weights for the taps floor(x) - 1 .. floor(x) + 2 at fraction t
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
    const float u = 1.f - t;
    w[0] = u * u * u / 6.f;
    w[1] = (t * t * (t - 2.f) * 3.f + 4.f) / 6.f;
    w[2] = (u * u * (u - 2.f) * 3.f + 4.f) / 6.f;
    w[3] = t * t * t / 6.f;
}

template <int ORDER>
__global__ __launch_bounds__(NT) void resample_kernel(const ResampleArgs a) {
    const int b = blockIdx.y;
    const long P = (long)a.pd * a.ph * a.pw;
    const float *m = a.matrix + b * 9, *ctr = a.centre + b * 3;
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    const float c0 = ctr[0], c1 = ctr[1], c2 = ctr[2];
    const float h0 = 0.5f * (float)(a.pd - 1), h1 = 0.5f * (float)(a.ph - 1), h2 = 0.5f * (float)(a.pw - 1);
    const bool f0 = a.mirror && a.mirror[b * 3 + 0], f1 = a.mirror && a.mirror[b * 3 + 1], f2 = a.mirror && a.mirror[b * 3 + 2];
    const int Dp = a.D + 2 * a.pad, Hp = a.H + 2 * a.pad, Wp = a.W + 2 * a.pad;
    const long SV = (long)Dp * Hp * Wp, LV = (long)a.D * a.H * a.W;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < P; v += (long)gridDim.x * NT) {
        const int ox = (int)(v % a.pw), oy = (int)((v / a.pw) % a.ph), oz = (int)(v / ((long)a.pw * a.ph));
        float p0 = (float)oz - h0, p1 = (float)oy - h1, p2 = (float)ox - h2;
        if (a.elastic) {
            const float *e = a.elastic + (long)b * 3 * P + v;
            p0 += e[0];
            p1 += e[P];
            p2 += e[2 * P];
        }
        const float x0 = ((m00 * p0 + m01 * p1) + m02 * p2) + c0;
        const float x1 = ((m10 * p0 + m11 * p1) + m12 * p2) + c1;
        const float x2 = ((m20 * p0 + m21 * p1) + m22 * p2) + c2;
        const long ov = ((long)(f0 ? a.pd - 1 - oz : oz) * a.ph + (f1 ? a.ph - 1 - oy : oy)) * a.pw + (f2 ? a.pw - 1 - ox : ox);
        if (a.src) {
            const float *sb = a.src + (long)b * a.C * SV;
            float *ob = a.out_img + (long)b * a.C * P + ov;
            if (ORDER == 3) {
                const float q0 = spline_coord(x0, Dp), q1 = spline_coord(x1, Hp), q2 = spline_coord(x2, Wp);
                const float g0 = floorf(q0), g1 = floorf(q1), g2 = floorf(q2);
                float w0[4], w1[4], w2[4];
                cubic_weights(q0 - g0, w0);
                cubic_weights(q1 - g1, w1);
                cubic_weights(q2 - g2, w2);
                int iz[4], iy[4], ix[4];       // offsets inside one channel: below 2^31 (checked on the host)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    iz[j] = clampi((int)g0 - 1 + j, Dp - 1) * Hp * Wp;
                    iy[j] = clampi((int)g1 - 1 + j, Hp - 1) * Wp;
                    ix[j] = clampi((int)g2 - 1 + j, Wp - 1);
                }
                for (int c = 0; c < a.C; ++c) {
                    const float *s = sb + c * SV;
                    float acc = 0.f;
#pragma unroll
                    for (int jz = 0; jz < 4; ++jz) {
                        float az = 0.f;
#pragma unroll
                        for (int jy = 0; jy < 4; ++jy) {
                            const float *row = s + (iz[jz] + iy[jy]);
                            const float ax = ((w2[0] * row[ix[0]] + w2[1] * row[ix[1]]) + w2[2] * row[ix[2]]) + w2[3] * row[ix[3]];
                            az += w1[jy] * ax;
                        }
                        acc += w0[jz] * az;
                    }
                    ob[c * P] = a.ia * acc + a.ib;
                }
            } else if (ORDER == 1) {
                const float q0 = clamp_coord(x0, a.D - 1), q1 = clamp_coord(x1, a.H - 1), q2 = clamp_coord(x2, a.W - 1);
                const float g0 = floorf(q0), g1 = floorf(q1), g2 = floorf(q2);
                const float t0 = q0 - g0, t1 = q1 - g1, t2 = q2 - g2;
                const int z0 = (int)g0, y0 = (int)g1, xx0 = (int)g2;
                const int z1 = z0 + 1 < a.D ? z0 + 1 : z0, y1 = y0 + 1 < a.H ? y0 + 1 : y0, xx1 = xx0 + 1 < a.W ? xx0 + 1 : xx0;
                for (int c = 0; c < a.C; ++c) {
                    const float *s = sb + c * SV;
                    const float *r00 = s + ((long)z0 * a.H + y0) * a.W, *r01 = s + ((long)z0 * a.H + y1) * a.W;
                    const float *r10 = s + ((long)z1 * a.H + y0) * a.W, *r11 = s + ((long)z1 * a.H + y1) * a.W;
                    const float a00 = r00[xx0] * (1.f - t2) + r00[xx1] * t2, a01 = r01[xx0] * (1.f - t2) + r01[xx1] * t2;
                    const float a10 = r10[xx0] * (1.f - t2) + r10[xx1] * t2, a11 = r11[xx0] * (1.f - t2) + r11[xx1] * t2;
                    const float b0 = a00 * (1.f - t1) + a01 * t1, b1 = a10 * (1.f - t1) + a11 * t1;
                    ob[c * P] = a.ia * (b0 * (1.f - t0) + b1 * t0) + a.ib;
                }
            } else {
                const int z = (int)floorf(clamp_coord(x0, a.D - 1) + 0.5f), y = (int)floorf(clamp_coord(x1, a.H - 1) + 0.5f),
                          x = (int)floorf(clamp_coord(x2, a.W - 1) + 0.5f);
                for (int c = 0; c < a.C; ++c) ob[c * P] = a.ia * sb[c * SV + ((long)z * a.H + y) * a.W + x] + a.ib;
            }
        }
        if (a.seg) {
            // scipy's mode='constant': a coordinate outside [0, n - 1] on any axis gives 0 (a NaN fails every comparison)
            const bool inside = x0 >= 0.f && x0 <= (float)(a.D - 1) && x1 >= 0.f && x1 <= (float)(a.H - 1) && x2 >= 0.f &&
                                x2 <= (float)(a.W - 1);
            int64_t *ob = a.out_seg + (long)b * a.Cs * P + ov;
            if (!inside) {
                for (int c = 0; c < a.Cs; ++c) ob[c * P] = 0;
            } else if (a.order_seg == 0) {
                const int z = clampi((int)floorf(x0 + 0.5f), a.D - 1), y = clampi((int)floorf(x1 + 0.5f), a.H - 1),
                          x = clampi((int)floorf(x2 + 0.5f), a.W - 1);
                for (int c = 0; c < a.Cs; ++c)
                    ob[c * P] = load_label(a.seg, a.seg_kind, ((long)b * a.Cs + c) * LV + ((long)z * a.H + y) * a.W + x);
            } else {
                // per label: the trilinear weight it holds among the 8 corners; the largest label at 0.5 or more wins, else 0
                const float g0 = floorf(x0), g1 = floorf(x1), g2 = floorf(x2);
                const float t0 = x0 - g0, t1 = x1 - g1, t2 = x2 - g2;
                const int zc[2] = {(int)g0, (int)g0 + 1 < a.D ? (int)g0 + 1 : (int)g0};
                const int yc[2] = {(int)g1, (int)g1 + 1 < a.H ? (int)g1 + 1 : (int)g1};
                const int xc[2] = {(int)g2, (int)g2 + 1 < a.W ? (int)g2 + 1 : (int)g2};
                const float wz[2] = {1.f - t0, t0}, wy[2] = {1.f - t1, t1}, wx[2] = {1.f - t2, t2};
                float w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = wz[j >> 2] * wy[(j >> 1) & 1] * wx[j & 1];
                for (int c = 0; c < a.Cs; ++c) {
                    const long base = ((long)b * a.Cs + c) * LV;
                    int lab[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        lab[j] = load_label(a.seg, a.seg_kind, base + ((long)zc[j >> 2] * a.H + yc[(j >> 1) & 1]) * a.W + xc[j & 1]);
                    int best = 0;
                    bool any = false;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float s = 0.f;
#pragma unroll
                        for (int j = 0; j < 8; ++j) s += lab[j] == lab[i] ? w[j] : 0.f;
                        if (s >= 0.5f && (!any || lab[i] > best)) {
                            best = lab[i];
                            any = true;
                        }
                    }
                    ob[c * P] = any ? best : 0;
                }
            }
        }
    }
}

inline int grid_for(long items) {
    const long n = (items + NT - 1) / NT;
    return (int)(n < 1 ? 1 : (n > MAX_GRID ? MAX_GRID : n));
}

}  // namespace

extern "C" int fsg_bspline_prefilter_axis_f32(const float *in, int64_t outer, int n, int64_t inner, float *out,
                                              fsg_stream_t stream) {
    const char *name = "fsg_bspline_prefilter_axis_f32";
    FSG_REQUIRE(outer > 0 && n > 0 && inner > 0, "%s: bad shape outer=%ld n=%d inner=%ld", name, (long)outer, n, (long)inner);
    FSG_REQUIRE(n <= (1 << 20) && (double)outer * (n + 2 * PAD) * (double)inner < 4611686018427387904.0,
                "%s: outer=%ld n=%d inner=%ld is too large", name, (long)outer, n, (long)inner);
    FSG_REQUIRE(in && out && in != out, "%s: NULL pointer or in == out", name);
    const long lines = (long)outer * inner;
    prefilter_axis_kernel<<<grid_for(lines), NT, 0, (hipStream_t)stream>>>(lines, n, (long)inner, in, out);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_gauss_axis_f32(const float *in, int B, int64_t outer, int n, int64_t inner, const float *sigma,
                                  const float *alpha, float *out, fsg_stream_t stream) {
    const char *name = "fsg_gauss_axis_f32";
    FSG_REQUIRE(B > 0 && B <= 65535 && outer > 0 && n > 0 && inner > 0, "%s: bad shape B=%d outer=%ld n=%d inner=%ld", name, B,
                (long)outer, n, (long)inner);
    FSG_REQUIRE((double)outer * n * (double)inner < 2147483648.0, "%s: outer n inner = %ld %d %ld is 2^31 values or more per item",
                name, (long)outer, n, (long)inner);
    FSG_REQUIRE(in && out && sigma && in != out, "%s: NULL pointer or in == out", name);
    const long work = (long)outer * ((n + GB - 1) / GB) * inner;
    long gx = (work + NT - 1) / NT;
    if (gx > 2048) gx = 2048;       // grid-strided: the taps are built once per workgroup
    gauss_axis_kernel<<<dim3((unsigned)gx, (unsigned)B), NT, 0, (hipStream_t)stream>>>((long)outer, n, (long)inner, sigma, alpha, in,
                                                                                       out);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_spatial_resample_f32(const float *src, int C, int order_data, const void *seg, int seg_kind, int Cs,
                                        int order_seg, int B, int D, int H, int W, int pd, int ph, int pw, const float *matrix,
                                        const float *centre, const float *elastic, const uint8_t *mirror, float ia, float ib,
                                        float *out_img, int64_t *out_seg, fsg_stream_t stream) {
    const char *name = "fsg_spatial_resample_f32";
    FSG_REQUIRE(B > 0 && B <= 65535 && D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0,
                "%s: bad shape B=%d volume %d %d %d patch %d %d %d", name, B, D, H, W, pd, ph, pw);
    FSG_REQUIRE((double)(D + 2 * PAD) * (H + 2 * PAD) * (W + 2 * PAD) < 2147483648.0 && (double)pd * ph * pw < 2147483648.0,
                "%s: volume %d %d %d (padded) or patch %d %d %d is 2^31 voxels or more", name, D, H, W, pd, ph, pw);
    FSG_REQUIRE(src || seg, "%s: neither an image nor a label map", name);
    FSG_REQUIRE(matrix && centre, "%s: NULL pointer", name);
    if (src) {
        FSG_REQUIRE(order_data == 0 || order_data == 1 || order_data == 3, "%s: order_data=%d (0, 1 or 3)", name, order_data);
        FSG_REQUIRE(C > 0 && out_img, "%s: C=%d or a NULL image output", name, C);
    }
    if (seg) {
        FSG_REQUIRE(order_seg == 0 || order_seg == 1, "%s: order_seg=%d (0 or 1)", name, order_seg);
        FSG_REQUIRE(seg_kind == FSG_LABEL_U8 || seg_kind == FSG_LABEL_I32 || seg_kind == FSG_LABEL_I64, "%s: seg_kind=%d", name,
                    seg_kind);
        FSG_REQUIRE(Cs > 0 && out_seg, "%s: Cs=%d or a NULL label output", name, Cs);
    }
    ResampleArgs a;
    a.src = src, a.seg = seg, a.matrix = matrix, a.centre = centre, a.elastic = elastic, a.mirror = mirror;
    a.out_img = out_img, a.out_seg = out_seg;
    a.C = C, a.Cs = Cs, a.seg_kind = seg_kind, a.order_seg = order_seg, a.pad = (src && order_data == 3) ? PAD : 0;
    a.D = D, a.H = H, a.W = W, a.pd = pd, a.ph = ph, a.pw = pw;
    a.ia = ia, a.ib = ib;
    const dim3 grid((unsigned)grid_for((long)pd * ph * pw), (unsigned)B);
    const int order = src ? order_data : 0;
    if (order == 3) resample_kernel<3><<<grid, NT, 0, (hipStream_t)stream>>>(a);
    else if (order == 1) resample_kernel<1><<<grid, NT, 0, (hipStream_t)stream>>>(a);
    else resample_kernel<0><<<grid, NT, 0, (hipStream_t)stream>>>(a);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}
