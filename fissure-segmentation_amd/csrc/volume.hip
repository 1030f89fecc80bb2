// Image front end on a single-channel fp32 volume -- include/fsg_hip.h: fsg_foerstner_dist_f32, fsg_nms_keypoints,
// fsg_mind_stats_f32, fsg_mind_eval_f32, fsg_mind_eval_kp_f32.
// Replaces the torch compositions of data_processing/foerstner.py:62-108 and data_processing/point_features.py:86-150.
//
// One skeleton serves the Foerstner distinctiveness and the MIND descriptors: "NCH channels that are pointwise functions of a
// source tile, smoothed by the separable Gaussian of utils/image_utils.py:22-35 (axis order 0, 1, 2, replicate padding),
// then a pointwise epilogue".  A workgroup owns a TZ x TY x TX output tile:
//   fill    the source tile goes to LDS once, halo included: the three 5-tap gradients (distinctiveness, halo R = N / 2) or
//           the image itself (MIND, halo R + dilation).  Tile coordinate c holds the value AT clamp(c): replicate padding of
//           the gradient / squared-difference VOLUME, whose own stencil is then taken around the clamped position (a second
//           clamp; clamping the image index once gives different border values).
//   plane   per output plane z: (A) the channels are formed on the fly and smoothed along z into a (TY + 2R) x (TX + 2R)
//           plane, (B) smoothed along y, (C) smoothed along x into registers and handed to the epilogue.
// The three gradient volumes, the six product volumes, the twelve squared-difference volumes and every partially smoothed
// volume of the torch composition stay in LDS; HBM sees the image (plus halo re-reads, mostly L2 hits) and the output.
// Sums run in a fixed order (taps ascending, channels ascending) and the build keeps -ffp-contract=off, so the keypoint
// variant of the MIND evaluation (a 1 x 1 x 1 tile per keypoint through the same code) is bitwise the volume variant.
//
// The non-maximum suppression is its own kernel: distinctiveness tile + window halo in LDS, separable NaN-propagating
// running maximum (x, y, z), then mask_eroded & (max == D) & (D >= thresh) as a byte flag per voxel.
#include "fsg_common.h"

namespace {

constexpr int MAXR = FSG_FRONTEND_MAX_TAP_RADIUS;   // Gaussian radius N / 2 (sigma <= 2.66)
constexpr int MAXN = 2 * MAXR + 1;
constexpr int MAXCH = 12;
constexpr int MAXDIL = 4;
constexpr int MAXNMS = 13;             // largest suppression window
constexpr size_t LDS_MAX = 160 * 1024;

enum { DIST = 0, MIND_STATS = 1, MIND_EVAL = 2, MIND_KP = 3 };

struct VolArgs {
    int B, D, H, W, R, dil, box;
    float w[MAXN];
    int s1[MAXCH][3], s2[MAXCH][3];   // MIND: the two voxels of every channel's pair, offsets in {-1, 0, 1}
    unsigned m1[MAXCH], m2[MAXCH];    // MIND, box form: the operands as 27-bit subsets of the stencil, bit (kz * 3 + ky) * 3 + kx
    int outch[MAXCH];                 // MIND: output position of channel c
};


template <int MODE, int NCH, int TZ, int TY, int TX, int NT>
__global__ __launch_bounds__(NT) void vol_kernel(VolArgs a, const float *__restrict__ img, float *__restrict__ out,
                                                 const int64_t *__restrict__ kp, int K, const float *__restrict__ meanp,
                                                 float *__restrict__ partial) {
    extern __shared__ __align__(16) float lds[];
    constexpr int SCH = MODE == DIST ? 3 : 1;
    const int tid = threadIdx.x, R = a.R, N = 2 * R + 1, D = a.D, H = a.H, W = a.W;
    const int HS = MODE == DIST ? R : R + a.dil;
    const int SZ = TZ + 2 * HS, SY = TY + 2 * HS, SX = TX + 2 * HS, S3 = SZ * SY * SX;
    const int AY = TY + 2 * R, AX = TX + 2 * R;
    float *src = lds;                       // [SCH][SZ][SY][SX]
    float *bufA = src + SCH * S3;           // [NCH][AY][AX]
    float *bufB = bufA + NCH * AY * AX;     // [NCH][TY][AX]
    int b = 0, z0, y0, x0;
    if (MODE == MIND_KP) {
        z0 = clampi((int)kp[(long)blockIdx.x * 3], D - 1);
        y0 = clampi((int)kp[(long)blockIdx.x * 3 + 1], H - 1);
        x0 = clampi((int)kp[(long)blockIdx.x * 3 + 2], W - 1);
    } else {
        const int ntz = (D + TZ - 1) / TZ;
        b = blockIdx.z / ntz;
        z0 = (blockIdx.z % ntz) * TZ;
        y0 = blockIdx.y * TY;
        x0 = blockIdx.x * TX;
    }
    const float *vol = img + (long)b * D * H * W;

    for (int e = tid; e < S3; e += NT) {
        const int sx = e % SX, sy = (e / SX) % SY, sz = e / (SX * SY);
        const int qz = clampi(z0 - HS + sz, D - 1), qy = clampi(y0 - HS + sy, H - 1), qx = clampi(x0 - HS + sx, W - 1);
        if (MODE == DIST) {   // foerstner.py:65-68: [1, -8, 0, 8, -1] / 12 around the clamped position, replicate padding
            const float c0 = (float)(1.0 / 12.0), c1 = (float)(-8.0 / 12.0), c3 = (float)(8.0 / 12.0), c4 = (float)(-1.0 / 12.0);
            const float *pz = vol + (long)qy * W + qx, *py = vol + (long)qz * H * W + qx, *px = vol + ((long)qz * H + qy) * W;
            const long hw = (long)H * W;
            // outer pair + inner pair: the antisymmetric taps cancel exactly where the image is constant, so the gradient
            // is exactly 0 there (and the distinctiveness NaN) whatever the constant is
            src[e] = (c0 * pz[clampi(qz - 2, D - 1) * hw] + c4 * pz[clampi(qz + 2, D - 1) * hw]) +
                     (c1 * pz[clampi(qz - 1, D - 1) * hw] + c3 * pz[clampi(qz + 1, D - 1) * hw]);
            src[e + S3] = (c0 * py[(long)clampi(qy - 2, H - 1) * W] + c4 * py[(long)clampi(qy + 2, H - 1) * W]) +
                          (c1 * py[(long)clampi(qy - 1, H - 1) * W] + c3 * py[(long)clampi(qy + 1, H - 1) * W]);
            src[e + 2 * S3] = (c0 * px[clampi(qx - 2, W - 1)] + c4 * px[clampi(qx + 2, W - 1)]) +
                              (c1 * px[clampi(qx - 1, W - 1)] + c3 * px[clampi(qx + 1, W - 1)]);
        } else {
            src[e] = vol[((long)qz * H + qy) * W + qx];
        }
    }
    __syncthreads();

    float accum = 0.f;   // MIND_STATS: this thread's share of sum over voxels of mean_c(ssd - min_c ssd)
    for (int z = 0; z < TZ; ++z) {
        if (MODE != MIND_KP && z0 + z >= D) break;   // uniform over the workgroup
        // (A) channels on the fly, smoothed along z
        for (int p = tid; p < AY * AX; p += NT) {
            const int ay = p / AX, ax = p % AX;
            float acc[NCH];
            int sy = ay, sx = ax;
            if (MODE != DIST) {   // source coordinate of the CLAMPED position (the squared-difference volume is replicated)
                sy = clampi(y0 + ay - R, H - 1) - (y0 - HS);
                sx = clampi(x0 + ax - R, W - 1) - (x0 - HS);
            }
            for (int i = 0; i < N; ++i) {
                float v[NCH];
                if (MODE == DIST) {
                    const int idx = ((z + i) * SY + sy) * SX + sx;
                    const float g0 = src[idx], g1 = src[idx + S3], g2 = src[idx + 2 * S3];
                    v[0] = g0 * g0; v[1] = g0 * g1; v[2] = g0 * g2; v[3] = g1 * g1; v[4] = g1 * g2; v[NCH - 1] = g2 * g2;
                } else {
                    const int sz = clampi(z0 + z + i - R, D - 1) - (z0 - HS);
                    const int idx = (sz * SY + sy) * SX + sx, dil = a.dil;
                    if (a.box) {   // general form: both operands are sums over subsets of the dilated 3 x 3 x 3 stencil
                        float u[NCH], t[NCH];
#pragma unroll
                        for (int c = 0; c < NCH; ++c) u[c] = t[c] = 0.f;
                        for (int k = 0; k < 27; ++k) {
                            const float sv = src[idx + (((k / 9 - 1) * SY + (k / 3 % 3 - 1)) * SX + (k % 3 - 1)) * dil];
#pragma unroll
                            for (int c = 0; c < NCH; ++c) {
                                if ((a.m1[c] >> k) & 1u) u[c] += sv;
                                if ((a.m2[c] >> k) & 1u) t[c] += sv;
                            }
                        }
#pragma unroll
                        for (int c = 0; c < NCH; ++c) { const float d = u[c] - t[c]; v[c] = d * d; }
                    } else {
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            const float d = src[idx + ((a.s1[c][0] * SY + a.s1[c][1]) * SX + a.s1[c][2]) * dil] -
                                            src[idx + ((a.s2[c][0] * SY + a.s2[c][1]) * SX + a.s2[c][2]) * dil];
                            v[c] = d * d;
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = i == 0 ? a.w[0] * v[c] : acc[c] + a.w[i] * v[c];
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) bufA[c * AY * AX + p] = acc[c];
        }
        __syncthreads();
        // (B) along y
        for (int p = tid; p < NCH * TY * AX; p += NT) {
            const int c = p / (TY * AX), r = p % (TY * AX);
            const float *col = bufA + c * AY * AX + r;   // r = y * AX + ax
            float acc = a.w[0] * col[0];
            for (int j = 1; j < N; ++j) acc = acc + a.w[j] * col[j * AX];
            bufB[p] = acc;
        }
        __syncthreads();
        // (C) along x, then the epilogue
        for (int p = tid; p < TY * TX; p += NT) {
            const int y = p / TX, x = p % TX;
            const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
            if (MODE != MIND_KP && (gy >= H || gx >= W)) continue;
            float s[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const float *row = bufB + c * TY * AX + y * AX + x;
                float acc = a.w[0] * row[0];
                for (int k = 1; k < N; ++k) acc = acc + a.w[k] * row[k];
                s[c] = acc;
            }
            if (MODE == DIST) {   // foerstner.py:40-59, 72
                const float sa = s[0], sb = s[1], sc = s[2], se = s[3], sf = s[4], si = s[NCH - 1];
                const float cA = se * si - sf * sf, cB = (-sb) * si + sc * sf, cC = sb * sf - sc * se;
                const float cE = sa * si - sc * sc, cI = sa * se - sb * sb;
                const float rdet = 1.f / ((sa * cA + sb * cB) + sc * cC);
                out[(((long)b * D + gz) * H + gy) * W + gx] = 1.f / ((rdet * cA + rdet * cE) + rdet * cI);
            } else {              // point_features.py:140-144
                float mn = s[0];
#pragma unroll
                for (int c = 1; c < NCH; ++c) mn = s[c] < mn ? s[c] : mn;
                float sum = 0.f;
#pragma unroll
                for (int c = 0; c < NCH; ++c) { s[c] = s[c] - mn; sum += s[c]; }
                float mv = sum / (float)NCH;
                if (MODE == MIND_STATS) {
                    accum += mv;
                } else {
                    const float mean = *meanp, lo = mean * 0.001f, hi = mean * 1000.f;
                    mv = mv < lo ? lo : (mv > hi ? hi : mv);
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        const float r = expf(-(s[c] / mv));
                        if (MODE == MIND_KP) out[(long)a.outch[c] * K + blockIdx.x] = r;
                        else out[((((long)b * NCH + a.outch[c]) * D + gz) * H + gy) * W + gx] = r;
                    }
                }
            }
        }
        // the next plane's (A) writes bufA only, and (B) -- which overwrites bufB -- comes after its barrier
    }
    if (MODE == MIND_STATS) {   // fixed-order tree, one partial per workgroup
        __syncthreads();
        bufA[tid] = accum;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (tid < s) bufA[tid] = bufA[tid] + bufA[tid + s];
            __syncthreads();
        }
        if (tid == 0) partial[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = bufA[0];
    }
}

// the workgroup partials -> mean over all voxels, in a fixed order (strided fp64 sums, then a tree)
__global__ __launch_bounds__(256) void mind_mean_kernel(const float *__restrict__ partial, int n, double count,
                                                        float *__restrict__ mean) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *mean = (float)(red[0] / count);
}

__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }   // max_pool3d's rule

template <int TZ, int TY, int TX, int NT>
__global__ __launch_bounds__(NT) void nms_kernel(const float *__restrict__ dist, const uint8_t *__restrict__ mask, int B,
                                                 int D, int H, int W, int lo, int hi, float thresh,
                                                 float *__restrict__ maxout, uint8_t *__restrict__ flags) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, d = lo + hi + 1;
    const int EZ = TZ + lo + hi, EY = TY + lo + hi, EX = TX + lo + hi;
    float *buf0 = lds;                   // [EZ][EY][EX], later [EZ][TY][TX]
    float *buf1 = buf0 + EZ * EY * EX;   // [EZ][EY][TX]
    const int ntz = (D + TZ - 1) / TZ;
    const int b = blockIdx.z / ntz, z0 = (blockIdx.z % ntz) * TZ, y0 = blockIdx.y * TY, x0 = blockIdx.x * TX;
    const float *vol = dist + (long)b * D * H * W;
    // window [i - lo, i + hi]; replicate padding adds nothing a truncated window does not already hold
    for (int e = tid; e < EZ * EY * EX; e += NT) {
        const int ex = e % EX, ey = (e / EX) % EY, ez = e / (EX * EY);
        buf0[e] = vol[((long)clampi(z0 - lo + ez, D - 1) * H + clampi(y0 - lo + ey, H - 1)) * W + clampi(x0 - lo + ex, W - 1)];
    }
    __syncthreads();
    for (int e = tid; e < EZ * EY * TX; e += NT) {
        const float *row = buf0 + (e / TX) * EX + e % TX;
        float m = row[0];
        for (int k = 1; k < d; ++k) m = nanmax(m, row[k]);
        buf1[e] = m;
    }
    __syncthreads();
    for (int e = tid; e < EZ * TY * TX; e += NT) {
        const int x = e % TX, y = (e / TX) % TY, ez = e / (TX * TY);
        const float *col = buf1 + (ez * EY + y) * TX + x;
        float m = col[0];
        for (int k = 1; k < d; ++k) m = nanmax(m, col[k * TX]);
        buf0[e] = m;
    }
    __syncthreads();
    for (int e = tid; e < TZ * TY * TX; e += NT) {
        const int x = e % TX, y = (e / TX) % TY, z = e / (TX * TY);
        const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
        if (gz >= D || gy >= H || gx >= W) continue;
        const float *col = buf0 + e;
        float m = col[0];
        for (int k = 1; k < d; ++k) m = nanmax(m, col[k * TY * TX]);
        const long o = (((long)b * D + gz) * H + gy) * W + gx;
        if (maxout) maxout[o] = m;
        if (flags) {
            const float dv = vol[((long)gz * H + gy) * W + gx];
            bool keep = m == dv && dv >= thresh;
            if (keep && mask) {   // foerstner.py:93-104: the six face neighbours only; outside the volume counts as inside
                const uint8_t *mk = mask + (long)b * D * H * W;
                const long c = ((long)gz * H + gy) * W + gx, hw = (long)H * W;
                keep = (gz == 0 || mk[c - hw]) && (gz == D - 1 || mk[c + hw]) && (gy == 0 || mk[c - W]) &&
                       (gy == H - 1 || mk[c + W]) && (gx == 0 || mk[c - 1]) && (gx == W - 1 || mk[c + 1]);
            }
            flags[o] = keep ? 1 : 0;
        }
    }
}

int fill_args(VolArgs &a, const char *name, int B, int D, int H, int W, const float *weights, int N) {
    FSG_REQUIRE(weights, "%s: NULL pointer", name);
    FSG_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && (long)B * D * H * W < (1L << 31), "%s: bad shape B=%d D=%d H=%d W=%d", name, B,
                D, H, W);
    FSG_REQUIRE(N >= 1 && N <= MAXN && (N & 1), "%s: %d smoothing taps (odd, at most %d: sigma <= 2.66)", name, N, MAXN);
    a = VolArgs{};
    a.B = B; a.D = D; a.H = H; a.W = W; a.R = N / 2; a.dil = 0;
    for (int i = 0; i < N; ++i) a.w[i] = weights[i];
    return FSG_OK;
}

int fill_mind(VolArgs &a, const char *name, int dilation, int nch, int box, const int *shifts, const int *outch) {
    FSG_REQUIRE(shifts, "%s: NULL pointer", name);
    FSG_REQUIRE(nch == 6 || nch == 12, "%s: %d channels (6 or 12)", name, nch);
    FSG_REQUIRE(dilation >= 1 && dilation <= MAXDIL, "%s: dilation %d outside [1, %d]", name, dilation, MAXDIL);
    a.dil = dilation;
    a.box = box != 0;
    bool used[MAXCH] = {};
    for (int c = 0; c < nch; ++c) {
        if (a.box) {
            a.m1[c] = (unsigned)shifts[c * 2];
            a.m2[c] = (unsigned)shifts[c * 2 + 1];
            FSG_REQUIRE(!((a.m1[c] | a.m2[c]) >> 27), "%s: stencil subsets have 27 bits", name);
        } else {
            for (int k = 0; k < 3; ++k) {
                a.s1[c][k] = shifts[(c * 2) * 3 + k];
                a.s2[c][k] = shifts[(c * 2 + 1) * 3 + k];
                FSG_REQUIRE(a.s1[c][k] >= -1 && a.s1[c][k] <= 1 && a.s2[c][k] >= -1 && a.s2[c][k] <= 1,
                            "%s: pair offsets must lie in {-1, 0, 1}", name);
            }
        }
        a.outch[c] = outch ? outch[c] : c;
        FSG_REQUIRE(a.outch[c] >= 0 && a.outch[c] < nch && !used[a.outch[c]], "%s: the channel order is not a permutation", name);
        used[a.outch[c]] = true;
    }
    return FSG_OK;
}

template <int MODE, int NCH, int TZ, int TY, int TX, int NT>
int launch_vol(const char *name, const VolArgs &a, dim3 grid, const float *img, float *out, const int64_t *kp, int K,
               const float *mean, float *partial, hipStream_t stream) {
    const int HS = MODE == DIST ? a.R : a.R + a.dil;
    const size_t floats = (size_t)(MODE == DIST ? 3 : 1) * (TZ + 2 * HS) * (TY + 2 * HS) * (TX + 2 * HS) +
                          (size_t)NCH * (TY + 2 * a.R) * (TX + 2 * a.R) + (size_t)NCH * TY * (TX + 2 * a.R);
    const size_t bytes = floats * sizeof(float);   // (the planes hold more than NT floats: the statistics tree fits)
    FSG_REQUIRE(bytes <= LDS_MAX, "%s: sigma / dilation need %zu bytes of LDS per tile, the CU has %zu", name, bytes, LDS_MAX);
    auto kernel = vol_kernel<MODE, NCH, TZ, TY, TX, NT>;
    FSG_REQUIRE(FSG_LDS_GRANTED(kernel, bytes), "%s: %zu bytes of LDS refused", name, bytes);
    kernel<<<grid, dim3(NT), bytes, stream>>>(a, img, out, kp, K, mean, partial);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

constexpr int VZ = 8, VY = 8, VX = 32, VT = 256;   // volume tile and its workgroup

int vol_grid(const char *name, const VolArgs &a, dim3 &grid) {
    const long gz = (long)a.B * fsg_cdiv(a.D, VZ);
    FSG_REQUIRE(gz <= 65535 && fsg_cdiv(a.H, VY) <= 65535, "%s: volume too large for one launch", name);
    grid = dim3(fsg_cdiv(a.W, VX), fsg_cdiv(a.H, VY), (unsigned)gz);
    return FSG_OK;
}

}  // namespace

extern "C" int fsg_foerstner_dist_f32(const float *img, int B, int D, int H, int W, const float *weights, int N, float *out,
                                      fsg_stream_t stream) {
    const char *name = "fsg_foerstner_dist_f32";
    FSG_REQUIRE(img && out, "%s: NULL pointer", name);
    VolArgs a;
    dim3 grid;
    if (int rc = fill_args(a, name, B, D, H, W, weights, N)) return rc;
    if (int rc = vol_grid(name, a, grid)) return rc;
    return launch_vol<DIST, 6, VZ, VY, VX, VT>(name, a, grid, img, out, nullptr, 0, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int fsg_nms_keypoints(const float *dist, const uint8_t *mask, int B, int D, int H, int W, int d, float thresh,
                                 float *maxout, uint8_t *flags, fsg_stream_t stream) {
    const char *name = "fsg_nms_keypoints";
    FSG_REQUIRE(dist && (maxout || flags), "%s: NULL pointer", name);
    FSG_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && (long)B * D * H * W < (1L << 31), "%s: bad shape B=%d D=%d H=%d W=%d", name, B,
                D, H, W);
    FSG_REQUIRE(d >= 1 && d <= MAXNMS, "%s: window %d outside [1, %d]", name, d, MAXNMS);
    const int hi = d / 2, lo = d - hi - 1;   // image_utils.py:46-48: an even window reaches further forward
    const long gz = (long)B * fsg_cdiv(D, VZ);
    FSG_REQUIRE(gz <= 65535 && fsg_cdiv(H, VY) <= 65535, "%s: volume too large for one launch", name);
    const size_t bytes = ((size_t)(VZ + d - 1) * (VY + d - 1) * (VX + d - 1) + (size_t)(VZ + d - 1) * (VY + d - 1) * VX) * sizeof(float);
    auto kernel = nms_kernel<VZ, VY, VX, VT>;
    FSG_REQUIRE(bytes <= LDS_MAX && FSG_LDS_GRANTED(kernel, bytes), "%s: %zu bytes of LDS refused",
                name, bytes);
    kernel<<<dim3(fsg_cdiv(W, VX), fsg_cdiv(H, VY), (unsigned)gz), dim3(VT), bytes, (hipStream_t)stream>>>(
        dist, mask, B, D, H, W, lo, hi, thresh, maxout, flags);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" size_t fsg_mind_stats_workspace_bytes(int B, int D, int H, int W) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * fsg_cdiv(D, VZ) * fsg_cdiv(H, VY) * fsg_cdiv(W, VX) * sizeof(float);
}

extern "C" int fsg_mind_stats_f32(const float *img, int B, int D, int H, int W, int dilation, int nch, int box,
                                  const int *shifts, const float *weights, int N, void *workspace, float *mean,
                                  fsg_stream_t stream) {
    const char *name = "fsg_mind_stats_f32";
    FSG_REQUIRE(img && workspace && mean, "%s: NULL pointer", name);
    VolArgs a;
    dim3 grid;
    if (int rc = fill_args(a, name, B, D, H, W, weights, N)) return rc;
    if (int rc = fill_mind(a, name, dilation, nch, box, shifts, nullptr)) return rc;
    if (int rc = vol_grid(name, a, grid)) return rc;
    float *partial = static_cast<float *>(workspace);
    const int rc = nch == 12 ? launch_vol<MIND_STATS, 12, VZ, VY, VX, VT>(name, a, grid, img, nullptr, nullptr, 0, nullptr, partial,
                                                                          (hipStream_t)stream)
                             : launch_vol<MIND_STATS, 6, VZ, VY, VX, VT>(name, a, grid, img, nullptr, nullptr, 0, nullptr, partial,
                                                                         (hipStream_t)stream);
    if (rc) return rc;
    mind_mean_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partial, (int)(grid.x * grid.y * grid.z), (double)B * D * H * W, mean);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_mind_eval_f32(const float *img, int B, int D, int H, int W, int dilation, int nch, int box, const int *shifts,
                                 const int *outch, const float *weights, int N, const float *mean, float *out,
                                 fsg_stream_t stream) {
    const char *name = "fsg_mind_eval_f32";
    FSG_REQUIRE(img && mean && out && outch, "%s: NULL pointer", name);
    VolArgs a;
    dim3 grid;
    if (int rc = fill_args(a, name, B, D, H, W, weights, N)) return rc;
    FSG_REQUIRE((long)B * D * H * W * 12 < (1L << 40), "%s: volume too large", name);
    if (int rc = fill_mind(a, name, dilation, nch, box, shifts, outch)) return rc;
    if (int rc = vol_grid(name, a, grid)) return rc;
    return nch == 12 ? launch_vol<MIND_EVAL, 12, VZ, VY, VX, VT>(name, a, grid, img, out, nullptr, 0, mean, nullptr, (hipStream_t)stream)
                     : launch_vol<MIND_EVAL, 6, VZ, VY, VX, VT>(name, a, grid, img, out, nullptr, 0, mean, nullptr, (hipStream_t)stream);
}

extern "C" int fsg_mind_eval_kp_f32(const float *img, int D, int H, int W, int dilation, int nch, int box, const int *shifts,
                                    const int *outch, const float *weights, int N, const float *mean, const int64_t *kp, int K,
                                    float *out, fsg_stream_t stream) {
    const char *name = "fsg_mind_eval_kp_f32";
    FSG_REQUIRE(img && mean && out && outch && kp, "%s: NULL pointer", name);
    FSG_REQUIRE(K > 0, "%s: K=%d keypoints", name, K);
    VolArgs a;
    if (int rc = fill_args(a, name, 1, D, H, W, weights, N)) return rc;
    if (int rc = fill_mind(a, name, dilation, nch, box, shifts, outch)) return rc;
    return nch == 12 ? launch_vol<MIND_KP, 12, 1, 1, 1, 64>(name, a, dim3(K), img, out, kp, K, mean, nullptr, (hipStream_t)stream)
                     : launch_vol<MIND_KP, 6, 1, 1, 1, 64>(name, a, dim3(K), img, out, kp, K, mean, nullptr, (hipStream_t)stream);
}
