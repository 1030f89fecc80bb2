// Hessian fissure enhancement and its keypoint candidates on a single-channel fp32 volume -- include/fsg_hip.h:
// fsg_fissure_enhance_f32, fsg_smooth_threshold_f32.
// Replaces HessianEnhancementFilter.forward + fissure_filter (data_processing/fissure_enhancement.py:47-99, 149-180), the
// lung-mask product of get_enhanced_fissure_image (:213-214) and the smoothing + thresholding in front of the top-k of
// get_hessian_fissure_enhancement_kpts (data_processing/keypoint_extraction.py:134-141).
//
// Enhancement.  The reference's "Hessian" is not a textbook one: H[a][a] is the second-derivative Gaussian taps along axis
// a ALONE (no smoothing along the other two), H[a][b] the first-derivative taps along a and then along b (no smoothing along
// the third).  A workgroup owns a TZ x TY x TX output tile:
//   fill    the image tile goes to LDS once with a halo of R in every axis.  Tile coordinate c holds the image AT clamp(c).
//           That single clamp per axis IS the reference's replicate padding here: the two passes of an off-diagonal entry act
//           on DIFFERENT axes, so padding the once-filtered volume along b replicates rows that were themselves filtered
//           along a with the image clamped along a.  (The distinctiveness kernel of volume.hip cannot do this: its gradient
//           products are smoothed along the axis the gradient was taken along, and needs a second clamp.)
//   derive  d/dz on TZ x (TY + 2R) x (TX + 2R) and d/dy on TZ x TY x (TX + 2R) go to LDS: H[z][y] and H[z][x] differentiate
//           the first along y / x, H[y][x] the second along x.  d/dx is never needed as a field.
//   solve   per voxel: three second derivatives from the image tile, three mixed ones from the two fields, the eigenvalues
//           of the symmetric 3 x 3 matrix, planeness, HU weight, mask.
// None of the nine filtered volumes nor the (D, H, W, 3, 3) tensor exists outside LDS / registers; HBM sees the image (plus
// halo re-reads; how many of them L2 serves has not been measured), optionally the mask, and the outputs.
//
// Exact zero on constant support (a deliberate deviation towards the fp64 value, like the exact-zero gradient of
// volume.hip).  The antisymmetric first-derivative taps are summed as pair differences k[i] (x[+i] - x[-i]) and the
// symmetric second-derivative taps as sum_i k[i] ((x[+i] - x0) + (x[-i] - x0)) + (sum k) x0.  Where the whole (2R + 1)^3
// support of a voxel is constant the mixed entries are exactly 0 and the three diagonal entries are the same number, the
// solver returns the diagonal untouched, and the planeness -- hence the output -- is exactly 0 whatever the constant.  The
// reference's fp32 sums leave rounding noise there, times an HU weight that need not be small.
//
// Eigenvalues: the trigonometric closed form evaluated in fp64 (fp64 is cheap on this part and only the 3 x 3 solve uses
// it).  Its error is about sqrt(eps_fp64) ~ 1e-8 relative where two eigenvalues nearly coincide, below the rounding of the
// fp32 matrix entries everywhere; the same form in fp32 would lose sqrt(eps_fp32) ~ 3e-4 there.
//
// Sums run in a fixed order (taps ascending) and the build keeps -ffp-contract=off: two runs are bitwise equal.
#include "fsg_common.h"

namespace {

constexpr int MAXR = FSG_ENHANCE_MAX_TAP_RADIUS;   // derivation sigma <= 1 (radius int(4 sigma + 0.5)); DiscreteGaussian of variance <= ~1.3
constexpr int TZ = 8, TY = 8, TX = 32, NT = 256;
constexpr size_t LDS_MAX = 160 * 1024;

struct EnhArgs {
    int B, D, H, W, R;
    float k1[MAXR + 1];   // first-derivative tap at offset +i (the tap at -i is its negative, the centre 0)
    float k2[MAXR + 1];   // second-derivative tap at offset +-i; k2[0] is unused
    float k2sum;          // the sum of all second-derivative taps
    float mu, denom;      // HU weight exp(-(x - mu)^2 / denom), denom = 2 sigma_hu^2
};

struct SmoothArgs {
    int B, D, H, W, R[3];
    float w[3][2 * MAXR + 1];
    float thresh;
};


__device__ __forceinline__ void fill_tile(float *src, const float *vol, int z0, int y0, int x0, int Rz, int Ry, int Rx, int D,
                                          int H, int W) {
    const int SY = TY + 2 * Ry, SX = TX + 2 * Rx, S3 = (TZ + 2 * Rz) * SY * SX;
    for (int e = threadIdx.x; e < S3; e += NT) {
        const int sx = e % SX, sy = (e / SX) % SY, sz = e / (SX * SY);
        src[e] = vol[((long)clampi(z0 - Rz + sz, D - 1) * H + clampi(y0 - Ry + sy, H - 1)) * W + clampi(x0 - Rx + sx, W - 1)];
    }
}

// eigenvalues of [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]] -> the two of largest absolute value, l1 the larger
__device__ __forceinline__ void top_two_eigenvalues(double a00, double a11, double a22, double a01, double a02, double a12,
                                                    double &l1, double &l2) {
    double e0 = a00, e1 = a11, e2 = a22;
    const double p1 = (a01 * a01 + a02 * a02) + a12 * a12;
    if (p1 != 0.0) {   // (a diagonal matrix keeps its diagonal bit for bit)
        const double q = ((a00 + a11) + a22) / 3.0;
        const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
        const double p = sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + 2.0 * p1) / 6.0);
        const double ip = 1.0 / p;
        const double c00 = b00 * ip, c11 = b11 * ip, c22 = b22 * ip, c01 = a01 * ip, c02 = a02 * ip, c12 = a12 * ip;
        double r = 0.5 * ((c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02)) + c02 * (c01 * c12 - c11 * c02));
        r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
        const double phi = acos(r) / 3.0;
        e0 = q + 2.0 * p * cos(phi);                               // largest
        e2 = q + 2.0 * p * cos(phi + 2.0943951023931954923);       // smallest (phi + 2 pi / 3)
        e1 = (3.0 * q - e0) - e2;
    }
    double m0 = fabs(e0), m1 = fabs(e1), m2 = fabs(e2), t;
    if (m1 > m0) { t = m0; m0 = m1; m1 = t; t = e0; e0 = e1; e1 = t; }
    if (m2 > m0) { t = m0; m0 = m2; m2 = t; t = e0; e0 = e2; e2 = t; }
    if (m2 > m1) { e1 = e2; }
    l1 = e0;
    l2 = e1;
}

__global__ __launch_bounds__(NT) void enhance_kernel(EnhArgs a, const float *__restrict__ img, const uint8_t *__restrict__ mask,
                                                     float *__restrict__ out, float *__restrict__ planeness,
                                                     float *__restrict__ hu_weight) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, R = a.R, D = a.D, H = a.H, W = a.W;
    const int SY = TY + 2 * R, SX = TX + 2 * R, SZ = TZ + 2 * R;
    float *src = lds;                    // [SZ][SY][SX] image
    float *gz = src + SZ * SY * SX;      // [TZ][SY][SX] d/dz
    float *gy = gz + TZ * SY * SX;       // [TZ][TY][SX] d/dy
    const int ntz = (D + TZ - 1) / TZ;
    const int b = blockIdx.z / ntz, z0 = (blockIdx.z % ntz) * TZ, y0 = blockIdx.y * TY, x0 = blockIdx.x * TX;
    const long vox = (long)D * H * W;
    fill_tile(src, img + b * vox, z0, y0, x0, R, R, R, D, H, W);
    __syncthreads();

    for (int e = tid; e < TZ * SY * SX; e += NT) {
        const float *c = src + e + R * SY * SX;   // (z + R, sy, sx)
        float acc = 0.f;
        for (int i = 1; i <= R; ++i) acc = acc + a.k1[i] * (c[i * SY * SX] - c[-i * SY * SX]);
        gz[e] = acc;
    }
    for (int e = tid; e < TZ * TY * SX; e += NT) {
        const int sx = e % SX, y = (e / SX) % TY, z = e / (SX * TY);
        const float *c = src + ((z + R) * SY + y + R) * SX + sx;
        float acc = 0.f;
        for (int i = 1; i <= R; ++i) acc = acc + a.k1[i] * (c[i * SX] - c[-i * SX]);
        gy[e] = acc;
    }
    __syncthreads();

    for (int e = tid; e < TZ * TY * TX; e += NT) {
        const int x = e % TX, y = (e / TX) % TY, z = e / (TX * TY);
        const int gzc = z0 + z, gyc = y0 + y, gxc = x0 + x;
        if (gzc >= D || gyc >= H || gxc >= W) continue;
        const float *c = src + ((z + R) * SY + y + R) * SX + x + R;
        const float *pz = gz + (z * SY + y + R) * SX + x + R;
        const float *py = gy + (z * TY + y) * SX + x + R;
        const float v = c[0];
        float hzz = 0.f, hyy = 0.f, hxx = 0.f, hzy = 0.f, hzx = 0.f, hyx = 0.f;
        for (int i = 1; i <= R; ++i) {
            const float k2 = a.k2[i], k1 = a.k1[i];
            hzz = hzz + k2 * ((c[i * SY * SX] - v) + (c[-i * SY * SX] - v));
            hyy = hyy + k2 * ((c[i * SX] - v) + (c[-i * SX] - v));
            hxx = hxx + k2 * ((c[i] - v) + (c[-i] - v));
            hzy = hzy + k1 * (pz[i * SX] - pz[-i * SX]);
            hzx = hzx + k1 * (pz[i] - pz[-i]);
            hyx = hyx + k1 * (py[i] - py[-i]);
        }
        const float base = a.k2sum * v;
        hzz = hzz + base;
        hyy = hyy + base;
        hxx = hxx + base;
        double l1, l2;
        top_two_eigenvalues((double)hzz, (double)hyy, (double)hxx, (double)hzy, (double)hzx, (double)hyx, l1, l2);
        // fissure_enhancement.py:152-156: planeness where the dominant eigenvalue is negative, 0 elsewhere
        const float P = l1 < 0.0 ? (float)((fabs(l1) - fabs(l2)) / (fabs(l1) + fabs(l2))) : 0.f;
        const float d = v - a.mu;
        const float hw = expf(-(d * d) / a.denom);   // :160
        const long o = b * vox + ((long)gzc * H + gyc) * W + gxc;
        float F = hw * P;
        if (mask) F = F * (float)(mask[o] != 0);
        out[o] = F;
        if (planeness) planeness[o] = P;
        if (hu_weight) hu_weight[o] = hw;
    }
}

// separable smoothing (axis order 0, 1, 2; replicate padding, which a single clamp per axis of the tile fill reproduces
// because every pass acts on its own axis), then value > thresh ? value : 0 and a byte flag for torch.nonzero
__global__ __launch_bounds__(NT) void smooth_threshold_kernel(SmoothArgs a, const float *__restrict__ vol_in,
                                                              float *__restrict__ out, uint8_t *__restrict__ flags) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, Rz = a.R[0], Ry = a.R[1], Rx = a.R[2], D = a.D, H = a.H, W = a.W;
    const int SY = TY + 2 * Ry, SX = TX + 2 * Rx, SZ = TZ + 2 * Rz;
    float *src = lds;                     // [SZ][SY][SX]
    float *bufA = src + SZ * SY * SX;     // [TZ][SY][SX] smoothed along z
    float *bufB = bufA + TZ * SY * SX;    // [TZ][TY][SX] and along y
    const int ntz = (D + TZ - 1) / TZ;
    const int b = blockIdx.z / ntz, z0 = (blockIdx.z % ntz) * TZ, y0 = blockIdx.y * TY, x0 = blockIdx.x * TX;
    const long vox = (long)D * H * W;
    fill_tile(src, vol_in + b * vox, z0, y0, x0, Rz, Ry, Rx, D, H, W);
    __syncthreads();
    for (int e = tid; e < TZ * SY * SX; e += NT) {
        const float *c = src + e;
        float acc = a.w[0][0] * c[0];
        for (int i = 1; i <= 2 * Rz; ++i) acc = acc + a.w[0][i] * c[i * SY * SX];
        bufA[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < TZ * TY * SX; e += NT) {
        const int sx = e % SX, y = (e / SX) % TY, z = e / (SX * TY);
        const float *c = bufA + (z * SY + y) * SX + sx;
        float acc = a.w[1][0] * c[0];
        for (int i = 1; i <= 2 * Ry; ++i) acc = acc + a.w[1][i] * c[i * SX];
        bufB[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < TZ * TY * TX; e += NT) {
        const int x = e % TX, y = (e / TX) % TY, z = e / (TX * TY);
        const int gzc = z0 + z, gyc = y0 + y, gxc = x0 + x;
        if (gzc >= D || gyc >= H || gxc >= W) continue;
        const float *c = bufB + (z * TY + y) * SX + x;
        float acc = a.w[2][0] * c[0];
        for (int i = 1; i <= 2 * Rx; ++i) acc = acc + a.w[2][i] * c[i];
        const long o = b * vox + ((long)gzc * H + gyc) * W + gxc;
        const bool keep = acc > a.thresh;
        if (out) out[o] = keep ? acc : 0.f;
        if (flags) flags[o] = keep ? 1 : 0;
    }
}

int check_shape(const char *name, int B, int D, int H, int W, dim3 &grid) {
    FSG_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && (long)B * D * H * W < (1L << 31), "%s: bad shape B=%d D=%d H=%d W=%d", name, B,
                D, H, W);
    const long gz = (long)B * fsg_cdiv(D, TZ);
    FSG_REQUIRE(gz <= 65535 && fsg_cdiv(H, TY) <= 65535, "%s: volume too large for one launch", name);
    grid = dim3(fsg_cdiv(W, TX), fsg_cdiv(H, TY), (unsigned)gz);
    return FSG_OK;
}

size_t tile_bytes(int Rz, int Ry, int Rx) {
    const size_t sy = TY + 2 * Ry, sx = TX + 2 * Rx;
    return ((size_t)(TZ + 2 * Rz) * sy * sx + (size_t)TZ * sy * sx + (size_t)TZ * TY * sx) * sizeof(float);
}

}  // namespace

extern "C" int fsg_fissure_enhance_f32(const float *img, const uint8_t *mask, int B, int D, int H, int W, const float *k1,
                                       const float *k2, int N, float mu, float sigma_hu, float *out, float *planeness,
                                       float *hu_weight, fsg_stream_t stream) {
    const char *name = "fsg_fissure_enhance_f32";
    // the host-side arguments are checked first and the device pointers last: a call with NULL volumes exercises every check
    // above without being able to reach the launch
    FSG_REQUIRE(k1 && k2, "%s: NULL tap pointer", name);
    FSG_REQUIRE(N >= 3 && N <= 2 * MAXR + 1 && (N & 1), "%s: %d derivative taps (odd, 3..%d: derivation sigma <= 1)", name, N,
                2 * MAXR + 1);
    FSG_REQUIRE(sigma_hu > 0.f, "%s: sigma_hu must be positive", name);
    EnhArgs a{};
    dim3 grid;
    if (int rc = check_shape(name, B, D, H, W, grid)) return rc;
    a.B = B; a.D = D; a.H = H; a.W = W; a.R = N / 2;
    const int R = a.R;
    FSG_REQUIRE(k1[R] == 0.f, "%s: the first-derivative taps must be antisymmetric", name);
    double sum = (double)k2[R];
    for (int i = 1; i <= R; ++i) {
        FSG_REQUIRE(k1[R + i] == -k1[R - i], "%s: the first-derivative taps must be antisymmetric", name);
        FSG_REQUIRE(k2[R + i] == k2[R - i], "%s: the second-derivative taps must be symmetric", name);
        a.k1[i] = k1[R + i];
        a.k2[i] = k2[R + i];
        sum += 2.0 * (double)k2[R + i];
    }
    a.k2sum = (float)sum;
    a.mu = mu;
    a.denom = 2.f * sigma_hu * sigma_hu;
    FSG_REQUIRE(img && out, "%s: NULL pointer", name);
    const size_t bytes = tile_bytes(R, R, R);
    FSG_REQUIRE(bytes <= LDS_MAX && FSG_LDS_GRANTED(enhance_kernel, bytes),
                "%s: %zu bytes of LDS refused", name, bytes);
    enhance_kernel<<<grid, dim3(NT), bytes, (hipStream_t)stream>>>(a, img, mask, out, planeness, hu_weight);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_smooth_threshold_f32(const float *vol, int B, int D, int H, int W, const float *wz, int Nz, const float *wy,
                                        int Ny, const float *wx, int Nx, float thresh, float *out, uint8_t *flags,
                                        fsg_stream_t stream) {
    const char *name = "fsg_smooth_threshold_f32";
    FSG_REQUIRE(wz && wy && wx, "%s: NULL tap pointer", name);   // device pointers last, as above
    SmoothArgs a{};
    dim3 grid;
    if (int rc = check_shape(name, B, D, H, W, grid)) return rc;
    a.B = B; a.D = D; a.H = H; a.W = W; a.thresh = thresh;
    const float *w[3] = {wz, wy, wx};
    const int n[3] = {Nz, Ny, Nx};
    for (int ax = 0; ax < 3; ++ax) {
        FSG_REQUIRE(n[ax] >= 1 && n[ax] <= 2 * MAXR + 1 && (n[ax] & 1), "%s: %d smoothing taps along axis %d (odd, at most %d)", name,
                    n[ax], ax, 2 * MAXR + 1);
        a.R[ax] = n[ax] / 2;
        for (int i = 0; i < n[ax]; ++i) a.w[ax][i] = w[ax][i];
    }
    FSG_REQUIRE(vol && (out || flags), "%s: NULL pointer", name);
    const size_t bytes = tile_bytes(a.R[0], a.R[1], a.R[2]);
    FSG_REQUIRE(bytes <= LDS_MAX && FSG_LDS_GRANTED(smooth_threshold_kernel, bytes),
                "%s: %zu bytes of LDS refused", name, bytes);
    smooth_threshold_kernel<<<grid, dim3(NT), bytes, (hipStream_t)stream>>>(a, vol, out, flags);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}
