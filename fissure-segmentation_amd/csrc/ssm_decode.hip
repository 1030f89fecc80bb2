// Statistical-shape-model decode + similarity transform, forward and backward -- include/fsg_hip.h: fsg_ssm_decode_*.
//
// DG-SSM's step behind the backbone (models/dg_ssm.py:128-135): shape_model/ssm.py:74-83 decodes the predicted mode weights,
// x = mean + evec w, and augmentations.py:78-113 moves the shape by the predicted rotation (axis-angle, so3_exp_map), scaling
// and translation.  Composed in torch that is ~30 tiny launches forward and more backward around one (B, M) x (M, 3P)
// product; here the forward is one launch and the backward two, and no (B, P, 3) intermediate reaches memory.
//
// A workgroup owns a tile of 64 points = 192 consecutive rows of evec (3P, M), i.e. one contiguous piece of 192 * M floats
// that it copies into LDS once with consecutive lanes on consecutive addresses (row stride M | 1: bank-conflict free for the
// row-per-thread products AND for the column-per-lane reduction), and then walks over its share of the batch.
// Backward: x is recomputed; per (cloud, tile) the M partial sums of dw and the 15 of dtr / ds / dR (R = the rotation matrix)
// go to the workspace, and a second launch adds the tiles in ascending order and turns dR into dv by the closed-form
// derivative of the Rodrigues formula.  No atomics anywhere: two runs give the same bits.
#include "fsg_common.h"

namespace {

constexpr int kTilePoints = 64;
constexpr int kTileRows = 3 * kTilePoints;   // threads per workgroup: one per row of evec
constexpr int kSmall = 15;                   // dtr (3), ds (3), dR (9) behind the M sums of dw
constexpr float kEps = 1e-4f;                // so3_exp_map's clamp of |v|^2

// R = I + a K + b K^2, K = hat(v), K^2 = v v^T - |v|^2 I, t = sqrt(max(|v|^2, eps)), a = sin t / t, b = (1 - cos t) / t^2
// (b as 2 sin^2(t/2) / t^2: no cancellation for small t)
__device__ __forceinline__ void rodrigues(const float *__restrict__ v, float R[9]) {
    const float x = v[0], y = v[1], z = v[2];
    const float n = x * x + y * y + z * z;
    const float t = sqrtf(fmaxf(n, kEps));
    const float a = sinf(t) / t;
    const float h = 0.5f * t, sh = sinf(h) / h;
    const float b = 0.5f * sh * sh;
    const float d = 1.0f - b * n;
    R[0] = d + b * x * x;      R[1] = b * x * y - a * z;  R[2] = b * x * z + a * y;
    R[3] = b * x * y + a * z;  R[4] = d + b * y * y;      R[5] = b * y * z - a * x;
    R[6] = b * x * z - a * y;  R[7] = b * y * z + a * x;  R[8] = d + b * z * z;
}

__device__ __forceinline__ float pick(int c, float v0, float v1, float v2) { return c == 0 ? v0 : (c == 1 ? v1 : v2); }

// rows [r0, r0 + rows) of evec -> LDS (row stride LD), the rest of the tile zero-filled
__device__ __forceinline__ void load_tile(const float *__restrict__ evec, long r0, int rows, int M, int LD, float *E) {
    const float *src = evec + r0 * M;
    const int n = rows * M;
    for (int i = threadIdx.x; i < kTileRows * M; i += kTileRows) {
        const int row = i / M, m = i - row * M;
        E[row * LD + m] = i < n ? src[i] : 0.0f;
    }
}

__device__ __forceinline__ float decode_row(const float *E, const float *wl, int LD, int M, float mu) {
    const float *e = E + threadIdx.x * LD;
    float x = mu;
    for (int m = 0; m < M; ++m) x = __builtin_fmaf(e[m], wl[m], x);
    return x;
}

__global__ __launch_bounds__(kTileRows) void ssm_decode_fwd_kernel(const float *__restrict__ w, const float *__restrict__ mean,
                                                                  const float *__restrict__ evec, const float *__restrict__ v,
                                                                  const float *__restrict__ s, const float *__restrict__ tr,
                                                                  int B, long R3, int M, int bpb, float *__restrict__ out) {
    extern __shared__ float lds[];
    const int LD = M | 1, tid = threadIdx.x;
    float *E = lds, *xs = E + kTileRows * LD, *wl = xs + kTileRows;
    const long r0 = (long)blockIdx.x * kTileRows, r = r0 + tid;
    const int rows = (int)(R3 - r0 < kTileRows ? R3 - r0 : kTileRows);
    const bool ok = tid < rows;
    load_tile(evec, r0, rows, M, LD, E);
    const float mu = ok ? mean[r] : 0.0f;
    const int c = tid % 3, q3 = tid - c;
    const int b1 = min(B, ((int)blockIdx.y + 1) * bpb);
    for (int b = blockIdx.y * bpb; b < b1; ++b) {
        __syncthreads();   // tile loaded / the previous cloud's readers of wl and xs are done
        if (tid < M) wl[tid] = w[(long)b * M + tid];
        __syncthreads();
        const float x = decode_row(E, wl, LD, M, mu);
        if (v == nullptr) {
            if (ok) out[(long)b * R3 + r] = x;
            continue;
        }
        xs[tid] = x;
        __syncthreads();
        float R[9];
        rodrigues(v + 3 * b, R);
        const float y = __builtin_fmaf(xs[q3 + 2], pick(c, R[6], R[7], R[8]),
                                       __builtin_fmaf(xs[q3 + 1], pick(c, R[3], R[4], R[5]), xs[q3] * pick(c, R[0], R[1], R[2])));
        if (ok) out[(long)b * R3 + r] = __builtin_fmaf(y, s[3 * b + c], tr[3 * b + c]);
    }
}

// partial[(b * tiles + tile) * (M + 15)]: [0, M) dw, then dtr[c], ds[c], dR[0][c], dR[1][c], dR[2][c] (3 each)
__global__ __launch_bounds__(kTileRows) void ssm_decode_bwd_kernel(const float *__restrict__ g, const float *__restrict__ w,
                                                                  const float *__restrict__ mean, const float *__restrict__ evec,
                                                                  const float *__restrict__ v, const float *__restrict__ s,
                                                                  int B, long R3, int M, int bpb, float *__restrict__ partial) {
    extern __shared__ float lds[];
    const int LD = M | 1, tid = threadIdx.x;
    float *E = lds, *xs = E + kTileRows * LD, *wl = xs + kTileRows, *gys = wl + 64, *gxs = gys + kTileRows,
          *pw = gxs + kTileRows, *red = pw + kTileRows;   // red: 5 x kTileRows
    const long r0 = (long)blockIdx.x * kTileRows, r = r0 + tid;
    const int rows = (int)(R3 - r0 < kTileRows ? R3 - r0 : kTileRows);
    const bool ok = tid < rows;
    load_tile(evec, r0, rows, M, LD, E);
    const float mu = ok ? mean[r] : 0.0f;
    const int c = tid % 3, q3 = tid - c, wave = tid >> 6, lane = tid & 63;
    const int stride = M + kSmall;
    const int b1 = min(B, ((int)blockIdx.y + 1) * bpb);
    for (int b = blockIdx.y * bpb; b < b1; ++b) {
        float *part = partial + ((long)b * gridDim.x + blockIdx.x) * stride;
        __syncthreads();
        if (tid < M) wl[tid] = w[(long)b * M + tid];
        __syncthreads();
        const float gval = ok ? g[(long)b * R3 + r] : 0.0f;
        float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        float gy = gval;
        if (v != nullptr) {
            xs[tid] = decode_row(E, wl, LD, M, mu);
            rodrigues(v + 3 * b, R);
            gy = gval * s[3 * b + c];
        }
        gys[tid] = gy;
        __syncthreads();
        // this thread's row is (point q, coordinate i = c) of x:  gx_i = sum_j R[i][j] gy_j
        gxs[tid] = __builtin_fmaf(pick(c, R[2], R[5], R[8]), gys[q3 + 2],
                                  __builtin_fmaf(pick(c, R[1], R[4], R[7]), gys[q3 + 1], pick(c, R[0], R[3], R[6]) * gys[q3]));
        if (v != nullptr) {   // ... and (point q, coordinate c) of the output: y_c = sum_i x_i R[i][c]
            const float x0 = xs[q3], x1 = xs[q3 + 1], x2 = xs[q3 + 2];
            const float y = __builtin_fmaf(x2, pick(c, R[6], R[7], R[8]),
                                           __builtin_fmaf(x1, pick(c, R[3], R[4], R[5]), x0 * pick(c, R[0], R[1], R[2])));
            red[tid] = gval;
            red[kTileRows + tid] = gval * y;
            red[2 * kTileRows + tid] = x0 * gy;
            red[3 * kTileRows + tid] = x1 * gy;
            red[4 * kTileRows + tid] = x2 * gy;
        }
        __syncthreads();
        if (lane < M) {       // dw: each wave sums its 64 rows, lane = mode
            const float *e = E + (wave * 64) * LD + lane, *gx = gxs + wave * 64;
            float acc = 0.0f;
            for (int j = 0; j < 64; ++j) acc = __builtin_fmaf(e[j * LD], gx[j], acc);
            pw[wave * 64 + lane] = acc;
        }
        __syncthreads();
        if (tid < M) {
            part[tid] = (pw[tid] + pw[64 + tid]) + pw[128 + tid];
        } else if (v != nullptr && tid >= 64 && tid < 64 + kSmall) {
            const int j = tid - 64, k = j / 3, cc = j - 3 * k;
            const float *src = red + k * kTileRows + cc;
            float acc = 0.0f;
            for (int q = 0; q < kTilePoints; ++q) acc += src[3 * q];
            part[M + j] = acc;
        }
    }
}

// sums the tiles in ascending order; dv from dR = G:
//   dv_k = a <G, L_k> + b ((G v)_k + (G^T v)_k - 2 v_k tr G) + (a' <G, K> + b' <G, K^2>) dt/dv_k,
//   dt/dv_k = v_k / t where |v|^2 >= eps and 0 inside the clamp, a' = (t cos t - sin t) / t^2, b' = (t sin t - 2 (1 - cos t)) / t^3
__global__ __launch_bounds__(128) void ssm_decode_bwd_finish_kernel(const float *__restrict__ partial, const float *__restrict__ v,
                                                                    int tiles, int M, float *__restrict__ dw,
                                                                    float *__restrict__ dv, float *__restrict__ ds,
                                                                    float *__restrict__ dtr) {
    __shared__ float fin[kSmall];
    const int b = blockIdx.x, tid = threadIdx.x, stride = M + kSmall;
    const int n = v != nullptr ? stride : M;
    if (tid < n) {
        const float *src = partial + (long)b * tiles * stride + tid;
        float acc = 0.0f;
        for (int t = 0; t < tiles; ++t) acc += src[(long)t * stride];
        if (tid < M)
            dw[(long)b * M + tid] = acc;
        else
            fin[tid - M] = acc;
    }
    if (v == nullptr) return;
    __syncthreads();
    if (tid < 3) {
        dtr[3 * b + tid] = fin[tid];
        ds[3 * b + tid] = fin[3 + tid];
    }
    if (tid == 0) {
        const float *G = fin + 6;   // G[3 i + c] = dLoss / dR[i][c]
        const double x = v[3 * b], y = v[3 * b + 1], z = v[3 * b + 2];
        const float nf = v[3 * b] * v[3 * b] + v[3 * b + 1] * v[3 * b + 1] + v[3 * b + 2] * v[3 * b + 2];
        const double n = x * x + y * y + z * z;
        const double t = sqrt(fmax(n, (double)kEps));
        const double st = sin(t), ct = cos(t), h = sin(0.5 * t);
        const double a = st / t, bb = 2.0 * h * h / (t * t);
        const double da = (t * ct - st) / (t * t), db = (t * st - 4.0 * h * h) / (t * t * t);
        const double G00 = G[0], G01 = G[1], G02 = G[2], G10 = G[3], G11 = G[4], G12 = G[5], G20 = G[6], G21 = G[7], G22 = G[8];
        const double trG = G00 + G11 + G22;
        const double GK = -z * G01 + y * G02 + z * G10 - x * G12 - y * G20 + x * G21;
        const double Gv0 = G00 * x + G01 * y + G02 * z, Gv1 = G10 * x + G11 * y + G12 * z, Gv2 = G20 * x + G21 * y + G22 * z;
        const double Gtv0 = G00 * x + G10 * y + G20 * z, Gtv1 = G01 * x + G11 * y + G21 * z, Gtv2 = G02 * x + G12 * y + G22 * z;
        const double GK2 = (x * Gv0 + y * Gv1 + z * Gv2) - n * trG;
        const double radial = nf >= kEps ? (da * GK + db * GK2) / t : 0.0;
        dv[3 * b] = (float)(a * (G21 - G12) + bb * (Gv0 + Gtv0 - 2.0 * x * trG) + radial * x);
        dv[3 * b + 1] = (float)(a * (G02 - G20) + bb * (Gv1 + Gtv1 - 2.0 * y * trG) + radial * y);
        dv[3 * b + 2] = (float)(a * (G10 - G01) + bb * (Gv2 + Gtv2 - 2.0 * z * trG) + radial * z);
    }
}

size_t fwd_lds_bytes(int M) { return ((size_t)kTileRows * (M | 1) + kTileRows + 64) * sizeof(float); }
size_t bwd_lds_bytes(int M) { return ((size_t)kTileRows * (M | 1) + 9 * kTileRows + 64) * sizeof(float); }

// clouds per workgroup: the tile of evec is read once per workgroup, so share it where the grid stays large enough to fill the chip
int clouds_per_block(int B, int tiles) {
    const long blocks = (long)B * tiles;
    return (int)(blocks >= 4096 ? 4 : blocks >= 2048 ? 2 : 1);
}

}  // namespace

#define FSG_SSM_SHAPE(name)                                                                                              \
    FSG_REQUIRE(B >= 0 && B <= 65535 && P >= 1 && P <= (1 << 29) && M >= 1, name ": bad shape B=%d P=%d M=%d", B, P, M); \
    if (M > FSG_SSM_MAX_MODES) {                                                                                         \
        fsg_set_error(name ": M=%d modes, this build serves up to %d", M, FSG_SSM_MAX_MODES);                            \
        return FSG_ERR_UNSUPPORTED;                                                                                      \
    }

extern "C" size_t fsg_ssm_decode_bwd_workspace_bytes(int B, int P, int M) {
    if (B <= 0 || P <= 0 || M <= 0) return 0;
    return (size_t)B * fsg_cdiv(P, kTilePoints) * (M + kSmall) * sizeof(float);
}

extern "C" int fsg_ssm_decode_fwd_f32(const float *w, const float *mean, const float *evec, const float *v, const float *s,
                                      const float *tr, int B, int P, int M, float *out, fsg_stream_t stream) {
    FSG_SSM_SHAPE("fsg_ssm_decode_fwd_f32");
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(w && mean && evec && out, "fsg_ssm_decode_fwd_f32: NULL pointer");
    FSG_REQUIRE(v ? (s && tr) : (!s && !tr), "fsg_ssm_decode_fwd_f32: v, s and tr come together (all or none)");
    const int tiles = fsg_cdiv(P, kTilePoints), bpb = clouds_per_block(B, tiles);
    hipLaunchKernelGGL(ssm_decode_fwd_kernel, dim3(tiles, fsg_cdiv(B, bpb)), dim3(kTileRows), fwd_lds_bytes(M),
                       (hipStream_t)stream, w, mean, evec, v, s, tr, B, 3L * P, M, bpb, out);
    FSG_CHECK_LAUNCH("fsg_ssm_decode_fwd_f32");
    return FSG_OK;
}

extern "C" int fsg_ssm_decode_bwd_f32(const float *grad_out, const float *w, const float *mean, const float *evec,
                                      const float *v, const float *s, int B, int P, int M, float *grad_w, float *grad_v,
                                      float *grad_s, float *grad_tr, void *workspace, size_t workspace_bytes,
                                      fsg_stream_t stream) {
    FSG_SSM_SHAPE("fsg_ssm_decode_bwd_f32");
    if (B == 0) return FSG_OK;
    FSG_REQUIRE(grad_out && w && mean && evec && grad_w && workspace, "fsg_ssm_decode_bwd_f32: NULL pointer");
    FSG_REQUIRE(v ? (s && grad_v && grad_s && grad_tr) : (!s && !grad_v && !grad_s && !grad_tr),
                "fsg_ssm_decode_bwd_f32: v, s, grad_v, grad_s and grad_tr come together (all or none)");
    FSG_REQUIRE(workspace_bytes >= fsg_ssm_decode_bwd_workspace_bytes(B, P, M),
                "fsg_ssm_decode_bwd_f32: workspace of %zu bytes, %zu needed", workspace_bytes,
                fsg_ssm_decode_bwd_workspace_bytes(B, P, M));
    const int tiles = fsg_cdiv(P, kTilePoints), bpb = clouds_per_block(B, tiles);
    float *partial = (float *)workspace;
    hipLaunchKernelGGL(ssm_decode_bwd_kernel, dim3(tiles, fsg_cdiv(B, bpb)), dim3(kTileRows), bwd_lds_bytes(M),
                       (hipStream_t)stream, grad_out, w, mean, evec, v, s, B, 3L * P, M, bpb, partial);
    FSG_CHECK_LAUNCH("fsg_ssm_decode_bwd_f32");
    hipLaunchKernelGGL(ssm_decode_bwd_finish_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, partial, v, tiles, M, grad_w,
                       grad_v, grad_s, grad_tr);
    FSG_CHECK_LAUNCH("fsg_ssm_decode_bwd_f32");
    return FSG_OK;
}
