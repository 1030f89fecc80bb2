// Voxel CNN (MobileNetASPP) inference -- include/fsg_hip.h: fsg_mbconv3d_fwd_f32, fsg_patch_accumulate_f32, fsg_patch_finalize_f32.
//
// fsg_mbconv3d_fwd_f32: one eval-mode inverted-residual block of the reference's models/mobilenet.py in one launch
//   expand (1x1x1, or block 0's dense 3x3x3 stride-2 from one channel) -> scale/shift -> ReLU6 -> depthwise 3x3x3 (stride 1 | 2,
//   zero border) -> scale/shift -> ReLU6 -> project 1x1x1 -> scale/shift (-> + input).  The expanded tensor never leaves the CU.
//
//   A 256-thread workgroup owns an output tile of 4x4x4 voxels (stride 1) or 2x4x4 (stride 2) of one item.  The positions of the
//   expanded tensor that the tile's depthwise taps reach form a 6x6x6 (5x9x9) box; the input voxels under them sit in LDS, one
//   row of channels per position (block 0: one row of its 27 input taps per position, so that its dense convolution is the same
//   product with K = 27).  Cmid is walked in chunks of 16 channels:
//     expand     rows = positions, 16 at a time, columns = the chunk's channels, K = Cin four at a time on
//                v_mfma_f32_16x16x4_f32 (exact fp32 products and sums); scale/shift, ReLU6, and a position outside the
//                expanded tensor becomes 0 (the depthwise stage pads the ACTIVATED tensor with zeros) -> LDS image of the chunk
//     depthwise  one thread per (output voxel, channel): 27 fmas from the LDS image, weights in registers; scale/shift, ReLU6
//     project    rows = output voxels, columns = Cout, K = the chunk: four MFMAs into accumulators that stay in registers
//                across the chunks
//   and the epilogue applies the third scale/shift, adds the residual and stores channels-last.  Every sum has a fixed order and
//   a workgroup sees one item only: the same bits on every run, alone or inside a batch.  No atomics.
//
// fsg_patch_accumulate_f32 / fsg_patch_finalize_f32: the tail of the reference's PatchBasedModule.predict_all_patches
//   (models/seg_cnn.py:48-62).  One launch per patch, in the order given, on one stream: overlapping patches add in that order.
#include "fsg_common.h"

namespace {

constexpr int MB_THREADS = 256;
constexpr int MB_CHUNK = 16;   // channels of the expanded tensor per pass
constexpr int MB_MS = 20;      // row stride of the chunk's LDS image (the accumulator stores of the four lane groups miss each other)
constexpr int MB_DS = 17;      // row stride of the depthwise output and of the project weights

template <int S>
struct MbTile {
    static constexpr int TD = S == 1 ? 4 : 2, TH = 4, TW = 4;
    static constexpr int NOUT = TD * TH * TW;
    static constexpr int MD = (TD - 1) * S + 3, MH = (TH - 1) * S + 3, MW = (TW - 1) * S + 3;
    static constexpr int NPOS = MD * MH * MW;
    static constexpr int NRT = (NPOS + 15) / 16, NROWS = NRT * 16;
    static constexpr int ORT = NOUT / 16;   // row tiles of the project product
};

struct MbArgs {
    const float *x, *w1, *s1, *b1, *wd, *s2, *b2, *w3, *s3, *b3, *res;
    float *y;
    int Di, Hi, Wi;   // input extents
    int Dm, Hm, Wm;   // extents of the expanded tensor
    int Do, Ho, Wo;   // output extents
    int Cin, Cmid, Cout;
    int K1, K1p;      // length of an expand weight row (Cin | 27) and the same rounded up to 4
    int first;        // block 0: the expand stage is the dense 3x3x3 stride-2 convolution of one channel
    int nth, ntw, ntd;
};

static size_t mb_lds_floats(int nrows, int nout, int K1p) {
    const int XS = K1p + 1;
    return (size_t)nrows * XS + (size_t)nrows * MB_MS + (size_t)nout * MB_DS + (size_t)MB_CHUNK * XS + 64 * MB_DS + 27 * MB_CHUNK + nrows;
}

static __device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

template <int S>
__global__ __launch_bounds__(MB_THREADS) void mbconv3d_kernel(const MbArgs a) {
    using T = MbTile<S>;
    extern __shared__ float lds[];
    const int XS = a.K1p + 1;
    float *X = lds;                          // NROWS x XS   input rows under the positions of the expanded box
    float *Mid = X + T::NROWS * XS;          // NROWS x MB_MS  the chunk of the expanded tensor, activated
    float *DWo = Mid + T::NROWS * MB_MS;     // NOUT x MB_DS   the chunk after the depthwise stage, activated
    float *W1s = DWo + T::NOUT * MB_DS;      // 16 x XS        expand weights of the chunk
    float *W3s = W1s + MB_CHUNK * XS;        // 64 x MB_DS     project weights of the chunk, rows >= Cout zero
    float *Wds = W3s + 64 * MB_DS;           // 27 x 16        depthwise taps of the chunk, tap-major
    float *valid = Wds + 27 * MB_CHUNK;      // NROWS          1 where the position lies inside the expanded tensor

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, l4 = lane >> 4;
    unsigned bid = blockIdx.x;
    const int tw = bid % a.ntw;
    bid /= a.ntw;
    const int th = bid % a.nth;
    bid /= a.nth;
    const int td = bid % a.ntd;
    const int b = bid / a.ntd;
    const int od0 = td * T::TD, oh0 = th * T::TH, ow0 = tw * T::TW;
    const int md0 = od0 * S - 1, mh0 = oh0 * S - 1, mw0 = ow0 * S - 1;   // corner of the expanded box

    // ---- the input under the box -> LDS (zero outside the tensors, in the padding columns and in the padding rows)
    for (int i = t; i < T::NROWS * XS; i += MB_THREADS) X[i] = 0.f;
    for (int p = t; p < T::NROWS; p += MB_THREADS) {
        const int md = md0 + p / (T::MH * T::MW), mh = mh0 + (p / T::MW) % T::MH, mw = mw0 + p % T::MW;
        valid[p] = (p < T::NPOS && md >= 0 && md < a.Dm && mh >= 0 && mh < a.Hm && mw >= 0 && mw < a.Wm) ? 1.f : 0.f;
    }
    __syncthreads();
    const int K1 = a.K1;
    for (int i = t; i < T::NPOS * K1; i += MB_THREADS) {
        const int p = i / K1, k = i - p * K1;
        const int md = md0 + p / (T::MH * T::MW), mh = mh0 + (p / T::MW) % T::MH, mw = mw0 + p % T::MW;
        if (md < 0 || md >= a.Dm || mh < 0 || mh >= a.Hm || mw < 0 || mw >= a.Wm) continue;
        if (a.first) {   // tap k of the stride-2, padding-1 convolution at this position
            const int id = 2 * md - 1 + k / 9, ih = 2 * mh - 1 + (k / 3) % 3, iw = 2 * mw - 1 + k % 3;
            if (id < 0 || id >= a.Di || ih < 0 || ih >= a.Hi || iw < 0 || iw >= a.Wi) continue;
            X[p * XS + k] = a.x[(((size_t)b * a.Di + id) * a.Hi + ih) * a.Wi + iw];
        } else {
            X[p * XS + k] = a.x[((((size_t)b * a.Di + md) * a.Hi + mh) * a.Wi + mw) * a.Cin + k];
        }
    }

    const int CT = (a.Cout + 15) >> 4;   // column tiles of the project product
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c = t & 15;                // this thread's channel of the chunk in the depthwise stage

    // The weights of a chunk travel global -> registers -> LDS, and the registers of chunk n + 1 are loaded while chunk n is
    // computed: with one or two workgroups per CU nothing else hides the latency of these loads.
    struct ChunkW {
        float w1[4], w3[4], wd[2], s1, b1, s2, b2;   // 16 x K1p <= 1024 expand, <= 64 x 16 project, 16 x 27 depthwise weights over 256 threads
    };
    auto fetch = [&](int cm0, ChunkW &w) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = t + q * MB_THREADS;
            const int j = i / a.K1p, k = i - j * a.K1p;
            // unconditional loads from clamped addresses: a select here would be a use, and a use waits for the load
            w.w1[q] = a.w1[(j < MB_CHUNK && k < K1) ? (size_t)(cm0 + j) * K1 + k : 0];
            w.w3[q] = a.w3[(i >> 4) < a.Cout ? (size_t)(i >> 4) * a.Cmid + cm0 + (i & 15) : 0];
        }
        w.wd[0] = a.wd[(size_t)cm0 * 27 + t];                                          // the chunk's 432 taps are contiguous
        w.wd[1] = a.wd[(size_t)cm0 * 27 + (t < 27 * MB_CHUNK - MB_THREADS ? t + MB_THREADS : 0)];
        w.s1 = a.s1[cm0 + l15], w.b1 = a.b1[cm0 + l15], w.s2 = a.s2[cm0 + c], w.b2 = a.b2[cm0 + c];
    };
    ChunkW nxt;
    fetch(0, nxt);

    for (int cm0 = 0; cm0 < a.Cmid; cm0 += MB_CHUNK) {
        // ---- the chunk's weights: product operands into LDS, the scale/shift pairs stay in registers
        const ChunkW cur = nxt;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = t + q * MB_THREADS;
            const int j = i / a.K1p, k = i - j * a.K1p;
            if (j < MB_CHUNK) W1s[j * XS + k] = k < K1 ? cur.w1[q] : 0.f;
            if (i < CT * 16 * MB_CHUNK) W3s[(i >> 4) * MB_DS + (i & 15)] = (i >> 4) < a.Cout ? cur.w3[q] : 0.f;
        }
        Wds[(t % 27) * MB_CHUNK + t / 27] = cur.wd[0];
        if (t < 27 * MB_CHUNK - MB_THREADS) Wds[((t + MB_THREADS) % 27) * MB_CHUNK + (t + MB_THREADS) / 27] = cur.wd[1];
        if (cm0 + MB_CHUNK < a.Cmid) fetch(cm0 + MB_CHUNK, nxt);
        const float s1 = cur.s1, b1 = cur.b1, s2 = cur.s2, b2 = cur.b2;
        __syncthreads();   // X (first pass) and the weights are in place

        // ---- expand: 16 positions x 16 channels per MFMA tile
        for (int rt = wave; rt < T::NRT; rt += MB_THREADS / 64) {
            f32x4 e = {0.f, 0.f, 0.f, 0.f};
            const float *xa = X + (rt * 16 + l15) * XS + l4, *wb = W1s + l15 * XS + l4;
            for (int k = 0; k < a.K1p; k += 4) e = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k], wb[k], e, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = rt * 16 + 4 * l4 + r;
                Mid[p * MB_MS + l15] = relu6f(__builtin_fmaf(e[r], s1, b1)) * valid[p];
            }
        }
        __syncthreads();

        // ---- depthwise 3x3x3 from the LDS image.  A thread's outputs are the TD voxels above each other (16 threads x 16
        // channels cover a d-plane of the tile), so neighbouring outputs share d-planes of taps; all results are formed before
        // the first store so that the compiler may keep the shared taps in registers
        constexpr int NI = T::NOUT * MB_CHUNK / MB_THREADS;
        static_assert(NI == T::TD && T::TH * T::TW == 16, "one d-plane of the tile per 256 threads");
        float dv[NI];
        {
            float wdr[27];
#pragma unroll
            for (int k = 0; k < 27; ++k) wdr[k] = Wds[k * MB_CHUNK + c];
            const int oh = (t >> 4) / T::TW, ow = (t >> 4) % T::TW;
            const float *m = Mid + ((oh * S) * T::MW + ow * S) * MB_MS + c;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                float v = 0.f;
#pragma unroll
                for (int kd = 0; kd < 3; ++kd)
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw)
                            v = __builtin_fmaf(m[(((i * S + kd) * T::MH + kh) * T::MW + kw) * MB_MS], wdr[(kd * 3 + kh) * 3 + kw], v);
                dv[i] = relu6f(__builtin_fmaf(v, s2, b2));
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) DWo[((t >> 4) + 16 * i) * MB_DS + c] = dv[i];
        __syncthreads();

        // ---- project: the (row tile, column tile) pairs go round the four waves
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pr = wave + 4 * i;
            if (pr < T::ORT * CT) {
                const int rt = pr % T::ORT, ct = pr / T::ORT;
                const float *da = DWo + (rt * 16 + l15) * MB_DS + l4, *wb = W3s + (ct * 16 + l15) * MB_DS + l4;
#pragma unroll
                for (int k = 0; k < MB_CHUNK; k += 4) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[k], wb[k], acc[i], 0, 0, 0);
            }
        }
        __syncthreads();   // the next chunk overwrites the weights and the two images
    }

    // ---- epilogue: third scale/shift, residual, channels-last store
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pr = wave + 4 * i;
        if (pr >= T::ORT * CT) continue;
        const int rt = pr % T::ORT, ct = pr / T::ORT;
        const int co = ct * 16 + l15;
        if (co >= a.Cout) continue;
        const float s3 = a.s3[co], b3 = a.b3[co];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = rt * 16 + 4 * l4 + r;
            const int od = od0 + o / (T::TH * T::TW), oh = oh0 + (o / T::TW) % T::TH, ow = ow0 + o % T::TW;
            if (od >= a.Do || oh >= a.Ho || ow >= a.Wo) continue;
            const size_t off = ((((size_t)b * a.Do + od) * a.Ho + oh) * a.Wo + ow) * a.Cout + co;
            float v = __builtin_fmaf(acc[i][r], s3, b3);
            if (a.res) v += a.res[off];
            a.y[off] = v;
        }
    }
}

template <int S>
static int mb_launch(MbArgs &a, int B, hipStream_t stream) {
    using T = MbTile<S>;
    a.ntd = fsg_cdiv(a.Do, T::TD);
    a.nth = fsg_cdiv(a.Ho, T::TH);
    a.ntw = fsg_cdiv(a.Wo, T::TW);
    const long blocks = (long)B * a.ntd * a.nth * a.ntw;
    FSG_REQUIRE(blocks < (1L << 31), "fsg_mbconv3d_fwd_f32: bad shape: too many tiles");
    const size_t bytes = mb_lds_floats(T::NROWS, T::NOUT, a.K1p) * sizeof(float);
    FSG_REQUIRE(bytes <= FSG_LDS_WHOLE_CU, "fsg_mbconv3d_fwd_f32: the tile needs %zu bytes of LDS", bytes);
    FSG_GRANT_LDS("fsg_mbconv3d_fwd_f32", mbconv3d_kernel<S>, bytes);
    mbconv3d_kernel<S><<<dim3((unsigned)blocks), MB_THREADS, bytes, stream>>>(a);
    FSG_CHECK_LAUNCH("fsg_mbconv3d_fwd_f32");
    return FSG_OK;
}

// ------------------------------------------------------------------------------------------------ patch accumulation
constexpr int PA_THREADS = 256;

// source cell and weight of output index i of a x2 linear up-sampling (align_corners = False) of n cells
static __device__ __forceinline__ void up2_src(int i, int n, int &i0, int &i1, float &l1) {
    float s = 0.5f * ((float)i + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 > n - 1 ? n - 1 : i0;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

struct PaArgs {
    const float *logits;   // (K, d, h, w) of this patch
    const float *wmap;     // (2d, 2h, 2w) | NULL
    float *sum;            // (K, D, H, W) of the patch's item
    float *wsum;           // (D, H, W)
    int K, d, h, w;
    int z0, y0, x0;        // the patch's corner in the volume
    int cz, cy, cx;        // the first patch voxel that survives the crop
    int nz, ny, nx;        // extent of the region
    int D, H, W;
};

__global__ __launch_bounds__(PA_THREADS) void patch_accumulate_kernel(const PaArgs a) {
    const long i = (long)blockIdx.x * PA_THREADS + threadIdx.x;
    if (i >= (long)a.nz * a.ny * a.nx) return;
    const int rx = (int)(i % a.nx), ry = (int)((i / a.nx) % a.ny), rz = (int)(i / ((long)a.nx * a.ny));
    const int pz = rz + a.cz, py = ry + a.cy, px = rx + a.cx;
    int d0, d1, h0, h1, w0, w1;
    float ld, lh, lw;
    up2_src(pz, a.d, d0, d1, ld);
    up2_src(py, a.h, h0, h1, lh);
    up2_src(px, a.w, w0, w1, lw);
    const float md = 1.f - ld, mh = 1.f - lh, mw = 1.f - lw;
    const size_t cs = (size_t)a.d * a.h * a.w;
    const size_t o00 = ((size_t)d0 * a.h + h0) * a.w, o01 = ((size_t)d0 * a.h + h1) * a.w, o10 = ((size_t)d1 * a.h + h0) * a.w,
                 o11 = ((size_t)d1 * a.h + h1) * a.w;
    auto logit = [&](int k) {
        const float *p = a.logits + k * cs;
        return md * (mh * (mw * p[o00 + w0] + lw * p[o00 + w1]) + lh * (mw * p[o01 + w0] + lw * p[o01 + w1])) +
               ld * (mh * (mw * p[o10 + w0] + lw * p[o10 + w1]) + lh * (mw * p[o11 + w0] + lw * p[o11 + w1]));
    };
    float mx = logit(0);
    for (int k = 1; k < a.K; ++k) mx = fmaxf(mx, logit(k));
    float den = 0.f;
    for (int k = 0; k < a.K; ++k) den += __expf(logit(k) - mx);
    const float g = a.wmap ? a.wmap[((size_t)pz * (2 * a.h) + py) * (2 * a.w) + px] : 1.f;
    const size_t vs = (size_t)a.D * a.H * a.W;
    const size_t vo = ((size_t)(a.z0 + rz) * a.H + (a.y0 + ry)) * a.W + (a.x0 + rx);
    for (int k = 0; k < a.K; ++k) a.sum[k * vs + vo] += __expf(logit(k) - mx) / den * g;
    a.wsum[vo] += g;
}

__global__ __launch_bounds__(PA_THREADS) void patch_finalize_kernel(const float *sum, const float *wsum, int K, long vs, long total,
                                                                    float *out) {
    const long i = (long)blockIdx.x * PA_THREADS + threadIdx.x;
    if (i >= total) return;
    const long b = i / vs, v = i - b * vs;
    const float *s = sum + (size_t)b * K * vs + v;
    float *o = out + (size_t)b * K * vs + v;
    const float wn = wsum[i];
    float mx = s[0] / wn;
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, s[(size_t)k * vs] / wn);
    float den = 0.f;
    for (int k = 0; k < K; ++k) den += __expf(s[(size_t)k * vs] / wn - mx);
    for (int k = 0; k < K; ++k) o[(size_t)k * vs] = __expf(s[(size_t)k * vs] / wn - mx) / den;
}

}   // namespace

extern "C" {

int fsg_mbconv3d_fwd_f32(const float *x, const float *w1, const float *s1, const float *b1, const float *wd, const float *s2,
                         const float *b2, const float *w3, const float *s3, const float *b3, int B, int Cin, int Cmid, int Cout,
                         int D, int H, int W, int stride, int first, int residual, float *y, fsg_stream_t stream) {
    FSG_REQUIRE(x && w1 && s1 && b1 && wd && s2 && b2 && w3 && s3 && b3 && y, "fsg_mbconv3d_fwd_f32: NULL pointer");
    FSG_REQUIRE(x != y, "fsg_mbconv3d_fwd_f32: x and y must differ");
    FSG_REQUIRE(B >= 1 && D >= 1 && H >= 1 && W >= 1, "fsg_mbconv3d_fwd_f32: bad shape: B=%d D=%d H=%d W=%d must be >= 1", B, D, H, W);
    FSG_REQUIRE((long)D * H * W < (1L << 31), "fsg_mbconv3d_fwd_f32: bad shape: D H W must be < 2^31");
    FSG_REQUIRE(Cin >= 1 && Cin <= FSG_MBCONV_MAX_CIN, "fsg_mbconv3d_fwd_f32: Cin=%d outside 1..64", Cin);
    FSG_REQUIRE(Cmid >= 16 && Cmid <= FSG_MBCONV_MAX_CMID && Cmid % 16 == 0, "fsg_mbconv3d_fwd_f32: Cmid=%d must be a multiple of 16 in 16..384", Cmid);
    FSG_REQUIRE(Cout >= 1 && Cout <= FSG_MBCONV_MAX_COUT, "fsg_mbconv3d_fwd_f32: Cout=%d outside 1..64", Cout);
    FSG_REQUIRE(stride == 1 || stride == 2, "fsg_mbconv3d_fwd_f32: stride=%d must be 1 or 2", stride);
    FSG_REQUIRE(!first || Cin == 1, "fsg_mbconv3d_fwd_f32: the dense first layer takes one input channel, got Cin=%d", Cin);
    FSG_REQUIRE(!residual || (!first && stride == 1 && Cin == Cout),
                "fsg_mbconv3d_fwd_f32: the residual add needs stride 1, Cin == Cout and the 1x1x1 expand stage");
    MbArgs a;
    a.x = x, a.w1 = w1, a.s1 = s1, a.b1 = b1, a.wd = wd, a.s2 = s2, a.b2 = b2, a.w3 = w3, a.s3 = s3, a.b3 = b3;
    a.res = residual ? x : nullptr;
    a.y = y;
    a.Di = D, a.Hi = H, a.Wi = W;
    a.Dm = first ? (D - 1) / 2 + 1 : D, a.Hm = first ? (H - 1) / 2 + 1 : H, a.Wm = first ? (W - 1) / 2 + 1 : W;
    a.Do = (a.Dm - 1) / stride + 1, a.Ho = (a.Hm - 1) / stride + 1, a.Wo = (a.Wm - 1) / stride + 1;
    a.Cin = Cin, a.Cmid = Cmid, a.Cout = Cout;
    a.K1 = first ? 27 : Cin;
    a.K1p = (a.K1 + 3) & ~3;
    a.first = first ? 1 : 0;
    return stride == 1 ? mb_launch<1>(a, B, (hipStream_t)stream) : mb_launch<2>(a, B, (hipStream_t)stream);
}

int fsg_patch_accumulate_f32(const float *logits, int P, int K, int pd, int ph, int pw, const int *starts, const float *wmap,
                             float *sum, float *wsum, int B, int D, int H, int W, fsg_stream_t stream) {
    FSG_REQUIRE(logits && starts && sum && wsum, "fsg_patch_accumulate_f32: NULL pointer");
    FSG_REQUIRE(P >= 1 && K >= 1 && B >= 1 && D >= 1 && H >= 1 && W >= 1, "fsg_patch_accumulate_f32: bad shape");
    FSG_REQUIRE(pd >= 2 && ph >= 2 && pw >= 2 && pd % 2 == 0 && ph % 2 == 0 && pw % 2 == 0,
                "fsg_patch_accumulate_f32: patch %dx%dx%d: every extent must be even and >= 2", pd, ph, pw);
    FSG_REQUIRE((long)D * H * W < (1L << 31) && (long)pd * ph * pw < (1L << 31),
                "fsg_patch_accumulate_f32: bad shape: D H W and the patch must hold fewer than 2^31 voxels");
    for (int p = 0; p < P; ++p) {
        const int *s = starts + 4 * p;
        FSG_REQUIRE(s[0] >= 0 && s[0] < B && s[1] >= 0 && s[1] < D && s[2] >= 0 && s[2] < H && s[3] >= 0 && s[3] < W,
                    "fsg_patch_accumulate_f32: patch %d starts at item %d, (%d, %d, %d): outside the volume", p, s[0], s[1], s[2], s[3]);
    }
    const size_t vs = (size_t)D * H * W, ps = (size_t)K * (pd / 2) * (ph / 2) * (pw / 2);
    for (int p = 0; p < P; ++p) {
        const int *s = starts + 4 * p;
        PaArgs a;
        a.logits = logits + p * ps;
        a.wmap = wmap;
        a.sum = sum + (size_t)s[0] * K * vs;
        a.wsum = wsum + (size_t)s[0] * vs;
        a.K = K, a.d = pd / 2, a.h = ph / 2, a.w = pw / 2;
        a.z0 = s[1], a.y0 = s[2], a.x0 = s[3];
        // a patch that overhangs the volume was replicate-padded, the larger half of an odd padding in front
        a.nz = pd < D - s[1] ? pd : D - s[1], a.ny = ph < H - s[2] ? ph : H - s[2], a.nx = pw < W - s[3] ? pw : W - s[3];
        a.cz = (pd - a.nz + 1) / 2, a.cy = (ph - a.ny + 1) / 2, a.cx = (pw - a.nx + 1) / 2;
        a.D = D, a.H = H, a.W = W;
        const long n = (long)a.nz * a.ny * a.nx;
        patch_accumulate_kernel<<<dim3((unsigned)fsg_cdiv(n, PA_THREADS)), PA_THREADS, 0, (hipStream_t)stream>>>(a);
        FSG_CHECK_LAUNCH("fsg_patch_accumulate_f32");
    }
    return FSG_OK;
}

int fsg_patch_finalize_f32(const float *sum, const float *wsum, int B, int K, int D, int H, int W, float *out, fsg_stream_t stream) {
    FSG_REQUIRE(sum && wsum && out, "fsg_patch_finalize_f32: NULL pointer");
    FSG_REQUIRE(B >= 1 && K >= 1 && D >= 1 && H >= 1 && W >= 1, "fsg_patch_finalize_f32: bad shape");
    FSG_REQUIRE((long)D * H * W < (1L << 31) && (long)B * D * H * W < (1L << 39), "fsg_patch_finalize_f32: bad shape: volume too large");
    const long vs = (long)D * H * W, total = (long)B * vs;
    patch_finalize_kernel<<<dim3((unsigned)fsg_cdiv(total, PA_THREADS)), PA_THREADS, 0, (hipStream_t)stream>>>(sum, wsum, K, vs, total, out);
    FSG_CHECK_LAUNCH("fsg_patch_finalize_f32");
    return FSG_OK;
}

}   // extern "C"
