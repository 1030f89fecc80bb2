// Adam over one flat fp32 buffer -- include/fsg_hip.h: fsg_adam_flat_f32, fsg_adam_flat_segments_f32.
//
// The reference's optimizer is torch.optim.Adam(model.parameters(), lr, weight_decay) (model_trainer.py:57).  Over the one
// flat buffer of optim.FlatAdam torch's fused kernel is a single launch, but a chunked one: 64 Ki elements per
// workgroup = 28 workgroups for the 1.8 M parameters of DGCNN-seg on a 256-CU chip (43 us per step in
// profiles/r1_bench_c2_kernel_stats.csv, against 50 MB of traffic = 6 us at HBM rate).  This kernel streams the four
// arrays as float4, 1024 grid-stride workgroups.
//
// The step count lives on the device (the update is replayed inside a hipGraph, so nothing per-step may come from the
// host): every workgroup reads it at entry, the LAST workgroup to finish (ticket counter) increments it -- by then all
// others have consumed the old value.  Update rule = torch's (torch/optim/adam.py, `_single_tensor_adam`):
//   g' = g + wd * p;  m = lerp(m, g', 1-b1);  v = b2 v + (1-b2) g'^2;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
#include "fsg_common.h"

namespace {

constexpr int FSG_ADAM_MAX_CHUNKS = 224;  // by-value table of fsg_adam_flat_segments_f32's kernel: 3.5 KB of kernel arguments

struct AdamState {  // the 8-byte `state` block of the C ABI
    float step;
    unsigned int ticket;
};

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, float b1, float b2, float eps, float wd,
                                         float step_size, float bc2_sqrt) {
    if (wd != 0.f) g = fmaf(wd, p, g);
    m = m + (1.f - b1) * (g - m);
    v = b2 * v + (1.f - b2) * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p -= step_size * (m / denom);
}

// thread 0's two fp64 pow() calls are the longest thing a workgroup does before its first update; every thread therefore REQUESTS
// its first operands before it waits for them, so the loads travel while thread 0 computes (the values are consumed after the
// barrier)
__device__ __forceinline__ void adam_bias_terms(float *sc, const AdamState *state, float lr_host, const float *lr_dev, float b1,
                                                float b2) {
    if (threadIdx.x == 0) {
        const double t = (double)state->step + 1.0;
        const double lr = lr_dev ? (double)lr_dev[0] : (double)lr_host;
        sc[0] = (float)(lr / (1.0 - pow((double)b1, t)));
        sc[1] = (float)sqrt(1.0 - pow((double)b2, t));
    }
    __syncthreads();
}

__device__ __forceinline__ void adam_four(float4 &p, const float4 &g, float4 &m, float4 &v, float b1, float b2, float eps, float wd,
                                          float step_size, float bc2_sqrt) {
    adam_one(p.x, g.x, m.x, v.x, b1, b2, eps, wd, step_size, bc2_sqrt);
    adam_one(p.y, g.y, m.y, v.y, b1, b2, eps, wd, step_size, bc2_sqrt);
    adam_one(p.z, g.z, m.z, v.z, b1, b2, eps, wd, step_size, bc2_sqrt);
    adam_one(p.w, g.w, m.w, v.w, b1, b2, eps, wd, step_size, bc2_sqrt);
}

// the LAST workgroup to finish increments the step: by then all others have consumed the old value
__device__ __forceinline__ void adam_finish(AdamState *state, unsigned int workgroups) {
    __syncthreads();  // every thread of this workgroup is past its read of sc[] (and thread 0 past state->step)
    if (threadIdx.x == 0) {
        const unsigned int done = atomicAdd(&state->ticket, 1u);
        if (done == workgroups - 1) {
            state->step += 1.f;
            state->ticket = 0u;
        }
    }
}

__global__ __launch_bounds__(256) void adam_flat_kernel(float *__restrict__ param, const float *__restrict__ grad,
                                                        float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                        AdamState *__restrict__ state, long n, float lr_host,
                                                        const float *__restrict__ lr_dev, float b1, float b2, float eps,
                                                        float wd) {
    __shared__ float sc[2];
    const long n4 = n >> 2, stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    float4 p, g, m, v;
    if (i < n4) {
        p = reinterpret_cast<float4 *>(param)[i];
        g = reinterpret_cast<const float4 *>(grad)[i];
        m = reinterpret_cast<float4 *>(exp_avg)[i];
        v = reinterpret_cast<float4 *>(exp_avg_sq)[i];
    }
    adam_bias_terms(sc, state, lr_host, lr_dev, b1, b2);
    const float step_size = sc[0], bc2_sqrt = sc[1];
    while (i < n4) {
        adam_four(p, g, m, v, b1, b2, eps, wd, step_size, bc2_sqrt);
        reinterpret_cast<float4 *>(param)[i] = p;
        reinterpret_cast<float4 *>(exp_avg)[i] = m;
        reinterpret_cast<float4 *>(exp_avg_sq)[i] = v;
        i += stride;
        if (i < n4) {
            p = reinterpret_cast<float4 *>(param)[i];
            g = reinterpret_cast<const float4 *>(grad)[i];
            m = reinterpret_cast<float4 *>(exp_avg)[i];
            v = reinterpret_cast<float4 *>(exp_avg_sq)[i];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
        const long t = (n4 << 2) + threadIdx.x;
        float pt = param[t], mt = exp_avg[t], vt = exp_avg_sq[t];
        adam_one(pt, grad[t], mt, vt, b1, b2, eps, wd, step_size, bc2_sqrt);
        param[t] = pt;
        exp_avg[t] = mt;
        exp_avg_sq[t] = vt;
    }
    adam_finish(state, gridDim.x);
}

// The same update with the gradient read where autograd left it: chunk c = blockIdx.x of the by-value table is `count` float4 of
// ONE parameter's gradient, to be applied at float4 offset `off` of the flat arrays (the host cuts the parameters into chunks, so
// a workgroup indexes the table and never searches it).  Workgroups of 1024 threads: one pair of pow() calls and one ticket per
// 1024 float4 instead of per 256 (DGCNN-seg, 631 K parameters: 8.8 us; 256 threads and four workgroups per chunk: 16.3 us).
// The gradient is also stored into the flat gradient buffer, which then holds what one concatenation of the gradients would
// have written.  (`flat_grad` and the chunk gradients carry no __restrict__: a parameter's gradient may BE its slice of the
// flat buffer.)
struct AdamChunks {
    const float *grad[FSG_ADAM_MAX_CHUNKS];
    unsigned int off[FSG_ADAM_MAX_CHUNKS], count[FSG_ADAM_MAX_CHUNKS];
};

__global__ __launch_bounds__(1024) void adam_flat_segments_kernel(float *__restrict__ param, float *flat_grad,
                                                                 float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                                 AdamState *__restrict__ state, AdamChunks chunks, float lr_host,
                                                                 const float *__restrict__ lr_dev, float b1, float b2, float eps,
                                                                 float wd) {
    __shared__ float sc[2];
    const float4 *src = reinterpret_cast<const float4 *>(chunks.grad[blockIdx.x]);
    const long base = chunks.off[blockIdx.x];
    const unsigned int cnt = chunks.count[blockIdx.x], stride = 1024;
    unsigned int i = threadIdx.x;
    float4 p, g, m, v;
    if (i < cnt) {
        p = reinterpret_cast<float4 *>(param)[base + i];
        g = src[i];
        m = reinterpret_cast<float4 *>(exp_avg)[base + i];
        v = reinterpret_cast<float4 *>(exp_avg_sq)[base + i];
    }
    adam_bias_terms(sc, state, lr_host, lr_dev, b1, b2);
    const float step_size = sc[0], bc2_sqrt = sc[1];
    while (i < cnt) {
        reinterpret_cast<float4 *>(flat_grad)[base + i] = g;
        adam_four(p, g, m, v, b1, b2, eps, wd, step_size, bc2_sqrt);
        reinterpret_cast<float4 *>(param)[base + i] = p;
        reinterpret_cast<float4 *>(exp_avg)[base + i] = m;
        reinterpret_cast<float4 *>(exp_avg_sq)[base + i] = v;
        i += stride;
        if (i < cnt) {
            p = reinterpret_cast<float4 *>(param)[base + i];
            g = src[i];
            m = reinterpret_cast<float4 *>(exp_avg)[base + i];
            v = reinterpret_cast<float4 *>(exp_avg_sq)[base + i];
        }
    }
    adam_finish(state, gridDim.x);
}

}  // namespace

extern "C" int fsg_adam_flat_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, void *state, int64_t n,
                                 float lr, const float *lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                 fsg_stream_t stream) {
    FSG_REQUIRE(param && grad && exp_avg && exp_avg_sq && state, "fsg_adam_flat_f32: NULL pointer");
    FSG_REQUIRE(n > 0, "fsg_adam_flat_f32: n=%ld", (long)n);
    FSG_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
                "fsg_adam_flat_f32: the four arrays must be 16-byte aligned");
    FSG_REQUIRE(((uintptr_t)state & 7) == 0, "fsg_adam_flat_f32: state must be 8-byte aligned");
    FSG_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f,
                "fsg_adam_flat_f32: bad hyper-parameters beta1=%g beta2=%g eps=%g", beta1, beta2, eps);
    // four workgroups per CU, grid-stride: every workgroup pays two fp64 pow() in one thread before its first load, so
    // few fat workgroups beat one per 1024 elements (7.8 M parameters: 96 us with 7.6 K workgroups)
    long blocks = ((n >> 2) + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, (AdamState *)state, (long)n, lr, lr_dev, beta1, beta2, eps, weight_decay);
    FSG_CHECK_LAUNCH("fsg_adam_flat_f32");
    return FSG_OK;
}

extern "C" int fsg_adam_flat_segments_f32(float *param, float *flat_grad, float *exp_avg, float *exp_avg_sq, void *state, int64_t n,
                                          const fsg_adam_segments *segments, float lr, const float *lr_dev, float beta1,
                                          float beta2, float eps, float weight_decay, fsg_stream_t stream) {
    FSG_REQUIRE(param && flat_grad && exp_avg && exp_avg_sq && state && segments, "fsg_adam_flat_segments_f32: NULL pointer");
    FSG_REQUIRE(n > 0 && n < (1L << 33), "fsg_adam_flat_segments_f32: n=%ld", (long)n);
    FSG_REQUIRE((((uintptr_t)param | (uintptr_t)flat_grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
                "fsg_adam_flat_segments_f32: the four arrays must be 16-byte aligned");
    FSG_REQUIRE(((uintptr_t)state & 7) == 0, "fsg_adam_flat_segments_f32: state must be 8-byte aligned");
    FSG_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f,
                "fsg_adam_flat_segments_f32: bad hyper-parameters beta1=%g beta2=%g eps=%g", beta1, beta2, eps);
    const int ns = segments->n;
    FSG_REQUIRE(ns >= 1 && ns <= FSG_ADAM_MAX_SEGMENTS, "fsg_adam_flat_segments_f32: 1..%d segments", FSG_ADAM_MAX_SEGMENTS);
    // the segments tile [0, n) in order: every element is updated exactly once, as by fsg_adam_flat_f32
    int64_t at = 0;
    for (int s = 0; s < ns; ++s) {
        FSG_REQUIRE(segments->grad[s] && ((uintptr_t)segments->grad[s] & 15) == 0 && segments->count[s] > 0 &&
                        (segments->count[s] & 3) == 0 && segments->offset[s] == at,
                    "fsg_adam_flat_segments_f32: segment %d must be 16-byte aligned, a multiple of 4 floats and start where "
                    "segment %d ends", s, s - 1);
        at += segments->count[s];
    }
    FSG_REQUIRE(at == n, "fsg_adam_flat_segments_f32: the segments cover %ld of %ld elements", (long)at, (long)n);
    // chunks of at most `per` float4: n / 4 / per whole ones plus at most one short one per segment
    const long n4 = n >> 2, per = fsg_cdiv(n4, (long)(FSG_ADAM_MAX_CHUNKS - ns));
    AdamChunks ch;
    int nc = 0;
    for (int s = 0; s < ns; ++s) {
        const long c4 = segments->count[s] >> 2, o4 = segments->offset[s] >> 2;
        for (long c0 = 0; c0 < c4; c0 += per, ++nc) {
            ch.grad[nc] = segments->grad[s] + 4 * c0;
            ch.off[nc] = (unsigned int)(o4 + c0);
            ch.count[nc] = (unsigned int)(c4 - c0 < per ? c4 - c0 : per);
        }
    }
    for (int c = nc; c < FSG_ADAM_MAX_CHUNKS; ++c) ch.grad[c] = nullptr, ch.off[c] = ch.count[c] = 0;
    // (a thread of a chunk longer than 1024 float4 strides over it: from 0.9 M parameters on)
    hipLaunchKernelGGL(adam_flat_segments_kernel, dim3((unsigned)nc), dim3(1024), 0, (hipStream_t)stream, param,
                       flat_grad, exp_avg, exp_avg_sq, (AdamState *)state, ch, lr, lr_dev, beta1, beta2, eps, weight_decay);
    FSG_CHECK_LAUNCH("fsg_adam_flat_segments_f32");
    return FSG_OK;
}
