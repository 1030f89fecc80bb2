// Random-walker lobe filling and lobes-to-fissures on label volumes -- include/fsg_hip.h: fsg_random_walk_workspace_bytes,
// fsg_random_walk_prep, fsg_random_walk_iterate, fsg_random_walk_finish, fsg_lobes_to_fissures_u8.
// Replaces compute_laplace_matrix + random_walk (data_processing/random_walk.py:15-116, with its pyamg solve :309-321) and
// the tensor part of fill_lobes / lobes_to_fissures (data_processing/find_lobes.py:17-30, 47-88).
//
// The operator is never a matrix.  Nodes are the voxels of a (D, H, W) volume, edges the axis neighbours inside it, and
//   w_ij = (im_i == im_j ? 1 : 0.01)                 'binary'    (im held as bytes)
//   w_ij = exp(-(im_i - im_j)^2 / 128)               'intensity' (im fp32; recomputed every iteration)
//   L    = diag(1e-5 + sum_j w_ij) - W               the degree counts EVERY in-volume neighbour (random_walk.py:70-75)
// random_walk() keeps the rows and columns of the unknown voxels (in the mask, no seed) and moves the seeded columns to the
// right-hand side; a neighbour outside the mask loses its column but stays in the degree, so it absorbs with value 0.  All
// vectors are planar (B, K, D, H, W) fp32 and ZERO at every voxel that is not unknown: the stencil then reads its six
// neighbours unconditionally and needs the state byte of its own voxel only.
//
// Jacobi-preconditioned conjugate gradients, all B K systems at once, a thread per voxel looping over the K systems:
//   prep     state byte, 1 / diagonal, r = b, x = p = q = 0, partials of r.z and r.r; a one-block-per-system scalar launch
//            turns them into rz, |b|^2 and the frozen flag of an all-zero right-hand side
//   stencil  p' = z + beta p with z = r / diagonal, written once and RECOMPUTED at the six neighbours by the same expression
//            (same bits, so the operator stays symmetric); q = A p'; partials of p'.q.  p is double-buffered by iteration parity
//            because neighbours read the old one while it is replaced
//   update   every workgroup sums the p'.q partials itself (fixed order) -> alpha = rz / p'.q; x += alpha p'; r -= alpha q;
//            partials of r.z and r.r
//   scalars  one workgroup per system sums those -> beta, rz, and freezes the system once |r| <= tol |b|: alpha = beta = 0
//            from then on and the streaming launches skip it, so its x never changes again and does not depend on how long
//            the rest of the batch runs
// Every reduction is carried in fp64 and summed in a fixed order (lanes by a shuffle tree, waves and workgroups ascending);
// there are no atomics: the same input gives the same bits.  The host only looks at the per-system stopping iterate.
#include "fsg_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXK = FSG_RW_MAX_LABELS;
constexpr int MAX_BLOCKS = 1024;   // streaming launches are grid-strided; this is also the number of partials per system
constexpr uint8_t ST_OUTSIDE = 0, ST_UNKNOWN = 1, ST_SEED0 = 2;   // ST_SEED0 + (label - 1); 255: a seed of no system

struct SysState {   // one per system, at the head of the workspace
    double rz, bb, rr;
    float beta;
    int frozen;
};

struct Layout {
    SysState *sys;
    double *pq, *rzp, *rrp;   // [B K][nblk]
    uint8_t *state;           // [B][V]
    float *dinv;              // [B][V]
    float *x, *r, *q, *p[2];  // [B K][V]
    size_t bytes;
};

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

inline int num_blocks(long V) { return (int)(V / NT + 1 < MAX_BLOCKS ? (V + NT - 1) / NT : MAX_BLOCKS); }

Layout make_layout(void *base, int B, int K, long V) {
    Layout l;
    const size_t S = (size_t)B * K, nblk = num_blocks(V);
    char *c = (char *)base;
    size_t off = 0;
    auto take = [&](size_t n) { char *p = c + off; off += align256(n); return p; };
    l.sys = (SysState *)take(S * sizeof(SysState));
    l.pq = (double *)take(S * nblk * sizeof(double));
    l.rzp = (double *)take(S * nblk * sizeof(double));
    l.rrp = (double *)take(S * nblk * sizeof(double));
    l.state = (uint8_t *)take((size_t)B * V);
    l.dinv = (float *)take((size_t)B * V * sizeof(float));
    l.x = (float *)take(S * V * sizeof(float));
    l.r = (float *)take(S * V * sizeof(float));
    l.q = (float *)take(S * V * sizeof(float));
    l.p[0] = (float *)take(S * V * sizeof(float));
    l.p[1] = (float *)take(S * V * sizeof(float));
    l.bytes = off;
    return l;
}

struct Dims {
    int B, D, H, W;
    long V;
};

// the six in-volume neighbours of voxel v in the order (z-, z+, y-, y+, x-, x+); a missing one points at v itself
struct Nbrs {
    long at[6];
    bool in[6];
};
__device__ __forceinline__ Nbrs neighbours(long v, const Dims &d) {
    const int x = (int)(v % d.W), y = (int)((v / d.W) % d.H), z = (int)(v / ((long)d.W * d.H));
    const long sy = d.W, sz = (long)d.W * d.H;
    Nbrs n;
    n.in[0] = z > 0;        n.at[0] = n.in[0] ? v - sz : v;
    n.in[1] = z + 1 < d.D;  n.at[1] = n.in[1] ? v + sz : v;
    n.in[2] = y > 0;        n.at[2] = n.in[2] ? v - sy : v;
    n.in[3] = y + 1 < d.H;  n.at[3] = n.in[3] ? v + sy : v;
    n.in[4] = x > 0;        n.at[4] = n.in[4] ? v - 1 : v;
    n.in[5] = x + 1 < d.W;  n.at[5] = n.in[5] ? v + 1 : v;
    return n;
}

// MODE 0: 'binary' on bytes (random_walk.py:52), MODE 1: 'intensity' on fp32 with sigma = 8 (:49)
template <int MODE>
struct Image;
template <>
struct Image<0> {
    typedef uint8_t T;
    static __device__ __forceinline__ float weight(uint8_t a, uint8_t b) { return a == b ? 1.f : 0.01f; }
};
template <>
struct Image<1> {
    typedef float T;
    static __device__ __forceinline__ float weight(float a, float b) {
        const float d = a - b;
        return expf(-(d * d) / 128.f);
    }
};

// the six weights of voxel v (0 for a missing neighbour) and the diagonal 1e-5 + degree, always summed in this order
template <int MODE>
__device__ __forceinline__ float weights(const typename Image<MODE>::T *im, long v, const Nbrs &n, float (&w)[6]) {
    const typename Image<MODE>::T c = im[v];
    float deg = 0.f;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        w[e] = n.in[e] ? Image<MODE>::weight(c, im[n.at[e]]) : 0.f;
        deg = deg + w[e];
    }
    return 1e-5f + deg;
}

// random_walk.py:95-101: outside the mask / unknown / seeded with label 1..K
template <typename LT>
__device__ __forceinline__ uint8_t voxel_state(const LT *labels, const uint8_t *mask, long v, int K) {
    if (mask && mask[v] == 0) return ST_OUTSIDE;
    const long lab = (long)labels[v];
    if (lab == 0) return ST_UNKNOWN;
    return lab >= 1 && lab <= K ? (uint8_t)(ST_SEED0 + lab - 1) : (uint8_t)255;
}

// sums of one fp64 value per thread over the workgroup in a fixed order: lanes by the shuffle tree, waves ascending.
// Every thread receives the total.  `red` holds NT / 64 doubles.
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum_lane0(v);
    __syncthreads();   // (the previous use of red is over)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) s = s + red[i];
    return s;
}

template <int MODE, typename LT, int K>
__global__ __launch_bounds__(NT) void prep_kernel(Dims d, const typename Image<MODE>::T *__restrict__ im,
                                                   const LT *__restrict__ labels, const uint8_t *__restrict__ mask, Layout l) {
    __shared__ double red[NT / 64];
    const int b = blockIdx.y, nblk = gridDim.x;
    const long V = d.V;
    im += b * V;
    labels += b * V;
    if (mask) mask += b * V;
    double rz[K], rr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rz[k] = rr[k] = 0.0;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < V; v += (long)nblk * NT) {
        const uint8_t st = voxel_state(labels, mask, v, K);
        float bk[K], di = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) bk[k] = 0.f;
        if (st == ST_UNKNOWN) {
            const Nbrs n = neighbours(v, d);
            float w[6];
            const float diag = weights<MODE>(im, v, n, w);
            di = 1.f / diag;
#pragma unroll
            for (int e = 0; e < 6; ++e) {
                if (!n.in[e]) continue;
                const uint8_t sn = voxel_state(labels, mask, n.at[e], K);
#pragma unroll
                for (int k = 0; k < K; ++k) bk[k] = bk[k] + (sn == ST_SEED0 + k ? w[e] : 0.f);   // -B^T onehot (:105-111)
            }
        }
        l.state[b * V + v] = st;
        l.dinv[b * V + v] = di;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long o = ((long)b * K + k) * V + v;
            l.x[o] = 0.f;
            l.r[o] = bk[k];
            l.q[o] = 0.f;
            l.p[0][o] = 0.f;
            l.p[1][o] = 0.f;
            rz[k] += (double)bk[k] * (double)(di * bk[k]);
            rr[k] += (double)bk[k] * (double)bk[k];
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double a = block_sum(rz[k], red), c = block_sum(rr[k], red);
        if (threadIdx.x == 0) {
            l.rzp[((long)b * K + k) * nblk + blockIdx.x] = a;
            l.rrp[((long)b * K + k) * nblk + blockIdx.x] = c;
        }
    }
}

template <int MODE, int K>
__global__ __launch_bounds__(NT) void stencil_kernel(Dims d, const typename Image<MODE>::T *__restrict__ im, Layout l, int parity) {
    __shared__ double red[NT / 64];
    const int b = blockIdx.y, nblk = gridDim.x;
    const long V = d.V;
    im += b * V;
    const uint8_t *state = l.state + b * V;
    const float *dinv = l.dinv + b * V;
    const float *pold = l.p[parity] + (long)b * K * V, *r = l.r + (long)b * K * V;
    float *pnew = l.p[parity ^ 1] + (long)b * K * V, *q = l.q + (long)b * K * V;
    float beta[K];
    bool live[K];
    double pq[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const SysState &s = l.sys[b * K + k];
        beta[k] = s.beta;
        live[k] = s.frozen == 0;
        pq[k] = 0.0;
    }
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < V; v += (long)nblk * NT) {
        if (state[v] != ST_UNKNOWN) continue;
        const Nbrs n = neighbours(v, d);
        float w[6], dn[6];
        const float diag = weights<MODE>(im, v, n, w);
        const float dc = dinv[v];
#pragma unroll
        for (int e = 0; e < 6; ++e) dn[e] = dinv[n.at[e]];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!live[k]) continue;
            const float *rk = r + k * V, *pk = pold + k * V;
            const float pc = dc * rk[v] + beta[k] * pk[v];
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < 6; ++e) acc = acc + w[e] * (dn[e] * rk[n.at[e]] + beta[k] * pk[n.at[e]]);
            const float qv = diag * pc - acc;
            pnew[k * V + v] = pc;
            q[k * V + v] = qv;
            pq[k] += (double)pc * (double)qv;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double a = block_sum(pq[k], red);
        if (threadIdx.x == 0) l.pq[((long)b * K + k) * nblk + blockIdx.x] = a;
    }
}

template <int K>
__global__ __launch_bounds__(NT) void update_kernel(Dims d, Layout l, int parity) {
    __shared__ double red[NT / 64];
    const int b = blockIdx.y, nblk = gridDim.x;
    const long V = d.V;
    const uint8_t *state = l.state + b * V;
    const float *dinv = l.dinv + b * V;
    const float *p = l.p[parity ^ 1] + (long)b * K * V, *q = l.q + (long)b * K * V;
    float *x = l.x + (long)b * K * V, *r = l.r + (long)b * K * V;
    float alpha[K];
    bool live[K];
    double rz[K], rr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const SysState &s = l.sys[b * K + k];
        live[k] = s.frozen == 0;
        alpha[k] = 0.f;
        rz[k] = rr[k] = 0.0;
        if (live[k]) {   // (uniform over the workgroup)
            const double *part = l.pq + ((long)b * K + k) * nblk;
            double a = 0.0;
            for (int i = threadIdx.x; i < nblk; i += NT) a += part[i];
            const double pq = block_sum(a, red);
            alpha[k] = pq > 0.0 ? (float)(s.rz / pq) : 0.f;
        }
    }
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < V; v += (long)nblk * NT) {
        if (state[v] != ST_UNKNOWN) continue;
        const float dc = dinv[v];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!live[k]) continue;
            const long o = k * V + v;
            const float xv = x[o] + alpha[k] * p[o];
            const float rv = r[o] - alpha[k] * q[o];
            x[o] = xv;
            r[o] = rv;
            rz[k] += (double)rv * (double)(dc * rv);
            rr[k] += (double)rv * (double)rv;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double a = block_sum(rz[k], red), c = block_sum(rr[k], red);
        if (threadIdx.x == 0) {
            l.rzp[((long)b * K + k) * nblk + blockIdx.x] = a;
            l.rrp[((long)b * K + k) * nblk + blockIdx.x] = c;
        }
    }
}

// one workgroup per system.  iteration < 0: after prep (rz, |b|^2; an all-zero right-hand side is solved by x = 0);
// otherwise after the update of iteration `iteration` (0-based): beta, rz, the stop test
__global__ __launch_bounds__(NT) void scalars_kernel(Layout l, int nblk, int iteration, double tol2, int *stop_iter, float *relres) {
    __shared__ double red[NT / 64];
    const int s = blockIdx.x;
    SysState &st = l.sys[s];
    if (iteration >= 0 && st.frozen) return;   // (uniform)
    double a = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NT) {
        a += l.rzp[(long)s * nblk + i];
        c += l.rrp[(long)s * nblk + i];
    }
    const double rz = block_sum(a, red), rr = block_sum(c, red);
    if (threadIdx.x != 0) return;
    if (iteration < 0) {
        st.rz = rz;
        st.bb = rr;
        st.rr = rr;
        st.beta = 0.f;
        st.frozen = rr == 0.0;
        stop_iter[s] = st.frozen ? 0 : -1;
        relres[s] = 0.f;
        return;
    }
    const bool done = rr <= tol2 * st.bb;
    st.beta = done || !(st.rz > 0.0) ? 0.f : (float)(rz / st.rz);
    st.rz = rz;
    st.rr = rr;
    st.frozen = done;
    relres[s] = (float)sqrt(rr / st.bb);
    if (done) stop_iter[s] = iteration + 1;
}

// probabilities (B, D, H, W, K) and the filled labels: first-index argmax + 1 inside the mask (find_lobes.py:27)
template <int K>
__global__ __launch_bounds__(NT) void finish_kernel(Dims d, Layout l, float *__restrict__ prob, uint8_t *__restrict__ filled) {
    const int b = blockIdx.y;
    const long V = d.V;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < V; v += (long)gridDim.x * NT) {
        const uint8_t st = l.state[b * V + v];
        float pr[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            pr[k] = st == ST_UNKNOWN ? l.x[((long)b * K + k) * V + v] : (st == ST_SEED0 + k ? 1.f : 0.f);
        int best = 0;
#pragma unroll
        for (int k = 1; k < K; ++k)
            if (pr[k] > pr[best]) best = k;
        if (prob) {
#pragma unroll
            for (int k = 0; k < K; ++k) prob[(b * V + v) * K + k] = pr[k];
        }
        if (filled) filled[b * V + v] = st == ST_OUTSIDE ? 0 : (uint8_t)(best + 1);
    }
}

// find_lobes.py:47-88 on labels: bit c of `seen` = channel c of the one-hot volume dilated by the 6-neighbour cross
__global__ __launch_bounds__(NT) void fissures_kernel(Dims d, const uint8_t *__restrict__ lobes, int n_lobes,
                                                      uint8_t *__restrict__ out) {
    const int b = blockIdx.y;
    const long V = d.V;
    lobes += b * V;
    for (long v = (long)blockIdx.x * NT + threadIdx.x; v < V; v += (long)gridDim.x * NT) {
        const Nbrs n = neighbours(v, d);
        unsigned seen = 1u << (lobes[v] & 31);
#pragma unroll
        for (int e = 0; e < 6; ++e) seen |= 1u << (lobes[n.at[e]] & 31);   // (a missing neighbour repeats the centre: zero padding)
        auto both = [seen](int a, int c) { return ((seen >> a) & (seen >> c) & 1u) != 0; };
        uint8_t f = both(3, 4) ? 1 : 0;                                    // left oblique
        if (both(1, 2) || (n_lobes == 5 && both(1, 5))) f = 2;             // right oblique overwrites it
        if (n_lobes == 5 && both(2, 5)) f = 3;                             // right horizontal overwrites both
        out[b * V + v] = f;
    }
}

int check_dims(const char *name, int B, int K, int D, int H, int W, Dims &d) {
    FSG_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535, "%s: bad shape B=%d D=%d H=%d W=%d", name, B, D, H, W);
    FSG_REQUIRE((long)B * (K > 0 ? K : 1) * D * H * W < (1L << 31), "%s: B K D H W = %d %d %d %d %d exceeds 2^31 elements", name, B,
                K, D, H, W);
    d.B = B; d.D = D; d.H = H; d.W = W;
    d.V = (long)D * H * W;
    return FSG_OK;
}

int check_solver_args(const char *name, int mode, int B, int K, int D, int H, int W, const void *workspace, size_t workspace_bytes,
                      Dims &d) {
    FSG_REQUIRE(mode == FSG_RW_BINARY || mode == FSG_RW_INTENSITY, "%s: unknown edge-weight mode %d", name, mode);
    if (K < 1 || K > MAXK) {
        fsg_set_error("%s: %d label systems (1..%d are built)", name, K, MAXK);
        return K < 1 ? FSG_ERR_ARG : FSG_ERR_UNSUPPORTED;
    }
    if (int rc = check_dims(name, B, K, D, H, W, d)) return rc;
    const size_t need = fsg_random_walk_workspace_bytes(B, K, D, H, W);
    FSG_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: NULL or misaligned workspace", name);
    return FSG_OK;
}

#define RW_FOR_K(K, ...)                       \
    switch (K) {                               \
        case 1: { constexpr int KK = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int KK = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int KK = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int KK = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int KK = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int KK = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int KK = 7; __VA_ARGS__; } break; \
        default: { constexpr int KK = 8; __VA_ARGS__; } break; \
    }

}  // namespace

extern "C" size_t fsg_random_walk_workspace_bytes(int B, int K, int D, int H, int W) {
    if (B < 1 || K < 1 || D < 1 || H < 1 || W < 1) return 0;
    return make_layout(nullptr, B, K, (long)D * H * W).bytes;
}

extern "C" int fsg_random_walk_prep(const void *im, int mode, const void *labels, int labels_are_i32, const uint8_t *mask, int B,
                                    int K, int D, int H, int W, void *workspace, size_t workspace_bytes, int32_t *stop_iter,
                                    float *relres, fsg_stream_t stream) {
    const char *name = "fsg_random_walk_prep";
    Dims d;
    if (int rc = check_solver_args(name, mode, B, K, D, H, W, workspace, workspace_bytes, d)) return rc;
    FSG_REQUIRE(im && labels && stop_iter && relres, "%s: NULL pointer", name);
    const Layout l = make_layout(workspace, B, K, d.V);
    const int nblk = num_blocks(d.V);
    const dim3 grid(nblk, B);
    hipStream_t s = (hipStream_t)stream;
    const int variant = mode * 2 + (labels_are_i32 ? 1 : 0);
    RW_FOR_K(K, {
        switch (variant) {
            case 0: prep_kernel<0, uint8_t, KK><<<grid, NT, 0, s>>>(d, (const uint8_t *)im, (const uint8_t *)labels, mask, l); break;
            case 1: prep_kernel<0, int32_t, KK><<<grid, NT, 0, s>>>(d, (const uint8_t *)im, (const int32_t *)labels, mask, l); break;
            case 2: prep_kernel<1, uint8_t, KK><<<grid, NT, 0, s>>>(d, (const float *)im, (const uint8_t *)labels, mask, l); break;
            default: prep_kernel<1, int32_t, KK><<<grid, NT, 0, s>>>(d, (const float *)im, (const int32_t *)labels, mask, l); break;
        }
    });
    FSG_CHECK_LAUNCH(name);
    scalars_kernel<<<B * K, NT, 0, s>>>(l, nblk, -1, 0.0, stop_iter, relres);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_random_walk_iterate(const void *im, int mode, int B, int K, int D, int H, int W, int first_iteration,
                                       int iterations, float tol, void *workspace, size_t workspace_bytes, int32_t *stop_iter,
                                       float *relres, fsg_stream_t stream) {
    const char *name = "fsg_random_walk_iterate";
    Dims d;
    if (int rc = check_solver_args(name, mode, B, K, D, H, W, workspace, workspace_bytes, d)) return rc;
    FSG_REQUIRE(first_iteration >= 0 && iterations >= 0 && tol >= 0.f, "%s: bad iteration range %d + %d or tolerance %g", name,
                first_iteration, iterations, (double)tol);
    FSG_REQUIRE(im && stop_iter && relres, "%s: NULL pointer", name);
    const Layout l = make_layout(workspace, B, K, d.V);
    const int nblk = num_blocks(d.V);
    const dim3 grid(nblk, B);
    hipStream_t s = (hipStream_t)stream;
    const double tol2 = (double)tol * (double)tol;
    for (int it = first_iteration; it < first_iteration + iterations; ++it) {
        const int parity = it & 1;
        RW_FOR_K(K, {
            if (mode == FSG_RW_BINARY) stencil_kernel<0, KK><<<grid, NT, 0, s>>>(d, (const uint8_t *)im, l, parity);
            else stencil_kernel<1, KK><<<grid, NT, 0, s>>>(d, (const float *)im, l, parity);
            update_kernel<KK><<<grid, NT, 0, s>>>(d, l, parity);
        });
        scalars_kernel<<<B * K, NT, 0, s>>>(l, nblk, it, tol2, stop_iter, relres);
        FSG_CHECK_LAUNCH(name);
    }
    return FSG_OK;
}

extern "C" int fsg_random_walk_finish(int B, int K, int D, int H, int W, const void *workspace, size_t workspace_bytes, float *prob,
                                      uint8_t *filled, fsg_stream_t stream) {
    const char *name = "fsg_random_walk_finish";
    Dims d;
    if (int rc = check_solver_args(name, FSG_RW_BINARY, B, K, D, H, W, workspace, workspace_bytes, d)) return rc;
    FSG_REQUIRE(prob || filled, "%s: no output asked for", name);
    const Layout l = make_layout(const_cast<void *>(workspace), B, K, d.V);
    const dim3 grid(num_blocks(d.V), B);
    RW_FOR_K(K, (finish_kernel<KK><<<grid, NT, 0, (hipStream_t)stream>>>(d, l, prob, filled)));
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

extern "C" int fsg_lobes_to_fissures_u8(const uint8_t *lobes, int B, int D, int H, int W, int n_lobes, uint8_t *fissures,
                                        fsg_stream_t stream) {
    const char *name = "fsg_lobes_to_fissures_u8";
    Dims d;
    FSG_REQUIRE(n_lobes >= 4 && n_lobes <= 31, "%s: %d lobe labels (at least 4, at most 31)", name, n_lobes);
    if (int rc = check_dims(name, B, 1, D, H, W, d)) return rc;
    FSG_REQUIRE(lobes && fissures, "%s: NULL pointer", name);
    fissures_kernel<<<dim3(num_blocks(d.V), B), NT, 0, (hipStream_t)stream>>>(d, lobes, n_lobes, fissures);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}
