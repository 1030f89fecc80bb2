// Device-side helpers shared by the kernels of libfsg_hip.so (gfx950, wave64).  Everything here is a typedef or a static
// forceinline function, so no translation unit gains a symbol.  The rule: a device helper lives in the one kernel file that
// uses it; its SECOND user moves it here instead of copying it.  One line each on WHAT a helper does -- WHY a kernel uses it
// stays at the use site.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ------------------------------------------------------------------------------------------------------- vector types
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------------------ scalars
static __device__ __forceinline__ float lrelu(float u, float slope) { return u > 0.f ? u : u * slope; }
// squared distance of two 3-D points: dx dx, then one fma per further axis
static __device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
// v clamped to [0, hi]
static __device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------------- ordered keys
// order-preserving uint32 image of a float (a < b  <=>  f2o(a) < f2o(b), -0 < +0) and its inverse
static __device__ __forceinline__ unsigned f2o(float d) {
    const unsigned u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
static __device__ __forceinline__ float o2f(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// --------------------------------------------------------------------------------------------------- wave collectives
// sum over the 64 lanes by a __shfl_down tree (float or double): the result is in LANE 0 only
template <typename T>
static __device__ __forceinline__ T wave_sum_lane0(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// one DPP move of a 32-bit value (int or float); a lane without a source reads 0 (BOUND_CTRL) or is left out of the write
// and keeps the 0 it started from (row mask)
template <int CTRL, int ROW_MASK, bool BOUND_CTRL, typename T>
static __device__ __forceinline__ T dpp_mov0(T x) {
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, BOUND_CTRL));
}
// the six-step DPP ladder: Kogge-Stone inside each row of 16 lanes, then the row totals travel down.  After it lane i holds
// the combination over lanes 0..i (an inclusive scan; lane 63 holds the total).  STEP(ctrl, row_mask, bound_ctrl) combines v
// with dpp_mov0<...>(v); 0 must be the identity of the combination.
#define FSG_DPP_LADDER(STEP)                                                                      \
    STEP(0x111, 0xf, true)   /* row_shr:1 */                                                      \
    STEP(0x112, 0xf, true)   /* row_shr:2 */                                                      \
    STEP(0x114, 0xf, true)   /* row_shr:4 */                                                      \
    STEP(0x118, 0xf, true)   /* row_shr:8 */                                                      \
    STEP(0x142, 0xa, false)  /* row_bcast:15 -> rows 1 and 3 */                                   \
    STEP(0x143, 0xc, false)  /* row_bcast:31 -> rows 2 and 3 */
#define FSG_DPP_ADD(ctrl, rm, bc) v += dpp_mov0<ctrl, rm, bc>(v);
#define FSG_DPP_FMAX(ctrl, rm, bc) v = fmaxf(v, dpp_mov0<ctrl, rm, bc>(v));
// inclusive prefix sum over the 64 lanes
static __device__ __forceinline__ int wave_incl_scan(int v) {
    FSG_DPP_LADDER(FSG_DPP_ADD)
    return v;
}
static __device__ __forceinline__ float wave_lane63_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// sum over the 64 lanes on the ladder, returned to EVERY lane (a scalar read of lane 63)
static __device__ __forceinline__ float wave_sum_bcast_f(float v) {
    FSG_DPP_LADDER(FSG_DPP_ADD)
    return wave_lane63_f(v);
}
// maximum of NON-NEGATIVE floats over the 64 lanes (+0 is the identity here), returned to every lane
static __device__ __forceinline__ float wave_max_nonneg_bcast_f(float v) {
    FSG_DPP_LADDER(FSG_DPP_FMAX)
    return wave_lane63_f(v);
}
// one step of the maximum of a 64-bit key over the 64 lanes on the DPP network (6 VALU steps instead of 6 LDS-crossbar
// shuffles): swaps inside the quads, mirrors inside the rows, then the row totals travel down
static __device__ __forceinline__ u64 dpp_max_step(u64 k, const int ctrl) {
    const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
    int olo, ohi;
    switch (ctrl) {   // the control word must be a compile-time constant
        case 0: olo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xf, 0xf, false); ohi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xf, 0xf, false); break;
        case 1: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xf, 0xf, false); ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xf, 0xf, false); break;
        case 2: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xf, 0xf, false); ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xf, 0xf, false); break;
        case 3: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xf, 0xf, false); ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xf, 0xf, false); break;
        case 4: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x142, 0xa, 0xf, false); ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x142, 0xa, 0xf, false); break;
        default: olo = __builtin_amdgcn_update_dpp(lo, lo, 0x143, 0xc, 0xf, false); ohi = __builtin_amdgcn_update_dpp(hi, hi, 0x143, 0xc, 0xf, false); break;
    }
    const u64 o = ((u64)(unsigned)ohi << 32) | (unsigned)olo;
    return o > k ? o : k;
}
// maximum of an unsigned 64-bit key over the 64 lanes, returned to EVERY lane (scalar reads of lane 63).  With the value in
// the high bits and (a constant - index) in the low bits of the key this is an arg-max whose ties go to the lowest index.
static __device__ __forceinline__ u64 wave_max_u64_bcast(u64 k) {
#pragma unroll
    for (int st = 0; st < 6; ++st) k = dpp_max_step(k, st);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
    return ((u64)hi << 32) | lo;
}
// sum of one int per thread over a workgroup of NT threads, and each thread's exclusive prefix; `red` holds NT / 64 ints
template <int NT>
static __device__ __forceinline__ int block_excl_scan(int c, int *red, int &total) {
    const int incl = wave_incl_scan(c);
    __syncthreads();   // (the previous use of red is over)
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        if (w < (int)(threadIdx.x >> 6)) before += red[w];
        total += red[w];
    }
    return before + incl - c;
}
#undef FSG_DPP_ADD
#undef FSG_DPP_FMAX
#undef FSG_DPP_LADDER

// -------------------------------------------------------------------------------------------------------- bf16 pieces
// (a, b) -> packed bf16 pair, a in the low half, round to nearest even
static __device__ __forceinline__ unsigned pk_bf16(float a, float b) {
    bf16x2 v;
    v[0] = (__bf16)a;
    v[1] = (__bf16)b;
    return __builtin_bit_cast(unsigned, v);
}
// peel the leading bf16 piece off a pair of fp32 values: returns it packed and leaves the (exact) remainders in (a, b)
static __device__ __forceinline__ unsigned bf16_peel(float &a, float &b) {
    const unsigned p = pk_bf16(a, b);
    a -= __uint_as_float(p << 16);
    b -= __uint_as_float(p & 0xffff0000u);
    return p;
}
// two fp32 values -> their three bf16 pieces x = h + m + l (+ a remainder below 2^-24 |x|), packed pairwise
static __device__ __forceinline__ void bf16_split3(float a, float b, unsigned &h, unsigned &m, unsigned &l) {
    h = bf16_peel(a, b);
    m = bf16_peel(a, b);
    l = pk_bf16(a, b);
}
// eight fp32 values -> operand fragments of their NP pieces (NP = 3: h, m, l; NP = 1: plain bf16)
template <int NP>
static __device__ __forceinline__ void split8(const float (&x)[8], u32x4 (&p)[NP]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if constexpr (NP == 3) {
            unsigned h, m, l;
            bf16_split3(x[2 * q], x[2 * q + 1], h, m, l);
            p[0][q] = h;
            p[1][q] = m;
            p[2][q] = l;
        } else {
            p[0][q] = pk_bf16(x[2 * q], x[2 * q + 1]);
        }
    }
}
// the three-piece form with named outputs
static __device__ __forceinline__ void split8(const float (&x)[8], u32x4 &h, u32x4 &m, u32x4 &l) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float a = x[2 * q], b = x[2 * q + 1];
        const unsigned ph = bf16_peel(a, b), pm = bf16_peel(a, b);
        h[q] = ph;
        m[q] = pm;
        l[q] = pk_bf16(a, b);
    }
}
// c += a b on v_mfma_f32_32x32x16_bf16 from NP pieces per operand.  NP = 3: six of the nine products, the low-order ones
// first and ah bh last (the order is part of the fp32-grade claim: do not change it)
template <int NP>
static __device__ __forceinline__ f32x16 mfma_split(const u32x4 (&a)[NP], const u32x4 (&b)[NP], f32x16 c) {
    const bf16x8 ah = __builtin_bit_cast(bf16x8, a[0]), bh = __builtin_bit_cast(bf16x8, b[0]);
    if constexpr (NP == 3) {
        const bf16x8 am = __builtin_bit_cast(bf16x8, a[1]), al = __builtin_bit_cast(bf16x8, a[2]);
        const bf16x8 bm = __builtin_bit_cast(bf16x8, b[1]), bl = __builtin_bit_cast(bf16x8, b[2]);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
}

// A DIFFERENT operation: bf16 of a FINITE float, round to nearest even in integer arithmetic, and the two-piece split
// x = hi + lo + r, |r| <= 2^-16 |x| built on it (the kNN coarse image; its error bound is derived in knn_split.hip)
static __device__ __forceinline__ unsigned bf16_rne_finite(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}
static __device__ __forceinline__ float bf16_f(unsigned h) { return __uint_as_float(h << 16); }
struct Bf16Split2 { unsigned hi, lo; };
static __device__ __forceinline__ Bf16Split2 bf16_split2_finite(float v) {
    Bf16Split2 s;
    s.hi = bf16_rne_finite(v);
    s.lo = bf16_rne_finite(v - bf16_f(s.hi));   // v - hi is exact in fp32
    return s;
}

// ----------------------------------------------------------------------------------------------------- buffer gathers
// a wave-uniform pointer the compiler cannot see to be one: both halves through v_readfirstlane
static __device__ __forceinline__ void *uniform_ptr(const void *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return reinterpret_cast<void *>(((uintptr_t)hi << 32) | lo);
}
// raw buffer resource over `bytes` bytes at `base`: a load at an offset outside it returns 0, a store there is dropped
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void *base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}

// row gathers with lanes = channels: the (wave-uniform) row goes into the SCALAR offset of a 4-byte buffer load, the lane's
// channel into its vector offset
struct RowGather {
    __amdgpu_buffer_rsrc_t rs;
    unsigned oob;   // a byte offset outside the resource
    __device__ __forceinline__ RowGather(const float *base, long bytes) {
        const void *p = uniform_ptr(base);
        const int n = __builtin_amdgcn_readfirstlane((int)bytes);
        rs = buffer_rsrc(p, n);
        oob = (unsigned)n;
    }
    // element `col` (per lane) of row `row` (uniform) of a matrix with `ld` floats per row; !ok -> 0
    __device__ __forceinline__ float load(bool ok, int row, int ld, int col) const {
        const unsigned so = ok ? (unsigned)row * (unsigned)(ld * 4) : oob;
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (unsigned)col * 4u,
                                                                             __builtin_amdgcn_readfirstlane(so), 0));
    }
};

// 16-byte gathers with a per-lane byte offset; !ok -> an offset outside the resource (0)
struct ChunkGather {
    __amdgpu_buffer_rsrc_t rs;
    unsigned oob;
    __device__ __forceinline__ ChunkGather(const float *base, long bytes) {
        const void *p = uniform_ptr(base);
        const int n = __builtin_amdgcn_readfirstlane((int)bytes);
        rs = buffer_rsrc(p, n);
        oob = (unsigned)n;
    }
    __device__ __forceinline__ float4 load(bool ok, unsigned byte_off) const {
        return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? byte_off : oob, 0, 0));
    }
};
