// In-plane binary thinning of bit planes, iterated to convergence inside one launch -- include/fsg_hip.h: fsg_thin_max_words,
// fsg_thin_bits.  Stands where sitk.BinaryThinning stands in poisson_reconstruction (data_processing/surface_fitting.py:109):
// ITK's BinaryThinningImageFilter as its documentation describes it, the two-sub-iteration algorithm of Gonzalez & Woods in the
// (y, x) plane of every slice (the filter's offsets have no z component), with clamped (zero-flux) borders.  Parity with
// SimpleITK is unpinned; tests/thinning_oracle.py is the authority.
//
// Rule.  Neighbours of p1 = (y, x): p2 (y-1, x), p3 (y-1, x+1), p4 (y, x+1), p5 (y+1, x+1), p6 (y+1, x), p7 (y+1, x-1),
// p8 (y, x-1), p9 (y-1, x-1); a neighbour outside the slice reads the nearest voxel inside it.  A step marks the set voxels with
//   (a) 2 <= p2 + ... + p9 <= 6,  (b) exactly one 0 -> 1 transition in the cycle p2, p3, ..., p9, p2,
//   (c, d) odd step: p2 p4 p6 = 0 and p4 p6 p8 = 0;  even step: p2 p4 p8 = 0 and p2 p6 p8 = 0,
// and clears all of them at once.  Odd and even steps alternate until a pair clears nothing in the slice.
//
// Words.  The planes are those of morphology.hip: (B, D, H, WW) 64-bit words, bit i of word j = voxel x = 64 j + i, bits past W
// always 0.  A step is bitwise on whole words, 64 voxels at a time:
//   p2 / p6 are the words of the rows above / below (the row itself at y = 0 / H - 1); the x + 1 plane of a row is
//   (c >> 1) | (right << 63) and its x - 1 plane (c << 1) | (left >> 63), where a missing neighbour word gives way to the border
//   bit: c & bit(W - 1) in the last word, c & 1 in the first (the voxel reads itself);
//   (a) is a bit-sliced add of the eight planes (full adders down to four count bits): not below 2, not 7 or 8;
//   (b) is "exactly one of the eight planes ~p_k & p_k+1": a running ones / twos pair;
//   (c, d) are ~(p4 & p6) | ~(p2 | p8) in an odd step and ~(p2 & p8) | ~(p4 | p6) in an even one.
// A mark is ANDed with p1, whose bits past W are 0, so the tail stays clean; it is masked again on the way in and out.
//
// Launch.  One workgroup per (item, slice).  The slice sits in LDS twice (2 * H * WW words, at most 2 * MAX_WORDS = 128 KiB):
// the odd step reads A and writes B, the even step reads B and writes A, so every mark is computed from the image as it was
// before the step.  Two barriers per pair, none under a divergent condition: after the pair's second barrier every thread reads
// the same flag word (set by any thread that cleared a bit in the pair -- plain stores of the value 1, no atomics) and takes
// the same branch.  The two flag words alternate, thread 0 re-arms the one the next pair will use.  A pair that goes on has
// cleared at least one voxel, so the loop is capped at H * W + 1 pairs.  No atomics, no scratch, no host read.
#include "fsg_common.h"

namespace {

constexpr int MAX_NT = 1024;
constexpr int MAX_WORDS = FSG_THIN_MAX_WORDS;   // words of one slice: 64 KiB per buffer; 512 x 1024 and 1024 x 512 voxels still fit

struct Slice {
    int H, W, WW, n;   // n = H * WW words
    u64 top;           // the bit of x = W - 1 in the last word of a row
    u64 tail;          // the voxel bits of the last word of a row
};

__device__ __forceinline__ void full_add(u64 a, u64 b, u64 c, u64 &sum, u64 &carry) {
    const u64 ab = a ^ b;
    sum = ab ^ c;
    carry = (a & b) | (c & ab);
}

// the x + 1 and x - 1 neighbour planes of the word j of a row (row points at its word 0), clamped at x = W - 1 and x = 0
__device__ __forceinline__ void east_west(const u64 *row, int j, const Slice &s, u64 c, u64 &east, u64 &west) {
    east = (c >> 1) | (j + 1 < s.WW ? row[j + 1] << 63 : c & s.top);
    west = (c << 1) | (j > 0 ? row[j - 1] >> 63 : c & 1ull);
}

// one step of this thread's words: dst = src without the marked voxels; returns the bits it cleared
template <bool ODD>
__device__ __forceinline__ u64 thin_step(const u64 *src, u64 *dst, const Slice &s) {
    u64 cleared = 0;
    for (int w = threadIdx.x; w < s.n; w += blockDim.x) {
        const int y = w / s.WW, j = w - y * s.WW;
        const u64 *cur = src + w - j;
        const u64 *up = y > 0 ? cur - s.WW : cur, *dn = y + 1 < s.H ? cur + s.WW : cur;
        const u64 p1 = cur[j], p2 = up[j], p6 = dn[j];
        u64 p3, p4, p5, p7, p8, p9;
        east_west(up, j, s, p2, p3, p9);
        east_west(cur, j, s, p1, p4, p8);
        east_west(dn, j, s, p6, p5, p7);
        // (a) count bits b3 b2 b1 b0 of p2 + ... + p9
        u64 s1, c1, s2, c2, b0, c4, t1, d1;
        full_add(p2, p3, p4, s1, c1);
        full_add(p5, p6, p7, s2, c2);
        const u64 s3 = p8 ^ p9, c3 = p8 & p9;
        full_add(s1, s2, s3, b0, c4);
        full_add(c1, c2, c3, t1, d1);
        const u64 b1 = t1 ^ c4, d2 = t1 & c4;
        const u64 b2 = d1 ^ d2, b3 = d1 & d2;
        const u64 cond_a = (b1 | b2 | b3) & ~(b3 | (b2 & b1 & b0));
        // (b) exactly one transition plane
        const u64 ring[9] = {p2, p3, p4, p5, p6, p7, p8, p9, p2};
        u64 ones = 0, twos = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const u64 t = ~ring[k] & ring[k + 1];
            twos |= ones & t;
            ones |= t;
        }
        const u64 cond_cd = ODD ? (~(p4 & p6) | ~(p2 | p8)) : (~(p2 & p8) | ~(p4 | p6));
        const u64 mark = p1 & cond_a & ones & ~twos & cond_cd;
        dst[w] = p1 & ~mark;
        cleared |= mark;
    }
    return cleared;
}

__global__ __launch_bounds__(MAX_NT) void thin_kernel(Slice s, const u64 *in, u64 *out, int *__restrict__ iters) {   // (in may be out)
    extern __shared__ u64 planes[];   // A = planes[0 .. n), B = planes[n .. 2 n)
    __shared__ int flag[2];
    u64 *A = planes, *B = planes + s.n;
    const long base = (long)blockIdx.x * s.n;
    for (int w = threadIdx.x; w < s.n; w += blockDim.x) {
        const int j = w % s.WW;
        A[w] = in[base + w] & (j == s.WW - 1 ? s.tail : ~0ull);
    }
    if (threadIdx.x == 0) flag[0] = flag[1] = 0;
    __syncthreads();
    const int cap = s.H * s.W + 1;   // a pair that goes on has cleared a voxel (n <= MAX_WORDS: H W <= 2^19)
    int pairs = 0;
    for (int pair = 0; pair < cap; ++pair) {   // (uniform: every thread reads the same flag after the same barrier)
        u64 cleared = thin_step<true>(A, B, s);
        __syncthreads();
        cleared |= thin_step<false>(B, A, s);
        if (cleared) flag[pair & 1] = 1;
        __syncthreads();
        const int go = flag[pair & 1];
        // the other word was last read after the previous pair's second barrier, which every thread has left: re-arm it for the
        // next pair, whose writers come after that pair's first barrier
        if (threadIdx.x == 0) flag[(pair + 1) & 1] = 0;
        if (!go) break;
        ++pairs;
    }
    // A holds the result (the last even step wrote it, the loop's last barrier published it); in may alias out: all of the slice
    // was read before the first barrier
    for (int w = threadIdx.x; w < s.n; w += blockDim.x) {
        const int j = w % s.WW;
        out[base + w] = A[w] & (j == s.WW - 1 ? s.tail : ~0ull);
    }
    if (iters && threadIdx.x == 0) iters[blockIdx.x] = pairs;
}

}  // namespace

extern "C" int fsg_thin_max_words(void) { return MAX_WORDS; }

extern "C" int fsg_thin_bits(const uint64_t *in, int B, int D, int H, int W, uint64_t *out, int32_t *iterations, fsg_stream_t stream) {
    const char *name = "fsg_thin_bits";
    FSG_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "%s: bad shape B=%d D=%d H=%d W=%d", name, B, D, H, W);
    const long WW = ((long)W + 63) / 64, n = (long)H * WW;
    FSG_REQUIRE(n <= MAX_WORDS, "%s: a slice of %d x %d voxels is %ld words, at most %d fit in LDS", name, H, W, n, MAX_WORDS);
    FSG_REQUIRE((long)B * D < (1L << 31), "%s: B D = %d x %d slices exceed the grid", name, B, D);
    FSG_REQUIRE(in && out, "%s: NULL pointer", name);
    Slice s;
    s.H = H; s.W = W; s.WW = (int)WW; s.n = (int)n;
    s.top = 1ull << ((W - 1) & 63);
    s.tail = (W & 63) ? ((1ull << (W & 63)) - 1ull) : ~0ull;
    const int nt = (int)(n >= MAX_NT ? MAX_NT : ((n + 63) / 64) * 64);
    const size_t lds = 2 * (size_t)n * sizeof(u64);
    FSG_GRANT_LDS(name, thin_kernel, lds);
    thin_kernel<<<(unsigned)((long)B * D), nt, lds, (hipStream_t)stream>>>(s, (const u64 *)in, (u64 *)out, (int *)iterations);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}
