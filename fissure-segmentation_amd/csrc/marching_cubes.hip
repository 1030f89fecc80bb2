// Marching cubes on a dense grid: indexed triangle meshes with vertex normals, in a canonical order -- include/fsg_hip.h:
// fsg_mc_workspace_bytes, fsg_mc_count_f32, fsg_mc_count_labels_i32, fsg_mc_emit_f32, fsg_mc_emit_labels_i32.
// Replaces pytorch3d.ops.marching_cubes + Meshes.verts_normals_padded of DifferentiableMarchingCubes (models/dpsr_utils.py:
// 60-64) and skimage.measure.marching_cubes of compute_surface_mesh_marching_cubes (data_processing/find_lobes.py).
//
// The case table (mc_table.h) is generated; the rule is in fissure-segmentation_amd/_mc_table.py.  Corner c of a cell sits at
// (x, y, z) = bits 0, 1, 2 of c from the cell's lower node, a corner is inside iff value < isolevel (NaN is outside), bit c of
// a case is set iff corner c is inside.  A cell is ACTIVE iff all 8 of its corner nodes are in the mask; an inactive cell is
// stored with case 0 and emits nothing.
//
// Vertices are owned by the lower node of their grid edge: node n = (z H + y) W + x owns the edges to x + 1, y + 1, z + 1
// (axes 0, 1, 2).  An edge carries a vertex iff one of the <= 4 cells round it is active and has the edge's two corners on
// different sides.  Canonical orders: vertices by (item, node, axis), faces by (item, cell = its lower node, table order), so
// both follow the linear node order and ranks come from prefix sums over chunks of 1024 nodes:
//   classify  node -> the case of the cell whose lower node it is (1 byte; 0 for nodes on an upper border)     [reads the field]
//   count     node -> its 3 vertex bits from the 7 cells that touch its edges, and its rank inside the chunk (2 bytes:
//             rank << 3 | bits); per chunk the number of vertices and of triangles
//   scan      one workgroup per item: exclusive sums of the chunk counts, per-item totals (int64)
//   bases     one wave: exclusive sums of the totals over the items (where an item's rows start in the packed outputs)
//   -- the host reads the totals and sizes the outputs --
//   verts     node -> its vertices p_a + t (p_b - p_a), t = (iso - v_a) / (v_b - v_a)                            [reads the field]
//   faces     cell -> its triangles; the vertex on edge e of a cell is looked up through the 2-byte code of the owning node
//   normals   vertex -> sum of (v1 - v0) x (v2 - v0) over its faces, a gather over the <= 4 cells round its edge in
//             (cell z, y, x, table order) order, divided by max(|n|, 1e-6)
// No floating-point atomics and none that decide an order (the only atomic is the OR of the non-finite flag): the same input
// gives the same bits, and an item's rows are the same bits alone and inside a batch.  No workgroup waits on another.
#include "fsg_common.h"

#define MC_TABLE_QUAL __device__ const __attribute__((aligned(16)))
#include "mc_table.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 1024;          // nodes per chunk: at most 3072 vertices, so rank << 3 | bits fits 16 bits
constexpr int PER = CHUNK / NT;      // consecutive nodes per thread
constexpr int MAX_BLOCKS = 4096;     // grid-strided launches

struct Dims {
    int B, D, H, W, HW;
    int V;         // nodes of one item (B V < 2^31)
    int nchunks;
};

struct FieldSrc {
    const float *f;
    __device__ __forceinline__ float at(int b, int V, long n) const { return f[(long)b * V + n]; }
};
// item b of a label volume shared by all items: 0 inside the object first + b, 1 outside, to be cut at 0.5
struct LabelSrc {
    const int *l;
    int first;
    __device__ __forceinline__ float at(int b, int, long n) const { return l[n] != first + b ? 1.f : 0.f; }
};

__device__ __forceinline__ void node_zyx(const Dims &d, int n, int &z, int &y, int &x) {
    z = n / d.HW;
    const int r = n - z * d.HW;
    y = r / d.W;
    x = r - y * d.W;
}
// node offset of corner c of a cell from the cell's lower node
__device__ __forceinline__ int corner_off(const Dims &d, int c) { return (c & 1) + ((c >> 1) & 1) * d.W + ((c >> 2) & 1) * d.HW; }
__device__ __forceinline__ int edge_corner(int e) { return (int)((MC_EDGE_CORNER >> (3 * e)) & 7ull); }
__device__ __forceinline__ int edge_axis(int e) { return (int)((MC_EDGE_AXIS >> (2 * e)) & 3u); }
__device__ __forceinline__ int edge_of(int corner, int axis) {
    const int i = 3 * corner + axis;
    return (int)(((i < 16 ? MC_EDGE_OF_LO >> (4 * i) : MC_EDGE_OF_HI >> (4 * (i - 16)))) & 15ull);
}

// the case table into LDS, 16 bytes per thread
__device__ __forceinline__ void load_table(unsigned char *tab) {
    reinterpret_cast<uint4 *>(tab)[threadIdx.x] = reinterpret_cast<const uint4 *>(&MC_TRI[0][0])[threadIdx.x];
    __syncthreads();
}

// item-local index of the vertex on the edge that node m owns along `axis` (the edge is known to carry one)
__device__ __forceinline__ int vertex_id(const uint16_t *vc, const int *voff, long m, int axis) {
    const unsigned code = vc[m];
    return voff[m / CHUNK] + (int)(code >> 3) + __popc(code & ((1u << axis) - 1u));
}

template <class Src>
__global__ __launch_bounds__(NT) void classify_kernel(Dims d, Src src, float iso, const uint8_t *__restrict__ mask, long mask_stride,
                                                      uint8_t *__restrict__ cellcase, long long *__restrict__ flag) {
    const int b = blockIdx.y;
    const uint8_t *m = mask ? mask + (long)b * mask_stride : nullptr;
    uint8_t *cc = cellcase + (long)b * d.V;
    bool bad = false;
    for (long n = (long)blockIdx.x * NT + threadIdx.x; n < d.V; n += (long)gridDim.x * NT) {
        int z, y, x;
        node_zyx(d, (int)n, z, y, x);
        const float v0 = src.at(b, d.V, n);
        bad |= !(fabsf(v0) < __builtin_inff());
        unsigned c = 0;
        if (x < d.W - 1 && y < d.H - 1 && z < d.D - 1) {
            bool active = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long nk = n + corner_off(d, k);
                const float v = k ? src.at(b, d.V, nk) : v0;
                c |= (unsigned)(v < iso) << k;
                if (m) active &= m[nk] != 0;
            }
            if (!active) c = 0;
        }
        cc[n] = (uint8_t)c;
    }
    if (flag && bad) atomicOr((unsigned long long *)flag, 1ull);
}

// the 3 vertex bits of node n: bit a is set iff the edge from n along axis a has its two corners on different sides in an
// active cell.  The cell at offset k = dx | dy << 1 | dz << 2 BELOW the node has the node as its corner k.
__device__ __forceinline__ unsigned node_vbits(const Dims &d, const uint8_t *cc, long n, int z, int y, int x) {
    unsigned c[8];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const bool ok = (!(k & 1) || x > 0) && (!(k & 2) || y > 0) && (!(k & 4) || z > 0);
        c[k] = ok ? cc[n - corner_off(d, k)] : 0u;
    }
    unsigned vb = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        unsigned cr = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (!((k >> a) & 1)) cr |= ((c[k] >> k) ^ (c[k] >> (k + (1 << a)))) & 1u;
        vb |= cr << a;
    }
    return vb;
}

__global__ __launch_bounds__(NT) void count_kernel(Dims d, const uint8_t *__restrict__ cellcase, uint16_t *__restrict__ vcode,
                                                   int *__restrict__ vcount, int *__restrict__ tcount) {
    __shared__ int red[NT / 64];
    __shared__ __attribute__((aligned(16))) unsigned char tab[256 * 16];
    load_table(tab);
    const int b = blockIdx.y;
    const uint8_t *cc = cellcase + (long)b * d.V;
    uint16_t *vc = vcode + (long)b * d.V;
    for (int ch = blockIdx.x; ch < d.nchunks; ch += gridDim.x) {   // (uniform)
        const long n0 = (long)ch * CHUNK + threadIdx.x * PER;
        unsigned vb[PER];
        int nv = 0, nt = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            vb[k] = 0;
            if (n0 + k < d.V) {
                int z, y, x;
                node_zyx(d, (int)(n0 + k), z, y, x);
                vb[k] = node_vbits(d, cc, n0 + k, z, y, x);
                nv += __popc(vb[k]);
                nt += tab[cc[n0 + k] * 16 + 15];
            }
        }
        int total_v, total_t;
        int ex = block_excl_scan<NT>(nv, red, total_v);
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (n0 + k < d.V) {
                vc[n0 + k] = (uint16_t)(((unsigned)ex << 3) | vb[k]);
                ex += __popc(vb[k]);
            }
        block_excl_scan<NT>(nt, red, total_t);
        if (threadIdx.x == 0) {
            vcount[(long)b * d.nchunks + ch] = total_v;
            tcount[(long)b * d.nchunks + ch] = total_t;
        }
    }
}

// one workgroup per item: both count arrays -> exclusive sums in place (int32: the host refuses an item whose total does not
// fit before anything reads them), totals[2 b] = vertices, totals[2 b + 1] = triangles
__global__ __launch_bounds__(NT) void scan_kernel(int nchunks, int *__restrict__ vcount, int *__restrict__ tcount,
                                                  long long *__restrict__ totals) {
    __shared__ int red[NT / 64];
    for (int which = 0; which < 2; ++which) {
        int *cnt = (which ? tcount : vcount) + (long)blockIdx.x * nchunks;
        long long carry = 0;
        for (int base = 0; base < nchunks; base += NT) {   // (uniform)
            const int i = base + threadIdx.x;
            const int c = i < nchunks ? cnt[i] : 0;
            int total;
            const int ex = block_excl_scan<NT>(c, red, total);
            if (i < nchunks) cnt[i] = (int)(carry + ex);
            carry += total;
        }
        if (threadIdx.x == 0) totals[2 * blockIdx.x + which] = carry;
    }
}

// one wave: totals[2 B + 1 + 2 b + which] = sum of totals[2 b' + which] over b' < b
__global__ __launch_bounds__(64) void bases_kernel(int B, long long *__restrict__ totals) {
    const int lane = threadIdx.x;
    for (int which = 0; which < 2; ++which) {
        long long carry = 0;
        for (int base = 0; base < B; base += 64) {   // (uniform)
            const int i = base + lane;
            const long long v = i < B ? totals[2 * i + which] : 0;
            long long incl = v;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const long long t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            if (i < B) totals[2 * B + 1 + 2 * i + which] = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
    }
}

// coordinate of node index i on an axis of S nodes
__device__ __forceinline__ float coord(int i, int S, int local, float sp) {
    return local ? 2.f * (float)i / (float)(S - 1) - 1.f : (float)i * sp;
}

template <class Src>
__global__ __launch_bounds__(NT) void verts_kernel(Dims d, Src src, float iso, int local, float sx, float sy, float sz,
                                                   const uint16_t *__restrict__ vcode, const int *__restrict__ voff_all,
                                                   const long long *__restrict__ totals, float *__restrict__ verts, long nv_total) {
    const int b = blockIdx.y;
    const uint16_t *vc = vcode + (long)b * d.V;
    const int *voff = voff_all + (long)b * d.nchunks;
    const long vbase = totals[2 * d.B + 1 + 2 * b];
    for (long n = (long)blockIdx.x * NT + threadIdx.x; n < d.V; n += (long)gridDim.x * NT) {
        const unsigned code = vc[n];
        if (!(code & 7u)) continue;
        long vi = vbase + voff[n / CHUNK] + (int)(code >> 3);
        int z, y, x;
        node_zyx(d, (int)n, z, y, x);
        const float va = src.at(b, d.V, n);
        const float p[3] = {coord(x, d.W, local, sx), coord(y, d.H, local, sy), coord(z, d.D, local, sz)};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((code >> a) & 1u)) continue;
            const float vb = src.at(b, d.V, n + (a == 0 ? 1 : (a == 1 ? d.W : d.HW)));
            const float t = (iso - va) / (vb - va);
            const float pb = a == 0 ? coord(x + 1, d.W, local, sx) : (a == 1 ? coord(y + 1, d.H, local, sy) : coord(z + 1, d.D, local, sz));
            float q[3] = {p[0], p[1], p[2]};
            q[a] = p[a] + t * (pb - p[a]);
            if (vi < nv_total) {
                verts[3 * vi] = q[0];
                verts[3 * vi + 1] = q[1];
                verts[3 * vi + 2] = q[2];
            }
            ++vi;
        }
    }
}

__global__ __launch_bounds__(NT) void faces_kernel(Dims d, const uint8_t *__restrict__ cellcase, const uint16_t *__restrict__ vcode,
                                                   const int *__restrict__ voff_all, const int *__restrict__ toff_all,
                                                   const long long *__restrict__ totals, long long *__restrict__ faces,
                                                   long nf_total) {
    __shared__ int red[NT / 64];
    __shared__ __attribute__((aligned(16))) unsigned char tab[256 * 16];
    load_table(tab);
    const int b = blockIdx.y;
    const uint8_t *cc = cellcase + (long)b * d.V;
    const uint16_t *vc = vcode + (long)b * d.V;
    const int *voff = voff_all + (long)b * d.nchunks;
    const long fbase = totals[2 * d.B + 1 + 2 * b + 1];
    for (int ch = blockIdx.x; ch < d.nchunks; ch += gridDim.x) {   // (uniform)
        const long n0 = (long)ch * CHUNK + threadIdx.x * PER;
        unsigned c[PER];
        int nt = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            c[k] = n0 + k < d.V ? cc[n0 + k] : 0u;
            nt += tab[c[k] * 16 + 15];
        }
        int total;
        long fi = fbase + toff_all[(long)b * d.nchunks + ch] + block_excl_scan<NT>(nt, red, total);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const unsigned char *row = tab + c[k] * 16;
            const int ntri = row[15];
            for (int t = 0; t < ntri; ++t, ++fi) {
                long long id[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int e = row[3 * t + j];
                    id[j] = vertex_id(vc, voff, n0 + k + corner_off(d, edge_corner(e)), edge_axis(e));
                }
                if (fi < nf_total) {
                    faces[3 * fi] = id[0];
                    faces[3 * fi + 1] = id[1];
                    faces[3 * fi + 2] = id[2];
                }
            }
        }
    }
}

__global__ __launch_bounds__(NT) void normals_kernel(Dims d, const uint8_t *__restrict__ cellcase, const uint16_t *__restrict__ vcode,
                                                     const int *__restrict__ voff_all, const long long *__restrict__ totals,
                                                     const float *__restrict__ verts, float *__restrict__ normals, long nv_total) {
    __shared__ __attribute__((aligned(16))) unsigned char tab[256 * 16];
    load_table(tab);
    const int b = blockIdx.y;
    const uint8_t *cc = cellcase + (long)b * d.V;
    const uint16_t *vc = vcode + (long)b * d.V;
    const int *voff = voff_all + (long)b * d.nchunks;
    const long vbase = totals[2 * d.B + 1 + 2 * b];
    const long nv_item = totals[2 * b];
    for (long n = (long)blockIdx.x * NT + threadIdx.x; n < d.V; n += (long)gridDim.x * NT) {
        const unsigned code = vc[n];
        if (!(code & 7u)) continue;
        long vi = vbase + voff[n / CHUNK] + (int)(code >> 3);
        int z, y, x;
        node_zyx(d, (int)n, z, y, x);
        for (int a = 0; a < 3; ++a) {
            if (!((code >> a) & 1u)) continue;
            float nx = 0.f, ny = 0.f, nz = 0.f;
            for (int k = 7; k >= 0; --k) {   // the cells round the edge, ascending in (z, y, x)
                if ((k >> a) & 1) continue;
                if (((k & 1) && x == 0) || ((k & 2) && y == 0) || ((k & 4) && z == 0)) continue;
                const long cell = n - corner_off(d, k);
                const unsigned char *row = tab + (unsigned)cc[cell] * 16;
                const int ntri = row[15], mine = edge_of(k, a);
                for (int t = 0; t < ntri; ++t) {
                    const int e0 = row[3 * t], e1 = row[3 * t + 1], e2 = row[3 * t + 2];
                    if (e0 != mine && e1 != mine && e2 != mine) continue;
                    float p[3][3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int e = j == 0 ? e0 : (j == 1 ? e1 : e2);
                        long id = vertex_id(vc, voff, cell + corner_off(d, edge_corner(e)), edge_axis(e));
                        id = id < nv_item ? id : 0;     // (never taken for the workspace of this field)
                        const float *q = verts + 3 * (vbase + id);
                        p[j][0] = q[0];
                        p[j][1] = q[1];
                        p[j][2] = q[2];
                    }
                    const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
                    const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
                    nx += ay * bz - az * by;
                    ny += az * bx - ax * bz;
                    nz += ax * by - ay * bx;
                }
            }
            const float den = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-6f);
            if (vi < nv_total) {
                normals[3 * vi] = nx / den;
                normals[3 * vi + 1] = ny / den;
                normals[3 * vi + 2] = nz / den;
            }
            ++vi;
        }
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

int check_dims(const char *name, int B, int D, int H, int W, Dims &d) {
    FSG_REQUIRE(B > 0 && B <= 65535 && D >= 2 && H >= 2 && W >= 2, "%s: bad shape B=%d D=%d H=%d W=%d (B in 1..65535, every size >= 2)",
                name, B, D, H, W);
    FSG_REQUIRE((long)B * D * H * W < (1L << 31), "%s: B D H W = %d %d %d %d exceeds 2^31 nodes", name, B, D, H, W);
    d.B = B; d.D = D; d.H = H; d.W = W;
    d.HW = H * W;
    d.V = D * H * W;
    d.nchunks = (d.V + CHUNK - 1) / CHUNK;
    return FSG_OK;
}

struct Workspace {
    uint8_t *cellcase;
    uint16_t *vcode;
    int *vcount, *tcount;
};

Workspace carve(void *workspace, const Dims &d) {
    char *p = (char *)workspace;
    Workspace w;
    const size_t nodes = (size_t)d.B * d.V, chunks = (size_t)d.B * d.nchunks;
    w.cellcase = (uint8_t *)p;
    p += align256(nodes);
    w.vcode = (uint16_t *)p;
    p += align256(nodes * sizeof(uint16_t));
    w.vcount = (int *)p;
    p += align256(chunks * sizeof(int));
    w.tcount = (int *)p;
    return w;
}

int check_workspace(const char *name, const Dims &d, const void *workspace, size_t workspace_bytes) {
    const size_t need = fsg_mc_workspace_bytes(d.B, d.D, d.H, d.W);
    FSG_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
    FSG_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: NULL or misaligned workspace", name);
    return FSG_OK;
}

inline int grid_nodes(const Dims &d) {
    const long n = ((long)d.V + NT - 1) / NT;
    return (int)(n > MAX_BLOCKS ? MAX_BLOCKS : n);
}

template <class Src>
int count(const char *name, Src src, float iso, const uint8_t *mask, int64_t mask_item_stride, int validate, int B, int D, int H,
          int W, void *workspace, size_t workspace_bytes, int64_t *totals, fsg_stream_t stream) {
    Dims d;
    if (int rc = check_dims(name, B, D, H, W, d)) return rc;
    if (int rc = check_workspace(name, d, workspace, workspace_bytes)) return rc;
    FSG_REQUIRE(totals, "%s: NULL pointer", name);
    FSG_REQUIRE(mask_item_stride == 0 || mask_item_stride == d.V, "%s: mask_item_stride %ld (0 or D H W)", name, (long)mask_item_stride);
    const Workspace w = carve(workspace, d);
    hipStream_t s = (hipStream_t)stream;
    long long *tot = (long long *)totals;
    if (hipMemsetAsync(tot + 2 * B, 0, sizeof(long long), s) != hipSuccess) {
        fsg_set_error("%s: hipMemsetAsync failed", name);
        return FSG_ERR_HIP;
    }
    const dim3 cgrid(d.nchunks < MAX_BLOCKS ? d.nchunks : MAX_BLOCKS, B);
    classify_kernel<Src><<<dim3(grid_nodes(d), B), NT, 0, s>>>(d, src, iso, mask, (long)mask_item_stride, w.cellcase,
                                                               validate ? tot + 2 * B : nullptr);
    count_kernel<<<cgrid, NT, 0, s>>>(d, w.cellcase, w.vcode, w.vcount, w.tcount);
    scan_kernel<<<B, NT, 0, s>>>(d.nchunks, w.vcount, w.tcount, tot);
    bases_kernel<<<1, 64, 0, s>>>(B, tot);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

template <class Src>
int emit(const char *name, Src src, float iso, int local, float sx, float sy, float sz, int B, int D, int H, int W,
         const void *workspace, size_t workspace_bytes, const int64_t *totals, int64_t total_verts, int64_t total_faces, float *verts,
         int64_t *faces, float *normals, fsg_stream_t stream) {
    Dims d;
    if (int rc = check_dims(name, B, D, H, W, d)) return rc;
    if (int rc = check_workspace(name, d, workspace, workspace_bytes)) return rc;
    FSG_REQUIRE(totals && total_verts >= 0 && total_faces >= 0, "%s: NULL totals or a negative total", name);
    FSG_REQUIRE((total_verts == 0 || (verts && normals)) && (total_faces == 0 || faces), "%s: NULL pointer", name);
    const Workspace w = carve(const_cast<void *>(workspace), d);
    hipStream_t s = (hipStream_t)stream;
    const long long *tot = (const long long *)totals;
    const dim3 ngrid(grid_nodes(d), B), cgrid(d.nchunks < MAX_BLOCKS ? d.nchunks : MAX_BLOCKS, B);
    if (total_verts > 0)
        verts_kernel<Src><<<ngrid, NT, 0, s>>>(d, src, iso, local, sx, sy, sz, w.vcode, w.vcount, tot, verts, (long)total_verts);
    if (total_faces > 0)
        faces_kernel<<<cgrid, NT, 0, s>>>(d, w.cellcase, w.vcode, w.vcount, w.tcount, tot, (long long *)faces, (long)total_faces);
    if (total_verts > 0)
        normals_kernel<<<ngrid, NT, 0, s>>>(d, w.cellcase, w.vcode, w.vcount, tot, verts, normals, (long)total_verts);
    FSG_CHECK_LAUNCH(name);
    return FSG_OK;
}

}  // namespace

extern "C" size_t fsg_mc_workspace_bytes(int B, int D, int H, int W) {
    if (B < 1 || D < 2 || H < 2 || W < 2 || (long)B * D * H * W >= (1L << 31)) return 0;
    const size_t nodes = (size_t)B * D * H * W, chunks = (size_t)B * (((size_t)D * H * W + CHUNK - 1) / CHUNK);
    return align256(nodes) + align256(nodes * sizeof(uint16_t)) + 2 * align256(chunks * sizeof(int));
}

extern "C" int fsg_mc_count_f32(const float *field, const uint8_t *mask, int64_t mask_item_stride, int B, int D, int H, int W,
                                float isolevel, int validate, void *workspace, size_t workspace_bytes, int64_t *totals,
                                fsg_stream_t stream) {
    const char *name = "fsg_mc_count_f32";
    FSG_REQUIRE(field, "%s: NULL pointer", name);
    return count(name, FieldSrc{field}, isolevel, mask, mask_item_stride, validate, B, D, H, W, workspace, workspace_bytes, totals,
                 stream);
}

extern "C" int fsg_mc_count_labels_i32(const int32_t *labels, const uint8_t *mask, int64_t mask_item_stride, int first_label, int B,
                                       int D, int H, int W, void *workspace, size_t workspace_bytes, int64_t *totals,
                                       fsg_stream_t stream) {
    const char *name = "fsg_mc_count_labels_i32";
    FSG_REQUIRE(labels, "%s: NULL pointer", name);
    return count(name, LabelSrc{labels, first_label}, 0.5f, mask, mask_item_stride, 0, B, D, H, W, workspace, workspace_bytes, totals,
                 stream);
}

extern "C" int fsg_mc_emit_f32(const float *field, int B, int D, int H, int W, float isolevel, int local_coords, float sx, float sy,
                               float sz, const void *workspace, size_t workspace_bytes, const int64_t *totals, int64_t total_verts,
                               int64_t total_faces, float *verts, int64_t *faces, float *normals, fsg_stream_t stream) {
    const char *name = "fsg_mc_emit_f32";
    FSG_REQUIRE(field, "%s: NULL pointer", name);
    return emit(name, FieldSrc{field}, isolevel, local_coords, sx, sy, sz, B, D, H, W, workspace, workspace_bytes, totals, total_verts,
                total_faces, verts, faces, normals, stream);
}

extern "C" int fsg_mc_emit_labels_i32(const int32_t *labels, int first_label, int B, int D, int H, int W, int local_coords, float sx,
                                      float sy, float sz, const void *workspace, size_t workspace_bytes, const int64_t *totals,
                                      int64_t total_verts, int64_t total_faces, float *verts, int64_t *faces, float *normals,
                                      fsg_stream_t stream) {
    const char *name = "fsg_mc_emit_labels_i32";
    FSG_REQUIRE(labels, "%s: NULL pointer", name);
    return emit(name, LabelSrc{labels, first_label}, 0.5f, local_coords, sx, sy, sz, B, D, H, W, workspace, workspace_bytes, totals,
                total_verts, total_faces, verts, faces, normals, stream);
}
