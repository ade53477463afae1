// Mesh extraction on the device: naive surface nets over a scalar volume, and the occupancy-culled lattice that fills it.
//   ngp_surface_nets_count   flags per lattice point (its cell is active; its three lattice edges cross the level), counted per workgroup
//                            and scanned: V vertices, F triangles
//   ngp_surface_nets_emit    the flags again (no mask volume is stored): the cell -> vertex map and the vertices, then -- a later launch --
//                            the faces from the map; every store bounded by the caller's capacities
//   ngp_lattice_points       the lattice points of a z-slab whose neighbourhood in the occupancy bitfield holds a set bit, compacted in
//                            lattice order with their linear index: where the field has to be evaluated at all
// All three are ONE scheme -- flag, scan, compact -- written once: one lane per lattice point (x fastest), a rank inside the wave from a ballot
// and a population count, the waves of a workgroup through LDS, the workgroups through `partials` and a looping one-workgroup scan (correct
// for any number of workgroups), and the same flags recomputed by the pass that writes.  The output order is the scan's order: no atomics
// anywhere, the same bits on every run.  Neighbour values are plain loads through L1 / L2 (a lattice point is read by the eight cells around
// it; EXPERIMENTS.md says what that costs).
#include "common.h"
#include "occupancy_index.h"

namespace ngp {

constexpr int SN_THREADS = 256, SN_WAVES = SN_THREADS / WAVE;
constexpr int SN_SCAN_THREADS = 1024, SN_SCAN_WAVES = SN_SCAN_THREADS / WAVE;
constexpr uint32_t SN_NO_FIT = 0xFFFFFFFFu;   // a count that does not fit int32
constexpr int LP_MAX_DILATE = 4;

// ---------------------------------------------------------------------------------------------
// flag, scan, compact
// ---------------------------------------------------------------------------------------------
// the lane's rank among the lanes of its wave that raise `flag` (exclusive), and the wave's total
__device__ __forceinline__ uint32_t wave_rank(bool flag, uint32_t& wave_total) {
    const unsigned long long b = __ballot(flag);
    wave_total = (uint32_t)__popcll(b);
    return (uint32_t)__popcll(b & ((1ull << (threadIdx.x & 63u)) - 1ull));
}
// W counters per wave -> per counter the sum over the earlier waves of the workgroup and the workgroup's total (all threads call it)
template <int W>
__device__ __forceinline__ void block_offsets(const uint32_t (&wave_total)[W], uint32_t (*lds)[W], uint32_t (&base)[W], uint32_t (&total)[W]) {
    const uint32_t w = threadIdx.x >> 6;
    __syncthreads();   // the readers of an earlier use are done
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int c = 0; c < W; c++) lds[w][c] = wave_total[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < W; c++) {
        base[c] = total[c] = 0u;
#pragma unroll
        for (uint32_t q = 0; q < (uint32_t)SN_WAVES; q++) {
            const uint32_t x = lds[q][c];
            base[c] += q < w ? x : 0u;
            total[c] += x;
        }
    }
}
// partials [n_blocks][W] -> their exclusive prefix sums in place, the W totals behind them (partials[n_blocks][.]) and in counts_out.  ONE
// workgroup walks the array 1024 workgroups at a time with a running carry: any n_blocks.  The last counter's total is multiplied by
// mult_last (two triangles per quad); a total above INT32_MAX is reported as SN_NO_FIT.
template <int W>
__global__ __launch_bounds__(SN_SCAN_THREADS) void k_scan_partials(uint32_t* __restrict__ partials, uint32_t n_blocks, uint32_t mult_last,
                                                                     uint32_t* __restrict__ counts_out) {
    __shared__ uint32_t wave_tot[SN_SCAN_WAVES][W];
    const uint32_t t = threadIdx.x, w = t >> 6;
    unsigned long long carry[W];
#pragma unroll
    for (int c = 0; c < W; c++) carry[c] = 0ull;
#pragma unroll 1
    for (uint32_t at = 0; at < n_blocks; at += SN_SCAN_THREADS) {   // (wave-uniform trip count: the barriers below are met by everyone)
        const uint32_t b = at + t;
        uint32_t v[W], inc[W];
#pragma unroll
        for (int c = 0; c < W; c++) {
            v[c] = b < n_blocks ? partials[(size_t)b * W + c] : 0u;
            inc[c] = wave_inclusive_scan(v[c]);
        }
        __syncthreads();
        if ((t & 63u) == 63u) {
#pragma unroll
            for (int c = 0; c < W; c++) wave_tot[w][c] = inc[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < W; c++) {
            uint32_t base = 0, total = 0;
#pragma unroll
            for (uint32_t q = 0; q < (uint32_t)SN_SCAN_WAVES; q++) {
                const uint32_t x = wave_tot[q][c];
                base += q < w ? x : 0u;
                total += x;
            }
            if (b < n_blocks) partials[(size_t)b * W + c] = (uint32_t)carry[c] + base + inc[c] - v[c];
            carry[c] += total;
        }
    }
    if (t == 0u) {
#pragma unroll
        for (int c = 0; c < W; c++) {
            const unsigned long long n = carry[c] * (c == W - 1 ? mult_last : 1u);
            const uint32_t out = n > 0x7FFFFFFFull ? SN_NO_FIT : (uint32_t)n;
            partials[(size_t)n_blocks * W + c] = out;
            counts_out[c] = out;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// surface nets
// ---------------------------------------------------------------------------------------------
struct SnVolume {   // wave-uniform
    const float* f;
    uint32_t nx, ny, nz, n;   // n = nx ny nz < 2^31
    float level;
    bool inside_below;
};
struct SnPoint {
    uint32_t i, j, k;
    bool cell;   // the cell whose lowest corner this lattice point is exists: i < nx - 1, j < ny - 1, k < nz - 1
};
__device__ __forceinline__ SnPoint sn_point(const SnVolume& v, uint32_t n) {
    SnPoint p;
    const uint32_t r = n / v.nx;
    p.i = n - r * v.nx;
    p.k = r / v.ny;
    p.j = r - p.k * v.ny;
    p.cell = n < v.n && p.i + 1u < v.nx && p.j + 1u < v.ny && p.k + 1u < v.nz;
    return p;
}
// s = f - level (inside_below: level - f); a lattice point is inside iff s > 0 (NaN and s == 0: outside)
__device__ __forceinline__ float sn_signed(const SnVolume& v, uint32_t n) {
    NGP_BOUNDS(n < v.n);
    const float f = v.f[n];
    return v.inside_below ? v.level - f : f - v.level;
}
// the eight corners of the cell at n, corner c = dx + 2 dy + 4 dz -> s[c]; returns the mask of the inside corners
__device__ __forceinline__ uint32_t sn_corners(const SnVolume& v, uint32_t n, float (&s)[8]) {
    const uint32_t sy = v.nx, sz = v.nx * v.ny;
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) {
        s[c] = sn_signed(v, n + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz);
        mask |= s[c] > 0.0f ? 1u << c : 0u;
    }
    return mask;
}
// The lattice edge p -> p + e_a emits a quad iff it is interior in the two other axes and its ends differ.  An edge with all of p_b + 1 < N_b,
// p_c + 1 < N_c (interior) and p_a + 1 < N_a (it exists) starts at a point that has a cell: only those are looked at, with the cell's mask.
__device__ __forceinline__ void sn_edges(const SnPoint& p, uint32_t mask, bool (&edge)[3]) {
    edge[0] = p.cell && p.j >= 1u && p.k >= 1u && (((mask >> 1) ^ mask) & 1u);
    edge[1] = p.cell && p.k >= 1u && p.i >= 1u && (((mask >> 2) ^ mask) & 1u);
    edge[2] = p.cell && p.i >= 1u && p.j >= 1u && (((mask >> 4) ^ mask) & 1u);
}
// the faces pass needs four of the eight corners only
__device__ __forceinline__ uint32_t sn_edge_mask(const SnVolume& v, uint32_t n) {
    const uint32_t sy = v.nx, sz = v.nx * v.ny;
    return (sn_signed(v, n) > 0.0f ? 1u : 0u) | (sn_signed(v, n + 1u) > 0.0f ? 2u : 0u) | (sn_signed(v, n + sy) > 0.0f ? 4u : 0u) |
           (sn_signed(v, n + sz) > 0.0f ? 16u : 0u);
}

__global__ __launch_bounds__(SN_THREADS) void k_surface_nets_count(SnVolume v, uint32_t* __restrict__ partials) {
    __shared__ uint32_t lds[SN_WAVES][2];
    const uint32_t n = blockIdx.x * SN_THREADS + threadIdx.x;
    const SnPoint p = sn_point(v, n);
    uint32_t mask = 0;
    if (p.cell) {
        float s[8];
        mask = sn_corners(v, n, s);
    }
    bool edge[3];
    sn_edges(p, mask, edge);
    uint32_t wave_total[2], base[2], total[2];
    wave_total[0] = (uint32_t)__popcll(__ballot(mask != 0u && mask != 255u));
    wave_total[1] = (uint32_t)(__popcll(__ballot(edge[0])) + __popcll(__ballot(edge[1])) + __popcll(__ballot(edge[2])));
    block_offsets<2>(wave_total, lds, base, total);
    if (threadIdx.x == 0u) {
        partials[2u * blockIdx.x] = total[0];
        partials[2u * blockIdx.x + 1u] = total[1];
    }
}

// The vertex of an active cell: the mean of the crossing points of its sign-changing edges, in coordinates local to the cell.  On the edge
// from corner a to b = a + e_axis the crossing sits at t = s_a / (s_a - s_b) clamped to [0, 1], a non-finite t replaced by 0.5.  Fixed order:
// the four x-edges, then y, then z, each four with the lower of the two remaining axes running fastest.
__device__ __forceinline__ float sn_crossing(float sa, float sb) {
    float t = sa / (sa - sb);
    t = __builtin_isfinite(t) ? t : 0.5f;
    return clampf(t, 0.0f, 1.0f);
}
__device__ __forceinline__ void sn_vertex(const float (&s)[8], uint32_t mask, float& x, float& y, float& z) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    uint32_t count = 0;
#pragma unroll
    for (uint32_t axis = 0; axis < 3u; axis++) {
        const uint32_t step = 1u << axis, lo = 1u << ((axis + 1u) % 3u), hi = 1u << ((axis + 2u) % 3u);
        const uint32_t u = lo < hi ? lo : hi, w = lo < hi ? hi : lo;   // the two remaining axes, the lower one fastest
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            const uint32_t a = (e & 1u) * u + (e >> 1) * w, b = a + step;
            if ((((mask >> a) ^ (mask >> b)) & 1u) != 0u) {
                const float t = sn_crossing(s[a], s[b]);
                sx += axis == 0u ? t : (float)(a & 1u);
                sy += axis == 1u ? t : (float)((a >> 1) & 1u);
                sz += axis == 2u ? t : (float)(a >> 2);
                count++;
            }
        }
    }
    const float c = (float)count;   // >= 3 for an active cell
    x = sx / c; y = sy / c; z = sz / c;
}

struct SnFrame {   // world = fma(lattice, h, o)
    float ox, oy, oz, hx, hy, hz;
};

__global__ __launch_bounds__(SN_THREADS) void k_surface_nets_vertices(SnVolume v, SnFrame fr, const uint32_t* __restrict__ partials,
                                                                        int32_t* __restrict__ map, float* __restrict__ vertices, uint32_t v_cap) {
    __shared__ uint32_t lds[SN_WAVES][1];
    const uint32_t n = blockIdx.x * SN_THREADS + threadIdx.x;
    const SnPoint p = sn_point(v, n);
    uint32_t mask = 0;
    float s[8];
    if (p.cell) mask = sn_corners(v, n, s);
    const bool active = mask != 0u && mask != 255u;
    uint32_t wave_total[1], base[1], total[1];
    const uint32_t rank = wave_rank(active, wave_total[0]);
    block_offsets<1>(wave_total, lds, base, total);
    if (!active) return;
    const uint32_t at = partials[2u * blockIdx.x] + base[0] + rank;
    map[n] = (int32_t)at;   // (n < v.n: the cell exists)
    if (at >= v_cap) return;
    float x, y, z;
    sn_vertex(s, mask, x, y, z);
    vertices[3u * (size_t)at] = __builtin_fmaf((float)p.i + x, fr.hx, fr.ox);
    vertices[3u * (size_t)at + 1u] = __builtin_fmaf((float)p.j + y, fr.hy, fr.oy);
    vertices[3u * (size_t)at + 2u] = __builtin_fmaf((float)p.k + z, fr.hz, fr.oz);
}

// One quad per crossing edge, ordered by (linear index of p) * 3 + axis.  Axes (a, b, c) cyclic; the quad's corners are the vertices of the
// cells q0 = p - e_b - e_c, q1 = p - e_c, q2 = p, q3 = p - e_b (all four hold the edge, so all four are active and in the map).  p inside:
// (q0, q1, q2), (q0, q2, q3); else (q0, q3, q2), (q0, q2, q1) -- normals point from inside to outside.
__global__ __launch_bounds__(SN_THREADS) void k_surface_nets_faces(SnVolume v, const uint32_t* __restrict__ partials, const int32_t* __restrict__ map,
                                                                     int32_t* __restrict__ faces, uint32_t f_cap) {
    __shared__ uint32_t lds[SN_WAVES][1];
    const uint32_t n = blockIdx.x * SN_THREADS + threadIdx.x;
    const SnPoint p = sn_point(v, n);
    const uint32_t mask = p.cell ? sn_edge_mask(v, n) : 0u;
    bool edge[3];
    sn_edges(p, mask, edge);
    uint32_t wave_total[1], base[1], total[1], part;
    uint32_t rank = wave_rank(edge[0], wave_total[0]);
    rank += wave_rank(edge[1], part); wave_total[0] += part;
    rank += wave_rank(edge[2], part); wave_total[0] += part;
    block_offsets<1>(wave_total, lds, base, total);
    uint32_t quad = partials[2u * blockIdx.x + 1u] + base[0] + rank;   // the lane's first quad; its edges follow in axis order
    const uint32_t stride[3] = {1u, v.nx, v.nx * v.ny};
    const bool inside = (mask & 1u) != 0u;
#pragma unroll
    for (uint32_t a = 0; a < 3u; a++) {
        if (!edge[a]) continue;
        const uint32_t sb = stride[(a + 1u) % 3u], sc = stride[(a + 2u) % 3u];
        NGP_BOUNDS(n >= sb + sc && n < v.n);
        const int32_t q0 = map[n - sb - sc], q1 = map[n - sc], q2 = map[n], q3 = map[n - sb];
        const uint64_t tri = 2ull * quad;   // (a stale workspace may hold any word: 64-bit, so that the bound below is the bound)
        if (tri < f_cap) {
            int32_t* o = faces + 3u * tri;
            o[0] = q0; o[1] = inside ? q1 : q3; o[2] = q2;
        }
        if (tri + 1u < f_cap) {
            int32_t* o = faces + 3u * (tri + 1u);
            o[0] = q0; o[1] = q2; o[2] = inside ? q3 : q1;
        }
        quad++;
    }
}

// ---------------------------------------------------------------------------------------------
// the culled lattice
// ---------------------------------------------------------------------------------------------
struct LpLattice {   // wave-uniform
    float ox, oy, oz, hx, hy, hz;
    uint32_t nx, ny, z0, m;   // m = nx ny (z1 - z0) points, first linear index nx ny z0
    const uint8_t* bits;
    float bound, rbound, Hf, Hm1, Cm1;
    uint32_t H, H3;
    int dilate;
};
// lattice point n of the slab -> its position; kept iff one of the (2 dilate + 1)^3 cells around its own cell, at its own cascade, is set
__device__ __forceinline__ bool lp_point(const LpLattice& a, uint32_t n, float& x, float& y, float& z) {
    const uint32_t r = n / a.nx, i = n - r * a.nx, k = r / a.ny, j = r - k * a.ny;
    x = __builtin_fmaf((float)i, a.hx, a.ox);
    y = __builtin_fmaf((float)j, a.hy, a.oy);
    z = __builtin_fmaf((float)(a.z0 + k), a.hz, a.oz);
    if (n >= a.m) return false;
    if (!a.bits) return true;
    // the marcher's position term of the cascade and its index statement (raymarching.hip: probe_geom -- `lp`, then mip_rbound .. index)
    const int level = mip_exponent(fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))), a.Cm1);
    const float pw = scalbnf(1.0f, level);
    const bool capped = !(pw < a.bound);
    const float mip_rbound = capped ? a.rbound : scalbnf(1.0f, -level);
    const int cx = (int)clamp_med3((0.5f * __builtin_fmaf(x, mip_rbound, 1.0f)) * a.Hf, 0.0f, a.Hm1);
    const int cy = (int)clamp_med3((0.5f * __builtin_fmaf(y, mip_rbound, 1.0f)) * a.Hf, 0.0f, a.Hm1);
    const int cz = (int)clamp_med3((0.5f * __builtin_fmaf(z, mip_rbound, 1.0f)) * a.Hf, 0.0f, a.Hm1);
    const int top = (int)a.H - 1, d = a.dilate;
    const int x0 = max(cx - d, 0), x1 = min(cx + d, top), y0 = max(cy - d, 0), y1 = min(cy + d, top), z0 = max(cz - d, 0), z1 = min(cz + d, top);
    // (clamping the neighbour coordinates to [0, H - 1] names cells of the same box again: the box [x0, x1] x [y0, y1] x [z0, z1] is that set)
    const uint32_t first = (uint32_t)level * a.H3;
    bool keep = false;
    for (int qz = z0; qz <= z1 && !keep; qz++)
        for (int qy = y0; qy <= y1 && !keep; qy++)
            for (int qx = x0; qx <= x1; qx++) {
                const uint32_t index = first + morton3D_1((uint32_t)qx, (uint32_t)qy, (uint32_t)qz);
                keep = keep || (a.bits[index >> 3] & (1u << (index & 7u))) != 0;
            }
    return keep;
}

__global__ __launch_bounds__(SN_THREADS) void k_lattice_count(LpLattice a, uint32_t* __restrict__ partials) {
    __shared__ uint32_t lds[SN_WAVES][1];
    float x, y, z;
    const bool keep = lp_point(a, blockIdx.x * SN_THREADS + threadIdx.x, x, y, z);
    uint32_t wave_total[1], base[1], total[1];
    wave_total[0] = (uint32_t)__popcll(__ballot(keep));
    block_offsets<1>(wave_total, lds, base, total);
    if (threadIdx.x == 0u) partials[blockIdx.x] = total[0];
}

__global__ __launch_bounds__(SN_THREADS) void k_lattice_emit(LpLattice a, const uint32_t* __restrict__ partials, float* __restrict__ points,
                                                               int32_t* __restrict__ index, uint32_t capacity) {
    __shared__ uint32_t lds[SN_WAVES][1];
    const uint32_t n = blockIdx.x * SN_THREADS + threadIdx.x;
    float x, y, z;
    const bool keep = lp_point(a, n, x, y, z);
    uint32_t wave_total[1], base[1], total[1];
    const uint32_t rank = wave_rank(keep, wave_total[0]);
    block_offsets<1>(wave_total, lds, base, total);
    const uint32_t at = partials[blockIdx.x] + base[0] + rank;
    if (!keep || at >= capacity) return;
    points[3u * (size_t)at] = x;
    points[3u * (size_t)at + 1u] = y;
    points[3u * (size_t)at + 2u] = z;
    index[at] = (int32_t)(a.nx * a.ny * a.z0 + n);
}

// workspace of the extraction: the cell -> vertex map (one int32 per lattice point, indexed like the volume), then [blocks + 1][2] partials
inline size_t sn_map_bytes(uint64_t n) { return (size_t)((n * 4u + 255u) / 256u * 256u); }
inline uint32_t sn_blocks(uint64_t n) { return (uint32_t)cdiv64(n, (uint64_t)SN_THREADS); }
inline bool sn_dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
    return nx >= 2u && ny >= 2u && nz >= 2u && (uint64_t)nx * ny < (1ull << 31) && (uint64_t)nx * ny * nz < (1ull << 31);
}

}  // namespace ngp

using namespace ngp;

extern "C" size_t ngp_surface_nets_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (!sn_dims_ok(nx, ny, nz)) return 0;
    const uint64_t n = (uint64_t)nx * ny * nz;
    return sn_map_bytes(n) + ((size_t)sn_blocks(n) + 1u) * 2u * sizeof(uint32_t);
}

static int sn_volume(SnVolume& v, const char* what, const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float level, int inside_below) {
    NGP_REQUIRE(volume, NGP_ERR_INVALID, "%s: NULL volume", what);
    NGP_REQUIRE(nx >= 2u && ny >= 2u && nz >= 2u, NGP_ERR_INVALID, "%s: every dimension must be at least 2 (got %u x %u x %u)", what, nx, ny, nz);
    NGP_REQUIRE(sn_dims_ok(nx, ny, nz), NGP_ERR_INVALID, "%s: nx * ny * nz must be below 2^31 (got %u x %u x %u)", what, nx, ny, nz);
    v.f = volume; v.nx = nx; v.ny = ny; v.nz = nz; v.n = nx * ny * nz;
    v.level = level; v.inside_below = inside_below != 0;
    return NGP_OK;
}

extern "C" int ngp_surface_nets_count(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float level, int inside_below, void* workspace,
                                      uint32_t* counts_dev, ngp_stream_t stream) {
    SnVolume v;
    if (const int rc = sn_volume(v, "surface_nets_count", volume, nx, ny, nz, level, inside_below)) return rc;
    NGP_REQUIRE(workspace && counts_dev, NGP_ERR_INVALID, "surface_nets_count: NULL workspace or counts");
    uint32_t* partials = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + sn_map_bytes(v.n));
    const uint32_t blocks = sn_blocks(v.n);
    NGP_LAUNCH(k_surface_nets_count, dim3(blocks), dim3(SN_THREADS), 0, as_stream(stream), v, partials);
    NGP_LAUNCH(k_scan_partials<2>, dim3(1), dim3(SN_SCAN_THREADS), 0, as_stream(stream), partials, blocks, 2u, counts_dev);
    return check_launch("surface_nets_count");
}

extern "C" int ngp_surface_nets_emit(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float level, int inside_below, float ox, float oy,
                                     float oz, float hx, float hy, float hz, void* workspace, float* vertices, uint32_t v_cap, int32_t* faces,
                                     uint32_t f_cap, ngp_stream_t stream) {
    SnVolume v;
    if (const int rc = sn_volume(v, "surface_nets_emit", volume, nx, ny, nz, level, inside_below)) return rc;
    NGP_REQUIRE(workspace && vertices && faces, NGP_ERR_INVALID, "surface_nets_emit: NULL workspace, vertices or faces");
    NGP_REQUIRE(v_cap > 0u && f_cap > 0u, NGP_ERR_INVALID, "surface_nets_emit: zero capacity (v_cap %u, f_cap %u): an empty mesh needs no emit", v_cap, f_cap);
    NGP_REQUIRE(v_cap <= 0x7FFFFFFFu && f_cap <= 0x7FFFFFFFu, NGP_ERR_INVALID, "surface_nets_emit: capacities must fit int32");
    NGP_REQUIRE(!cmdlist::recording(), NGP_ERR_INVALID, "surface_nets_emit: reads its counts back (an export op); not recordable");
    int32_t* map = static_cast<int32_t*>(workspace);
    uint32_t* partials = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + sn_map_bytes(v.n));
    const uint32_t blocks = sn_blocks(v.n);
    const SnFrame fr{ox, oy, oz, hx, hy, hz};
    NGP_LAUNCH(k_surface_nets_vertices, dim3(blocks), dim3(SN_THREADS), 0, as_stream(stream), v, fr, partials, map, vertices, v_cap);
    NGP_LAUNCH(k_surface_nets_faces, dim3(blocks), dim3(SN_THREADS), 0, as_stream(stream), v, partials, map, faces, f_cap);
    if (const int rc = check_launch("surface_nets_emit")) return rc;
    // the counts ngp_surface_nets_count left behind the partials: a caller whose capacities are below them got a truncated mesh
    uint32_t counts[2] = {0u, 0u};
    hipError_t e = memcpy_async(counts, partials + 2u * (size_t)blocks, sizeof(counts), hipMemcpyDeviceToHost, as_stream(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
    NGP_REQUIRE(e == hipSuccess, NGP_ERR_DEVICE, "surface_nets_emit: reading the counts back failed: %s", hipGetErrorString(e));
    NGP_REQUIRE(counts[0] <= v_cap && counts[1] <= f_cap, NGP_ERR_INVALID,
                "surface_nets_emit: the mesh has %u vertices and %u triangles, the buffers hold %u and %u: truncated", counts[0], counts[1], v_cap, f_cap);
    return NGP_OK;
}

extern "C" size_t ngp_lattice_points_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz_slab) {
    const uint64_t m = (uint64_t)nx * ny * nz_slab;
    if (m == 0 || m >= (1ull << 31)) return 0;
    return ((size_t)sn_blocks(m) + 1u) * sizeof(uint32_t);
}

extern "C" int ngp_lattice_points(float ox, float oy, float oz, float hx, float hy, float hz, uint32_t nx, uint32_t ny, uint32_t z0, uint32_t z1,
                                  const uint8_t* bitfield, float bound, uint32_t cascade, uint32_t grid_size, uint32_t dilate, void* workspace,
                                  float* points, int32_t* index, uint32_t* count_dev, uint32_t capacity, ngp_stream_t stream) {
    NGP_REQUIRE(workspace && points && index && count_dev, NGP_ERR_INVALID, "lattice_points: NULL workspace, points, index or count");
    NGP_REQUIRE(nx >= 1u && ny >= 1u && z0 < z1, NGP_ERR_INVALID, "lattice_points: empty lattice (nx %u, ny %u, slab [%u, %u))", nx, ny, z0, z1);
    NGP_REQUIRE((uint64_t)nx * ny < (1ull << 31) && (uint64_t)nx * ny * z1 < (1ull << 31), NGP_ERR_INVALID,
                "lattice_points: nx * ny * z1 must be below 2^31 (the index is int32)");
    NGP_REQUIRE(capacity > 0u, NGP_ERR_INVALID, "lattice_points: zero capacity");
    if (bitfield) {
        NGP_REQUIRE(bound > 0.0f, NGP_ERR_INVALID, "lattice_points: bound must be positive");
        NGP_REQUIRE(cascade >= 1u && cascade <= 8u, NGP_ERR_INVALID, "lattice_points: cascade must be in [1, 8] (got %u)", cascade);
        // (a power of two: the Morton code of a cell of the grid is then below grid_size^3, as the marcher assumes too)
        NGP_REQUIRE(grid_size >= 1u && grid_size <= 1024u && (grid_size & (grid_size - 1u)) == 0u &&
                        (uint64_t)cascade * grid_size * grid_size * grid_size < (1ull << 32),
                    NGP_ERR_INVALID, "lattice_points: grid_size must be a power of two in [1, 1024] with cascade * grid_size^3 below 2^32 (got %u)", grid_size);
        NGP_REQUIRE(dilate <= (uint32_t)LP_MAX_DILATE, NGP_ERR_INVALID, "lattice_points: dilate must be in [0, %d] (got %u)", LP_MAX_DILATE, dilate);
    }
    LpLattice a;
    a.ox = ox; a.oy = oy; a.oz = oz; a.hx = hx; a.hy = hy; a.hz = hz;
    a.nx = nx; a.ny = ny; a.z0 = z0; a.m = nx * ny * (z1 - z0);
    a.bits = bitfield;
    a.bound = bound; a.rbound = 1.0f / bound;
    a.H = grid_size; a.H3 = grid_size * grid_size * grid_size;
    a.Hf = (float)grid_size; a.Hm1 = (float)(grid_size - 1u); a.Cm1 = (float)cascade - 1.0f;
    a.dilate = (int)dilate;
    uint32_t* partials = static_cast<uint32_t*>(workspace);
    const uint32_t blocks = sn_blocks(a.m);
    NGP_LAUNCH(k_lattice_count, dim3(blocks), dim3(SN_THREADS), 0, as_stream(stream), a, partials);
    NGP_LAUNCH(k_scan_partials<1>, dim3(1), dim3(SN_SCAN_THREADS), 0, as_stream(stream), partials, blocks, 1u, count_dev);
    NGP_LAUNCH(k_lattice_emit, dim3(blocks), dim3(SN_THREADS), 0, as_stream(stream), a, partials, points, index, capacity);
    return check_launch("lattice_points");
}
