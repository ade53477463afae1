// Camera-pose gradients through the training rays -- EXTENSION, not in the reference: the reference's cuda_ray path hands
// the marcher's xyzs / dirs to the network as leaves (raymarching/raymarching.py:164-196), so nothing there is differentiable in the camera.
//
// Semantics.  The marcher's sample parameters are constants (stop-gradient): a sample of ray n is x_i = clamp(o_n + t_i d_n, -bound, bound)
// with t_i, deltas and the choice of samples independent of the pose.  m_ij = 1 if |x_ij| < bound else 0: a clamped coordinate passes no
// gradient.  Row r of `rays` is (n, off, cnt); a row with cnt == 0 or off + cnt > M wrote no samples and gets zero gradients.
//   t_i            = sum_j m_ij d_j (x_ij - o_j) / sum_j m_ij d_j^2     (0 when the denominator is 0)                    k_ray_sample_ts
//   grad_o[n, j]   = sum_i m_ij g_x[i, j]                                                                                 k_ray_points_bwd
//   grad_d[n, j]   = sum_i t_i m_ij g_x[i, j] + sum_i g_dir[i, j] + (J_SH4(d_n)^T sum_i g_sh[i, 0:16])_j
//   grad_x[i, j]   = 1 / (2 bound) sum_l sum_c g_enc[l, i, c] dy_dx[i, l, j, c]        (dy_dx recomputed from the table)  k_grid_input_gradient
//   grad_pose[b, r, 3] = sum_n grad_o[b, n, r],  grad_pose[b, r, c] = sum_n grad_d[b, n, r] dcam[n, c],  row 3 = 0        k_rays_from_pixels_bwd
// Every sum has a fixed order (a lane's samples in order, then a butterfly over the lanes: a + b and b + a are the same bits): no float
// atomics, the same bits from every launch, and nothing depends on the order of the rows of `rays`.
//
// Launch shapes: the per-ray kernels use one wavefront per row of `rays` like the training compositor (raymarching.hip), RG_WAVES rays per
// workgroup; the grid kernel one lane per sample, all levels in a lane (the sum over the levels stays in a register: no partial sums in
// memory); the pose kernel one workgroup per pose.
#include "common.h"
#include "grid_index.h"
#include "sh_poly.inc"

namespace ngp {

constexpr int RG_WAVES = 4;
constexpr int RG_THREADS = 256;

// a row of `rays` that owns samples: (ray index, first sample, sample count)
struct RayRow {
    uint32_t index, offset, num;
    bool live;
};
__device__ __forceinline__ RayRow ray_row(const int32_t* __restrict__ rays, uint32_t r, uint32_t M, uint32_t N) {
    RayRow q;
    q.index = (uint32_t)rays[r * 3];
    q.offset = (uint32_t)rays[r * 3 + 1];
    q.num = (uint32_t)rays[r * 3 + 2];
    q.live = q.num != 0u && (uint64_t)q.offset + q.num <= (uint64_t)M && q.index < N;
    return q;
}

// sum over the wave, every lane gets it (butterfly: the lanes agree bit for bit)
template <typename F>
__device__ __forceinline__ F wave_butterfly(F v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// t of every sample a ray owns.  The quotient is formed in double from the operands as stored (exact products and differences of fp32
// values), rounded once: the recovered t carries the rounding of x alone.
template <typename F>
__global__ __launch_bounds__(RG_WAVES * 64) void k_ray_sample_ts(const F* __restrict__ xyzs, const F* __restrict__ rays_o,
                                                                 const F* __restrict__ rays_d, const int32_t* __restrict__ rays, uint32_t M,
                                                                 uint32_t N, F bound, F* __restrict__ ts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * RG_WAVES + (threadIdx.x >> 6);
    if (r >= N) return;
    const RayRow q = ray_row(rays, r, M, N);
    if (!q.live) return;
    double o[3], d[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        o[j] = (double)rays_o[(size_t)q.index * 3 + j];
        d[j] = (double)rays_d[(size_t)q.index * 3 + j];
    }
    for (uint32_t s = lane; s < q.num; s += 64u) {
        const size_t row = (size_t)q.offset + s;
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const F x = xyzs[row * 3 + j];
            if (fabs((double)x) < (double)bound) {
                num = fma(d[j], (double)x - o[j], num);
                den = fma(d[j], d[j], den);
            }
        }
        ts[row] = den != 0.0 ? (F)(num / den) : (F)0;
    }
}

template <typename F>
__device__ __forceinline__ F fma_t(F a, F b, F c);
template <>
__device__ __forceinline__ float fma_t<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <>
__device__ __forceinline__ double fma_t<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the marcher's statement of a sample (raymarching.hip: clampf(fmaf(t, d, o), -bound, bound)) and its direction
template <typename F>
__global__ __launch_bounds__(RG_WAVES * 64) void k_ray_points_fwd(const F* __restrict__ rays_o, const F* __restrict__ rays_d,
                                                                  const F* __restrict__ ts, const int32_t* __restrict__ rays, uint32_t M,
                                                                  uint32_t N, F bound, F* __restrict__ xyzs, F* __restrict__ dirs) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * RG_WAVES + (threadIdx.x >> 6);
    if (r >= N) return;
    const RayRow q = ray_row(rays, r, M, N);
    if (!q.live) return;
    F o[3], d[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        o[j] = rays_o[(size_t)q.index * 3 + j];
        d[j] = rays_d[(size_t)q.index * 3 + j];
    }
    for (uint32_t s = lane; s < q.num; s += 64u) {
        const size_t row = (size_t)q.offset + s;
        const F t = ts[row];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const F x = fma_t<F>(t, d[j], o[j]);
            xyzs[row * 3 + j] = x < -bound ? -bound : (x > bound ? bound : x);
            dirs[row * 3 + j] = d[j];
        }
    }
}

// One wavefront per row of `rays`: lane l sums the samples l, l + 64, ... of the ray in order, the lanes are added in a butterfly.
// SH: grad_sh16 [M,32] fp16 (the colour net's input gradient, columns 0..15 = dL/dSH4(d)) -- F = float only.
template <typename F, bool SH>
__global__ __launch_bounds__(RG_WAVES * 64) void k_ray_points_bwd(const F* __restrict__ grad_xyzs, const F* __restrict__ grad_dirs,
                                                                  const half_t* __restrict__ grad_sh16, const F* __restrict__ xyzs,
                                                                  const F* __restrict__ ts, const F* __restrict__ rays_d,
                                                                  const int32_t* __restrict__ rays, uint32_t M, uint32_t N, F bound,
                                                                  F* __restrict__ grad_rays_o, F* __restrict__ grad_rays_d) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * RG_WAVES + (threadIdx.x >> 6);
    if (r >= N) return;
    const RayRow q = ray_row(rays, r, M, N);
    if (!q.live) return;   // (the outputs were zeroed by the entry: a ray without samples keeps its zeros)
    F go[3] = {0, 0, 0}, gd[3] = {0, 0, 0};
    float gsh[SH ? 16 : 1] = {};
    for (uint32_t s = lane; s < q.num; s += 64u) {
        const size_t row = (size_t)q.offset + s;
        const F t = ts[row];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const F x = xyzs[row * 3 + j];
            const bool open = (x < (F)0 ? -x : x) < bound;
            const F g = open ? grad_xyzs[row * 3 + j] : (F)0;
            go[j] += g;
            gd[j] = fma_t<F>(t, g, gd[j]);
            if (grad_dirs) gd[j] += grad_dirs[row * 3 + j];
        }
        if constexpr (SH) {
            const half8_t a = *reinterpret_cast<const half8_t*>(grad_sh16 + row * 32);
            const half8_t b = *reinterpret_cast<const half8_t*>(grad_sh16 + row * 32 + 8);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                gsh[i] += (float)a[i];
                gsh[8 + i] += (float)b[i];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        go[j] = wave_butterfly<F>(go[j]);
        gd[j] = wave_butterfly<F>(gd[j]);
    }
    if constexpr (SH) {
#pragma unroll
        for (int i = 0; i < 16; i++) gsh[i] = wave_butterfly<float>(gsh[i]);
        // d is constant along the ray: J_SH4(d)^T times the summed gradient, on the raw direction as k_mid_forward evaluates the basis
        const float x = (float)rays_d[(size_t)q.index * 3], y = (float)rays_d[(size_t)q.index * 3 + 1], z = (float)rays_d[(size_t)q.index * 3 + 2];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
#define SH_DX(i, v) sx = __builtin_fmaf(gsh[i], (v), sx)
#define SH_DY(i, v) sy = __builtin_fmaf(gsh[i], (v), sy)
#define SH_DZ(i, v) sz = __builtin_fmaf(gsh[i], (v), sz)
        SH_BAND_0_GRADS;
        SH_BAND_1_GRADS;
        SH_BAND_2_GRADS;
        SH_BAND_3_GRADS;
#undef SH_DX
#undef SH_DY
#undef SH_DZ
        gd[0] += (F)sx;
        gd[1] += (F)sy;
        gd[2] += (F)sz;
    }
    if (lane < 3u) {
        grad_rays_o[(size_t)q.index * 3 + lane] = lane == 0u ? go[0] : (lane == 1u ? go[1] : go[2]);
        grad_rays_d[(size_t)q.index * 3 + lane] = lane == 0u ? gd[0] : (lane == 1u ? gd[1] : gd[2]);
    }
}

// grad_xyzs of the fused path's encoder (fp16 table, D = 3, C = 2) without dy_dx in memory: what k_grid_forward<half, 3, 2, true>
// (gridencoder.hip) would have written for the point -- level scale * phi' * the weights of the other two coordinates * the difference of
// the two table values, summed over the four corner pairs of the coordinate, in that kernel's order -- contracted with grad_enc as
// k_grid_input_backward (grid_index.h) does, in fp32 and without the two roundings to the table dtype between them.  One gather of a
// cell's eight corners per level serves all three derivatives; on a dense level the two corners that differ in x come in one 8-byte load
// (load_x_pair, as in k_grid_forward_fast).  One lane per point, the levels in order in the lane.
template <bool MAPPED>
__global__ __launch_bounds__(RG_THREADS) void k_grid_input_gradient(const half_t* __restrict__ grad_enc, const float* __restrict__ xyzs,
                                                                    const half_t* __restrict__ grid, const int32_t* __restrict__ offsets,
                                                                    uint32_t M, uint32_t L, GridLevels lv, uint32_t gridtype, bool align_corners,
                                                                    uint32_t interp, InputMap im, float* __restrict__ grad_xyzs) {
    constexpr int D = 3, C = 2;
    const uint32_t b = blockIdx.x * RG_THREADS + threadIdx.x;
    if (b >= M) return;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = xyzs[(size_t)b * D + d];
    float acc[D] = {0.0f, 0.0f, 0.0f};
    for (uint32_t level = 0; level < L; level++) {
        const uint32_t off0 = (uint32_t)offsets[level];
        const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
        const float scale = lv.scale[level];
        LevelIndexer<D> indexer;
        indexer.init(gridtype, align_corners, hashmap_size, lv.res[level]);
        const half_t* __restrict__ table = grid + (size_t)off0 * C;
        float frac[D], deriv[D];
        uint32_t cell[D];
        if (!locate<D>(x, scale, align_corners, interp, frac, deriv, cell, MAPPED ? im : InputMap{0.0f, 0.0f})) break;  // outside: zeros
        const half2_t g = *reinterpret_cast<const half2_t*>(grad_enc + ((size_t)level * M + b) * C);
        float corner[1 << D][C];
        const bool pairs = !indexer.hashed && !indexer.need_mod && indexer.stride[0] == 1u;   // (wave-uniform)
        if (pairs) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t i0 = cell[0] + (cell[1] + (uint32_t)(j & 1)) * indexer.stride[1] + (cell[2] + (uint32_t)(j >> 1)) * indexer.stride[2];
                NGP_BOUNDS(i0 + 1u < hashmap_size);
                const uint2 q = load_x_pair(table, i0);
                const half2_t lo = __builtin_bit_cast(half2_t, q.x), hi = __builtin_bit_cast(half2_t, q.y);
                corner[2 * j][0] = (float)lo.x; corner[2 * j][1] = (float)lo.y;
                corner[2 * j + 1][0] = (float)hi.x; corner[2 * j + 1][1] = (float)hi.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < (1 << D); k++) {
                uint32_t pg[D];
#pragma unroll
                for (int d = 0; d < D; d++) pg[d] = cell[d] + (uint32_t)((k >> d) & 1);
                const uint32_t idx = indexer(pg);
                NGP_BOUNDS(idx < hashmap_size);
                const half2_t v = *reinterpret_cast<const half2_t*>(table + (size_t)idx * C);
                corner[k][0] = (float)v.x; corner[k][1] = (float)v.y;
            }
        }
#pragma unroll
        for (int gdim = 0; gdim < D; gdim++) {
            float ga[C] = {0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < (1 << D); k++) {
                if ((k >> gdim) & 1) continue;   // the "left" corners, as k_grid_forward enumerates them
                float w = scale;
#pragma unroll
                for (int d = 0; d < D; d++)
                    if (d != gdim) w *= ((k >> d) & 1) ? frac[d] : (1.0f - frac[d]);
#pragma unroll
                for (int c = 0; c < C; c++) ga[c] = __builtin_fmaf(w * deriv[gdim], corner[k | (1 << gdim)][c] - corner[k][c], ga[c]);
            }
            acc[gdim] = __builtin_fmaf((float)g.x, ga[0], acc[gdim]);
            acc[gdim] = __builtin_fmaf((float)g.y, ga[1], acc[gdim]);
        }
    }
#pragma unroll
    for (int d = 0; d < D; d++) grad_xyzs[(size_t)b * D + d] = MAPPED ? acc[d] * im.scale : acc[d];
}

// the transpose of k_rays_from_pixels (pipeline.hip): dcam recomputed per pixel with that kernel's statements; one workgroup per pose, thread
// t sums rays t, t + RG_THREADS, ... in order, a butterfly per wave, the waves in order
__global__ __launch_bounds__(RG_THREADS) void k_rays_from_pixels_bwd(const float* __restrict__ grad_rays_o, const float* __restrict__ grad_rays_d,
                                                                     float fx, float fy, float cx, float cy, uint32_t W,
                                                                     const long long* __restrict__ inds, uint32_t inds_batch_stride, uint32_t N,
                                                                     float* __restrict__ grad_poses) {
    __shared__ float part[RG_THREADS / 64][12];
    const uint32_t b = blockIdx.x;
    float acc[12] = {};   // [r * 4 + c], c = 3: the translation column
    for (uint32_t n = threadIdx.x; n < N; n += RG_THREADS) {
        const long long pix = inds ? inds[(size_t)b * inds_batch_stride + n] : (long long)n;
        const float i = (float)(uint32_t)(pix % W) + 0.5f, j = (float)(uint32_t)(pix / W) + 0.5f;
        const float xs = (i - cx) / fx, ys = (j - cy) / fy;
        const float len = sqrtf((xs * xs + ys * ys) + 1.0f);
        const float dc[3] = {xs / len, ys / len, 1.0f / len};
        const size_t t = (size_t)b * N + n;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float gd = grad_rays_d[t * 3 + r];
#pragma unroll
            for (int c = 0; c < 3; c++) acc[r * 4 + c] = __builtin_fmaf(gd, dc[c], acc[r * 4 + c]);
            acc[r * 4 + 3] += grad_rays_o[t * 3 + r];
        }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const float v = wave_butterfly<float>(acc[k]);
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16u) {
        float v = 0.0f;
        if (threadIdx.x < 12u) {
#pragma unroll
            for (int w = 0; w < RG_THREADS / 64; w++) v += part[w][threadIdx.x];
        }
        grad_poses[(size_t)b * 16 + threadIdx.x] = v;   // row 3 = 0
    }
}

static bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

#define RG_REQUIRE_PTR(fn, p, a) \
    NGP_REQUIRE((p) && aligned_to((p), (a)), NGP_ERR_INVALID, "%s: %s is %s", fn, #p, (p) ? "misaligned" : "NULL")

template <typename F>
static int ray_sample_ts(const char* fn, const F* xyzs, const F* rays_o, const F* rays_d, const int32_t* rays, uint32_t M, uint32_t N, float bound,
                         F* ts, ngp_stream_t stream) {
    NGP_REQUIRE(bound > 0.0f, NGP_ERR_INVALID, "%s: bound must be positive (got %g)", fn, (double)bound);
    if (M == 0) return NGP_OK;
    RG_REQUIRE_PTR(fn, ts, sizeof(F));
    if (N != 0) {   // (every pointer is checked before the first stream operation)
        RG_REQUIRE_PTR(fn, xyzs, sizeof(F));
        RG_REQUIRE_PTR(fn, rays_o, sizeof(F));
        RG_REQUIRE_PTR(fn, rays_d, sizeof(F));
        RG_REQUIRE_PTR(fn, rays, sizeof(int32_t));
    }
    NGP_REQUIRE(memset_async(ts, 0, (size_t)M * sizeof(F), as_stream(stream)) == hipSuccess, NGP_ERR_LAUNCH, "%s: memset failed", fn);
    if (N == 0) return NGP_OK;
    NGP_LAUNCH(k_ray_sample_ts<F>, dim3(cdiv(N, RG_WAVES)), dim3(RG_WAVES * 64), 0, as_stream(stream), xyzs, rays_o, rays_d, rays, M, N, (F)bound, ts);
    return check_launch(fn);
}

template <typename F>
static int ray_points_forward(const char* fn, const F* rays_o, const F* rays_d, const F* ts, const int32_t* rays, uint32_t M, uint32_t N,
                              float bound, F* xyzs, F* dirs, ngp_stream_t stream) {
    NGP_REQUIRE(bound > 0.0f, NGP_ERR_INVALID, "%s: bound must be positive (got %g)", fn, (double)bound);
    if (M == 0) return NGP_OK;
    RG_REQUIRE_PTR(fn, xyzs, sizeof(F));
    RG_REQUIRE_PTR(fn, dirs, sizeof(F));
    if (N != 0) {
        RG_REQUIRE_PTR(fn, rays_o, sizeof(F));
        RG_REQUIRE_PTR(fn, rays_d, sizeof(F));
        RG_REQUIRE_PTR(fn, ts, sizeof(F));
        RG_REQUIRE_PTR(fn, rays, sizeof(int32_t));
    }
    NGP_REQUIRE(memset_async(xyzs, 0, (size_t)M * 3 * sizeof(F), as_stream(stream)) == hipSuccess &&
                    memset_async(dirs, 0, (size_t)M * 3 * sizeof(F), as_stream(stream)) == hipSuccess,
                NGP_ERR_LAUNCH, "%s: memset failed", fn);
    if (N == 0) return NGP_OK;
    NGP_LAUNCH(k_ray_points_fwd<F>, dim3(cdiv(N, RG_WAVES)), dim3(RG_WAVES * 64), 0, as_stream(stream), rays_o, rays_d, ts, rays, M, N, (F)bound, xyzs,
               dirs);
    return check_launch(fn);
}

template <typename F>
static int ray_points_backward(const char* fn, const F* grad_xyzs, const F* grad_dirs, const void* grad_sh16, const F* xyzs, const F* ts,
                               const F* rays_d, const int32_t* rays, uint32_t M, uint32_t N, float bound, F* grad_rays_o, F* grad_rays_d,
                               ngp_stream_t stream) {
    NGP_REQUIRE(bound > 0.0f, NGP_ERR_INVALID, "%s: bound must be positive (got %g)", fn, (double)bound);
    if (N == 0) return NGP_OK;
    RG_REQUIRE_PTR(fn, grad_rays_o, sizeof(F));
    RG_REQUIRE_PTR(fn, grad_rays_d, sizeof(F));
    if (M != 0) {
        RG_REQUIRE_PTR(fn, grad_xyzs, sizeof(F));
        RG_REQUIRE_PTR(fn, xyzs, sizeof(F));
        RG_REQUIRE_PTR(fn, ts, sizeof(F));
        RG_REQUIRE_PTR(fn, rays_d, sizeof(F));
        RG_REQUIRE_PTR(fn, rays, sizeof(int32_t));
        NGP_REQUIRE(!grad_dirs || aligned_to(grad_dirs, sizeof(F)), NGP_ERR_INVALID, "%s: grad_dirs is misaligned", fn);
        NGP_REQUIRE(!grad_sh16 || aligned_to(grad_sh16, 16), NGP_ERR_INVALID, "%s: grad_sh16 must be 16-byte aligned", fn);
    }
    NGP_REQUIRE(memset_async(grad_rays_o, 0, (size_t)N * 3 * sizeof(F), as_stream(stream)) == hipSuccess &&
                    memset_async(grad_rays_d, 0, (size_t)N * 3 * sizeof(F), as_stream(stream)) == hipSuccess,
                NGP_ERR_LAUNCH, "%s: memset failed", fn);
    if (M == 0) return NGP_OK;
    const dim3 grid(cdiv(N, RG_WAVES)), block(RG_WAVES * 64);
    if constexpr (sizeof(F) == 4) {
        if (grad_sh16) {
            NGP_LAUNCH((k_ray_points_bwd<F, true>), grid, block, 0, as_stream(stream), grad_xyzs, grad_dirs, (const half_t*)grad_sh16, xyzs, ts, rays_d,
                       rays, M, N, (F)bound, grad_rays_o, grad_rays_d);
            return check_launch(fn);
        }
    }
    NGP_LAUNCH((k_ray_points_bwd<F, false>), grid, block, 0, as_stream(stream), grad_xyzs, grad_dirs, (const half_t*)nullptr, xyzs, ts, rays_d, rays, M,
               N, (F)bound, grad_rays_o, grad_rays_d);
    return check_launch(fn);
}

}  // namespace ngp

using namespace ngp;

extern "C" int ngp_ray_sample_ts(const float* xyzs, const float* rays_o, const float* rays_d, const int32_t* rays, uint32_t M, uint32_t N,
                                 float bound, float* ts, ngp_stream_t stream) {
    return ray_sample_ts<float>("ray_sample_ts", xyzs, rays_o, rays_d, rays, M, N, bound, ts, stream);
}
extern "C" int ngp_ray_sample_ts_f64(const double* xyzs, const double* rays_o, const double* rays_d, const int32_t* rays, uint32_t M, uint32_t N,
                                     float bound, double* ts, ngp_stream_t stream) {
    return ray_sample_ts<double>("ray_sample_ts_f64", xyzs, rays_o, rays_d, rays, M, N, bound, ts, stream);
}

extern "C" int ngp_ray_points_forward(const float* rays_o, const float* rays_d, const float* ts, const int32_t* rays, uint32_t M, uint32_t N,
                                      float bound, float* xyzs, float* dirs, ngp_stream_t stream) {
    return ray_points_forward<float>("ray_points_forward", rays_o, rays_d, ts, rays, M, N, bound, xyzs, dirs, stream);
}
extern "C" int ngp_ray_points_forward_f64(const double* rays_o, const double* rays_d, const double* ts, const int32_t* rays, uint32_t M, uint32_t N,
                                          float bound, double* xyzs, double* dirs, ngp_stream_t stream) {
    return ray_points_forward<double>("ray_points_forward_f64", rays_o, rays_d, ts, rays, M, N, bound, xyzs, dirs, stream);
}

extern "C" int ngp_ray_points_backward(const float* grad_xyzs, const float* grad_dirs, const void* grad_sh16, const float* xyzs, const float* ts,
                                       const float* rays_d, const int32_t* rays, uint32_t M, uint32_t N, float bound, float* grad_rays_o,
                                       float* grad_rays_d, ngp_stream_t stream) {
    return ray_points_backward<float>("ray_points_backward", grad_xyzs, grad_dirs, grad_sh16, xyzs, ts, rays_d, rays, M, N, bound, grad_rays_o,
                                      grad_rays_d, stream);
}
extern "C" int ngp_ray_points_backward_f64(const double* grad_xyzs, const double* grad_dirs, const double* xyzs, const double* ts,
                                           const double* rays_d, const int32_t* rays, uint32_t M, uint32_t N, float bound, double* grad_rays_o,
                                           double* grad_rays_d, ngp_stream_t stream) {
    return ray_points_backward<double>("ray_points_backward_f64", grad_xyzs, grad_dirs, nullptr, xyzs, ts, rays_d, rays, M, N, bound, grad_rays_o,
                                       grad_rays_d, stream);
}

extern "C" int ngp_grid_input_gradient(const void* grad_enc, const float* xyzs, const void* embeddings, const int32_t* offsets, uint32_t M,
                                       uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                       uint32_t interp, int dtype, float bound, float* grad_xyzs, ngp_stream_t stream) {
    const char* fn = "grid_input_gradient";
    NGP_REQUIRE(D == 3 && C == 2 && dtype == NGP_F16, NGP_ERR_INVALID,
                "%s: provided for D = 3, C = 2 and a float16 table, the fused path's layout (got D = %u, C = %u, dtype %d)", fn, D, C, dtype);
    NGP_REQUIRE(L >= 1 && L <= NGP_MAX_LEVELS, NGP_ERR_INVALID, "%s: number of levels must be in [1, %d] (got %u)", fn, NGP_MAX_LEVELS, L);
    NGP_REQUIRE(gridtype <= 1u && interp <= 1u, NGP_ERR_INVALID, "%s: gridtype and interp must be 0 or 1 (got %u, %u)", fn, gridtype, interp);
    NGP_REQUIRE(bound >= 0.0f, NGP_ERR_INVALID, "%s: bound must be positive, or 0 for unit coordinates (got %g)", fn, (double)bound);
    if (M == 0) return NGP_OK;
    RG_REQUIRE_PTR(fn, grad_enc, 4);
    RG_REQUIRE_PTR(fn, xyzs, 4);
    RG_REQUIRE_PTR(fn, embeddings, 4);
    RG_REQUIRE_PTR(fn, offsets, 4);
    RG_REQUIRE_PTR(fn, grad_xyzs, 4);
    GridLevels lv;
    fill_levels(lv, L, S, H);
    const InputMap im = make_input_map(bound);
    const dim3 grid(cdiv(M, RG_THREADS)), block(RG_THREADS);
    if (bound > 0.0f)
        NGP_LAUNCH(k_grid_input_gradient<true>, grid, block, 0, as_stream(stream), (const half_t*)grad_enc, xyzs, (const half_t*)embeddings, offsets, M,
                   L, lv, gridtype, align_corners != 0, interp, im, grad_xyzs);
    else
        NGP_LAUNCH(k_grid_input_gradient<false>, grid, block, 0, as_stream(stream), (const half_t*)grad_enc, xyzs, (const half_t*)embeddings, offsets,
                   M, L, lv, gridtype, align_corners != 0, interp, im, grad_xyzs);
    return check_launch(fn);
}

extern "C" int ngp_rays_from_pixels_backward(const float* grad_rays_o, const float* grad_rays_d, uint32_t B, float fx, float fy, float cx, float cy,
                                             uint32_t W, const int64_t* inds, uint32_t inds_batch_stride, uint32_t N, float* grad_poses,
                                             ngp_stream_t stream) {
    const char* fn = "rays_from_pixels_backward";
    NGP_REQUIRE(W > 0 && fx != 0.0f && fy != 0.0f, NGP_ERR_INVALID, "%s: W, fx and fy must be non-zero", fn);
    NGP_REQUIRE((uint64_t)B * N <= 0xffffffffull, NGP_ERR_INVALID, "%s: B * N must fit 32 bits", fn);
    if (B == 0) return NGP_OK;
    RG_REQUIRE_PTR(fn, grad_poses, 4);
    if (N == 0) {
        NGP_REQUIRE(memset_async(grad_poses, 0, (size_t)B * 16 * sizeof(float), as_stream(stream)) == hipSuccess, NGP_ERR_LAUNCH, "%s: memset failed", fn);
        return NGP_OK;
    }
    RG_REQUIRE_PTR(fn, grad_rays_o, 4);
    RG_REQUIRE_PTR(fn, grad_rays_d, 4);
    NGP_REQUIRE(!inds || aligned_to(inds, 8), NGP_ERR_INVALID, "%s: inds is misaligned", fn);
    NGP_LAUNCH(k_rays_from_pixels_bwd, dim3(B), dim3(RG_THREADS), 0, as_stream(stream), grad_rays_o, grad_rays_d, fx, fy, cx, cy, W,
               (const long long*)inds, inds_batch_stride, N, grad_poses);
    return check_launch(fn);
}
