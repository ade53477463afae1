// fp64 kernels for gfx950 (MI355X): the grid encoder, its total-variation gradient, the SH encoder, the training and inference
// compositors and the ray utilities (near/far, sph, packbits) -- the ops the reference dispatches with AT_DISPATCH_FLOATING_TYPES_AND_HALF,
// so that torch.autograd.gradcheck can run against this backend.  A correctness tool, not a hot path: straightforward one-lane-per-item
// kernels, kept in a unit of their own so that no fp16/fp32 kernel is compiled differently.
//
// Numerics (DESIGN.md "The fp64 path"):
//   * grid forward: positions, fractions and interpolation weights come from the fp32 inputs through the fp32 path's own code
//     (grid_index.h: locate, the fp32 weight product); every product with a table entry and every sum is fp64, nothing is rounded
//     through fp32 after the weights;
//   * grid backward, first and second order: bit-reproducible.  Per level, the record sort of grid_records.h groups the (point, corner)
//     records of an entry in slot order, and one lane per entry sums its run in that order in fp64 (grid_second.h: record_coeff, w_k or
//     a_k) and adds the sum once.  No float atomics, so two calls give the same bits;
//   * TV: fp64 throughout, fp64 atomics (not on an autograd path);
//   * SH: fp64 arithmetic and constants (sh_poly64.inc, tools/gen_sh.py);
//   * compositing / near-far / sph / packbits: the reference's per-ray loops in fp64 (exp in double, T < T_thresh compared in double);
//   * sdf_sigmas: the fp32 kernels' own source (sdf_sigmas.h) instantiated for double.
#include "common.h"
#include "grid_index.h"
#include "grid_records.h"
#include "grid_second.h"
#include "fp64.h"
#include "sh_poly64.inc"
#include "sdf_sigmas.h"
#include <float.h>
#include <math.h>

namespace ngp {

constexpr int F64_THREADS = 256;

// ------------------------------------------------------------------------------------------------
// grid encoder: forward (gridencoder.cu:87-245)
// ------------------------------------------------------------------------------------------------
template <int D, int C, bool WITH_DYDX>
__global__ __launch_bounds__(F64_THREADS) void k_f64_grid_fwd(const float* __restrict__ inputs, const double* __restrict__ grid,
                                                               const int32_t* __restrict__ offsets, double* __restrict__ outputs, uint32_t B,
                                                               uint32_t L, GridLevels lv, double* __restrict__ dy_dx, uint32_t gridtype,
                                                               bool align_corners, uint32_t interp) {
    const uint32_t level = blockIdx.y;
    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
    const float scale = lv.scale[level];
    LevelIndexer<D> indexer;
    indexer.init(gridtype, align_corners, hashmap_size, lv.res[level]);
    const double* __restrict__ table = grid + (size_t)off0 * C;

    for (uint32_t b = blockIdx.x * F64_THREADS + threadIdx.x; b < B; b += gridDim.x * F64_THREADS) {
        float frac[D], deriv[D];
        uint32_t cell[D];
        double* out = outputs + ((size_t)level * B + b) * C;
        double* dyo = WITH_DYDX ? dy_dx + ((size_t)b * L + level) * D * C : nullptr;
        if (!locate<D>(inputs + (size_t)b * D, scale, align_corners, interp, frac, deriv, cell)) {
#pragma unroll
            for (int c = 0; c < C; c++) out[c] = 0.0;
            if (WITH_DYDX) {
#pragma unroll
                for (int i = 0; i < D * C; i++) dyo[i] = 0.0;
            }
            continue;
        }
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 0.0;
        // corners one after the other (unrolled, the 2^D * C fp64 loads are hoisted and D = 5, C = 8 spills)
#pragma unroll 1
        for (int k = 0; k < (1 << D); k++) {
            uint32_t pg[D];
#pragma unroll
            for (int d = 0; d < D; d++) pg[d] = cell[d] + ((k >> d) & 1);
            const double* v = table + (size_t)indexer(pg) * C;
            NGP_BOUNDS(indexer(pg) < hashmap_size);
            const double w = (double)corner_weight<D>(frac, (uint32_t)k);
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = __builtin_fma(w, v[c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < C; c++) out[c] = acc[c];

        if (WITH_DYDX) {
            // gridencoder.cu:201-244: d out / d x_g = scale * sum_{left corners} w_other * deriv_g * (v_right - v_left); the weight factor is
            // the fp32 path's, the difference and the sum are fp64
#pragma unroll
            for (int g = 0; g < D; g++) {
                double ga[C];
#pragma unroll
                for (int c = 0; c < C; c++) ga[c] = 0.0;
#pragma unroll 1
                for (int k = 0; k < (1 << D); k++) {
                    if ((k >> g) & 1) continue;
                    float w = scale;
#pragma unroll
                    for (int d = 0; d < D; d++)
                        if (d != g) w *= ((k >> d) & 1) ? frac[d] : (1.0f - frac[d]);
                    const double wd = (double)(w * deriv[g]);
                    uint32_t pl[D], pr[D];
#pragma unroll
                    for (int d = 0; d < D; d++) {
                        pl[d] = cell[d] + ((k >> d) & 1);
                        pr[d] = pl[d] + (d == g ? 1u : 0u);
                    }
                    const double* vl = table + (size_t)indexer(pl) * C;
                    const double* vr = table + (size_t)indexer(pr) * C;
#pragma unroll
                    for (int c = 0; c < C; c++) ga[c] = __builtin_fma(wd, vr[c] - vl[c], ga[c]);
                }
#pragma unroll
                for (int c = 0; c < C; c++) dyo[g * C + c] = ga[c];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// grid encoder: deterministic table gradients, one level at a time: the record sort of grid_records.h, then this run sum.
// One lane per run of equal entries (the run's first record): the contributions in slot order, fma into fp64 from 0, added to the entry
// once.  ORDER 1: w_k g, the backward; ORDER 2: a_k g with u = uin[b], the backward's backward (grid_second.hip)
// ------------------------------------------------------------------------------------------------
template <int D, int C, int ORDER>
__global__ __launch_bounds__(F64_THREADS) void k_f64_grid_run_sum(const uint32_t* __restrict__ keys0, const uint32_t* __restrict__ vals0,
                                                                   const uint32_t* __restrict__ keys1, const uint32_t* __restrict__ vals1, uint32_t n,
                                                                   const double* __restrict__ grad, const float* __restrict__ inputs,
                                                                   const double* __restrict__ uin, const int32_t* __restrict__ offsets,
                                                                   double* __restrict__ grad_grid, uint32_t B, uint32_t level, float scale,
                                                                   bool align_corners, uint32_t interp) {
    const uint32_t level_size = level_size_of(offsets, level);
    const bool odd = rec_sorted_side(level_size) != 0u;
    const uint32_t* __restrict__ keys = odd ? keys1 : keys0;
    const uint32_t* __restrict__ vals = odd ? vals1 : vals0;
    double* __restrict__ table = grad_grid + (size_t)(uint32_t)offsets[level] * C;
    for (uint32_t i = blockIdx.x * F64_THREADS + threadIdx.x; i < n; i += gridDim.x * F64_THREADS) {
        const uint32_t e = keys[i];
        if (e >= level_size || (i > 0u && keys[i - 1u] == e)) continue;   // (level_size: a record of a point outside [0,1]^D)
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 0.0;
        for (uint32_t j = i; j < n && keys[j] == e; j++) {
            const uint32_t slot = vals[j], b = slot >> D, k = slot & ((1u << D) - 1u);
            NGP_BOUNDS(b < B);
            const double w = record_coeff<D, ORDER>(inputs + (size_t)b * D, ORDER == 2 ? uin + (size_t)b * D : nullptr, k, scale, align_corners, interp,
                                                    InputMap{0.0f, 0.0f});
            const double* g = grad + ((size_t)level * B + b) * C;
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = __builtin_fma(w, g[c], acc[c]);
        }
        double* dst = table + (size_t)e * C;
#pragma unroll
        for (int c = 0; c < C; c++) dst[c] += acc[c];
    }
}

// gridencoder.cu:343-369: grad_inputs[b, d] = sum_{l, c} grad[l, b, c] * dy_dx[b, l, d, c]
__global__ __launch_bounds__(F64_THREADS) void k_f64_grid_input_bwd(const double* __restrict__ grad, const double* __restrict__ dy_dx,
                                                                     double* __restrict__ grad_inputs, uint32_t B, uint32_t L, uint32_t D, uint32_t C) {
    const uint32_t t = blockIdx.x * F64_THREADS + threadIdx.x;
    if (t >= B * D) return;
    const uint32_t b = t / D, d = t - b * D;
    const double* dd = dy_dx + (size_t)b * L * D * C;
    double r = 0.0;
    for (uint32_t l = 0; l < L; l++)
        for (uint32_t c = 0; c < C; c++) r = __builtin_fma(grad[((size_t)l * B + b) * C + c], dd[(l * D + d) * C + c], r);
    grad_inputs[t] = r;
}

// ------------------------------------------------------------------------------------------------
// grid encoder: total-variation gradient (gridencoder.cu:506-610), fp64 throughout
// ------------------------------------------------------------------------------------------------
template <int D, int C>
__global__ __launch_bounds__(F64_THREADS) void k_f64_grad_tv(const double* __restrict__ inputs, const double* __restrict__ grid,
                                                              double* __restrict__ grad, const int32_t* __restrict__ offsets, float weight, uint32_t B,
                                                              GridLevels lv, uint32_t gridtype, bool align_corners) {
    const uint32_t level = blockIdx.y;
    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
    const uint32_t resolution = lv.res[level];
    const double scale = (double)lv.scale[level];
    LevelIndexer<D> indexer;
    indexer.init(gridtype, align_corners, hashmap_size, resolution);
    const double* __restrict__ table = grid + (size_t)off0 * C;
    double* __restrict__ gtable = grad + (size_t)off0 * C;
    const double w = (double)weight / (double)(2 * D);
    for (uint32_t b = blockIdx.x * F64_THREADS + threadIdx.x; b < B; b += gridDim.x * F64_THREADS) {
        double x[D];
        bool inside = true;
#pragma unroll
        for (int d = 0; d < D; d++) {
            x[d] = inputs[(size_t)b * D + d];
            inside = inside && !(x[d] < 0.0 || x[d] > 1.0);
        }
        if (!inside) continue;
        uint32_t pg[D];
#pragma unroll
        for (int d = 0; d < D; d++) pg[d] = (uint32_t)floor(__builtin_fma(x[d], scale, align_corners ? 0.0 : 0.5));
        const double* ctr = table + (size_t)indexer(pg) * C;
        double* gctr = gtable + (size_t)indexer(pg) * C;
        double res[C], idelta[C];
#pragma unroll
        for (int c = 0; c < C; c++) res[c] = idelta[c] = 0.0;
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t cur = pg[d];
            if (cur < resolution) {
                pg[d] = cur + 1u;
                const double* o = table + (size_t)indexer(pg) * C;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const double gv = ctr[c] - o[c];
                    res[c] += gv;
                    idelta[c] = __builtin_fma(gv, gv, idelta[c]);
                }
            }
            if (cur > 0u) {
                pg[d] = cur - 1u;
                const double* o = table + (size_t)indexer(pg) * C;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const double gv = ctr[c] - o[c];
                    res[c] += gv;
                    idelta[c] = __builtin_fma(gv, gv, idelta[c]);
                }
            }
            pg[d] = cur;
        }
#pragma unroll
        for (int c = 0; c < C; c++) atomicAdd(gctr + c, w * res[c] / sqrt(idelta[c] + 1e-9));
    }
}

// ------------------------------------------------------------------------------------------------
// SH encoder (shencoder.cu:27-382): one lane per direction, fp64 polynomials of sh_poly64.inc
// ------------------------------------------------------------------------------------------------
template <int BANDS, bool WITH_GRAD>
__global__ __launch_bounds__(F64_THREADS) void k_f64_sh_fwd(const double* __restrict__ inputs, double* __restrict__ outputs, uint32_t B,
                                                             double* __restrict__ dy_dx) {
    constexpr int N = BANDS * BANDS;
    const uint32_t b = blockIdx.x * F64_THREADS + threadIdx.x;
    if (b >= B) return;
    const double x = inputs[(size_t)b * 3], y = inputs[(size_t)b * 3 + 1], z = inputs[(size_t)b * 3 + 2];
    double* out = outputs + (size_t)b * N;
#define SH_OUT(i, v) out[i] = (v)
    SH64_BAND_0_VALUES;
    if constexpr (BANDS > 1) { SH64_BAND_1_VALUES; }
    if constexpr (BANDS > 2) { SH64_BAND_2_VALUES; }
    if constexpr (BANDS > 3) { SH64_BAND_3_VALUES; }
    if constexpr (BANDS > 4) { SH64_BAND_4_VALUES; }
    if constexpr (BANDS > 5) { SH64_BAND_5_VALUES; }
    if constexpr (BANDS > 6) { SH64_BAND_6_VALUES; }
    if constexpr (BANDS > 7) { SH64_BAND_7_VALUES; }
#undef SH_OUT
    if constexpr (WITH_GRAD) {
        // dy_dx [B, 3, N]
        double* gx = dy_dx + (size_t)b * 3 * N;
        double* gy = gx + N;
        double* gz = gx + 2 * N;
#define SH_DX(i, v) gx[i] = (v)
#define SH_DY(i, v) gy[i] = (v)
#define SH_DZ(i, v) gz[i] = (v)
        SH64_BAND_0_GRADS;
        if constexpr (BANDS > 1) { SH64_BAND_1_GRADS; }
        if constexpr (BANDS > 2) { SH64_BAND_2_GRADS; }
        if constexpr (BANDS > 3) { SH64_BAND_3_GRADS; }
        if constexpr (BANDS > 4) { SH64_BAND_4_GRADS; }
        if constexpr (BANDS > 5) { SH64_BAND_5_GRADS; }
        if constexpr (BANDS > 6) { SH64_BAND_6_GRADS; }
        if constexpr (BANDS > 7) { SH64_BAND_7_GRADS; }
#undef SH_DX
#undef SH_DY
#undef SH_DZ
    }
}

__global__ __launch_bounds__(F64_THREADS) void k_f64_sh_bwd(const double* __restrict__ grad, uint32_t B, uint32_t N, const double* __restrict__ dy_dx,
                                                             double* __restrict__ grad_inputs) {
    const uint32_t t = blockIdx.x * F64_THREADS + threadIdx.x;
    if (t >= B * 3) return;
    const uint32_t b = t / 3, d = t - b * 3;
    const double* g = grad + (size_t)b * N;
    const double* dd = dy_dx + ((size_t)b * 3 + d) * N;
    double r = grad_inputs[t];
    for (uint32_t i = 0; i < N; i++) r = __builtin_fma(g[i], dd[i], r);
    grad_inputs[t] = r;
}

// ------------------------------------------------------------------------------------------------
// ray utilities (raymarching.cu:92-300)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(F64_THREADS) void k_f64_near_far(const double* __restrict__ rays_o, const double* __restrict__ rays_d,
                                                               const double* __restrict__ aabb, uint32_t N, float min_near, double* __restrict__ nears,
                                                               double* __restrict__ fars) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= N) return;
    const double ox = rays_o[(size_t)n * 3], oy = rays_o[(size_t)n * 3 + 1], oz = rays_o[(size_t)n * 3 + 2];
    const double rdx = 1.0 / rays_d[(size_t)n * 3], rdy = 1.0 / rays_d[(size_t)n * 3 + 1], rdz = 1.0 / rays_d[(size_t)n * 3 + 2];
    nears[n] = fars[n] = DBL_MAX;
    double near = (aabb[0] - ox) * rdx, far = (aabb[3] - ox) * rdx, t;
    if (near > far) { t = near; near = far; far = t; }
    double ny = (aabb[1] - oy) * rdy, fy = (aabb[4] - oy) * rdy;
    if (ny > fy) { t = ny; ny = fy; fy = t; }
    if (near > fy || ny > far) return;
    if (ny > near) near = ny;
    if (fy < far) far = fy;
    double nz = (aabb[2] - oz) * rdz, fz = (aabb[5] - oz) * rdz;
    if (nz > fz) { t = nz; nz = fz; fz = t; }
    if (near > fz || nz > far) return;
    if (nz > near) near = nz;
    if (fz < far) far = fz;
    if (near < (double)min_near) near = (double)min_near;
    nears[n] = near;
    fars[n] = far;
}

__global__ __launch_bounds__(F64_THREADS) void k_f64_sph_from_ray(const double* __restrict__ rays_o, const double* __restrict__ rays_d, float radius,
                                                                   uint32_t N, double* __restrict__ coords) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= N) return;
    const double ox = rays_o[(size_t)n * 3], oy = rays_o[(size_t)n * 3 + 1], oz = rays_o[(size_t)n * 3 + 2];
    const double dx = rays_d[(size_t)n * 3], dy = rays_d[(size_t)n * 3 + 1], dz = rays_d[(size_t)n * 3 + 2];
    const double r = (double)radius;
    const double A = dx * dx + dy * dy + dz * dz;
    const double Bh = ox * dx + oy * dy + oz * dz;
    const double Cc = ox * ox + oy * oy + oz * oz - r * r;
    const double t = (-Bh + sqrt(Bh * Bh - A * Cc)) / A;
    const double x = ox + t * dx, y = oy + t * dy, z = oz + t * dz;
    const double theta = atan2(sqrt(x * x + z * z), y);
    const double phi = atan2(z, x);
    const double RPI = 0.31830988618379067;  // 1 / pi
    coords[(size_t)n * 2] = 2.0 * theta * RPI - 1.0;
    coords[(size_t)n * 2 + 1] = phi * RPI;
}

__global__ __launch_bounds__(F64_THREADS) void k_f64_packbits(const double* __restrict__ grid, uint32_t N, float thresh, uint8_t* __restrict__ bitfield) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= N) return;
    const double* g = grid + (size_t)n * 8;
    const double th = (double)thresh;
    uint32_t bits = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) bits |= g[i] > th ? (1u << i) : 0u;
    bitfield[n] = (uint8_t)bits;
}

// ------------------------------------------------------------------------------------------------
// compositing (raymarching.cu:488-661, 819-905): the reference's per-ray loops, one lane per ray
// ------------------------------------------------------------------------------------------------
// GEO (raymarching.hip: k_composite_train_geo_fwd / _bwd): differentiable depth and the distortion
// L = sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 d0_i as L = sum_i 2 w_i (t_i W_<i - D_<i) + 1/3 sum_i w_i^2 d0_i, running sums in double.
// Its terms sit under `if constexpr`, not behind zero factors: 0 * inf and -0 + 0 would change the plain op's bits.
template <bool GEO>
__global__ __launch_bounds__(F64_THREADS) void k_f64_composite_train_fwd(const double* __restrict__ sigmas, const double* __restrict__ rgbs,
                                                                          const double* __restrict__ deltas, const int32_t* __restrict__ rays, uint32_t M,
                                                                          uint32_t N, float T_thresh, double* __restrict__ weights_sum,
                                                                          double* __restrict__ depth, double* __restrict__ image,
                                                                          double* __restrict__ distortion) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num = (uint32_t)rays[n * 3 + 2];
    const double th = (double)T_thresh;
    double r = 0.0, g = 0.0, b = 0.0, ws = 0.0, d = 0.0, dist = 0.0, T = 1.0, t = 0.0;
    if (num != 0u && offset + num <= M) {
        for (uint32_t s = 0; s < num; s++) {
            const size_t o = (size_t)offset + s;
            const double d0 = deltas[o * 2];
            const double alpha = 1.0 - exp(-sigmas[o] * d0);
            const double w = alpha * T;
            r += w * rgbs[o * 3];
            g += w * rgbs[o * 3 + 1];
            b += w * rgbs[o * 3 + 2];
            t += deltas[o * 2 + 1];
            if constexpr (GEO) dist += 2.0 * w * (t * ws - d) + (1.0 / 3.0) * (w * w * d0);  // ws, d: the exclusive prefixes W_<i, D_<i
            d += w * t;
            ws += w;
            T *= 1.0 - alpha;
            if (T < th) break;  // the sample that drives T below the threshold is composited (raymarching.cu:557-560)
        }
    }
    weights_sum[index] = ws;
    depth[index] = d;
    image[index * 3] = r;
    image[index * 3 + 1] = g;
    image[index * 3 + 2] = b;
    if constexpr (GEO) distortion[index] = dist;
}

// one sweep.  GEO: g_i = dL/dw_i = 2 (t_i W_<i - D_<i) + 2 ((D - D_<=i) - t_i (W - W_<=i)) + 2/3 w_i d0_i, dD/dsigma_i = d0_i (T_{i+1} t_i - (D - D_<=i)),
// dL/dsigma_i = d0_i (g_i T_{i+1} - (G - G_<=i)) with G = sum_j g_j w_j = 2 L; a NULL gradient is a zero gradient (the plain entry requires its two)
template <bool GEO>
__global__ __launch_bounds__(F64_THREADS) void k_f64_composite_train_bwd(const double* __restrict__ grad_ws, const double* __restrict__ grad_depth,
                                                                          const double* __restrict__ grad_image, const double* __restrict__ grad_dist,
                                                                          const double* __restrict__ sigmas, const double* __restrict__ rgbs,
                                                                          const double* __restrict__ deltas, const int32_t* __restrict__ rays,
                                                                          const double* __restrict__ weights_sum, const double* __restrict__ depth,
                                                                          const double* __restrict__ image, const double* __restrict__ distortion,
                                                                          uint32_t M, uint32_t N, float T_thresh, double* __restrict__ grad_sigmas,
                                                                          double* __restrict__ grad_rgbs) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num = (uint32_t)rays[n * 3 + 2];
    if (num == 0u || offset + num > M) return;
    const double th = (double)T_thresh;
    const double gi0 = grad_image ? grad_image[index * 3] : 0.0, gi1 = grad_image ? grad_image[index * 3 + 1] : 0.0,
                 gi2 = grad_image ? grad_image[index * 3 + 2] : 0.0;
    const double gw = grad_ws ? grad_ws[index] : 0.0;
    const double rf = image[index * 3], gf = image[index * 3 + 1], bf = image[index * 3 + 2], wsf = weights_sum[index];
    double gd = 0.0, gl = 0.0, df = 0.0, gtot = 0.0;
    if constexpr (GEO) {
        gd = grad_depth ? grad_depth[index] : 0.0;
        gl = grad_dist ? grad_dist[index] : 0.0;
        df = depth[index];
        gtot = 2.0 * distortion[index];
    }
    double r = 0.0, g = 0.0, b = 0.0, ws = 0.0, d = 0.0, gg = 0.0, T = 1.0, t = 0.0;
    for (uint32_t s = 0; s < num; s++) {
        const size_t o = (size_t)offset + s;
        const double d0 = deltas[o * 2];
        const double cr = rgbs[o * 3], cg = rgbs[o * 3 + 1], cb = rgbs[o * 3 + 2];
        const double alpha = 1.0 - exp(-sigmas[o] * d0);
        const double w = alpha * T;
        r += w * cr;
        g += w * cg;
        b += w * cb;
        T *= 1.0 - alpha;  // transmittance after this sample
        double plain = gi0 * (T * cr - (rf - r)) + gi1 * (T * cg - (gf - g)) + gi2 * (T * cb - (bf - b)) + gw * (1.0 - wsf);
        if constexpr (GEO) {
            t += deltas[o * 2 + 1];
            const double before = t * ws - d;  // t_i W_<i - D_<i
            ws += w;
            d += w * t;
            const double gwi = 2.0 * before + 2.0 * ((df - d) - t * (wsf - ws)) + (2.0 / 3.0) * (w * d0);
            gg += gwi * w;
            plain = plain + gd * (T * t - (df - d)) + gl * (gwi * T - (gtot - gg));
        }
        grad_rgbs[o * 3] = gi0 * w;
        grad_rgbs[o * 3 + 1] = gi1 * w;
        grad_rgbs[o * 3 + 2] = gi2 * w;
        grad_sigmas[o] = d0 * plain;
        if (T < th) break;
    }
}

// compositing of per-sample feature channels (raymarching.hip: k_composite_feat_fwd / _bwd): out[index, c] = sum_i w_i feats[i, c]
__global__ __launch_bounds__(F64_THREADS) void k_f64_composite_feat_fwd(const double* __restrict__ sigmas, const double* __restrict__ feats,
                                                                         const double* __restrict__ deltas, const int32_t* __restrict__ rays, uint32_t M,
                                                                         uint32_t N, uint32_t C, float T_thresh, double* __restrict__ out) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num = (uint32_t)rays[n * 3 + 2];
    const double th = (double)T_thresh;
    double* __restrict__ acc = out + (size_t)index * C;  // the ray's own output row is its accumulator
    for (uint32_t c = 0; c < C; c++) acc[c] = 0.0;
    if (num == 0u || offset + num > M) return;
    double T = 1.0;
    for (uint32_t s = 0; s < num; s++) {
        const size_t o = (size_t)offset + s;
        const double alpha = 1.0 - exp(-sigmas[o] * deltas[o * 2]);
        const double w = alpha * T;
        for (uint32_t c = 0; c < C; c++) acc[c] += w * feats[o * C + c];
        T *= 1.0 - alpha;
        if (T < th) break;  // the sample that drives T below the threshold is composited (raymarching.cu:557-560)
    }
}

// q_i = sum_c grad_out[c] feats[i, c], Q = sum_c grad_out[c] out[c]:  grad_feats[i, c] = w_i grad_out[c],
// grad_sigmas[i] = d0_i (T_{i+1} q_i - (Q - sum_{j<=i} w_j q_j))
__global__ __launch_bounds__(F64_THREADS) void k_f64_composite_feat_bwd(const double* __restrict__ grad_out, const double* __restrict__ sigmas,
                                                                         const double* __restrict__ feats, const double* __restrict__ deltas,
                                                                         const int32_t* __restrict__ rays, const double* __restrict__ out, uint32_t M,
                                                                         uint32_t N, uint32_t C, float T_thresh, double* __restrict__ grad_sigmas,
                                                                         double* __restrict__ grad_feats) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num = (uint32_t)rays[n * 3 + 2];
    if (num == 0u || offset + num > M) return;
    const double th = (double)T_thresh;
    const double* __restrict__ g = grad_out + (size_t)index * C;
    double Q = 0.0;
    for (uint32_t c = 0; c < C; c++) Q += g[c] * out[(size_t)index * C + c];
    double T = 1.0, done = 0.0;
    for (uint32_t s = 0; s < num; s++) {
        const size_t o = (size_t)offset + s;
        const double d0 = deltas[o * 2];
        const double alpha = 1.0 - exp(-sigmas[o] * d0);
        const double w = alpha * T;
        double q = 0.0;
        for (uint32_t c = 0; c < C; c++) {
            q += g[c] * feats[o * C + c];
            grad_feats[o * C + c] = g[c] * w;
        }
        done += w * q;
        T *= 1.0 - alpha;  // transmittance after this sample
        grad_sigmas[o] = d0 * (T * q - (Q - done));
        if (T < th) break;
    }
}

__global__ __launch_bounds__(F64_THREADS) void k_f64_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* __restrict__ rays_alive,
                                                                     double* __restrict__ rays_t, const double* __restrict__ sigmas,
                                                                     const double* __restrict__ rgbs, const double* __restrict__ deltas,
                                                                     double* __restrict__ weights_sum, double* __restrict__ depth,
                                                                     double* __restrict__ image) {
    const uint32_t n = blockIdx.x * F64_THREADS + threadIdx.x;
    if (n >= n_alive) return;
    const uint32_t index = (uint32_t)rays_alive[n];
    const double* sg = sigmas + (size_t)n * n_step;
    const double* rg = rgbs + (size_t)n * n_step * 3;
    const double* de = deltas + (size_t)n * n_step * 2;
    const double th = (double)T_thresh;
    double t = rays_t[index], ws = weights_sum[index], d = depth[index];
    double r = image[index * 3], g = image[index * 3 + 1], b = image[index * 3 + 2];
    uint32_t step = 0;
    while (step < n_step) {
        const double d0 = de[step * 2];
        if (d0 == 0.0) break;
        const double alpha = 1.0 - exp(-sg[step] * d0);
        const double T = 1.0 - ws;
        const double w = alpha * T;
        ws += w;
        t += de[step * 2 + 1];
        d += w * t;
        r += w * rg[step * 3];
        g += w * rg[step * 3 + 1];
        b += w * rg[step * 3 + 2];
        if (T < th) break;
        step++;
    }
    if (step < n_step) rays_alive[n] = -1;
    else rays_t[index] = t;
    weights_sum[index] = ws;
    depth[index] = d;
    image[index * 3] = r;
    image[index * 3 + 1] = g;
    image[index * 3 + 2] = b;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
template <int D, int C>
static int launch_f64_forward(const float* inputs, const void* emb, const int32_t* offsets, void* outputs, uint32_t B, uint32_t L, const GridLevels& lv,
                              void* dy_dx, uint32_t gridtype, bool ac, uint32_t interp, hipStream_t st) {
    const dim3 grid(grid_blocks(B, F64_THREADS), L, 1);
    if (dy_dx)
        NGP_LAUNCH((k_f64_grid_fwd<D, C, true>), grid, dim3(F64_THREADS), 0, st, inputs, (const double*)emb, offsets, (double*)outputs, B, L, lv,
                           (double*)dy_dx, gridtype, ac, interp);
    else
        NGP_LAUNCH((k_f64_grid_fwd<D, C, false>), grid, dim3(F64_THREADS), 0, st, inputs, (const double*)emb, offsets, (double*)outputs, B, L,
                           lv, (double*)nullptr, gridtype, ac, interp);
    return check_launch("grid_encode_forward(fp64)");
}

int f64_grid_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                     float S, uint32_t H, void* dy_dx, uint32_t gridtype, bool align_corners, uint32_t interp, hipStream_t st) {
    if (B == 0) return NGP_OK;
    GridLevels lv;
    fill_levels(lv, L, S, H);
    NGP_DISPATCH_DC(D, C, launch_f64_forward<D_, C_>(inputs, embeddings, offsets, outputs, B, L, lv, dy_dx, gridtype, align_corners, interp, st))
    set_error("grid_encode_forward: unsupported (D=%u, C=%u)", D, C);
    return NGP_ERR_INVALID;
}

// workspace: the record sort's alone (grid_records.h: rec_layout)
size_t f64_grid_backward_workspace_bytes(uint32_t B, uint32_t D) {
    if (B == 0 || D < 2 || D > 5) return 0;
    return rec_layout(B, D).bytes;
}

int f64_grid_check_workspace(const char* fn, const char* query, uint32_t B, uint32_t D, const void* workspace, size_t workspace_bytes) {
    return rec_check_workspace(fn, "fp64", query, B, D, f64_grid_backward_workspace_bytes(B, D), workspace, workspace_bytes);
}

template <int D, int C, int ORDER>
static int launch_f64_table_grad(const void* grad, const float* inputs, const int32_t* offsets, const void* u, void* grad_emb, uint32_t B, uint32_t L,
                                 const GridLevels& lv, uint32_t gridtype, bool ac, uint32_t interp, void* workspace, hipStream_t st) {
    for (uint32_t level = 0; level < L; level++) {
        const RecSides r = rec_sort_level(D, inputs, offsets, B, level, lv.scale[level], lv.res[level], gridtype, ac, interp, InputMap{0.0f, 0.0f},
                                          workspace, st);
        NGP_LAUNCH((k_f64_grid_run_sum<D, C, ORDER>), dim3(grid_blocks(r.n, F64_THREADS)), dim3(F64_THREADS), 0, st, r.keys[0], r.vals[0], r.keys[1],
                           r.vals[1], r.n, (const double*)grad, inputs, (const double*)u, offsets, (double*)grad_emb, B, level, lv.scale[level], ac,
                           interp);
        const int rc = check_launch(ORDER == 1 ? "grid_encode_backward(fp64)" : "grid_encode_backward_backward(fp64)");
        if (rc) return rc;
    }
    return NGP_OK;
}

int f64_grid_table_grad(uint32_t order, const void* grad, const float* inputs, const int32_t* offsets, const void* u, void* grad_embeddings,
                        uint32_t B, uint32_t D, uint32_t C, uint32_t L, const GridLevels& lv, uint32_t gridtype, bool align_corners, uint32_t interp,
                        void* workspace, hipStream_t st) {
    if (order == 1) {
        NGP_DISPATCH_DC(D, C, launch_f64_table_grad<D_, C_, 1>(grad, inputs, offsets, u, grad_embeddings, B, L, lv, gridtype, align_corners, interp,
                                                               workspace, st))
    } else {
        NGP_DISPATCH_DC(D, C, launch_f64_table_grad<D_, C_, 2>(grad, inputs, offsets, u, grad_embeddings, B, L, lv, gridtype, align_corners, interp,
                                                               workspace, st))
    }
    return NGP_ERR_INVALID;   // (D and C are checked by the entries)
}

int f64_grid_backward(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                      uint32_t L, float S, uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype, bool align_corners, uint32_t interp,
                      void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (B == 0) return NGP_OK;
    int rc = f64_grid_check_workspace("grid_encode_backward", "ngp_grid_backward_workspace_bytes", B, D, workspace, workspace_bytes);
    if (rc) return rc;
    GridLevels lv;
    fill_levels(lv, L, S, H);
    rc = f64_grid_table_grad(1, grad, inputs, offsets, nullptr, grad_embeddings, B, D, C, L, lv, gridtype, align_corners, interp, workspace, st);
    if (rc || !(dy_dx && grad_inputs)) return rc;
    NGP_LAUNCH(k_f64_grid_input_bwd, dim3(cdiv(B * D, F64_THREADS)), dim3(F64_THREADS), 0, st, (const double*)grad, (const double*)dy_dx,
                       (double*)grad_inputs, B, L, D, C);
    return check_launch("grid_encode_backward(fp64 input)");
}

template <int D, int C>
static int launch_f64_tv(const void* inputs, const void* emb, void* grad, const int32_t* offsets, float weight, uint32_t B, uint32_t L,
                         const GridLevels& lv, uint32_t gridtype, bool ac, hipStream_t st) {
    NGP_LAUNCH((k_f64_grad_tv<D, C>), dim3(grid_blocks(B, F64_THREADS), L, 1), dim3(F64_THREADS), 0, st, (const double*)inputs, (const double*)emb,
                       (double*)grad, offsets, weight, B, lv, gridtype, ac);
    return check_launch("grad_total_variation(fp64)");
}

int f64_grad_tv(const void* inputs, const void* embeddings, void* grad, const int32_t* offsets, float weight, uint32_t B, uint32_t D, uint32_t C,
                uint32_t L, float S, uint32_t H, uint32_t gridtype, bool align_corners, hipStream_t st) {
    if (B == 0) return NGP_OK;
    GridLevels lv;
    fill_levels(lv, L, S, H);
    NGP_DISPATCH_DC(D, C, launch_f64_tv<D_, C_>(inputs, embeddings, grad, offsets, weight, B, L, lv, gridtype, align_corners, st))
    set_error("grad_total_variation: unsupported (D=%u, C=%u)", D, C);
    return NGP_ERR_INVALID;
}

template <int BANDS>
static int launch_f64_sh(const void* inputs, void* outputs, uint32_t B, void* dy_dx, hipStream_t st) {
    const dim3 grid(cdiv(B, F64_THREADS));
    if (dy_dx)
        NGP_LAUNCH((k_f64_sh_fwd<BANDS, true>), grid, dim3(F64_THREADS), 0, st, (const double*)inputs, (double*)outputs, B, (double*)dy_dx);
    else
        NGP_LAUNCH((k_f64_sh_fwd<BANDS, false>), grid, dim3(F64_THREADS), 0, st, (const double*)inputs, (double*)outputs, B, (double*)nullptr);
    return check_launch("sh_encode_forward(fp64)");
}

int f64_sh_forward(const void* inputs, void* outputs, uint32_t B, uint32_t C, void* dy_dx, hipStream_t st) {
    if (B == 0) return NGP_OK;
    switch (C) {
        case 1: return launch_f64_sh<1>(inputs, outputs, B, dy_dx, st);
        case 2: return launch_f64_sh<2>(inputs, outputs, B, dy_dx, st);
        case 3: return launch_f64_sh<3>(inputs, outputs, B, dy_dx, st);
        case 4: return launch_f64_sh<4>(inputs, outputs, B, dy_dx, st);
        case 5: return launch_f64_sh<5>(inputs, outputs, B, dy_dx, st);
        case 6: return launch_f64_sh<6>(inputs, outputs, B, dy_dx, st);
        case 7: return launch_f64_sh<7>(inputs, outputs, B, dy_dx, st);
        default: return launch_f64_sh<8>(inputs, outputs, B, dy_dx, st);
    }
}

int f64_sh_backward(const void* grad, uint32_t B, uint32_t C, const void* dy_dx, void* grad_inputs, hipStream_t st) {
    if (B == 0) return NGP_OK;
    NGP_LAUNCH(k_f64_sh_bwd, dim3(cdiv(B * 3, F64_THREADS)), dim3(F64_THREADS), 0, st, (const double*)grad, B, C * C, (const double*)dy_dx,
                       (double*)grad_inputs);
    return check_launch("sh_encode_backward(fp64)");
}

}  // namespace ngp

using namespace ngp;

#define F64_LAUNCH_1D(kernel, count, st, ...) NGP_LAUNCH(kernel, dim3(cdiv((count), F64_THREADS)), dim3(F64_THREADS), 0, st, __VA_ARGS__)

extern "C" int ngp_near_far_from_aabb_f64(const double* rays_o, const double* rays_d, const double* aabb, uint32_t N, float min_near, double* nears,
                                          double* fars, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_o && rays_d && aabb && nears && fars, NGP_ERR_INVALID, "near_far_from_aabb_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_near_far, N, as_stream(stream), rays_o, rays_d, aabb, N, min_near, nears, fars);
    return check_launch("near_far_from_aabb_f64");
}

extern "C" int ngp_sph_from_ray_f64(const double* rays_o, const double* rays_d, float radius, uint32_t N, double* coords, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_o && rays_d && coords, NGP_ERR_INVALID, "sph_from_ray_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_sph_from_ray, N, as_stream(stream), rays_o, rays_d, radius, N, coords);
    return check_launch("sph_from_ray_f64");
}

extern "C" int ngp_packbits_f64(const double* grid, uint32_t N, float density_thresh, uint8_t* bitfield, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grid && bitfield, NGP_ERR_INVALID, "packbits_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_packbits, N, as_stream(stream), grid, N, density_thresh, bitfield);
    return check_launch("packbits_f64");
}

extern "C" int ngp_composite_rays_train_forward_f64(const double* sigmas, const double* rgbs, const double* deltas, const int32_t* rays, uint32_t M,
                                                    uint32_t N, float T_thresh, double* weights_sum, double* depth, double* image,
                                                    ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(sigmas && rgbs && deltas && rays && weights_sum && depth && image, NGP_ERR_INVALID, "composite_rays_train_forward_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_composite_train_fwd<false>, N, as_stream(stream), sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image,
                  (double*)nullptr);
    return check_launch("composite_rays_train_forward_f64");
}

extern "C" int ngp_composite_rays_train_backward_f64(const double* grad_weights_sum, const double* grad_image, const double* sigmas, const double* rgbs,
                                                     const double* deltas, const int32_t* rays, const double* weights_sum, const double* image,
                                                     uint32_t M, uint32_t N, float T_thresh, double* grad_sigmas, double* grad_rgbs,
                                                     ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grad_weights_sum && grad_image && sigmas && rgbs && deltas && rays && weights_sum && image && grad_sigmas && grad_rgbs, NGP_ERR_INVALID,
                "composite_rays_train_backward_f64: NULL tensor");
    const double* none = nullptr;  // the geometry arguments of the shared kernel
    F64_LAUNCH_1D(k_f64_composite_train_bwd<false>, N, as_stream(stream), grad_weights_sum, none, grad_image, none, sigmas, rgbs, deltas, rays,
                  weights_sum, none, image, none, M, N, T_thresh, grad_sigmas, grad_rgbs);
    return check_launch("composite_rays_train_backward_f64");
}

extern "C" int ngp_composite_rays_train_geo_forward_f64(const double* sigmas, const double* rgbs, const double* deltas, const int32_t* rays,
                                                        uint32_t M, uint32_t N, float T_thresh, double* weights_sum, double* depth, double* image,
                                                        double* distortion, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(sigmas && rgbs && deltas && rays && weights_sum && depth && image && distortion, NGP_ERR_INVALID,
                "composite_rays_train_geo_forward_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_composite_train_fwd<true>, N, as_stream(stream), sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image,
                  distortion);
    return check_launch("composite_rays_train_geo_forward_f64");
}

extern "C" int ngp_composite_rays_train_geo_backward_f64(const double* grad_weights_sum, const double* grad_depth, const double* grad_image,
                                                         const double* grad_distortion, const double* sigmas, const double* rgbs,
                                                         const double* deltas, const int32_t* rays, const double* weights_sum,
                                                         const double* depth, const double* image, const double* distortion, uint32_t M,
                                                         uint32_t N, float T_thresh, double* grad_sigmas, double* grad_rgbs, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(sigmas && rgbs && deltas && rays && weights_sum && depth && image && distortion && grad_sigmas && grad_rgbs, NGP_ERR_INVALID,
                "composite_rays_train_geo_backward_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_composite_train_bwd<true>, N, as_stream(stream), grad_weights_sum, grad_depth, grad_image, grad_distortion, sigmas, rgbs,
                  deltas, rays, weights_sum, depth, image, distortion, M, N, T_thresh, grad_sigmas, grad_rgbs);
    return check_launch("composite_rays_train_geo_backward_f64");
}

extern "C" int ngp_composite_rays_train_features_forward_f64(const double* sigmas, const double* feats, const double* deltas, const int32_t* rays,
                                                             uint32_t M, uint32_t N, uint32_t C, float T_thresh, double* out, ngp_stream_t stream) {
    NGP_REQUIRE(C >= 1 && C <= 256, NGP_ERR_INVALID, "composite_rays_train_features_forward_f64: C = %u is outside 1 .. 256", C);
    if (N == 0 || M == 0) return NGP_OK;
    NGP_REQUIRE(sigmas && feats && deltas && rays && out, NGP_ERR_INVALID, "composite_rays_train_features_forward_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_composite_feat_fwd, N, as_stream(stream), sigmas, feats, deltas, rays, M, N, C, T_thresh, out);
    return check_launch("composite_rays_train_features_forward_f64");
}

extern "C" int ngp_composite_rays_train_features_backward_f64(const double* grad_out, const double* sigmas, const double* feats, const double* deltas,
                                                              const int32_t* rays, const double* out, uint32_t M, uint32_t N, uint32_t C,
                                                              float T_thresh, double* grad_sigmas, double* grad_feats, ngp_stream_t stream) {
    NGP_REQUIRE(C >= 1 && C <= 256, NGP_ERR_INVALID, "composite_rays_train_features_backward_f64: C = %u is outside 1 .. 256", C);
    if (N == 0 || M == 0) return NGP_OK;
    NGP_REQUIRE(grad_out && sigmas && feats && deltas && rays && out && grad_sigmas && grad_feats, NGP_ERR_INVALID,
                "composite_rays_train_features_backward_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_composite_feat_bwd, N, as_stream(stream), grad_out, sigmas, feats, deltas, rays, out, M, N, C, T_thresh, grad_sigmas,
                  grad_feats);
    return check_launch("composite_rays_train_features_backward_f64");
}

extern "C" int ngp_composite_rays_f64(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive, double* rays_t, const double* sigmas,
                                      const double* rgbs, const double* deltas, double* weights_sum, double* depth, double* image,
                                      ngp_stream_t stream) {
    if (n_alive == 0) return NGP_OK;
    NGP_REQUIRE(rays_alive && rays_t && sigmas && rgbs && deltas && weights_sum && depth && image, NGP_ERR_INVALID, "composite_rays_f64: NULL tensor");
    F64_LAUNCH_1D(k_f64_composite_rays, n_alive, as_stream(stream), n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum,
                  depth, image);
    return check_launch("composite_rays_f64");
}

// fp64 twins of ngp_sdf_sigmas_forward / _backward (sdf_sigmas.h: the same kernel bodies and host half instantiated for double)
namespace ngp {
SDF_SIGMAS_KERNELS(double, k_f64_sdf_sigmas)
static const SdfKernels<double> sdf_kernels_f64 = {k_f64_sdf_sigmas_fwd, k_f64_sdf_sigmas_bwd, k_f64_sdf_sigmas_inv_s};
}  // namespace ngp

extern "C" int ngp_sdf_sigmas_forward_f64(const double* sdf, const double* normals, const double* dirs, const double* deltas, const double* inv_s,
                                          uint32_t M, float cos_anneal, double* sigmas, ngp_stream_t stream) {
    return sdf_sigmas_forward<double>("sdf_sigmas_forward_f64", sdf_kernels_f64, sdf, normals, dirs, deltas, inv_s, M, cos_anneal, sigmas, as_stream(stream));
}

extern "C" int ngp_sdf_sigmas_backward_f64(const double* grad_sigmas, const double* sdf, const double* normals, const double* dirs, const double* deltas,
                                           const double* inv_s, uint32_t M, float cos_anneal, double* grad_sdf, double* grad_normals, double* grad_dirs,
                                           double* grad_inv_s, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    return sdf_sigmas_backward<double>("sdf_sigmas_backward_f64", sdf_kernels_f64, grad_sigmas, sdf, normals, dirs, deltas, inv_s, M, cos_anneal, grad_sdf,
                                       grad_normals, grad_dirs, grad_inv_s, workspace, workspace_bytes, as_stream(stream));
}
