// Error-map ray sampling on the device: the two places where the reference's `-O --error_map` recipe leaves the library --
//   ngp_error_map_draw    get_rays' error-map branch (nerf/utils.py:85-106: torch.multinomial without replacement over the 128 x 128 map,
//                         then a uniform offset inside each drawn cell), as ONE launch with a counter-based generator and no torch RNG;
//   ngp_error_map_update  the Trainer's per-step update of the map (nerf/utils.py: train_step's error-map branch: gather, 0.1 / 0.9 EMA of
//                         the per-ray squared error, scatter_), as one launch.
// The draw is the exponential race torch.multinomial itself runs (key = Exp(1) / weight, the N smallest keys win): successive sampling
// without replacement proportional to the weights.  One workgroup per image; every lane keeps 16 keys in registers, the N-th smallest key is
// found by a radix select (most significant byte first) over one 256-bin LDS histogram, ties at the threshold go to the lowest cell
// indices, and the winners are written in ascending cell order after a block scan.  No global atomics, no workspace, no host read-back.
#include "common.h"

namespace ngp {

constexpr int EM_THREADS = 1024, EM_KEYS = 16, EM_WAVES = EM_THREADS / WAVE;   // 1024 x 16 = 128 x 128 cells
constexpr uint32_t EM_MAX_RES = 128;
constexpr uint32_t EM_NO_CELL = 0xFFFFFFFFu;   // key of a register slot past the map: above +inf, never selected (N <= cells), never counted
constexpr int EM_PEEL = 4;                     // histogram: bins a wave adds as ONE atomic each before its lanes go one by one
constexpr int EM_UPDATE_THREADS = 256;

// the finaliser of seeded_noise (raymarching.hip)
__device__ __forceinline__ uint32_t em_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
// cell i under seed word sk = s * 0x85EBCA6B + 0x27D4EB2F; em_word(...) = word(i, b, k) of include/ngp_hip.h
__device__ __forceinline__ uint32_t em_cell_hash(uint32_t i, uint32_t sk) { return em_mix((i * 0x9E3779B9u) ^ sk); }
__device__ __forceinline__ uint32_t em_word(uint32_t cell_hash, uint32_t b, uint32_t k) {
    return em_mix(cell_hash ^ (b * 0xC2B2AE35u + k * 0x165667B1u + 0x27D4EB2Fu));
}

struct EmShared {
    uint32_t hist[256];
    uint32_t wave_tot[EM_WAVES];
    uint32_t bin, rank, drawable;
};

// exclusive prefix sum of v over the block's threads (all threads call it)
__device__ __forceinline__ uint32_t em_block_exclusive_scan(uint32_t v, uint32_t* wave_tot) {
    const uint32_t t = threadIdx.x, w = t >> 6;
    const uint32_t inc = wave_inclusive_scan(v);
    __syncthreads();   // the readers of an earlier use are done
    if ((t & 63u) == 63u) wave_tot[w] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (uint32_t q = 0; q < (uint32_t)EM_WAVES; q++) {
        const uint32_t x = wave_tot[q];
        base += q < w ? x : 0u;
    }
    return base + inc - v;
}

// one histogram increment per candidate lane.  Keys are floats: in the first pass (sign + seven exponent bits) most of a wave's lanes meet
// in a handful of bins, and same-address LDS atomics serialise -- there the first EM_PEEL distinct bins of the wave are added by one lane
// each (population count of the ballot; the bin travels through a scalar register), what is left goes lane by lane.  The later passes see
// few candidates spread over 256 bins and add lane by lane at once.
template <bool PEEL>
__device__ __forceinline__ void em_histogram_add(uint32_t* hist, bool cand, uint32_t bin) {
    unsigned long long rem = __ballot(cand);
    if (PEEL) {
#pragma unroll 1
        for (int r = 0; r < EM_PEEL && rem != 0ull; r++) {
            const int first = __ffsll((long long)rem) - 1;
            const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
            const unsigned long long same = __ballot(cand && bin == lead) & rem;
            if ((int)(threadIdx.x & 63u) == first) atomicAdd(&hist[lead], (uint32_t)__popcll(same));
            rem &= ~same;
        }
    }
    if (cand && ((rem >> (threadIdx.x & 63u)) & 1ull)) atomicAdd(&hist[bin], 1u);
}

__global__ __launch_bounds__(EM_THREADS) void k_error_map_draw(const float* __restrict__ error_map, uint32_t res, uint32_t N, uint32_t H, uint32_t W,
                                                               uint32_t seed, const uint32_t* __restrict__ seed_dev, long long* __restrict__ inds,
                                                               long long* __restrict__ inds_coarse, float* __restrict__ keys_out,
                                                               uint32_t* __restrict__ n_drawable) {
    __shared__ EmShared sh;
    const uint32_t b = blockIdx.x, t = threadIdx.x, cells = res * res;
    const uint32_t s = seed + (seed_dev ? seed_dev[0] : 0u);
    const uint32_t sk = s * 0x85EBCA6Bu + 0x27D4EB2Fu;
    const float* __restrict__ weights = error_map + (size_t)b * cells;
    if (t == 0u) sh.drawable = 0u;

    // ---- keys: lane t owns cells 16 t .. 16 t + 15 (ascending: the compaction below writes them in order) ----
    uint32_t key[EM_KEYS];
    uint32_t drawable = 0;
#pragma unroll
    for (int j = 0; j < EM_KEYS; j++) {
        const uint32_t i = t * EM_KEYS + j;
        key[j] = EM_NO_CELL;
        if (i < cells) {
            const float w = weights[i];
            const uint32_t word = em_word(em_cell_hash(i, sk), b, 0u);
            const float u = (float)(((word >> 9) << 1) | 1u) * 0x1p-24f;   // odd 24-bit integer / 2^24: exact, inside (0, 1)
            const bool ok = __builtin_isfinite(w) && w > 0.0f;
            const float k = ok ? (-logf(u)) / w : __builtin_inff();
            key[j] = __float_as_uint(k);                                    // positive or +inf: the bits order as the values
            drawable += ok ? 1u : 0u;
            if (keys_out) keys_out[(size_t)b * cells + i] = k;
        }
    }
    __syncthreads();
    if (n_drawable) {
        const uint32_t inc = wave_inclusive_scan(drawable);
        if ((t & 63u) == 63u) atomicAdd(&sh.drawable, inc);
    }

    // ---- the N-th smallest key: radix select, most significant byte first ----
    uint32_t prefix = 0, mask = 0, rank = N;   // rank: 1-based position of the wanted key among the keys that still match prefix
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (t < 256u) sh.hist[t] = 0u;
        __syncthreads();
        if (shift == 24) {
#pragma unroll
            for (int j = 0; j < EM_KEYS; j++) em_histogram_add<true>(sh.hist, key[j] != EM_NO_CELL, key[j] >> 24);
        } else {
#pragma unroll
            for (int j = 0; j < EM_KEYS; j++)
                em_histogram_add<false>(sh.hist, key[j] != EM_NO_CELL && (key[j] & mask) == prefix, (key[j] >> shift) & 255u);
        }
        __syncthreads();
        const uint32_t v = t < 256u ? sh.hist[t] : 0u;
        const uint32_t inc = wave_inclusive_scan(v);
        if (t < 256u && (t & 63u) == 63u) sh.wave_tot[t >> 6] = inc;
        __syncthreads();
        if (t < 256u) {
            uint32_t base = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) base += q < (t >> 6) ? sh.wave_tot[q] : 0u;
            const uint32_t upto = base + inc, before = upto - v;
            if (before < rank && rank <= upto) {   // exactly one bin: the histogram holds >= rank keys
                sh.bin = t;
                sh.rank = rank - before;
            }
        }
        __syncthreads();
        prefix |= sh.bin << shift;
        mask |= 255u << shift;
        rank = sh.rank;
    }
    if (n_drawable && t == 0u) n_drawable[b] = sh.drawable;   // (ordered behind the waves' additions by the barriers above)

    // ---- selection: every key below the threshold, and the `rank` lowest-indexed cells whose key IS the threshold ----
    const uint32_t threshold = prefix;
    uint32_t ties = 0;
#pragma unroll
    for (int j = 0; j < EM_KEYS; j++) ties += key[j] == threshold ? 1u : 0u;
    uint32_t tie_at = em_block_exclusive_scan(ties, sh.wave_tot);
    uint32_t chosen = 0, count = 0;
#pragma unroll
    for (int j = 0; j < EM_KEYS; j++) {
        bool take = key[j] < threshold;
        if (key[j] == threshold) take = tie_at++ < rank;
        chosen |= take ? 1u << j : 0u;
        count += take ? 1u : 0u;
    }
    uint32_t at = em_block_exclusive_scan(count, sh.wave_tot);

    // ---- refinement to pixels (plain fp32: the library is built with -ffp-contract=off) and the outputs, ascending cell order ----
    const float cell_h = (float)H / (float)res, cell_w = (float)W / (float)res;
    uint32_t cell_row = (t * EM_KEYS) / res, cell_col = (t * EM_KEYS) % res;   // i / res, i % res of the lane's cells: one division, then steps
#pragma unroll
    for (int j = 0; j < EM_KEYS; j++) {
        if (((chosen >> j) & 1u) && at < N) {   // (at < N always: exactly N cells are chosen; the guard keeps the stores inside [B,N] regardless)
            const uint32_t i = t * EM_KEYS + j;
            NGP_BOUNDS(i < cells);
            const uint32_t h = em_cell_hash(i, sk);
            const float r = (float)(em_word(h, b, 1u) >> 8) * 0x1p-24f, c = (float)(em_word(h, b, 2u) >> 8) * 0x1p-24f;
            const float fr = (float)cell_row * cell_h + r * cell_h, fc = (float)cell_col * cell_w + c * cell_w;
            const uint32_t row = min((uint32_t)fr, H - 1u), col = min((uint32_t)fc, W - 1u);
            const size_t o = (size_t)b * N + at;
            inds[o] = (long long)(row * W + col);
            inds_coarse[o] = (long long)i;
            at++;
        }
        if (++cell_col == res) {
            cell_col = 0;
            cell_row++;
        }
    }
}

__global__ __launch_bounds__(EM_UPDATE_THREADS) void k_error_map_update(float* __restrict__ row, const long long* __restrict__ inds_coarse,
                                                                        const float* __restrict__ image, const float* __restrict__ target, uint32_t N,
                                                                        uint32_t n_cells, float keep, float take) {
    const uint32_t n = blockIdx.x * EM_UPDATE_THREADS + threadIdx.x;
    if (n >= N) return;
    const long long c = inds_coarse[n];
    if (c < 0 || c >= (long long)n_cells) return;
    const float e0 = image[3u * n] - target[3u * n], e1 = image[3u * n + 1u] - target[3u * n + 1u], e2 = image[3u * n + 2u] - target[3u * n + 2u];
    const float err = ((e0 * e0 + e1 * e1) + e2 * e2) / 3.0f;
    row[c] = keep * row[c] + take * err;
}

}  // namespace ngp

using namespace ngp;

extern "C" int ngp_error_map_draw(const float* error_map, uint32_t B, uint32_t res, uint32_t N, uint32_t H, uint32_t W, uint32_t seed,
                                  const uint32_t* seed_dev, int64_t* inds, int64_t* inds_coarse, float* keys_out, uint32_t* n_drawable,
                                  ngp_stream_t stream) {
    NGP_REQUIRE(error_map && inds && inds_coarse, NGP_ERR_INVALID, "error_map_draw: NULL tensor");
    NGP_REQUIRE(res >= 1u && res <= EM_MAX_RES, NGP_ERR_INVALID, "error_map_draw: res must be in [1, %u] (got %u)", EM_MAX_RES, res);
    NGP_REQUIRE(N <= res * res, NGP_ERR_INVALID, "error_map_draw: N = %u cells cannot be drawn without replacement from %u", N, res * res);
    NGP_REQUIRE(H > 0u && W > 0u && (uint64_t)H * W < (1ull << 31), NGP_ERR_INVALID, "error_map_draw: H and W must be positive with H * W < 2^31");
    if (B == 0 || N == 0) return NGP_OK;
    NGP_LAUNCH(k_error_map_draw, dim3(B), dim3(EM_THREADS), 0, as_stream(stream), error_map, res, N, H, W, seed, seed_dev, (long long*)inds,
               (long long*)inds_coarse, keys_out, n_drawable);
    return check_launch("error_map_draw");
}

extern "C" int ngp_error_map_update(float* error_map_row, const int64_t* inds_coarse, const float* image, const float* target, uint32_t N,
                                    uint32_t n_cells, float keep, float take, ngp_stream_t stream) {
    NGP_REQUIRE(error_map_row && inds_coarse && image && target, NGP_ERR_INVALID, "error_map_update: NULL tensor");
    NGP_REQUIRE(N <= 0xffffffffu / 3u, NGP_ERR_INVALID, "error_map_update: 3 N must fit 32 bits");
    if (N == 0 || n_cells == 0) return NGP_OK;
    NGP_LAUNCH(k_error_map_update, dim3(cdiv(N, (uint32_t)EM_UPDATE_THREADS)), dim3(EM_UPDATE_THREADS), 0, as_stream(stream), error_map_row,
               (const long long*)inds_coarse, image, target, N, n_cells, keep, take);
    return check_launch("error_map_update");
}
