// Fused optimizer + loss-scaling step for the instant-ngp parameter set.
//
// The reference trains with torch.optim.Adam + torch.cuda.amp.GradScaler (main_nerf.py:132, nerf/utils.py:393,557-560).  On the
// 12.24 M-entry hash table that is, per iteration: zero a fp16 gradient table, scatter into it, cast it to fp32 (autograd), sweep
// it for non-finite values, run Adam (read p, g, m, v; write p, m, v and the unscaled g), and cast the fp32 table back to fp16 for
// the next forward -- six table-sized passes.  Here the gradient stays in the fp16 buffer the scatter kernel wrote:
//   k_check_finite : one read of the fp16 gradients -> found_inf flag
//   k_adam         : g (fp16, still loss-scaled) * inv_scale -> Adam moments and fp32 master weights, plus the fp16 shadow copy the
//                    next forward reads, and the gradient buffer is zeroed in the same sweep (nothing else has to touch it)
//   k_update_scale : GradScaler's dynamic loss scale (grow after `growth_interval` clean steps, back off on overflow) and the
//                    Adam step counter, on device -- the whole step is free of host synchronisation and graph-capturable.
// Update rule = PyTorch's Adam (amsgrad = False, weight_decay = 0, maximize = False), restated from its documented formula:
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
// A step with a non-finite gradient anywhere is skipped as a whole (moments, weights and t untouched), as GradScaler.step does; with more
// than 8 tensors the caller runs the phases separately (check every chunk, then update every chunk, then commit once) so that "as a
// whole" holds across chunks.
// Optional, in the same sweep: the exponential moving average of the parameters the reference Trainer keeps with torch_ema
// (nerf/utils.py:388-391,760-761,891-892): shadow -= (1 - decay) * (shadow - param), computed on the UPDATED parameter -- one extra
// fp32 read-modify-write stream instead of a separate pass over every parameter.
#include "common.h"
#include <math.h>
#include <stdlib.h>

namespace ngp {

constexpr int OPT_THREADS = 256;
constexpr int OPT_MAX_TENSORS = 8;

struct OptTensors {
    int count;
    uint64_t n[OPT_MAX_TENSORS];
    float* p[OPT_MAX_TENSORS];
    float* m[OPT_MAX_TENSORS];
    float* v[OPT_MAX_TENSORS];
    void* g[OPT_MAX_TENSORS];       // fp16 or fp32 gradient (g_is_half)
    half_t* p16[OPT_MAX_TENSORS];   // optional fp16 shadow of the weights
    int g_is_half[OPT_MAX_TENSORS];
    float lr[OPT_MAX_TENSORS];
    float* ema[OPT_MAX_TENSORS];    // optional EMA shadow (fp32), updated when ema_omd > 0
};

typedef float float1_t __attribute__((ext_vector_type(1)));
typedef _Float16 half1_t __attribute__((ext_vector_type(1)));

// what a standing step applies to one tensor (or to the table prefix): the unscale factor and adam_element's constants
struct AdamRule {
    float inv_scale, beta1, beta2, eps, step_size, bc2_sqrt;
};
__device__ __forceinline__ AdamRule adam_rule(const AdamConsts& ac, float beta1, float beta2, float eps, float lr) {
    return AdamRule{ac.inv_scale, beta1, beta2, eps, lr * ac.lr_mult / ac.bc1, ac.bc2_sqrt};
}

// torch_ema's rule: the average moves towards the parameter by omd = 1 - decay (float or float2_t)
template <typename F>
__device__ __forceinline__ F ema_toward(F e, F p, float omd) {
    return e - omd * (e - p);
}

// THE update of a register-resident group: loss-scaled gradients `x` (fp16 or fp32 lanes) -> unscale -> adam_element on the moments and master
// weights lane by lane; returns the fp16 shadow.  Loads and stores belong to the caller.  The four-wide group of k_adam's wide path and of
// the prefix sweep of k_adam_small_commit is adam_group<half4_t>(half4_t, float4_t& ...); k_adam's pair loop uses it two wide, adam_element_at one.
template <typename H, typename G, typename F>
__device__ __forceinline__ H adam_group(G x, F& pm, F& pv, F& pp, const AdamRule& r) {
    H ph;
#pragma unroll
    for (int c = 0; c < (int)(sizeof(F) / sizeof(float)); c++) {
        float m_ = pm[c], v_ = pv[c], p_ = pp[c];   // (a vector element does not bind to a reference)
        adam_element((float)x[c] * r.inv_scale, m_, v_, p_, r.beta1, r.beta2, r.eps, r.step_size, r.bc2_sqrt);
        pm[c] = m_; pv[c] = v_; pp[c] = p_;
        ph[c] = (half_t)p_;
    }
    return ph;
}

// THE element form (k_adam's odd tail and the small tensors of k_adam_small_commit): element i of one tensor, `g` = its loss-scaled gradient
// (the caller loaded it, and zeroed it where it has to).  A standing step updates moments and master weights and stores the fp16 shadow
// (p16, optional); the average (ema, optional) then moves towards the parameter -- the UPDATED one, or on a skipped step the unchanged
// one, as torch_ema's update() would.  (k_adam's pair loop is this form two wide, written out there: see its comment.)
__device__ __forceinline__ void adam_element_at(float g, bool skip, const AdamRule& r, float* __restrict__ p, float* __restrict__ m,
                                                float* __restrict__ v, half_t* __restrict__ p16, float* __restrict__ ema, float ema_omd, uint64_t i) {
    if (!skip) {
        float1_t pm = {m[i]}, pv = {v[i]}, pp = {p[i]};
        const half1_t ph = adam_group<half1_t>(float1_t{g}, pm, pv, pp, r);
        m[i] = pm.x; v[i] = pv.x; p[i] = pp.x;
        if (p16) p16[i] = ph.x;
    }
    if (ema) ema[i] = ema_toward(ema[i], p[i], ema_omd);
}

// (the eight words of `state`: OptState in common.h, documented in include/ngp_hip.h at ngp_optim_adam_step)
__global__ __launch_bounds__(OPT_THREADS) void k_check_finite(OptTensors ts, float* __restrict__ state) {
    bool bad = false;
    for (int k = 0; k < ts.count; k++) {
        const uint64_t n = ts.n[k];
        if (ts.g_is_half[k] & 1) {
            const half8_t* g = reinterpret_cast<const half8_t*>(ts.g[k]);
            const uint64_t n8 = n / 8;
            for (uint64_t i = (uint64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n8; i += (uint64_t)gridDim.x * OPT_THREADS) {
                const half8_t x = g[i];
#pragma unroll
                for (int j = 0; j < 8; j++) bad = bad || !__builtin_isfinite((float)x[j]);
            }
            const half_t* gt = reinterpret_cast<const half_t*>(ts.g[k]);
            for (uint64_t i = n8 * 8 + (uint64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * OPT_THREADS)
                bad = bad || !__builtin_isfinite((float)gt[i]);
        } else {
            const float* g = reinterpret_cast<const float*>(ts.g[k]);
            for (uint64_t i = (uint64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * OPT_THREADS)
                bad = bad || !__builtin_isfinite(g[i]);
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) state[OPT_FOUND_INF] = 1.0f;  // benign race: every writer stores the same value
}

// (Folding k_update_scale into this kernel behind a last-workgroup ticket was measured and dropped: the kernel took 74 instead of 62 us --
// presumably the 2048 workgroups, which finish together, queueing on ONE device-scope atomic -- for 4 us of launch saved.)
__global__ __launch_bounds__(OPT_THREADS) void k_adam(OptTensors ts, const float* __restrict__ state, float beta1, float beta2, float eps,
                                                      float grad_mult, float ema_omd) {
    // A loss scale that has underflowed (a long run of overflowing steps halves it to a denormal, then to 0): GradScaler unscales BEFORE it
    // checks, so its 1 / scale = inf turns every gradient into inf or NaN and the step is skipped -- for good, the run is dead, but the weights
    // stay what they were.  Checking the SCALED gradient (the producers do) would let a zero gradient through and 0 * inf = NaN into every
    // parameter (seen in a 200 000-step soak of the bench workload, tools/soak_train.py): the unusable scale is an overflow of its own
    // (adam_consts, common.h).
    const AdamConsts ac = adam_consts(state, beta1, beta2, grad_mult);
    const bool skip = ac.skip;
    for (int k = 0; k < ts.count; k++) {
        const uint64_t n = ts.n[k];
        const AdamRule r = adam_rule(ac, beta1, beta2, eps, ts.lr[k]);
        float* __restrict__ p = ts.p[k];
        float* __restrict__ m = ts.m[k];
        float* __restrict__ v = ts.v[k];
        half_t* __restrict__ p16 = ts.p16[k];
        float* __restrict__ ema = ema_omd > 0.0f ? ts.ema[k] : nullptr;
        const bool gh = (ts.g_is_half[k] & 1) != 0;
        // bit 1: the gradient's producer OVERWRITES the whole buffer every step (grid backward in overwrite mode): nothing to zero here,
        // and a skipped step has nothing to do for this tensor at all (unless it keeps an average)
        const bool keep = (ts.g_is_half[k] & 2) != 0;
        if (keep && skip && !ema) continue;
        half_t* g16 = reinterpret_cast<half_t*>(ts.g[k]);
        float* g32 = reinterpret_cast<float*>(ts.g[k]);
        // Fast path of the training configuration (fp16 gradient + fp16 shadow, no EMA, length a multiple of 4, 16-byte aligned streams):
        // four elements per lane and iteration, 16-byte accesses (8-byte global accesses run at 0.5-0.7x the 16-byte rate on this chip).
        // Same arithmetic per element as the general loop below; -7 us per iteration in a same-box A/B.
        const bool wide = gh && p16 && !ema && (n & 3u) == 0 &&
                          ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15u) == 0 &&
                          ((reinterpret_cast<uintptr_t>(g16) | reinterpret_cast<uintptr_t>(p16)) & 7u) == 0;
        if (wide) {
            const uint64_t n4 = n / 4;
            for (uint64_t i = (uint64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * OPT_THREADS) {
                const half4_t x = reinterpret_cast<half4_t*>(g16)[i];
                if (!keep) reinterpret_cast<half4_t*>(g16)[i] = half4_t{(half_t)0.0f, (half_t)0.0f, (half_t)0.0f, (half_t)0.0f};
                if (skip) continue;
                float4_t pm = __builtin_nontemporal_load(reinterpret_cast<float4_t*>(m) + i), pv = __builtin_nontemporal_load(reinterpret_cast<float4_t*>(v) + i),
                         pp = __builtin_nontemporal_load(reinterpret_cast<float4_t*>(p) + i);
                const half4_t ph = adam_group<half4_t>(x, pm, pv, pp, r);
                __builtin_nontemporal_store(pm, reinterpret_cast<float4_t*>(m) + i);
                __builtin_nontemporal_store(pv, reinterpret_cast<float4_t*>(v) + i);
                __builtin_nontemporal_store(pp, reinterpret_cast<float4_t*>(p) + i);
                reinterpret_cast<half4_t*>(p16)[i] = ph;
            }
            continue;
        }
        // two elements per lane and iteration (all our tensors have an even length; a trailing odd element is handled below)
        const uint64_t n2 = n / 2;
        for (uint64_t i = (uint64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * OPT_THREADS) {
            float2_t g;
            if (gh) {
                const half2_t x = reinterpret_cast<half2_t*>(g16)[i];
                g = float2_t{(float)x.x, (float)x.y};
                if (!keep) reinterpret_cast<half2_t*>(g16)[i] = half2_t{(half_t)0.0f, (half_t)0.0f};
            } else {
                g = reinterpret_cast<float2_t*>(g32)[i];
                if (!keep) reinterpret_cast<float2_t*>(g32)[i] = float2_t{0.0f, 0.0f};
            }
            // adam_element_at's form two wide, written out: behind a shared width-templated routine this kernel keeps its registers but gains
            // a load and a store in the tail below (EXPERIMENTS.md)
            if (skip) {
                if (ema) reinterpret_cast<float2_t*>(ema)[i] = ema_toward(reinterpret_cast<float2_t*>(ema)[i], reinterpret_cast<float2_t*>(p)[i], ema_omd);
                continue;
            }
            // the moment / master-weight streams pass exactly once per step: non-temporal, they do not displace the L2 (measured with the
            // activation stores of the network forward: -11 us per iteration on one box)
            float2_t pm = __builtin_nontemporal_load(reinterpret_cast<float2_t*>(m) + i), pv = __builtin_nontemporal_load(reinterpret_cast<float2_t*>(v) + i),
                     pp = __builtin_nontemporal_load(reinterpret_cast<float2_t*>(p) + i);
            const half2_t ph = adam_group<half2_t>(g, pm, pv, pp, r);
            __builtin_nontemporal_store(pm, reinterpret_cast<float2_t*>(m) + i);
            __builtin_nontemporal_store(pv, reinterpret_cast<float2_t*>(v) + i);
            __builtin_nontemporal_store(pp, reinterpret_cast<float2_t*>(p) + i);
            if (p16) reinterpret_cast<half2_t*>(p16)[i] = ph;
            if (ema) reinterpret_cast<float2_t*>(ema)[i] = ema_toward(reinterpret_cast<float2_t*>(ema)[i], pp, ema_omd);
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const uint64_t i = n - 1;
            const float g = gh ? (float)g16[i] : g32[i];
            if (!keep) { if (gh) g16[i] = (half_t)0.0f; else g32[i] = 0.0f; }
            adam_element_at(g, skip, r, p, m, v, p16, ema, ema_omd, i);
        }
    }
}

// torch.amp.GradScaler.update (_amp_update_scale_): found_inf -> scale *= backoff, tracker = 0; else tracker += 1 and, when it reaches
// growth_interval, scale *= growth (only if the result is finite) and tracker = 0.  Also commits the Adam step count.
__device__ __forceinline__ void update_scale(float* state, float growth, float backoff, float growth_interval, bool flip_parity = false) {
    // (all eight words are read in ONE request and the changed ones written back: written as read-modify-writes of single words this was a
    // chain of six dependent memory round trips -- 4 us of a 4 us kernel)
    constexpr int HI = 4;   // `b` holds the words from HI on
    float4_t a = *reinterpret_cast<const float4_t*>(state), b = *reinterpret_cast<const float4_t*>(state + HI);
    float scale = a[OPT_SCALE], tracker = a[OPT_GROWTH_TRACKER], t = a[OPT_STEP_COUNT], parity = b[OPT_TABLE_PARITY - HI], dead = b[OPT_SCALE_DEAD - HI];
    const bool scale_dead = !__builtin_isfinite(1.0f / scale);
    if (a[OPT_FOUND_INF] != 0.0f || scale_dead) {   // (an underflowed scale counts as an overflow: see k_adam)
        // GradScaler has no lower bound either: a scale that has underflowed stays 0 and every later step is skipped -- the run is dead,
        // silently.  The OPT_SCALE_DEAD word is the signal (sticky): optim.NGPAdam.scale_is_dead() / bench.py report it.
        if (scale_dead) dead = 1.0f;
        scale *= backoff;
        tracker = 0.0f;
    } else {
        t += 1.0f;
        const float tr = tracker + 1.0f;
        if (tr >= growth_interval) {
            const float grown = scale * growth;
            if (__builtin_isfinite(grown)) scale = grown;
            tracker = 0.0f;
        } else {
            tracker = tr;
        }
        // the step stands: the buffer set the grid backward wrote speculatively (ngp_table_adam_t) becomes the current one.  A skipped
        // step leaves the parity -- and with it the table, its moments and its fp16 shadow -- exactly as they were.
        if (flip_parity) parity = parity != 0.0f ? 0.0f : 1.0f;
    }
    a[OPT_SCALE] = scale; a[OPT_GROWTH_TRACKER] = tracker; a[OPT_FOUND_INF] = 0.0f; a[OPT_STEP_COUNT] = t;
    *reinterpret_cast<float4_t*>(state) = a;
    state[OPT_TABLE_PARITY] = parity;
    state[OPT_SCALE_DEAD] = dead;
}
__global__ void k_update_scale(float* __restrict__ state, float growth, float backoff, float growth_interval, int flip_parity) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    update_scale(state, growth, backoff, growth_interval, flip_parity != 0);
}

// The rest of a step whose TABLE was updated inside the grid backward (ngp_table_adam_t): Adam on what is left -- the dense-level prefix of
// the double-buffered table (contiguous here; the accumulate's round-robin bins could only have reached it 8 bytes at a stride of 1 KiB)
// and the few small tensors (the two MLPs' weights: 18 k parameters, in place) -- and the commit, in ONE launch of a few workgroups: every
// workgroup has read the scalars before it draws its ticket (the OPT_TICKET word); the last one commits behind it.  ~8 us where k_adam (60 us over
// the table) + k_update_scale used to be.  Same arithmetic per element as k_adam.
constexpr int OPT_SMALL_THREADS = 1024;
__global__ __launch_bounds__(OPT_SMALL_THREADS) void k_adam_small_commit(OptTensors ts, float* __restrict__ state, float beta1, float beta2, float eps,
                                                                        float grad_mult, float growth, float backoff, float growth_interval,
                                                                        int flip_parity, TableAdam ta, const half_t* __restrict__ tgrad,
                                                                        uint64_t tprefix, uint32_t prefix_blocks) {
    const AdamConsts ac = adam_consts(state, beta1, beta2, grad_mult);
    // two kinds of workgroups -- the first `prefix_blocks` sweep the table prefix, the others the small tensors -- so that the two dependent
    // load -> store chains run side by side instead of one behind the other in every lane
    const bool prefix_role = blockIdx.x < prefix_blocks;
    const uint32_t role_blocks = prefix_role ? prefix_blocks : gridDim.x - prefix_blocks;
    const uint64_t gtid = (uint64_t)(prefix_role ? blockIdx.x : blockIdx.x - prefix_blocks) * OPT_SMALL_THREADS + threadIdx.x;
    const uint64_t gstride = (uint64_t)role_blocks * OPT_SMALL_THREADS;
    if (prefix_role && tprefix && !ac.skip) {   // (a skipped step writes nothing: the current set stays what it is, the other one is never read)
        const uint32_t src = state[OPT_TABLE_PARITY] != 0.0f ? 1u : 0u, dst = src ^ 1u;
        const AdamRule r = adam_rule(ac, ta.beta1, ta.beta2, ta.eps, ta.lr);   // (the table brings its own constants in `ta`)
        const float4_t* __restrict__ p_in = reinterpret_cast<const float4_t*>(ta.p[src]);
        const float4_t* __restrict__ m_in = reinterpret_cast<const float4_t*>(ta.m[src]);
        const float4_t* __restrict__ v_in = reinterpret_cast<const float4_t*>(ta.v[src]);
        float4_t* __restrict__ p_out = reinterpret_cast<float4_t*>(ta.p[dst]);
        float4_t* __restrict__ m_out = reinterpret_cast<float4_t*>(ta.m[dst]);
        float4_t* __restrict__ v_out = reinterpret_cast<float4_t*>(ta.v[dst]);
        half4_t* __restrict__ h_out = reinterpret_cast<half4_t*>(ta.p16[dst]);
        const half4_t* __restrict__ g4 = reinterpret_cast<const half4_t*>(tgrad);
        // two independent 4-element groups per lane and trip (all eight loads in flight before the first dependent instruction)
        const uint64_t n4 = tprefix / 4;
        for (uint64_t i = gtid; i < n4; i += 2 * gstride) {
            const uint64_t j = i + gstride;
            const bool two = j < n4;
            const uint64_t jj = two ? j : i;
            const half4_t x0 = g4[i], x1 = g4[jj];
            float4_t pm0 = m_in[i], pv0 = v_in[i], pp0 = p_in[i];
            float4_t pm1 = m_in[jj], pv1 = v_in[jj], pp1 = p_in[jj];
            const half4_t ph0 = adam_group<half4_t>(x0, pm0, pv0, pp0, r), ph1 = adam_group<half4_t>(x1, pm1, pv1, pp1, r);
            m_out[i] = pm0; v_out[i] = pv0; p_out[i] = pp0; h_out[i] = ph0;
            if (two) { m_out[j] = pm1; v_out[j] = pv1; p_out[j] = pp1; h_out[j] = ph1; }
        }
    }
    for (int k = 0; !prefix_role && k < ts.count; k++) {
        const uint64_t n = ts.n[k];
        const AdamRule r = adam_rule(ac, beta1, beta2, eps, ts.lr[k]);
        const bool gh = (ts.g_is_half[k] & 1) != 0, keep = (ts.g_is_half[k] & 2) != 0;
        half_t* g16 = reinterpret_cast<half_t*>(ts.g[k]);
        float* g32 = reinterpret_cast<float*>(ts.g[k]);
        for (uint64_t i = gtid; i < n; i += gstride) {
            const float g = gh ? (float)g16[i] : g32[i];
            if (!keep) { if (gh) g16[i] = (half_t)0.0f; else g32[i] = 0.0f; }
            adam_element_at(g, ac.skip, r, ts.p[k], ts.m[k], ts.v[k], ts.p16[k], nullptr, 0.0f, i);
        }
    }
    // every lane of this workgroup has read state[] (adam_consts, parity) before the workgroup draws its ticket; the last ticket commits
    // (No __threadfence() around the ticket: on this chip it writes back the XCD's whole dirty L2 -- full of the accumulate's Adam output at
    // this point -- once per workgroup, and nothing here needs it: what must be ordered are this workgroup's READS of state[], and a
    // load whose value has been consumed -- every one of them steers a branch above -- cannot be served later; what the last workgroup
    // writes is for the NEXT launch.  The ticket itself is a device-scope atomic.)
    __syncthreads();
    if (threadIdx.x == 0) {
        const float old = __hip_atomic_fetch_add(&state[OPT_TICKET], 1.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == (float)(gridDim.x - 1u)) {
            update_scale(state, growth, backoff, growth_interval, flip_parity != 0);
            __hip_atomic_store(&state[OPT_TICKET], 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Data-parallel sharded update, the "skipped as a whole" verdict WITHOUT a collective of its own: a rank whose local gradient is not finite
// (the OPT_FOUND_INF word, set by the producers or by the CHECK phase) writes NaN into the first element of EVERY shard of its flat fp16
// gradient before the reduce-scatter; the average of a shard that any rank poisoned is NaN on its owner, so after the exchange every rank
// reads the global verdict off the first element of ITS OWN shard (k_shard_verdict) -- the 4-byte all-reduce(MAX) that used to sit on the
// critical path next to the reduce-scatter is gone.  (The poisoned step is skipped, so the clobbered gradient elements are never used.)
__global__ void k_poison_shards(half_t* __restrict__ grad, uint32_t shards, uint64_t payload, const float* __restrict__ state) {
    if (state[OPT_FOUND_INF] == 0.0f) return;
    for (uint32_t r = threadIdx.x; r < shards; r += blockDim.x) grad[(uint64_t)r * payload] = (half_t)__builtin_nanf("");
}
// ... and takes the poison out of the flat buffer again (the exchange has consumed it): with a producer that OVERWRITES its gradients and an
// optimizer that therefore does not zero the flat buffer, a poisoned element that lies in padding would otherwise stay NaN forever
__global__ void k_shard_verdict(const half_t* __restrict__ shard, float* __restrict__ state, half_t* __restrict__ flat, uint32_t shards,
                                uint64_t payload) {
    if (threadIdx.x == 0 && !__builtin_isfinite((float)shard[0])) state[OPT_FOUND_INF] = 1.0f;
    if (flat)
        for (uint32_t r = threadIdx.x; r < shards; r += blockDim.x)
            if (!__builtin_isfinite((float)flat[(uint64_t)r * payload])) flat[(uint64_t)r * payload] = (half_t)0.0f;
}

// torch_ema's update() on its own (the Trainer calls it once per epoch, not per step): shadow -= omd * (shadow - param)
__global__ __launch_bounds__(OPT_THREADS) void k_ema(OptTensors ts, float omd) {
    for (int k = 0; k < ts.count; k++) {
        const uint64_t n = ts.n[k];
        const float* __restrict__ p = ts.p[k];
        float* __restrict__ e = ts.ema[k];
        for (uint64_t i = (uint64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * OPT_THREADS) e[i] = ema_toward(e[i], p[i], omd);
    }
}

}  // namespace ngp

using namespace ngp;

static uint32_t opt_blocks(uint64_t total) {
    uint32_t blocks = (uint32_t)cdiv64(total / 2 + 1, OPT_THREADS * 4);  // ~8 elements per lane
// grid cap: 768 workgroups = 3 per CU.  Swept in round 5 (EXPERIMENTS.md): 256 / 384 / 512 / 768 / 1024 / 2048 workgroups -> step 0.4419 /
// 0.4335 / 0.4255 / 0.4245 / 0.4291 / 0.4297 ms, k_adam itself 63.3 us at 512-1024 against 66.0 at 2048: fewer, longer-lived workgroups stream as
// fast and leave room for the lookahead march that starts beside this kernel
#ifndef NGP_ADAM_MAX_BLOCKS
#define NGP_ADAM_MAX_BLOCKS 768u
#endif
    if (blocks > NGP_ADAM_MAX_BLOCKS) blocks = NGP_ADAM_MAX_BLOCKS;
    if (blocks < 1u) blocks = 1u;
    return blocks;
}

// The C arrays of an entry as the kernels take them, for `entry` (its name in the messages).  `need` says which arrays the entry requires
// (checked as arrays, then per tensor); what it does not require stays NULL / 0 in `ts`, params_fp16 and ema are optional where given.
enum : unsigned { OPT_GRADS = 1u, OPT_PARAMS = 2u, OPT_MOMENTS = 4u, OPT_EMA = 8u };   // grads + grad_is_half, params, exp_avg + exp_avg_sq + lr, ema
static int fill_opt_tensors(OptTensors& ts, uint64_t& total, const char* entry, unsigned need, int count, const uint64_t* n, float* const* params,
                            float* const* exp_avg, float* const* exp_avg_sq, void* const* grads, void* const* params_fp16, const int* grad_is_half,
                            const float* lr, float* const* ema, float ema_omd) {
    const bool gr = need & OPT_GRADS, pa = need & OPT_PARAMS, mo = need & OPT_MOMENTS, em = need & OPT_EMA;
    NGP_REQUIRE(count == 0 || (n && (!gr || (grads && grad_is_half)) && (!pa || params) && (!mo || (exp_avg && exp_avg_sq && lr)) && (!em || ema)),
                NGP_ERR_INVALID, "%s: NULL argument", entry);
    NGP_REQUIRE(!(ema_omd > 0.0f) || ema, NGP_ERR_INVALID, "%s: EMA decay given without shadow tensors", entry);
    ts = {};
    ts.count = count;
    total = 0;
    for (int k = 0; k < count; k++) {
        NGP_REQUIRE((!gr || grads[k]) && (!pa || params[k]) && (!mo || (exp_avg[k] && exp_avg_sq[k])) && (!em || ema[k]), NGP_ERR_INVALID,
                    "%s: NULL tensor %d", entry, k);
        ts.n[k] = n[k];
        ts.p[k] = pa ? params[k] : nullptr;   // (a CHECK-only call needs the gradients alone)
        ts.m[k] = mo ? exp_avg[k] : nullptr;
        ts.v[k] = mo ? exp_avg_sq[k] : nullptr;
        ts.g[k] = gr ? grads[k] : nullptr;
        ts.p16[k] = params_fp16 ? reinterpret_cast<half_t*>(params_fp16[k]) : nullptr;
        ts.g_is_half[k] = gr ? grad_is_half[k] : 0;
        ts.lr[k] = mo ? lr[k] : 0.0f;
        ts.ema[k] = ema ? ema[k] : nullptr;
        total += n[k];
    }
    return NGP_OK;
}

static int check_state(const char* entry, const float* state) {
    NGP_REQUIRE(state, NGP_ERR_INVALID, "%s: NULL state", entry);
    NGP_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15u) == 0, NGP_ERR_INVALID, "%s: state (8 floats) must be 16-byte aligned", entry);
    return NGP_OK;
}

extern "C" int ngp_optim_adam_step_ex(int count, const uint64_t* n, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                                      void* const* grads, void* const* params_fp16, const int* grad_is_half, const float* lr, float beta1,
                                      float beta2, float eps, float grad_mult, float growth_factor, float backoff_factor, float growth_interval,
                                      float* state, float* const* ema, float ema_one_minus_decay, uint32_t phases, ngp_stream_t stream) {
    int rc = check_state("optim_adam_step", state);
    if (rc) return rc;
    NGP_REQUIRE((phases & ~15u) == 0 && (phases & 7u) != 0, NGP_ERR_INVALID, "optim_adam_step: phases must be a non-empty subset of CHECK|UPDATE|COMMIT (+FLIP)");
    NGP_REQUIRE(!(phases & NGP_OPT_PHASE_FLIP) || (phases & NGP_OPT_PHASE_COMMIT), NGP_ERR_INVALID, "optim_adam_step: FLIP rides in the COMMIT phase");
    hipStream_t st = as_stream(stream);
    if (phases & (NGP_OPT_PHASE_CHECK | NGP_OPT_PHASE_UPDATE)) {
        NGP_REQUIRE(count >= 1 && count <= OPT_MAX_TENSORS, NGP_ERR_INVALID, "optim_adam_step: between 1 and %d tensors per call (got %d)",
                    OPT_MAX_TENSORS, count);
        OptTensors ts;
        uint64_t total;
        rc = fill_opt_tensors(ts, total, "optim_adam_step", OPT_GRADS | ((phases & NGP_OPT_PHASE_UPDATE) ? OPT_PARAMS | OPT_MOMENTS : 0u), count, n, params,
                              exp_avg, exp_avg_sq, grads, params_fp16, grad_is_half, lr, ema, ema_one_minus_decay);
        if (rc) return rc;
        const uint32_t blocks = opt_blocks(total);
        if (phases & NGP_OPT_PHASE_CHECK) {
            NGP_LAUNCH(k_check_finite, dim3(blocks), dim3(OPT_THREADS), 0, st, ts, state);
            rc = check_launch("optim_adam_step(check)");
            if (rc) return rc;
        }
        if (phases & NGP_OPT_PHASE_UPDATE) {
            NGP_LAUNCH(k_adam, dim3(blocks), dim3(OPT_THREADS), 0, st, ts, (const float*)state, beta1, beta2, eps, grad_mult,
                               ema_one_minus_decay > 0.0f ? ema_one_minus_decay : 0.0f);
            rc = check_launch("optim_adam_step(adam)");
            if (rc) return rc;
        }
    }
    if (phases & NGP_OPT_PHASE_COMMIT) {
        NGP_LAUNCH(k_update_scale, dim3(1), dim3(64), 0, st, state, growth_factor, backoff_factor, growth_interval,
                           (phases & NGP_OPT_PHASE_FLIP) ? 1 : 0);
        return check_launch("optim_adam_step(scale)");
    }
    return NGP_OK;
}

extern "C" int ngp_optim_adam_step(int count, const uint64_t* n, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                                   void* const* grads, void* const* params_fp16, const int* grad_is_half, const float* lr, float beta1,
                                   float beta2, float eps, float grad_mult, float growth_factor, float backoff_factor, float growth_interval,
                                   float* state, ngp_stream_t stream) {
    const uint32_t phases = NGP_OPT_PHASE_CHECK | NGP_OPT_PHASE_UPDATE | (growth_interval < 0.0f ? 0u : NGP_OPT_PHASE_COMMIT);
    return ngp_optim_adam_step_ex(count, n, params, exp_avg, exp_avg_sq, grads, params_fp16, grad_is_half, lr, beta1, beta2, eps, grad_mult,
                                  growth_factor, backoff_factor, growth_interval, state, nullptr, 0.0f, phases, stream);
}

extern "C" int ngp_optim_adam_small_commit(int count, const uint64_t* n, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                                           void* const* grads, void* const* params_fp16, const int* grad_is_half, const float* lr, float beta1,
                                           float beta2, float eps, float grad_mult, float growth_factor, float backoff_factor,
                                           float growth_interval, float* state, int flip_parity, const ngp_table_adam_t* table,
                                           const void* table_grad_fp16, uint64_t table_prefix_params, ngp_stream_t stream) {
    int rc = check_state("optim_adam_small_commit", state);
    if (rc) return rc;
    NGP_REQUIRE(count >= 0 && count <= OPT_MAX_TENSORS, NGP_ERR_INVALID, "optim_adam_small_commit: at most %d tensors per call (got %d)", OPT_MAX_TENSORS,
                count);
    OptTensors ts;
    uint64_t total;
    rc = fill_opt_tensors(ts, total, "optim_adam_small_commit", OPT_GRADS | OPT_PARAMS | OPT_MOMENTS, count, n, params, exp_avg, exp_avg_sq, grads,
                          params_fp16, grad_is_half, lr, nullptr, 0.0f);
    if (rc) return rc;
    TableAdam ta = {};
    if (table_prefix_params) {
        NGP_REQUIRE(table && table_grad_fp16 && table->state == state, NGP_ERR_INVALID,
                    "optim_adam_small_commit: a table prefix needs the table's buffer sets (on the same state) and its stored fp16 gradient");
        NGP_REQUIRE((table_prefix_params & 3u) == 0, NGP_ERR_INVALID, "optim_adam_small_commit: table_prefix_params must be a multiple of 4");
        const int null_set = table_adam_from(ta, *table);
        NGP_REQUIRE(null_set < 0, NGP_ERR_INVALID, "optim_adam_small_commit: NULL buffer in table set %d", null_set);
        total += table_prefix_params;
    }
    // a few workgroups: meant for what is left when the table is updated elsewhere (the 12 M-entry table itself belongs in ngp_optim_adam_step_ex)
    NGP_REQUIRE(total <= (1u << 22), NGP_ERR_INVALID, "optim_adam_small_commit: %llu parameters -- this entry serves small tensors (<= 4 M); use "
                "ngp_optim_adam_step_ex", (unsigned long long)total);
    // (every workgroup ends with one atomic on the ticket word: ~100 of them keep that queue short)
    // workgroups of two kinds (see the kernel): one trip per lane where the cap allows it -- eight prefix parameters, one small-tensor element
    uint32_t prefix_blocks = (uint32_t)cdiv64(table_prefix_params, (uint64_t)OPT_SMALL_THREADS * 8);
    if (prefix_blocks > 192u) prefix_blocks = 192u;
    uint32_t small_blocks = (uint32_t)cdiv64(total - table_prefix_params, (uint64_t)OPT_SMALL_THREADS);
    small_blocks = small_blocks < 1u ? 1u : (small_blocks > 32u ? 32u : small_blocks);   // (>= 1: somebody has to draw the last ticket)
    NGP_LAUNCH(k_adam_small_commit, dim3(prefix_blocks + small_blocks), dim3(OPT_SMALL_THREADS), 0, as_stream(stream), ts, state, beta1, beta2, eps,
                       grad_mult, growth_factor, backoff_factor, growth_interval, flip_parity, ta, reinterpret_cast<const half_t*>(table_grad_fp16),
                       table_prefix_params, prefix_blocks);
    return check_launch("optim_adam_small_commit");
}

extern "C" int ngp_optim_poison_shards(void* flat_grad_fp16, uint32_t shards, uint64_t payload, const float* state, ngp_stream_t stream) {
    NGP_REQUIRE(flat_grad_fp16 && state && shards >= 1 && payload >= 1, NGP_ERR_INVALID, "optim_poison_shards: NULL / empty argument");
    NGP_LAUNCH(k_poison_shards, dim3(1), dim3(64), 0, as_stream(stream), reinterpret_cast<half_t*>(flat_grad_fp16), shards, payload, state);
    return check_launch("optim_poison_shards");
}

extern "C" int ngp_optim_shard_verdict(const void* shard_grad_fp16, float* state, void* flat_grad_fp16, uint32_t shards, uint64_t payload,
                                       ngp_stream_t stream) {
    NGP_REQUIRE(shard_grad_fp16 && state, NGP_ERR_INVALID, "optim_shard_verdict: NULL argument");
    NGP_REQUIRE(!flat_grad_fp16 || (shards >= 1 && payload >= 1), NGP_ERR_INVALID, "optim_shard_verdict: empty shard layout");
    NGP_LAUNCH(k_shard_verdict, dim3(1), dim3(64), 0, as_stream(stream), reinterpret_cast<const half_t*>(shard_grad_fp16), state,
                       reinterpret_cast<half_t*>(flat_grad_fp16), shards, payload);
    return check_launch("optim_shard_verdict");
}

extern "C" int ngp_optim_ema_update(int count, const uint64_t* n, float* const* params, float* const* ema, float one_minus_decay,
                                    ngp_stream_t stream) {
    NGP_REQUIRE(count >= 1 && count <= OPT_MAX_TENSORS, NGP_ERR_INVALID, "optim_ema_update: between 1 and %d tensors per call (got %d)",
                OPT_MAX_TENSORS, count);
    OptTensors ts;
    uint64_t total;
    const int rc = fill_opt_tensors(ts, total, "optim_ema_update", OPT_PARAMS | OPT_EMA, count, n, params, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    ema, 0.0f);
    if (rc) return rc;
    NGP_LAUNCH(k_ema, dim3(opt_blocks(total)), dim3(OPT_THREADS), 0, as_stream(stream), ts, one_minus_decay);
    return check_launch("optim_ema_update");
}
