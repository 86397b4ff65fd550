// AdamW (torch.optim.AdamW: the optimizer main.py:168-175 builds for --optim AdamW, the default of every shipped launcher) and
// the global gradient clipping of torch.nn.utils.clip_grad_norm_ (main.py:316-333) as multi-tensor launches.
//
// One record table (cc_adamw_item, include/centerclip_hip.h) drives all four kernels: workgroup b finds its tensor by bisection
// over the records' first-block numbers and grid-strides over that tensor with the tensor's own block count.  Every element is
// handled by exactly one lane and the arithmetic is elementwise, so the partition (one launch per tensor or one for all) does
// not change a bit.  The norm is the exception: per-workgroup fp64 partials, then ONE workgroup adds them in a fixed order
// (no atomics: bitwise reproducible from run to run).
//
// Floating point: this file is compiled without contraction (the pragma below), so every multiply and add rounds on its own in
// the order written, as the separate torch ops do; sqrtf and the divisions are IEEE (correctly rounded, the hipcc default).
#include "cc_common.h"

#pragma clang fp contract(off)

namespace {

struct AdamWItem {
    float* p; float* g; float* m; float* v;
    int64_t n;
    int32_t blk0, blocks, scal, reserved;
};
static_assert(sizeof(AdamWItem) == 56, "cc_adamw_item layout");

struct AdamWScalars {
    float decay, b1, omb1, b2, omb2, step_size, bc2_sqrt, eps;
};
static_assert(sizeof(AdamWScalars) == 32, "cc_adamw_scalars layout");

constexpr int AW_THREADS = 256;
constexpr int64_t AW_ELEMS_PER_BLOCK = 8192;      // 8 float4 per lane per workgroup: a small tensor (n <= 8192) is one workgroup
constexpr int32_t AW_MAX_BLOCKS = 1024;           // per tensor; larger tensors grid-stride
constexpr int AW_FINISH_THREADS = 256;

__device__ __forceinline__ int adamw_find(const AdamWItem* __restrict__ items, int count, int blk) {
    int lo = 0, hi = count - 1;                   // last record whose first block <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
// the records' pointers come from memory, so the compiler cannot prove them global: say so (global_* instead of flat_* access)
typedef __attribute__((address_space(1))) float gfloat;
typedef float fv4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) fv4 gfloat4;

// torch.optim.AdamW (_single_tensor_adam, decoupled weight decay), one element; g already clipped by the caller when SCALE
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamWScalars& s) {
    p = p * s.decay;                                               // p *= 1 - lr * wd
    const float d = g - m;                                         // m = b1 m + (1 - b1) g, as torch's lerp_(g, 1 - b1)
    m = s.omb1 < 0.5f ? m + s.omb1 * d : g - d * (1.f - s.omb1);   // computes it (the small term rounds, not 0.9 m)
    v = s.b2 * v + (s.omb2 * g) * g;                               // v = b2 v + (1 - b2) g g
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;             // sqrt(v) / sqrt(1 - b2^t) + eps
    p = p - s.step_size * (m / denom);                             // p -= lr / (1 - b1^t) * m / denom
}

// SKIP (the loss-scaled step, cc_adamw_multi_scaled_f32): *found_inf != 0 -> the whole launch writes nothing (GradScaler.step
// skipping optimizer.step()); coef_dev then holds inv_scale * clip coefficient (cc_grad_scaler_stats_f32)
template <bool SCALE, bool SKIP>
__global__ __launch_bounds__(AW_THREADS) void adamw_multi_kernel(const AdamWItem* __restrict__ items, int count,
                                                                 const AdamWScalars* __restrict__ scal,
                                                                 const float* __restrict__ coef_dev,
                                                                 const float* __restrict__ found_inf) {
    if (SKIP && *found_inf != 0.f) return;                         // (uniform over the grid)
    const int ii = adamw_find(items, count, blockIdx.x);
    const AdamWItem it = items[ii];
    const int64_t bid = (int64_t)blockIdx.x - it.blk0;
    if (bid < 0 || bid >= it.blocks) return;                       // (an inconsistent table: touch nothing)
    const AdamWScalars s = scal[it.scal];
    const float coef = SCALE ? *coef_dev : 1.f;
    gfloat* __restrict__ P = (gfloat*)it.p; gfloat* __restrict__ G = (gfloat*)it.g;
    gfloat* __restrict__ M = (gfloat*)it.m; gfloat* __restrict__ V = (gfloat*)it.v;
    const int64_t n = it.n, stride = (int64_t)it.blocks * AW_THREADS;
    const int64_t n4 = (aligned16(it.p) && aligned16(it.g) && aligned16(it.m) && aligned16(it.v)) ? (n >> 2) : 0;
    for (int64_t i = bid * AW_THREADS + threadIdx.x; i < n4; i += stride) {
        fv4 p = ((gfloat4*)P)[i], g = ((gfloat4*)G)[i];
        fv4 m = ((gfloat4*)M)[i], v = ((gfloat4*)V)[i];
        if (SCALE) {
            g.x = g.x * coef; g.y = g.y * coef; g.z = g.z * coef; g.w = g.w * coef;
            ((gfloat4*)G)[i] = g;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = p[k], mk = m[k], vk = v[k];
            adamw_elem(pk, g[k], mk, vk, s);
            p[k] = pk; m[k] = mk; v[k] = vk;
        }
        ((gfloat4*)P)[i] = p;
        ((gfloat4*)M)[i] = m;
        ((gfloat4*)V)[i] = v;
    }
    for (int64_t i = (n4 << 2) + bid * AW_THREADS + threadIdx.x; i < n; i += stride) {
        float p = P[i], g = G[i], m = M[i], v = V[i];
        if (SCALE) { g = g * coef; G[i] = g; }
        adamw_elem(p, g, m, v, s);
        P[i] = p; M[i] = m; V[i] = v;
    }
}

// the partials as grad_clip_coef_kernel adds them (same order, same bits) for gradients that still carry the loss scale S:
// out[0] = ||g / S|| (fp64 scaling by inv_scale^2 before the root: exact for a power-of-two S, so the float norm is the one
// of the divided gradients), out[1] = inv_scale * min(1, max_norm / (||g / S|| + 1e-6)) (max_norm < 0: inv_scale alone) - the
// ONE multiplier the step applies - and out[2] = found_inf (1.f / 0.f): a sum of fp64 squares of fp32 values cannot overflow,
// so it is non-finite exactly when an element is inf or NaN.
__global__ __launch_bounds__(AW_FINISH_THREADS) void grad_scaler_stats_kernel(const double* __restrict__ partial, int nblocks,
                                                                              const float* __restrict__ inv_scale_dev,
                                                                              float max_norm, float* __restrict__ out) {
    double t = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += AW_FINISH_THREADS) t += partial[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, CC_WAVE);
    __shared__ double red[AW_FINISH_THREADS / CC_WAVE];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sumsq = (red[0] + red[1]) + (red[2] + red[3]);
        const float inv = *inv_scale_dev;
        const float total = (float)sqrt(sumsq * ((double)inv * (double)inv));
        float c = 1.f;
        if (max_norm >= 0.f) {
            c = max_norm / (total + 1e-6f);
            c = c > 1.f ? 1.f : c;
        }
        out[0] = total;
        out[1] = inv * c;
        out[2] = (sumsq - sumsq == 0.0) ? 0.f : 1.f;               // (x - x is 0 for every finite x, NaN for inf and NaN)
    }
}

// GradScaler.update (torch's amp_update_scale kernel), one lane: scale2 = {scale, 1 / scale for the next step},
// ctr = {growth tracker, steps taken, steps skipped}
__global__ void grad_scaler_update_kernel(float* __restrict__ scale2, const float* __restrict__ found_inf,
                                          int32_t* __restrict__ ctr, float growth, float backoff, int32_t interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = scale2[0];
    int32_t tr = ctr[0];
    if (*found_inf != 0.f) {
        s = s * backoff;
        tr = 0;
        ctr[2] = ctr[2] + 1;
    } else {
        ctr[1] = ctr[1] + 1;
        tr = tr + 1;
        if (tr == interval) {
            const float grown = s * growth;
            if (grown - grown == 0.f) s = grown;                   // (torch keeps the scale when growing would overflow)
            tr = 0;
        }
    }
    scale2[0] = s;
    scale2[1] = (float)(1.0 / (double)s);                          // torch: scale.double().reciprocal().float()
    ctr[0] = tr;
}

// sum of squares of every record's gradient: one fp64 partial per workgroup (partial[blockIdx.x])
__global__ __launch_bounds__(AW_THREADS) void grad_sumsq_kernel(const AdamWItem* __restrict__ items, int count,
                                                                double* __restrict__ partial) {
    const int ii = adamw_find(items, count, blockIdx.x);
    const AdamWItem it = items[ii];
    const int64_t bid = (int64_t)blockIdx.x - it.blk0;
    double s = 0.0;
    if (bid >= 0 && bid < it.blocks) {
        const gfloat* __restrict__ G = (const gfloat*)it.g;
        const int64_t n = it.n, stride = (int64_t)it.blocks * AW_THREADS;
        const int64_t n4 = aligned16(it.g) ? (n >> 2) : 0;
        for (int64_t i = bid * AW_THREADS + threadIdx.x; i < n4; i += stride) {
            const fv4 g = ((const gfloat4*)G)[i];
            s += ((double)g.x * g.x + (double)g.y * g.y) + ((double)g.z * g.z + (double)g.w * g.w);
        }
        for (int64_t i = (n4 << 2) + bid * AW_THREADS + threadIdx.x; i < n; i += stride) {
            const double g = (double)G[i];
            s += g * g;
        }
    }
    __shared__ double red[AW_THREADS / CC_WAVE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, CC_WAVE);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the partials in a fixed order (lane t: t, t + 256, ...; then the wave trees, then the four waves) -> ||g|| and the clip
// coefficient of torch.nn.utils.clip_grad_norm_: min(1, max_norm / (||g|| + 1e-6)), in fp32 as torch computes it
__global__ __launch_bounds__(AW_FINISH_THREADS) void grad_clip_coef_kernel(const double* __restrict__ partial, int nblocks,
                                                                           float max_norm, float* __restrict__ out) {
    double t = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += AW_FINISH_THREADS) t += partial[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, CC_WAVE);
    __shared__ double red[AW_FINISH_THREADS / CC_WAVE];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float total = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
        const float c = max_norm / (total + 1e-6f);
        out[0] = total;
        out[1] = c > 1.f ? 1.f : c;                                // (NaN stays NaN, as torch.clamp(max=1) leaves it)
    }
}

__global__ __launch_bounds__(AW_THREADS) void grad_scale_kernel(const AdamWItem* __restrict__ items, int count,
                                                                const float* __restrict__ coef_dev) {
    const int ii = adamw_find(items, count, blockIdx.x);
    const AdamWItem it = items[ii];
    const int64_t bid = (int64_t)blockIdx.x - it.blk0;
    if (bid < 0 || bid >= it.blocks) return;
    const float coef = *coef_dev;
    gfloat* __restrict__ G = (gfloat*)it.g;
    const int64_t n = it.n, stride = (int64_t)it.blocks * AW_THREADS;
    const int64_t n4 = aligned16(it.g) ? (n >> 2) : 0;
    for (int64_t i = bid * AW_THREADS + threadIdx.x; i < n4; i += stride) {
        fv4 g = ((gfloat4*)G)[i];
        g.x = g.x * coef; g.y = g.y * coef; g.z = g.z * coef; g.w = g.w * coef;
        ((gfloat4*)G)[i] = g;
    }
    for (int64_t i = (n4 << 2) + bid * AW_THREADS + threadIdx.x; i < n; i += stride) G[i] = G[i] * coef;
}

}  // namespace

extern "C" {

int32_t cc_adamw_blocks(int64_t n) {
    if (n <= 0) return 0;
    const int64_t b = (n + AW_ELEMS_PER_BLOCK - 1) / AW_ELEMS_PER_BLOCK;
    return (int32_t)(b < AW_MAX_BLOCKS ? b : AW_MAX_BLOCKS);
}

int cc_adamw_multi_f32(const void* items_dev, int32_t count, int32_t total_blocks, const void* scalars_dev, const float* coef_dev,
                       void* stream) {
    if (!items_dev || !scalars_dev || count <= 0 || total_blocks < count) return CC_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AdamWItem* items = static_cast<const AdamWItem*>(items_dev);
    const AdamWScalars* scal = static_cast<const AdamWScalars*>(scalars_dev);
    const float* none = nullptr;
    if (coef_dev)
        hipLaunchKernelGGL((adamw_multi_kernel<true, false>), dim3(total_blocks), dim3(AW_THREADS), 0, st, items, (int)count, scal,
                           coef_dev, none);
    else
        hipLaunchKernelGGL((adamw_multi_kernel<false, false>), dim3(total_blocks), dim3(AW_THREADS), 0, st, items, (int)count, scal,
                           coef_dev, none);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

int cc_adamw_multi_scaled_f32(const void* items_dev, int32_t count, int32_t total_blocks, const void* scalars_dev,
                              const float* mult_dev, const float* found_inf_dev, void* stream) {
    if (!items_dev || !scalars_dev || !mult_dev || !found_inf_dev || count <= 0 || total_blocks < count) return CC_ERR_INVALID;
    hipLaunchKernelGGL((adamw_multi_kernel<true, true>), dim3(total_blocks), dim3(AW_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamWItem*>(items_dev), (int)count, static_cast<const AdamWScalars*>(scalars_dev), mult_dev,
                       found_inf_dev);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

int cc_grad_scaler_stats_f32(const void* ws, int32_t total_blocks, const float* inv_scale_dev, float max_norm, float* out3,
                             void* stream) {
    if (!ws || !inv_scale_dev || !out3 || total_blocks <= 0) return CC_ERR_INVALID;
    hipLaunchKernelGGL(grad_scaler_stats_kernel, dim3(1), dim3(AW_FINISH_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const double*>(ws), (int)total_blocks, inv_scale_dev, max_norm, out3);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

int cc_grad_scaler_update_f32(float* scale2, const float* found_inf_dev, int32_t* counters3, float growth_factor,
                              float backoff_factor, int32_t growth_interval, void* stream) {
    if (!scale2 || !found_inf_dev || !counters3 || growth_interval <= 0) return CC_ERR_INVALID;
    hipLaunchKernelGGL(grad_scaler_update_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), scale2, found_inf_dev,
                       counters3, growth_factor, backoff_factor, growth_interval);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

size_t cc_grad_norm_workspace_bytes(int32_t total_blocks) { return total_blocks > 0 ? (size_t)total_blocks * sizeof(double) : 0; }

int cc_grad_norm_partials_f32(const void* items_dev, int32_t count, int32_t total_blocks, void* ws, size_t ws_bytes, void* stream) {
    if (!items_dev || count <= 0 || total_blocks < count) return CC_ERR_INVALID;
    if (!ws || ws_bytes < cc_grad_norm_workspace_bytes(total_blocks)) return CC_ERR_WORKSPACE;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(total_blocks), dim3(AW_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamWItem*>(items_dev), (int)count, static_cast<double*>(ws));
    CC_LAUNCH_CHECK();
    return CC_OK;
}

int cc_grad_clip_coef_f32(const void* ws, int32_t total_blocks, float max_norm, float* norm_coef, void* stream) {
    if (!ws || !norm_coef || total_blocks <= 0) return CC_ERR_INVALID;
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(AW_FINISH_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const double*>(ws), (int)total_blocks, max_norm, norm_coef);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

int cc_grad_scale_f32(const void* items_dev, int32_t count, int32_t total_blocks, const float* coef_dev, void* stream) {
    if (!items_dev || !coef_dev || count <= 0 || total_blocks < count) return CC_ERR_INVALID;
    hipLaunchKernelGGL(grad_scale_kernel, dim3(total_blocks), dim3(AW_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamWItem*>(items_dev), (int)count, coef_dev);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // extern "C"
