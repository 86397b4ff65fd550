// BertAdam (utils/optimization.py:100-170, the optimizer main.py:161-167 builds) as multi-tensor launches: per-tensor gradient
// clipping (clip_grad_norm_(p, max_grad_norm): g *= max / (||g|| + 1e-6) when that factor is < 1 - the gradient tensor is
// rescaled in place as the reference does), moments, update = m / (sqrt(v) + e) [+ weight_decay * p], p -= lr_scheduled * update.
// No bias correction - this is the BERT variant.
//
// One record table (cc_bertadam_item, include/centerclip_hip.h) drives both kernels: the workgroups of every tensor's sum of
// squares (per-workgroup fp64 partials - double atomics would make the sum order dependent), then the workgroups of every tensor's
// step, which add their tensor's partials in block order first.  A workgroup finds its tensor by bisection over the records'
// first-block numbers and sees its tensor's own block count and block id, so a tensor's bits do not depend on what else the
// table holds.  A tensor of n <= CC_BERTADAM_MULTI_MAX_N elements (biases, LayerNorm parameters: two thirds of a CLIP model's
// tensors) has no norm workgroups (norm_blocks == 0): its ONE step workgroup forms the sum of squares itself.
//
// Floating point: the compiler's default contraction (a multiply and the add behind it may fuse) - this file is NOT in
// build.py's STRICT set, and a pragma or flag that changed that would change the bits of every trained model.
#include "cc_common.h"

namespace {

constexpr int BA_BLOCKS = 512;                    // norm workgroups per tensor, at most
constexpr int BA_STEP_BLOCKS = 8192;              // step workgroups per tensor, at most; larger tensors grid-stride
constexpr int64_t BA_ELEMS_PER_BLOCK = 1024;

struct BertAdamItem {
    float* p; float* g; float* m; float* v;
    const float* lr_dev;
    int64_t n;
    float lr, wd;
    int32_t norm_blk0, norm_blocks, step_blk0, step_blocks;
};
static_assert(sizeof(BertAdamItem) == 72, "cc_bertadam_item layout");

// Records with norm_blocks == 0 share their norm_blk0 with the record behind them.  "The last record whose first block <= blk"
// settles that tie for the record that owns the block: the zero-width records of a run come before the owner, whose first
// block is still <= blk, and the record after the owner starts at least one block later.  (Zero-width records at the table's
// end share total_norm_blocks, which no workgroup of the grid reaches.)  Every record has step_blocks >= 1: no ties there.
template <bool STEP>
__device__ __forceinline__ int bertadam_find(const BertAdamItem* __restrict__ items, int count, int blk) {
    int lo = 0, hi = count - 1;                                   // last record whose first block <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((STEP ? items[mid].step_blk0 : items[mid].norm_blk0) <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// SC (the *_scaled_f32 entry point, a step under a device-side loss scale): every gradient is first multiplied by *mult_dev
// (inv_scale, times the global clip coefficient: cc_grad_scaler_stats_f32) and rounded to fp32 - the value an unscaling pass
// would have stored - and *found_inf != 0 ends every workgroup before it writes anything (GradScaler.step skipping the step).
template <bool SC>
__global__ __launch_bounds__(256) void bertadam_multi_norm_kernel(const BertAdamItem* __restrict__ items, int count,
                                                                   double* __restrict__ partial,
                                                                   const float* __restrict__ mult_dev,
                                                                   const float* __restrict__ found_inf) {
    if (SC && *found_inf != 0.f) return;
    const float mult = SC ? *mult_dev : 1.f;
    const int ii = bertadam_find<false>(items, count, blockIdx.x);
    const float* __restrict__ g = items[ii].g;
    const int64_t n = items[ii].n;
    const int64_t bid = (int)blockIdx.x - items[ii].norm_blk0, nblk = items[ii].norm_blocks;
    double s = 0.0;
    if (bid >= 0 && bid < nblk) {                                 // (an inconsistent table: a partial of zero)
        const int64_t n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? (n >> 2) : 0;   // (gradients may be views of a flat bucket)
        for (int64_t i = bid * 256 + threadIdx.x; i < n4; i += nblk * 256) {
            float4 v = reinterpret_cast<const float4*>(g)[i];
            if (SC) { v.x = v.x * mult; v.y = v.y * mult; v.z = v.z * mult; v.w = v.w * mult; }
            s += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
        }
        for (int64_t i = (n4 << 2) + bid * 256 + threadIdx.x; i < n; i += nblk * 256) {
            const double v = (double)(SC ? g[i] * mult : g[i]);
            s += v * v;
        }
    }
    __shared__ double red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// a one-workgroup tensor: norm and step by the same workgroup
template <bool SC>
__device__ __forceinline__ void bertadam_small_body(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int n, float lr, float b1, float b2, float eps, float wd,
                                                    float max_norm, float mult) {
    float coef = 1.f;
    if (max_norm > 0.f) {
        __shared__ double red[4];
        double s = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) { const double x = (double)(SC ? g[i] * mult : g[i]); s += x * x; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        const float c = max_norm / ((float)sqrt((red[0] + red[1]) + (red[2] + red[3])) + 1e-6f);
        coef = c < 1.f ? c : 1.f;
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        const float gi = (SC ? g[i] * mult : g[i]) * coef;
        const float mi = m[i] * b1 + (1.f - b1) * gi;
        const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
        float upd = mi / (sqrtf(vi) + eps);
        const float pi = p[i];
        if (wd > 0.f) upd += wd * pi;
        g[i] = gi; m[i] = mi; v[i] = vi;
        p[i] = pi - lr * upd;
    }
}

template <bool SC>
__global__ __launch_bounds__(256) void bertadam_multi_step_kernel(const BertAdamItem* __restrict__ items, int count,
                                                                   const double* __restrict__ partial, float b1, float b2, float eps,
                                                                   float max_norm, const float* __restrict__ mult_dev,
                                                                   const float* __restrict__ found_inf) {
    if (SC && *found_inf != 0.f) return;
    const float mult = SC ? *mult_dev : 1.f;
    const int ii = bertadam_find<true>(items, count, blockIdx.x);
    const BertAdamItem it = items[ii];
    const int64_t bid = (int)blockIdx.x - it.step_blk0;
    if (bid < 0 || bid >= it.step_blocks) return;                 // (an inconsistent table: touch nothing)
    const float lr = it.lr_dev ? *it.lr_dev : it.lr;              // (a captured step: the schedule's value arrives through memory)
    if (it.norm_blocks == 0) {                                    // (uniform over the workgroup)
        bertadam_small_body<SC>(it.p, it.g, it.m, it.v, (int)it.n, lr, b1, b2, eps, it.wd, max_norm, mult);
        return;
    }
    float coef = 1.f;
    if (max_norm > 0.f) {
        // the tensor's block partials, summed by the first wave in a fixed order (lane l takes l, l + 64, ...; then the wave tree)
        __shared__ double tot_s;
        if (threadIdx.x < 64) {
            double t = 0.0;
            for (int b = threadIdx.x; b < it.norm_blocks; b += 64) t += partial[it.norm_blk0 + b];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
            if (threadIdx.x == 0) tot_s = t;
        }
        __syncthreads();
        const float c = max_norm / ((float)sqrt(tot_s) + 1e-6f);
        coef = c < 1.f ? c : 1.f;
    }
    float* __restrict__ p = it.p; float* __restrict__ g = it.g; float* __restrict__ m = it.m; float* __restrict__ v = it.v;
    for (int64_t i = bid * 256 + threadIdx.x; i < it.n; i += (int64_t)it.step_blocks * 256) {
        const float gi = (SC ? g[i] * mult : g[i]) * coef;
        const float mi = m[i] * b1 + (1.f - b1) * gi;
        const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
        float upd = mi / (sqrtf(vi) + eps);
        const float pi = p[i];
        if (it.wd > 0.f) upd += it.wd * pi;
        g[i] = gi; m[i] = mi; v[i] = vi;
        p[i] = pi - lr * upd;
    }
}

template <bool SC>
int bertadam_multi_launch(const void* items_dev, int32_t count, int32_t total_norm_blocks, int32_t total_step_blocks, float b1,
                          float b2, float e, float max_grad_norm, void* ws, size_t ws_bytes, const float* mult_dev,
                          const float* found_inf_dev, void* stream) {
    if (!items_dev || count <= 0 || total_norm_blocks < 0 || total_step_blocks < count) return CC_ERR_INVALID;
    if (SC && (!mult_dev || !found_inf_dev)) return CC_ERR_INVALID;
    if (total_norm_blocks > 0 && (!ws || ws_bytes < (size_t)total_norm_blocks * sizeof(double))) return CC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BertAdamItem* items = static_cast<const BertAdamItem*>(items_dev);
    double* partial = static_cast<double*>(ws);
    if (max_grad_norm > 0.f && total_norm_blocks > 0)
        hipLaunchKernelGGL(bertadam_multi_norm_kernel<SC>, dim3(total_norm_blocks), dim3(256), 0, st, items, (int)count, partial,
                           mult_dev, found_inf_dev);
    hipLaunchKernelGGL(bertadam_multi_step_kernel<SC>, dim3(total_step_blocks), dim3(256), 0, st, items, (int)count, partial, b1, b2,
                       e, max_grad_norm, mult_dev, found_inf_dev);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // namespace

extern "C" {

int32_t cc_bertadam_norm_blocks(int64_t n) {
    if (n <= CC_BERTADAM_MULTI_MAX_N) return 0;
    const int64_t b = (n + BA_ELEMS_PER_BLOCK - 1) / BA_ELEMS_PER_BLOCK;
    return (int32_t)(b < BA_BLOCKS ? b : BA_BLOCKS);
}

int32_t cc_bertadam_step_blocks(int64_t n) {
    if (n <= 0) return 0;
    if (n <= CC_BERTADAM_MULTI_MAX_N) return 1;
    const int64_t b = (n + BA_ELEMS_PER_BLOCK - 1) / BA_ELEMS_PER_BLOCK;
    return (int32_t)(b < BA_STEP_BLOCKS ? b : BA_STEP_BLOCKS);
}

int cc_bertadam_multi_f32(const void* items_dev, int32_t count, int32_t total_norm_blocks, int32_t total_step_blocks, float b1,
                          float b2, float e, float max_grad_norm, void* ws, size_t ws_bytes, void* stream) {
    return bertadam_multi_launch<false>(items_dev, count, total_norm_blocks, total_step_blocks, b1, b2, e, max_grad_norm, ws,
                                        ws_bytes, nullptr, nullptr, stream);
}

int cc_bertadam_multi_scaled_f32(const void* items_dev, int32_t count, int32_t total_norm_blocks, int32_t total_step_blocks,
                                 float b1, float b2, float e, float max_grad_norm, void* ws, size_t ws_bytes,
                                 const float* mult_dev, const float* found_inf_dev, void* stream) {
    return bertadam_multi_launch<true>(items_dev, count, total_norm_blocks, total_step_blocks, b1, b2, e, max_grad_norm, ws, ws_bytes,
                                       mult_dev, found_inf_dev, stream);
}

}  // extern "C"
