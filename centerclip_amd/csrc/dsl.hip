// CAMoE dual softmax (camoe_dsl; github.com/starmemda/CAMoE, the lines the reference keeps commented out at
// modules/clip4clip.py:430-432 and main.py:526-532) on the evaluation matrix:
//   D = S * softmax(S, dim=0) * len(S)
// S [rows, cols] fp32 row-major with a row stride, texts as rows: the softmax runs over the texts of each video column.
//   m_j = max_i S_ij     s_j = sum_i exp(S_ij - m_j)     D_ij = n_total * S_ij * exp(S_ij - m_j) / s_j
// Three entry points, so that a row-sharded matrix (eval_epoch(shard=True)) can combine its ranks' statistics between them:
// column statistics of a row block, the rescale of s to a common maximum, and the in-place rewrite.
// Summation order (fixed - no atomics, the same bits on every run): the rows are cut into slabs of DSL_SLAB; inside a slab
// wave w of the workgroup walks rows w, w + 4, ... of its 64 columns (a lane = a column: 256-byte coalesced row segments),
// the four waves' (m, s) pairs are merged in wave order, and a second launch merges the slabs' pairs in slab order.
// NaN behaves as in torch.softmax: fmaxf drops a NaN operand, so a flag carries it and the column's m (then s, then D) is NaN.
#include "cc_kernels.h"

namespace {

constexpr int DSL_SLAB = 128;        // rows per workgroup: 32 per wave
constexpr int DSL_APPLY_ROWS = 32;   // rows per workgroup of the rewrite

__global__ __launch_bounds__(256) void dsl_col_partial_kernel(const float* __restrict__ sim, int rows, int cols, int64_t rs,
                                                              float* __restrict__ part) {
    __shared__ float sm[4][64], ss[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * DSL_SLAB, r1 = min(rows, r0 + DSL_SLAB);
    float m = -INFINITY, s = 0.f;
    if (c < cols) {
        bool nan = false;
        for (int r = r0 + wave; r < r1; r += 4) {
            const float x = sim[(int64_t)r * rs + c];
            nan |= (x != x);
            m = fmaxf(m, x);
        }
        if (nan) m = NAN;
        for (int r = r0 + wave; r < r1; r += 4) s += expf(sim[(int64_t)r * rs + c] - m);      // (the slab is in cache)
    }
    sm[wave][lane] = m;
    ss[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < cols) {
        float mm = sm[0][lane];
        bool nan = mm != mm;
#pragma unroll
        for (int w = 1; w < 4; ++w) { nan |= (sm[w][lane] != sm[w][lane]); mm = fmaxf(mm, sm[w][lane]); }
        if (nan) mm = NAN;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) t += cc_dsl_share(ss[w][lane], sm[w][lane], mm);
        float* p = part + ((int64_t)blockIdx.y * cols + c) * 2;
        p[0] = mm;
        p[1] = t;
    }
}

// a thread per column: the slabs' pairs in slab order.  slabs == 0: the neutral element (-inf, 0).
__global__ __launch_bounds__(256) void dsl_col_merge_kernel(const float* __restrict__ part, int slabs, int cols,
                                                            float* __restrict__ m_out, float* __restrict__ s_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float m = -INFINITY;
    bool nan = false;
    for (int k = 0; k < slabs; ++k) {
        const float mk = part[((int64_t)k * cols + c) * 2];
        nan |= (mk != mk);
        m = fmaxf(m, mk);
    }
    if (nan) m = NAN;
    float s = 0.f;
    for (int k = 0; k < slabs; ++k) {
        const float* p = part + ((int64_t)k * cols + c) * 2;
        s += cc_dsl_share(p[1], p[0], m);
    }
    m_out[c] = m;
    s_out[c] = s;
}

__global__ __launch_bounds__(256) void dsl_rescale_kernel(const float* __restrict__ m_local, const float* __restrict__ m_global,
                                                          float* __restrict__ s, int cols) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < cols) s[c] = cc_dsl_share(s[c], m_local[c], m_global[c]);
}

__global__ __launch_bounds__(256) void dsl_apply_kernel(float* __restrict__ sim, int rows, int cols, int64_t rs,
                                                        const float* __restrict__ m, const float* __restrict__ s, float nt) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const float mc = m[c], sc = s[c];
    const int r0 = blockIdx.y * DSL_APPLY_ROWS, r1 = min(rows, r0 + DSL_APPLY_ROWS);
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        float* p = sim + (int64_t)r * rs + c;
        const float x = *p;
        *p = cc_dsl_value(nt, x, mc, sc);
    }
}

inline int dsl_slabs(int rows) { return (rows + DSL_SLAB - 1) / DSL_SLAB; }

}  // namespace

// [slabs][cols] pairs -> m, s [cols] (search.hip's statistics pass ends with the same merge)
int cc_launch_dsl_col_merge(const float* part, int slabs, int cols, float* m, float* s, hipStream_t st) {
    hipLaunchKernelGGL(dsl_col_merge_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, part, slabs, cols, m, s);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

extern "C" {

size_t cc_dsl_col_stats_workspace_bytes(int32_t rows, int32_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)dsl_slabs(rows) * cols * 2 * sizeof(float);
}

int cc_dsl_col_stats_f32(const float* sim, int32_t rows, int32_t cols, int64_t row_stride, float* m, float* s, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!m || !s || rows < 0 || cols <= 0 || (rows > 0 && (!sim || row_stride < cols))) return CC_ERR_INVALID;
    if (dsl_slabs(rows) > 65535) return CC_ERR_UNSUPPORTED;                 // (grid.y; 8.3 M rows)
    if (rows > 0 && (!ws || ws_bytes < cc_dsl_col_stats_workspace_bytes(rows, cols))) return CC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int slabs = dsl_slabs(rows);
    float* part = static_cast<float*>(ws);
    if (slabs > 0) {
        hipLaunchKernelGGL(dsl_col_partial_kernel, dim3((cols + 63) / 64, slabs), dim3(256), 0, st, sim, rows, cols, row_stride,
                           part);
        CC_LAUNCH_CHECK();
    }
    return cc_launch_dsl_col_merge(part, slabs, cols, m, s, st);
}

int cc_dsl_rescale_stats_f32(const float* m_local, const float* m_global, float* s, int32_t cols, void* stream) {
    if (!m_local || !m_global || !s || cols <= 0) return CC_ERR_INVALID;
    hipLaunchKernelGGL(dsl_rescale_kernel, dim3((cols + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), m_local,
                       m_global, s, cols);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

int cc_dsl_apply_f32(float* sim, int32_t rows, int32_t cols, int64_t row_stride, const float* m, const float* s,
                     int32_t n_total, void* stream) {
    if (!m || !s || rows < 0 || cols <= 0 || n_total < 0 || (rows > 0 && (!sim || row_stride < cols))) return CC_ERR_INVALID;
    if (rows == 0) return CC_OK;
    if ((rows + DSL_APPLY_ROWS - 1) / DSL_APPLY_ROWS > 65535) return CC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dsl_apply_kernel, dim3((cols + 255) / 256, (rows + DSL_APPLY_ROWS - 1) / DSL_APPLY_ROWS), dim3(256), 0,
                       static_cast<hipStream_t>(stream), sim, rows, cols, row_stride, m, s, (float)n_total);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // extern "C"
