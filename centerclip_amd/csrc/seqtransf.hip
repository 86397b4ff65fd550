// sim_header 'seqTransf' (modules/clip4clip.py:335-349): the similarity head that runs a small transformer over the
// per-segment video features before the meanP pooling.
//   key-masked attention    softmax(q k^T / 8 + (1 - mask[key]) * -1e6) v per 64-wide head, forward and backward; the
//                           additive mask is the same for every query and head (module_cross.py:102-104)
//   cc_seqtransf_forward_f32  position rows + the N blocks (LayerNorm / GEMM kernels of the encoders, the attention
//                           below) + the outer residual, one enqueue, no host synchronisation
// The head runs on 48 to 768 rows.  The attention kernels are plain fp32 loops over LDS - one workgroup per (sequence, head),
// every reduction in a fixed order (identical bits on every run).  Measured: 0.18 ms per head call at
// B = 16, T = 3 and 0.23 ms at B = 64, T = 12, about the cost of its ~20 launches; 0.60 ms at B = 8, T = 64, where these
// loops (work ∝ T^2 per sequence and head) set the time.
//
// Masking.  A key with mask 0 gets weight exactly 0: in fp32 exp(s - 1e6 - max) underflows to 0 whenever one key of the
// sequence is live, so the kernels never read a masked key's k or v.  When every key of a sequence is masked the -1e6 shifts
// all scores alike and the formula's exact value is the unmasked softmax, which is what the kernels compute then.
#include "cc_kernels.h"

namespace {

constexpr int KM_D = 64;
constexpr int KM_MAX_L = 80;               // >= 77, the length of the reference's frame position table
constexpr int KM_S = KM_D + 1;             // LDS row stride (floats) of q / k / v / dO

__host__ __device__ inline size_t km_fwd_smem(int L) { return (size_t)(3 * L * KM_S + L * (L + 1) + L) * 4; }
__host__ __device__ inline size_t km_bwd_smem(int L) { return (size_t)(4 * L * KM_S + 2 * L * (L + 1) + L) * 4; }

// live[j] = 1 for a key that takes part; all keys when none is live (see the header).  Returns after a barrier.
__device__ inline void km_live_keys(const int64_t* __restrict__ mask, int64_t row_stride, int64_t col_stride, int seq, int L,
                                    int* live) {
    __shared__ int any_live;
    if (threadIdx.x == 0) any_live = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        const int v = mask[(int64_t)seq * row_stride + (int64_t)j * col_stride] != 0;
        live[j] = v;
        if (v) atomicOr(&any_live, 1);
    }
    __syncthreads();
    if (!any_live)
        for (int j = threadIdx.x; j < L; j += blockDim.x) live[j] = 1;
    __syncthreads();
}

// q (and, for live keys, k and v) of head `head` of sequence `seq` -> LDS fp32; rows of masked keys are not read
__device__ inline void km_stage(const _Float16* __restrict__ qkv, int64_t row0, int L, int W, int head, const int* live,
                                float* Q, float* K, float* V) {
    for (int idx = threadIdx.x; idx < L * KM_D; idx += blockDim.x) {
        const int t = idx / KM_D, d = idx - t * KM_D;
        const _Float16* r = qkv + (row0 + t) * 3 * W + head * KM_D + d;
        Q[t * KM_S + d] = (float)r[0];
        K[t * KM_S + d] = live[t] ? (float)r[W] : 0.f;
        V[t * KM_S + d] = live[t] ? (float)r[2 * W] : 0.f;
    }
}

// P[i][j] = softmax_j(Q_i K_j / 8) over the live keys, exactly 0 elsewhere; one thread per query row, keys in index order
__device__ inline void km_probs(const float* Q, const float* K, const int* live, int L, float* P) {
    const int PS = L + 1;
    for (int idx = threadIdx.x; idx < L * L; idx += blockDim.x) {
        const int i = idx / L, j = idx - i * L;
        float s = 0.f;
        if (live[j])
            for (int d = 0; d < KM_D; ++d) s = fmaf(Q[i * KM_S + d], K[j * KM_S + d], s);
        P[i * PS + j] = s * 0.125f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        float mx = -INFINITY;
        for (int j = 0; j < L; ++j)
            if (live[j]) mx = fmaxf(mx, P[i * PS + j]);
        float sum = 0.f;
        for (int j = 0; j < L; ++j) {
            const float e = live[j] ? expf(P[i * PS + j] - mx) : 0.f;
            P[i * PS + j] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
        for (int j = 0; j < L; ++j) P[i * PS + j] *= inv;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void key_masked_attention_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ out,
                                                                   const int64_t* __restrict__ mask, int64_t mrow, int64_t mcol,
                                                                   int L, int heads, int W) {
    extern __shared__ __attribute__((aligned(16))) float km_smem[];
    float* Q = km_smem;
    float* K = Q + L * KM_S;
    float* V = K + L * KM_S;
    float* P = V + L * KM_S;
    int* live = reinterpret_cast<int*>(P + L * (L + 1));
    const int seq = blockIdx.x / heads, head = blockIdx.x - seq * heads;
    const int64_t row0 = (int64_t)seq * L;
    km_live_keys(mask, mrow, mcol, seq, L, live);
    km_stage(qkv, row0, L, W, head, live, Q, K, V);
    __syncthreads();
    km_probs(Q, K, live, L, P);
    // O_i[d] = sum_j P_ij V_j[d], keys in index order (masked keys add exact zeros and are skipped)
    for (int idx = threadIdx.x; idx < L * KM_D; idx += blockDim.x) {
        const int i = idx / KM_D, d = idx - i * KM_D;
        float o = 0.f;
        for (int j = 0; j < L; ++j)
            if (live[j]) o = fmaf(P[i * (L + 1) + j], V[j * KM_S + d], o);
        out[(row0 + i) * W + head * KM_D + d] = (_Float16)o;
    }
}

// the largest magnitude a workgroup wrote, into *bits (non-negative floats order as their bit patterns; as backward.hip)
__device__ inline void km_publish_absmax(float m, unsigned* __restrict__ bits) {
    __shared__ float wmax[4];
    m = cc_wave_max(m);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned mine = __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
        if (mine > __atomic_load_n(bits, __ATOMIC_RELAXED)) atomicMax(bits, mine);
    }
}

// dV_j = sum_i P_ij dO_i, dP_ij = dO_i V_j, dS_ij = P_ij (dP_ij - sum_k P_ik dP_ik), dQ_i = sum_j dS_ij K_j / 8,
// dK_j = sum_i dS_ij Q_i / 8.  Masked keys: P and dS are exactly 0, so their dK / dV rows are exactly 0.
__global__ __launch_bounds__(256) void key_masked_attention_backward_kernel(const _Float16* __restrict__ qkv,
                                                                            const int64_t* __restrict__ mask, int64_t mrow,
                                                                            int64_t mcol, const float* __restrict__ d_out,
                                                                            float* __restrict__ d_qkv, int L, int heads, int W,
                                                                            unsigned* __restrict__ amax_bits) {
    extern __shared__ __attribute__((aligned(16))) float km_smem[];
    float* Q = km_smem;
    float* K = Q + L * KM_S;
    float* V = K + L * KM_S;
    float* dO = V + L * KM_S;
    float* P = dO + L * KM_S;
    float* dS = P + L * (L + 1);
    int* live = reinterpret_cast<int*>(dS + L * (L + 1));
    const int PS = L + 1;
    const int seq = blockIdx.x / heads, head = blockIdx.x - seq * heads;
    const int64_t row0 = (int64_t)seq * L;
    km_live_keys(mask, mrow, mcol, seq, L, live);
    km_stage(qkv, row0, L, W, head, live, Q, K, V);
    for (int idx = threadIdx.x; idx < L * KM_D; idx += blockDim.x) {
        const int t = idx / KM_D, d = idx - t * KM_D;
        dO[t * KM_S + d] = d_out[(row0 + t) * W + head * KM_D + d];
    }
    __syncthreads();
    km_probs(Q, K, live, L, P);
    for (int idx = threadIdx.x; idx < L * L; idx += blockDim.x) {
        const int i = idx / L, j = idx - i * L;
        float s = 0.f;
        if (live[j])
            for (int d = 0; d < KM_D; ++d) s = fmaf(dO[i * KM_S + d], V[j * KM_S + d], s);
        dS[i * PS + j] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        float dot = 0.f;
        for (int j = 0; j < L; ++j) dot = fmaf(dS[i * PS + j], P[i * PS + j], dot);
        for (int j = 0; j < L; ++j) dS[i * PS + j] = live[j] ? P[i * PS + j] * (dS[i * PS + j] - dot) : 0.f;
    }
    __syncthreads();
    float am = 0.f;
    for (int idx = threadIdx.x; idx < L * KM_D; idx += blockDim.x) {
        const int t = idx / KM_D, d = idx - t * KM_D;
        float dq = 0.f, dk = 0.f, dv = 0.f;
        for (int j = 0; j < L; ++j)
            if (live[j]) dq = fmaf(dS[t * PS + j], K[j * KM_S + d], dq);
        if (live[t])
            for (int i = 0; i < L; ++i) {
                dk = fmaf(dS[i * PS + t], Q[i * KM_S + d], dk);
                dv = fmaf(P[i * PS + t], dO[i * KM_S + d], dv);
            }
        dq *= 0.125f;
        dk *= 0.125f;
        float* o = d_qkv + (row0 + t) * 3 * W + head * KM_D + d;
        o[0] = dq;
        o[W] = dk;
        o[2 * W] = dv;
        am = fmaxf(am, fmaxf(fabsf(dq), fmaxf(fabsf(dk), fabsf(dv))));
    }
    if (amax_bits) km_publish_absmax(am, amax_bits);
}

// x[r] = feat[r] + pos[r % T]  (the frame position rows)
__global__ __launch_bounds__(256) void add_position_rows_kernel(const float* __restrict__ feat, const float* __restrict__ pos,
                                                               float* __restrict__ x, int rows, int T, int D) {
    const int64_t n = (int64_t)rows * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / D), c = (int)(i - (int64_t)r * D);
        x[i] = feat[i] + pos[(int64_t)(r % T) * D + c];
    }
}

// out = x + feat  (the residual around the whole transformer, clip4clip.py:349)
__global__ __launch_bounds__(256) void add_rows_kernel(const float* __restrict__ x, const float* __restrict__ feat,
                                                      float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = x[i] + feat[i];
}

int km_check(const void* qkv, const int64_t* mask, int nseq, int L, int heads, int W) {
    if (!qkv || !mask || nseq <= 0 || L <= 0 || heads <= 0 || W != heads * KM_D) return CC_ERR_INVALID;
    if (L > KM_MAX_L) return CC_ERR_UNSUPPORTED;
    return CC_OK;
}

int km_launch_forward(const _Float16* qkv, _Float16* out, int nseq, int L, int heads, int W, const int64_t* mask, int64_t mrow,
                      int64_t mcol, hipStream_t st) {
    const int rc = cc_allow_dynamic_lds(reinterpret_cast<const void*>(key_masked_attention_kernel), km_fwd_smem(KM_MAX_L));
    if (rc != CC_OK) return rc;
    hipLaunchKernelGGL(key_masked_attention_kernel, dim3(nseq * heads), dim3(256), km_fwd_smem(L), st, qkv, out, mask, mrow, mcol,
                       L, heads, W);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

constexpr size_t km_align(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

extern "C" {

int cc_key_masked_attention_f16(const void* qkv_f16, void* out_f16, int32_t nseq, int32_t L, int32_t heads, int32_t W,
                                const int64_t* mask, int64_t mask_row_stride, int64_t mask_col_stride, void* stream) {
    int rc = km_check(qkv_f16, mask, nseq, L, heads, W);
    if (rc != CC_OK) return rc;
    if (!out_f16) return CC_ERR_INVALID;
    return km_launch_forward(static_cast<const _Float16*>(qkv_f16), static_cast<_Float16*>(out_f16), nseq, L, heads, W, mask,
                             mask_row_stride, mask_col_stride, static_cast<hipStream_t>(stream));
}

int cc_key_masked_attention_backward_f16(const void* qkv_f16, const int64_t* mask, int64_t mask_row_stride,
                                         int64_t mask_col_stride, const float* d_out, float* d_qkv, int32_t nseq, int32_t L,
                                         int32_t heads, int32_t W, float* out_amax, void* stream) {
    int rc = km_check(qkv_f16, mask, nseq, L, heads, W);
    if (rc != CC_OK) return rc;
    if (!d_out || !d_qkv) return CC_ERR_INVALID;
    rc = cc_allow_dynamic_lds(reinterpret_cast<const void*>(key_masked_attention_backward_kernel), km_bwd_smem(KM_MAX_L));
    if (rc != CC_OK) return rc;
    hipLaunchKernelGGL(key_masked_attention_backward_kernel, dim3(nseq * heads), dim3(256), km_bwd_smem(L),
                       static_cast<hipStream_t>(stream), static_cast<const _Float16*>(qkv_f16), mask, mask_row_stride,
                       mask_col_stride, d_out, d_qkv, L, heads, W, reinterpret_cast<unsigned*>(out_amax));
    CC_LAUNCH_CHECK();
    return CC_OK;
}

size_t cc_seqtransf_workspace_bytes(int32_t B, int32_t T, int32_t D) {
    if (B <= 0 || T <= 0 || D <= 0) return 0;
    const size_t M = (size_t)B * T;
    return km_align(M * D * 4) + km_align(M * D * 2) + km_align(M * 3 * D * 2) + km_align(M * D * 2) + km_align(M * 4 * D * 2);
}

int cc_seqtransf_forward_f32(const float* feat, const int64_t* mask, int64_t mask_row_stride, int64_t mask_col_stride,
                             const float* pos, const cc_block_weights* blocks, int32_t layers, int32_t B, int32_t T, int32_t D,
                             int32_t heads, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!feat || !mask || !pos || !out || (layers > 0 && !blocks) || layers < 0 || B <= 0 || T <= 0) return CC_ERR_INVALID;
    if (heads <= 0 || D != heads * KM_D || D > 1024) return CC_ERR_INVALID;
    if (T > KM_MAX_L) return CC_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < cc_seqtransf_workspace_bytes(B, T, D)) return CC_ERR_WORKSPACE;
    for (int l = 0; l < layers; ++l) {
        const cc_block_weights& b = blocks[l];
        if (!b.ln_1_weight || !b.ln_1_bias || !b.in_proj_weight_f16 || !b.in_proj_bias || !b.out_proj_weight_f16 ||
            !b.out_proj_bias || !b.ln_2_weight || !b.ln_2_bias || !b.c_fc_weight_f16 || !b.c_fc_bias || !b.c_proj_weight_f16 ||
            !b.c_proj_bias)
            return CC_ERR_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int M = B * T;
    unsigned char* p = static_cast<unsigned char*>(ws);
    float* x = reinterpret_cast<float*>(p);                  p += km_align((size_t)M * D * 4);
    _Float16* n16 = reinterpret_cast<_Float16*>(p);          p += km_align((size_t)M * D * 2);
    _Float16* qkv = reinterpret_cast<_Float16*>(p);          p += km_align((size_t)M * 3 * D * 2);
    _Float16* att = reinterpret_cast<_Float16*>(p);          p += km_align((size_t)M * D * 2);
    _Float16* u = reinterpret_cast<_Float16*>(p);
    const int64_t n = (int64_t)M * D;
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(add_position_rows_kernel, dim3(grid), dim3(256), 0, st, feat, pos, x, M, T, D);
    CC_LAUNCH_CHECK();
    for (int l = 0; l < layers; ++l) {
        const cc_block_weights& b = blocks[l];
        // x = x + out_proj(attention(in_proj(ln_1(x)), key mask))
        LnArgs ln{};
        ln.in = x; ln.in_stride = D; ln.gamma = b.ln_1_weight; ln.beta = b.ln_1_bias; ln.out = n16; ln.out_stride = D;
        ln.rows = M; ln.W = D;
        int rc = cc_launch_layernorm2(ln, nullptr, 1e-5f, 1, st);
        if (rc != CC_OK) return rc;
        GemmArgs g{};
        g.A = n16; g.W = static_cast<const _Float16*>(b.in_proj_weight_f16); g.bias = b.in_proj_bias; g.C = qkv;
        g.M = M; g.N = 3 * D; g.K = D; g.ldc = 3 * D;
        if ((rc = cc_gemm_dispatch(g, EPI_F16, 0, st)) != CC_OK) return rc;
        if ((rc = km_launch_forward(qkv, att, B, T, heads, D, mask, mask_row_stride, mask_col_stride, st)) != CC_OK) return rc;
        g = GemmArgs{};
        g.A = att; g.W = static_cast<const _Float16*>(b.out_proj_weight_f16); g.bias = b.out_proj_bias; g.C = x;
        g.M = M; g.N = D; g.K = D; g.ldc = D;
        if ((rc = cc_gemm_dispatch(g, EPI_F32_RESID, 0, st)) != CC_OK) return rc;
        // x = x + c_proj(QuickGELU(c_fc(ln_2(x))))
        ln.gamma = b.ln_2_weight; ln.beta = b.ln_2_bias;
        if ((rc = cc_launch_layernorm2(ln, nullptr, 1e-5f, 1, st)) != CC_OK) return rc;
        g = GemmArgs{};
        g.A = n16; g.W = static_cast<const _Float16*>(b.c_fc_weight_f16); g.bias = b.c_fc_bias; g.C = u;
        g.M = M; g.N = 4 * D; g.K = D; g.ldc = 4 * D;
        if ((rc = cc_gemm_dispatch(g, EPI_F16_GELU, 0, st)) != CC_OK) return rc;
        g = GemmArgs{};
        g.A = u; g.W = static_cast<const _Float16*>(b.c_proj_weight_f16); g.bias = b.c_proj_bias; g.C = x;
        g.M = M; g.N = D; g.K = 4 * D; g.ldc = D;
        if ((rc = cc_gemm_dispatch(g, EPI_F32_RESID, 0, st)) != CC_OK) return rc;
    }
    hipLaunchKernelGGL(add_rows_kernel, dim3(grid), dim3(256), 0, st, x, feat, out, n);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // extern "C"
