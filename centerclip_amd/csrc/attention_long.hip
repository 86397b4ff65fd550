// Attention for sequences longer than the resident-K kernel of transformer.hip holds (256 < L <= 640: ViT-L/14 at 224 px
// has 257 tokens per frame, at 336 px 577).  K and V^T of 577 keys would fill the CU's whole LDS, so the keys are STREAMED:
//   one workgroup (4 waves) per (sequence, head, 64 queries); wave w owns queries 16w .. 16w + 15 of the tile
//   per 64-key tile:  K   -> LDS [64 keys][64] fp16, 128-byte rows, 16-byte chunks XOR-swizzled by (row & 7)       8 KB
//                     V^T -> LDS [64 d][64 keys], 16-byte chunks XOR-swizzled by (d ^ d >> 3) & 7                   8 KB
//                     S^T = K Q^T (MFMA, K fragment as A operand: a lane owns 4 consecutive keys of one query)
//                     online softmax in fp32: running row maximum m and row sum l, O rescaled by exp(m_old - m_new)
//                     P = exp(S - m) (fp16, unnormalised, <= 1) -> per-wave LDS strip [16][72]                 4 x 2.25 KB
//                     O^T += V^T P^T (MFMA)
//   the next tile's K / V rows are fetched into registers while the current tile is multiplied (one tile in LDS)
//   epilogue: O / l -> fp16, 4 consecutive d per lane
// 25 KB of LDS and 256 threads per workgroup: six workgroups (24 waves) fit a CU - the 577-token frames of one clip
// (12 frames x 16 heads x 10 query tiles = 1,920 workgroups) cover the chip more than once.
// Causal form: key tiles behind the query tile are skipped.  seq_len / seq_off as in AttArgs (L is the upper bound that
// sizes the grid; query tiles behind a sequence's own length exit at once).
#include "cc_kernels.h"

typedef _Float16 alh8 __attribute__((ext_vector_type(8)));
typedef _Float16 alh4 __attribute__((ext_vector_type(4)));
typedef float alf4 __attribute__((ext_vector_type(4)));

#define ATL_D 64
#define ATL_KT 64            // keys per streamed tile
#define ATL_QT 64            // queries per workgroup
#define ATL_PS 72            // row stride of a P strip in halfs

__global__ __launch_bounds__(256) void attention_long_kernel(AttArgs at, int qtiles, float scale) {
    __shared__ __attribute__((aligned(16))) _Float16 Ks[ATL_KT * ATL_D];
    __shared__ __attribute__((aligned(16))) _Float16 Vt[ATL_D * ATL_KT];
    __shared__ __attribute__((aligned(16))) _Float16 Ps[4 * 16 * ATL_PS];
    const int heads = at.heads, W = at.W;
    const bool CAUSAL = at.causal != 0;
    const int qt = (int)blockIdx.x % qtiles, sh = (int)blockIdx.x / qtiles;
    const int seq = sh / heads, head = sh - seq * heads;
    const int L = at.seq_len ? at.seq_len[seq] : at.L;
    if (qt * ATL_QT >= L) return;                              // workgroup-uniform: no barrier is skipped by a part of it
    const int64_t seq_row0 = at.seq_off ? at.seq_off[seq] : (int64_t)seq * at.seq_rows;
    const int64_t ld = 3 * (int64_t)W * at.tok_rows;           // qkv stride between consecutive tokens of a sequence
    const _Float16* base = at.qkv + seq_row0 * 3 * W + head * ATL_D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int nk = (L + ATL_KT - 1) / ATL_KT;
    const int ntiles = CAUSAL ? min(nk, qt + 1) : nk;

    const int q = qt * ATL_QT + wave * 16 + l15;               // this lane's query row (as B-operand column)
    const int qc = min(q, L - 1);
    alh8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const alh8*>(base + (int64_t)qc * ld + (ks * 4 + lg) * 8);

    // staging: 64 rows x 8 chunks of 16 bytes = 512 items, two per thread (rows tid / 8 and 32 + tid / 8)
    const alh8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const int sc = tid & 7;
    alh8 kreg[2], vreg[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int r = u * 32 + (tid >> 3);
        kreg[u] = vreg[u] = zero;
        if (r < L) {
            kreg[u] = *reinterpret_cast<const alh8*>(base + (int64_t)r * ld + W + sc * 8);
            vreg[u] = *reinterpret_cast<const alh8*>(base + (int64_t)r * ld + 2 * W + sc * 8);
        }
    }

    float m_run = -3.0e38f, l_run = 0.f;
    alf4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = alf4{0.f, 0.f, 0.f, 0.f};
    _Float16* Pw = Ps + wave * 16 * ATL_PS;

    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                                       // the previous tile is no longer read
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = u * 32 + (tid >> 3);
            *reinterpret_cast<alh8*>(reinterpret_cast<unsigned char*>(Ks) + r * 128 + ((sc ^ (r & 7)) << 4)) = kreg[u];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int d = sc * 8 + e;
                Vt[d * ATL_KT + (((r >> 3) ^ ((d ^ (d >> 3)) & 7)) << 3) + (r & 7)] = vreg[u][e];
            }
        }
        __syncthreads();
        if (t + 1 < ntiles) {                                  // the next tile's rows travel while this one is multiplied
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = (t + 1) * ATL_KT + u * 32 + (tid >> 3);
                kreg[u] = vreg[u] = zero;
                if (r < L) {
                    kreg[u] = *reinterpret_cast<const alh8*>(base + (int64_t)r * ld + W + sc * 8);
                    vreg[u] = *reinterpret_cast<const alh8*>(base + (int64_t)r * ld + 2 * W + sc * 8);
                }
            }
        }
        // ---- S^T of this tile: lane holds S[q][key = t*64 + kt*16 + lg*4 + e]
        alf4 s[4];
        float mt = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            alf4 a = {0.f, 0.f, 0.f, 0.f};
            const int r = kt * 16 + l15;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const alh8 kf = *reinterpret_cast<const alh8*>(reinterpret_cast<const unsigned char*>(Ks) + r * 128 +
                                                               (((ks * 4 + lg) ^ (r & 7)) << 4));
                a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], a, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int key = t * ATL_KT + kt * 16 + lg * 4 + e;
                const bool ok = key < L && (!CAUSAL || key <= q);
                a[e] = ok ? a[e] * scale : -3.0e38f;
                mt = fmaxf(mt, a[e]);
            }
            s[kt] = a;
        }
        mt = cc_rows_max(mt);
        const float m_new = fmaxf(m_run, mt);
        const float alpha = (m_run > -1.0e38f) ? __expf(m_run - m_new) : 0.f;
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pexp = (s[kt][e] > -1.0e38f) ? __expf(s[kt][e] - m_new) : 0.f;
                s[kt][e] = pexp;
                psum += pexp;
            }
            const alh4 ph = {(_Float16)s[kt][0], (_Float16)s[kt][1], (_Float16)s[kt][2], (_Float16)s[kt][3]};
            *reinterpret_cast<alh4*>(Pw + l15 * ATL_PS + kt * 16 + lg * 4) = ph;
        }
        psum = cc_rows_sum(psum);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[dt][e] *= alpha;
        __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0): the strip is private to this wave
        __builtin_amdgcn_wave_barrier();
        // ---- O^T += V^T P^T : lane holds O[q = l15][d = dt*16 + lg*4 + e]
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const alh8 pf = *reinterpret_cast<const alh8*>(Pw + l15 * ATL_PS + kb * 32 + lg * 8);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int d = dt * 16 + l15;
                const alh8 vf = *reinterpret_cast<const alh8*>(Vt + d * ATL_KT + (((kb * 4 + lg) ^ ((d ^ (d >> 3)) & 7)) << 3));
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dt], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (q < L) {
        const float inv = 1.0f / l_run;
        _Float16* dst = at.out + (seq_row0 + (int64_t)q * at.tok_rows) * W + head * ATL_D;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const alh4 oh = {(_Float16)(o[dt][0] * inv), (_Float16)(o[dt][1] * inv), (_Float16)(o[dt][2] * inv),
                             (_Float16)(o[dt][3] * inv)};
            *reinterpret_cast<alh4*>(dst + dt * 16 + lg * 4) = oh;
        }
    }
}

int cc_launch_attention_long(const AttArgs& a0, hipStream_t st) {
    if (a0.L <= 0 || a0.L > CC_ATT_LONG_MAX_L || a0.nseq <= 0 || a0.W != a0.heads * ATL_D) return CC_ERR_UNSUPPORTED;
    AttArgs a = a0;
    if (a.seq_rows == 0 && a.tok_rows == 0) { a.seq_rows = a.L; a.tok_rows = 1; }
    const int qtiles = (a.L + ATL_QT - 1) / ATL_QT;
    const int64_t grid = (int64_t)a.nseq * a.heads * qtiles;
    if (grid > 0x7FFFFFFF) return CC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(attention_long_kernel, dim3((unsigned)grid), dim3(256), 0, st, a, qtiles, 0.125f);
    CC_LAUNCH_CHECK();
    return CC_OK;
}
