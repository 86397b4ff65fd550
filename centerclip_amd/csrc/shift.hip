// cluster_algo 'temporal_shift' / 'token_shift' (modules/cluster/shift.py:15-61, cluster.py:343-347): a fixed 0/1 linear map
// over the frames of each segment of `segment` consecutive frames.  Channels [0, fold) of a shifted row take the value of
// the NEXT frame (zero in the segment's last frame), channels [fold, 2 fold) that of the PREVIOUS frame (zero in the first),
// channels >= 2 fold are unchanged; fold = W / fold_div.  temporal_shift shifts every token but the CLS row, token_shift the
// CLS row only.  The adjoint swaps the two directions (the gradient of "take next" is "take previous").
//
// Only copies and zeros: every output is bit-identical to the reference's.
#include "cc_kernels.h"

#define CC_SHIFT_ROWS_MAX_LDS 65536      /* phase-1 parking of the rows kernel: segment * 2 fold floats */

namespace {

typedef _Float16 h4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool shift_token(int mode, int j) {
    return mode == CC_CLUSTER_TOKEN_SHIFT ? j == 0 : j != 0;
}

// Layout check of a [F, L, W] view through (tok_stride, frame_stride) (element units, W contiguous): no two elements alias.
// The inner of the two dimensions needs a stride >= W, the outer one >= its extent times the inner stride.
bool layout_ok(int64_t tok, int64_t frame, int F, int L, int64_t W) {
    if (tok <= 0 || frame <= 0) return false;
    if (tok <= frame)
        return (L == 1 || tok >= W) && (F == 1 || frame >= (L == 1 ? W : (int64_t)L * tok));
    return (F == 1 || frame >= W) && (L == 1 || tok >= (F == 1 ? W : (int64_t)F * frame));
}

// ---- out of place: one thread per output element (channels fastest: coalesced in both layouts)
__global__ __launch_bounds__(256) void shift_copy_kernel(const float* __restrict__ x, int64_t ts, int64_t fs,
                                                         float* __restrict__ out, int64_t ots, int64_t ofs, int F, int L,
                                                         int W, int seg, int fold, int mode, int adjoint) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)F * L * W) return;
    const int c = (int)(idx % W);
    const int64_t r = idx / W;
    const int j = (int)(r % L), f = (int)(r / L);
    const int t = f % seg;
    int src = f;                                     // source frame; -1 = zero
    if (c < 2 * fold && shift_token(mode, j)) {
        const bool next = (c < fold) != (adjoint != 0);
        src = next ? (t + 1 < seg ? f + 1 : -1) : (t > 0 ? f - 1 : -1);
    }
    out[(int64_t)f * ofs + (int64_t)j * ots + c] = src < 0 ? 0.f : x[(int64_t)src * fs + (int64_t)j * ts + c];
}

// ---- in place: one thread per (segment, shifted token, channel < 2 fold) walks the segment's frames in ascending order.
// "take next": x[t] = x[t + 1] reads frame t + 1 before the step that overwrites it; "take previous": the original of frame
// t - 1 is carried in a register.  Channels >= 2 fold and the unshifted tokens are not touched.
__global__ __launch_bounds__(256) void shift_inplace_kernel(float* __restrict__ x, int64_t ts, int64_t fs, int segments,
                                                            int ntok, int seg, int W, int fold, int mode, int adjoint) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int C = min(2 * fold, W);
    if (idx >= (int64_t)segments * ntok * C) return;
    const int c = (int)(idx % C);
    const int64_t r = idx / C;
    const int k = (int)(r % ntok), s = (int)(r / ntok);
    const int j = mode == CC_CLUSTER_TOKEN_SHIFT ? 0 : k + 1;
    float* p = x + (int64_t)s * seg * fs + (int64_t)j * ts + c;
    const bool next = (c < fold) != (adjoint != 0);
    if (next) {
        for (int t = 0; t < seg; ++t) p[(int64_t)t * fs] = t + 1 < seg ? p[(int64_t)(t + 1) * fs] : 0.f;
    } else {
        float prev = 0.f;
        for (int t = 0; t < seg; ++t) {
            const float cur = p[(int64_t)t * fs];
            p[(int64_t)t * fs] = prev;
            prev = cur;
        }
    }
}

// ---- fused-encoder form: contiguous fp32 rows h [*, W] (row of frame f, token j = f * frame_rows + j * tok_rows), shifted in
// place, and for every row it rewrites: the fp16 copy centred on the row mean, (sum, sum of squares) of that copy in slot 0
// and zeros in slots 1 .. slots - 1 of stats [row][slots][2] (the folded-LayerNorm GEMMs add the slots of a row: they see the
// full sums), the centre in shift[row] - the by-products row_stats_kernel (transformer.hip) writes, in the GEMMs' layout.
// One workgroup per (segment, token): phase 1 parks channels [0, 2 fold) of the segment's frames in LDS, then every wave
// owns whole rows and reads its other channels from memory - all reads of a channel that gets written precede the barrier,
// so the update is in place.  token_shift has one workgroup per segment only (16 at cfg 2): 16 waves, so that a wave walks
// ceil(segment / 16) rows instead of segment / 4 (the launch is latency bound); temporal_shift keeps 4 waves, the grid
// (segments x tokens) fills the device.  temporal_shift rewrites the CLS rows as well (unchanged values, fresh
// statistics): every row then carries the one-slot layout, which is what lets the encoder continue with slots = 1.
struct ShiftRowsArgs {
    float* h;
    _Float16* h16;
    float* stats;
    float* shift;
    int64_t tok_rows, frame_rows;
    int L, W, seg, fold, mode, slots, ntok;
};

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void shift_rows_kernel(ShiftRowsArgs a) {
    extern __shared__ float parked[];                            // [seg][min(2 fold, W)]
    const int s = blockIdx.x / a.ntok, k = blockIdx.x % a.ntok;
    const int j = a.mode == CC_CLUSTER_TOKEN_SHIFT ? 0 : k;
    const bool shifted = shift_token(a.mode, j);
    const int W = a.W, C = min(2 * a.fold, W);
    const int f0 = s * a.seg;
    auto row_of = [&](int t) { return (int64_t)(f0 + t) * a.frame_rows + (int64_t)j * a.tok_rows; };
    if (shifted) {
        for (int i = threadIdx.x; i < a.seg * C; i += WAVES * 64) {
            const int t = i / C, c = i - t * C;
            parked[i] = a.h[row_of(t) * W + c];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < a.seg; t += WAVES) {
        const int64_t row = row_of(t);
        float* hr = a.h + row * W;
        float4 v[4];
        float tot = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int w = lane * 4 + q * 256;
            v[q] = (w < W) ? *reinterpret_cast<const float4*>(hr + w) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (shifted && w < C) {
                float e[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = w + u;
                    if (c < C) {
                        const int src = c < a.fold ? t + 1 : t - 1;
                        e[u] = (src >= 0 && src < a.seg) ? parked[src * C + c] : 0.f;
                    }
                }
                v[q] = make_float4(e[0], e[1], e[2], e[3]);
                *reinterpret_cast<float4*>(hr + w) = v[q];
            }
            tot += (v[q].x + v[q].y) + (v[q].z + v[q].w);
        }
        const float om = cc_wave_sum_fast(tot) / (float)W;
        float sm = 0.f, sq = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int w = lane * 4 + q * 256;
            if (w < W) {
                h4 o = {(_Float16)(v[q].x - om), (_Float16)(v[q].y - om), (_Float16)(v[q].z - om), (_Float16)(v[q].w - om)};
                *reinterpret_cast<h4*>(a.h16 + row * W + w) = o;
                const float q0 = (float)o[0], q1 = (float)o[1], q2 = (float)o[2], q3 = (float)o[3];
                sm += (q0 + q1) + (q2 + q3);
                sq += (q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3);
            }
        }
        sm = cc_wave_sum_fast(sm);
        sq = cc_wave_sum_fast(sq);
        float2* st = reinterpret_cast<float2*>(a.stats) + row * a.slots;
        for (int u = lane; u < a.slots; u += 64) st[u] = u == 0 ? make_float2(sm, sq) : make_float2(0.f, 0.f);
        if (lane == 0) a.shift[row] = om;
    }
}

bool mode_ok(int mode) { return mode == CC_CLUSTER_TEMPORAL_SHIFT || mode == CC_CLUSTER_TOKEN_SHIFT; }

}  // namespace

extern "C" {

int cc_token_shift_f32(const float* x, int64_t tok_stride, int64_t frame_stride, int32_t F, int32_t L, int32_t W,
                       int32_t segment, int32_t fold_div, int32_t mode, int32_t adjoint, float* out,
                       int64_t out_tok_stride, int64_t out_frame_stride, void* stream) {
    if (!x || !out || F <= 0 || L <= 0 || W <= 0 || segment <= 0 || F % segment || fold_div <= 0 || !mode_ok(mode) ||
        (adjoint != 0 && adjoint != 1))
        return CC_ERR_INVALID;
    if (!layout_ok(tok_stride, frame_stride, F, L, W) || !layout_ok(out_tok_stride, out_frame_stride, F, L, W))
        return CC_ERR_INVALID;
    const bool inplace = out == x;
    if (inplace && (out_tok_stride != tok_stride || out_frame_stride != frame_stride)) return CC_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int fold = W / fold_div;
    if (!inplace) {
        const int64_t n = (int64_t)F * L * W;
        shift_copy_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(x, tok_stride, frame_stride, out, out_tok_stride,
                                                                        out_frame_stride, F, L, W, segment, fold, mode, adjoint);
        CC_LAUNCH_CHECK();
        return CC_OK;
    }
    const int ntok = mode == CC_CLUSTER_TOKEN_SHIFT ? 1 : L - 1;
    const int64_t n = (int64_t)(F / segment) * ntok * (2 * fold < W ? 2 * fold : W);
    if (n == 0) return CC_OK;                     // fold 0 (W < fold_div) or no patch tokens: the identity
    shift_inplace_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(out, tok_stride, frame_stride, F / segment, ntok,
                                                                      segment, W, fold, mode, adjoint);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

size_t cc_token_shift_rows_lds_bytes(int32_t segment, int32_t W, int32_t fold_div) {
    if (segment <= 0 || W <= 0 || fold_div <= 0) return 0;
    const int64_t C = 2 * (int64_t)(W / fold_div);
    return (size_t)segment * (C < W ? C : W) * sizeof(float);
}

int cc_token_shift_rows_f32(float* h, int64_t tok_rows, int64_t frame_rows, int32_t F, int32_t L, int32_t W,
                            int32_t segment, int32_t fold_div, int32_t mode, void* h16, float* stats, int32_t slots,
                            float* shift, void* stream) {
    if (!h || !h16 || !stats || !shift || F <= 0 || L <= 0 || W <= 0 || (W & 3) || W > 1024 || segment <= 0 ||
        F % segment || fold_div <= 0 || !mode_ok(mode) || slots < 1 || slots > CC_LN_MAX_SLOTS)
        return CC_ERR_INVALID;
    if (!layout_ok(tok_rows, frame_rows, F, L, 1)) return CC_ERR_INVALID;
    const size_t lds = cc_token_shift_rows_lds_bytes(segment, W, fold_div);
    if (lds > CC_SHIFT_ROWS_MAX_LDS) return CC_ERR_UNSUPPORTED;
    ShiftRowsArgs a{h, static_cast<_Float16*>(h16), stats, shift, tok_rows, frame_rows, L, W, segment, W / fold_div, mode,
                    slots, mode == CC_CLUSTER_TOKEN_SHIFT ? 1 : L};
    const int64_t blocks = (int64_t)(F / segment) * a.ntok;
    if (mode == CC_CLUSTER_TOKEN_SHIFT)
        shift_rows_kernel<16><<<(unsigned)blocks, 16 * 64, lds, static_cast<hipStream_t>(stream)>>>(a);
    else
        shift_rows_kernel<4><<<(unsigned)blocks, 4 * 64, lds, static_cast<hipStream_t>(stream)>>>(a);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // extern "C"
