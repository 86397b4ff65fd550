// Train-time augmentation of decoded uint8 frames on the device: one crop box and one flip bit per clip, resized to
// n_px x n_px - what the reference's training loader does per clip with TensorMultiScaleCrop / RandomResizedCrop and
// TensorRandomHorizontalFlip (dataloaders/decode.py:32-41, dataloaders/transforms.py:37-134, 168-196), i.e.
// torch.nn.functional.interpolate(crop, n_px, mode, align_corners=False) without antialias and a column reversal.  The boxes
// are drawn on the host (preprocess.TrainFrameTransform.sample); this file only applies them.
//
// One launch, no workspace, no plan: without antialias an output sample has 2 x 2 (bilinear) or 4 x 4 (bicubic) taps whatever
// the crop's size, so a thread computes its taps itself.  A thread owns output pixel (f, oy, ox) and its three channels, ox
// along the lanes.  The box table stays on the device - the host never reads it, so the call is capturable and a replay
// follows whatever the table holds by then; a row that does not lie inside the frame is never turned into an address.
//
// Coordinates are exact: the source coordinate (o + 0.5) crop / n_px - 0.5 is the rational ((2 o + 1) crop - n_px) / (2 n_px);
// its floor is an integer division and its fraction the remainder over 2 n_px, one correctly rounded fp32 division of two
// small integers.  THIS TRANSLATION UNIT IS COMPILED WITH -ffp-contract=off (build.py STRICT): the weights and the sums are
// IEEE single operations in source order - the error bound the tests hold the bytes to ("Train-time
// augmentation") counts them.
#include "cc_common.h"

namespace {

// byte strides of (frame, channel, row, column) of a uint8 image batch
struct View {
    int64_t sf, sc, sy, sx;
};

View view_of(int fmt, int64_t rows, int64_t cols) {
    if (fmt == CC_FRAMES_U8_CHW) return View{3 * rows * cols, rows * cols, cols, 1};
    return View{3 * rows * cols, 1, 3 * cols, 3};
}

bool u8_format(int fmt) { return fmt == CC_FRAMES_U8_CHW || fmt == CC_FRAMES_U8_HWC; }

constexpr int kTileX = 64, kTileY = 4;
constexpr int kBoxInts = 5;                         // (top, left, height, width, flip)

// The taps of output index o of an axis resized from `crop` to `n_px` samples: idx[k] in [0, crop), w[k] their weights.
// (2 o + 1) crop <= 2047 * 8192 < 2^31.
template <int TAPS>
__device__ __forceinline__ void axis_taps(int o, int crop, int n_px, int* idx, float* w) {
    const int den = 2 * n_px;
    int num = (2 * o + 1) * crop - n_px;
    if (TAPS == 2 && num < 0) num = 0;              // bilinear: the coordinate is clamped below at 0
    int i0 = num / den, rem = num - i0 * den;
    if (rem < 0) {                                  // floor, not truncation (bicubic, first samples of an upscale)
        rem += den;
        --i0;
    }
    const float t = (float)rem / (float)den;        // in [0, 1): both integers are exact in fp32
    const float s = 1.0f - t;
    const int last = crop - 1;
    if (TAPS == 2) {
        idx[0] = i0;                                // (i0 <= last: the coordinate stays below crop - 1/2)
        idx[1] = i0 < last ? i0 + 1 : last;
        w[0] = s;
        w[1] = t;
    } else {
        // cubic convolution, A = -0.75: |x| <= 1: ((A + 2) x - (A + 3)) x^2 + 1;  1 < |x| < 2: A (x - 1) (x - 2)^2 - the
        // outer taps in this factored form, which has no cancellation (x = 1 + t: A t (1 - t)^2; x = 2 - t: A (1 - t) t^2)
        const float A = -0.75f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 - 1 + k;
            idx[k] = i < 0 ? 0 : (i > last ? last : i);
        }
        w[0] = A * t * s * s;
        w[1] = (1.25f * t - 2.25f) * t * t + 1.0f;
        w[2] = (1.25f * s - 2.25f) * s * s + 1.0f;
        w[3] = A * s * t * t;
    }
}

__device__ __forceinline__ uint8_t to_byte(float v) {
    const float r = rintf(v);                       // half to even, as numpy.rint
    return (uint8_t)(r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r));
}

template <int TAPS>
__global__ __launch_bounds__(kTileX* kTileY) void resized_crop_flip_u8_kernel(const uint8_t* __restrict__ in, View iv, int H,
                                                                                int W, int frames_per_clip,
                                                                                const int32_t* __restrict__ boxes,
                                                                                uint8_t* __restrict__ out, View ov, int n_px,
                                                                                int tiles_x, int tiles_y) {
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, f = blockIdx.x / (tiles_x * tiles_y);
    const int ox = bx * kTileX + threadIdx.x, oy = by * kTileY + threadIdx.y;
    if (ox >= n_px || oy >= n_px) return;
    uint8_t* q = out + (int64_t)f * ov.sf + (int64_t)oy * ov.sy + (int64_t)ox * ov.sx;
    const int32_t* box = boxes + (int64_t)(f / frames_per_clip) * kBoxInts;
    const int top = box[0], left = box[1], bh = box[2], bw = box[3], flip = box[4];
    // the row is followed only when the box lies inside the frame (H - bh, W - bw cannot overflow: bh, bw >= 1)
    if (top < 0 || left < 0 || bh < 1 || bw < 1 || top > H - bh || left > W - bw) {
        q[0] = 0;
        q[ov.sc] = 0;
        q[2 * ov.sc] = 0;
        return;
    }
    int ix[TAPS], iy[TAPS];
    float wx[TAPS], wy[TAPS];
    axis_taps<TAPS>(flip ? n_px - 1 - ox : ox, bw, n_px, ix, wx);
    axis_taps<TAPS>(oy, bh, n_px, iy, wy);
    const uint8_t* base = in + (int64_t)f * iv.sf;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
#pragma unroll
    for (int r = 0; r < TAPS; ++r) {
        const uint8_t* row = base + (int64_t)(top + iy[r]) * iv.sy;
        float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const uint8_t* p = row + (int64_t)(left + ix[k]) * iv.sx;
            h0 += wx[k] * (float)p[0];
            h1 += wx[k] * (float)p[iv.sc];
            h2 += wx[k] * (float)p[2 * iv.sc];
        }
        v0 += wy[r] * h0;
        v1 += wy[r] * h1;
        v2 += wy[r] * h2;
    }
    q[0] = to_byte(v0);
    q[ov.sc] = to_byte(v1);
    q[2 * ov.sc] = to_byte(v2);
}

}  // namespace

extern "C" {

int cc_resized_crop_flip_u8(const void* src, int32_t fmt, int32_t F, int32_t H, int32_t W, int32_t frames_per_clip,
                            const int32_t* boxes_dev, int32_t n_px, int32_t interp, void* dst, int32_t dst_fmt, void* stream) {
    if (!src || !dst || !boxes_dev || F <= 0 || frames_per_clip <= 0 || !u8_format(fmt) || !u8_format(dst_fmt) ||
        (interp != 0 && interp != 1))
        return CC_ERR_INVALID;
    if (n_px < 1 || n_px > 1024 || H < 4 || W < 4 || H > 8192 || W > 8192) return CC_ERR_UNSUPPORTED;
    const int tiles_x = (n_px + kTileX - 1) / kTileX, tiles_y = (n_px + kTileY - 1) / kTileY;
    if ((int64_t)F * tiles_x * tiles_y > 0x7fffffffLL) return CC_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* in = static_cast<const uint8_t*>(src);
    uint8_t* out = static_cast<uint8_t*>(dst);
    const View sv = view_of(fmt, H, W), dv = view_of(dst_fmt, n_px, n_px);
    const dim3 block(kTileX, kTileY);
    const unsigned grid = (unsigned)(F * tiles_x * tiles_y);
    if (interp == 0)
        resized_crop_flip_u8_kernel<2><<<grid, block, 0, st>>>(in, sv, H, W, frames_per_clip, boxes_dev, out, dv, n_px, tiles_x,
                                                                tiles_y);
    else
        resized_crop_flip_u8_kernel<4><<<grid, block, 0, st>>>(in, sv, H, W, frames_per_clip, boxes_dev, out, dv, n_px, tiles_x,
                                                                tiles_y);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // extern "C"
