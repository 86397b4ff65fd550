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
// A ragged batch (cc_collate_crop_flip_u8): the same thread's work per output pixel, the box in a table row per output frame.
//
// Coordinates are exact: the source coordinate (o + 0.5) crop / n_px - 0.5 is the rational ((2 o + 1) crop - n_px) / (2 n_px);
// its floor is an integer division and its fraction the remainder over 2 n_px, one correctly rounded fp32 division of two
// small integers.  THIS TRANSLATION UNIT IS COMPILED WITH -ffp-contract=off (build.py STRICT): the weights and the sums are
// IEEE single operations in source order - the error bound the tests hold the bytes to ("Train-time
// augmentation") counts them.
#include "cc_common.h"
#include "cc_pixels.h"

namespace {

using cc_px::PixelSource;
using cc_px::View;
using cc_px::fetch_pixel;
using cc_px::rgb_source;
using cc_px::u8_format;
using cc_px::view_of;
using cc_px::YuvCoef;
using cc_px::YuvFormat;
using cc_px::kRgb;

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

// The work of the thread that owns output pixel (oy, ox) of one frame, the one statement of the arithmetic: the per-size
// kernel below and the ragged-batch kernel behind it both call it.  in / out: the frame's first byte; the box is followed only
// when it lies inside the H x W frame, else the pixel is zero.  SRC: what the fetch reads and converts
// (cc_pixels.h).
template <int TAPS, int SRC>
__device__ __forceinline__ void crop_flip_pixel(const uint8_t* __restrict__ base, const PixelSource& iv, int H, int W, int top, int left,
                                                int bh, int bw, int flip, int n_px, int oy, int ox, uint8_t* __restrict__ out,
                                                const View& ov) {
    uint8_t* q = out + (int64_t)oy * ov.sy + (int64_t)ox * ov.sx;
    // (H - bh, W - bw cannot overflow: bh, bw >= 1)
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
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
#pragma unroll
    for (int r = 0; r < TAPS; ++r) {
        float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            int c0, c1, c2;
            fetch_pixel<SRC>(base, iv, top + iy[r], left + ix[k], c0, c1, c2);
            h0 += wx[k] * (float)c0;
            h1 += wx[k] * (float)c1;
            h2 += wx[k] * (float)c2;
        }
        v0 += wy[r] * h0;
        v1 += wy[r] * h1;
        v2 += wy[r] * h2;
    }
    q[0] = to_byte(v0);
    q[ov.sc] = to_byte(v1);
    q[2 * ov.sc] = to_byte(v2);
}

template <int TAPS, int SRC>
__global__ __launch_bounds__(kTileX* kTileY) void resized_crop_flip_u8_kernel(const uint8_t* __restrict__ in, PixelSource iv, int H,
                                                                                int W, int frames_per_clip,
                                                                                const int32_t* __restrict__ boxes,
                                                                                uint8_t* __restrict__ out, View ov, int n_px,
                                                                                int tiles_x, int tiles_y) {
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, f = blockIdx.x / (tiles_x * tiles_y);
    const int ox = bx * kTileX + threadIdx.x, oy = by * kTileY + threadIdx.y;
    if (ox >= n_px || oy >= n_px) return;
    const int32_t* box = boxes + (int64_t)(f / frames_per_clip) * kBoxInts;
    crop_flip_pixel<TAPS, SRC>(in + (int64_t)f * iv.sf, iv, H, W, box[0], box[1], box[2], box[3], box[4], n_px, oy, ox,
                          out + (int64_t)f * ov.sf, ov);
}

// A ragged batch (cc_collate_crop_flip_u8 in the header): one table row per OUTPUT frame, blockIdx.z over output frames, folded
// where there are more frames than planes.  Every workgroup reads its frame's row first - the same address in every lane.  The
// host never reads the table: a row whose frame does not lie inside the packed buffer, or whose kind is not 1, gives a zero
// frame, and crop_flip_pixel does the same for a box outside the frame.
// fmt: the RGB format code, or (a YUV source) yf: the tight format with k its conversion.
template <int SRC>
__global__ __launch_bounds__(kTileX* kTileY) void collate_crop_flip_u8_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                                int fmt, YuvFormat yf, YuvCoef k,
                                                                                const int64_t* __restrict__ rows,
                                                                                int n_out, uint8_t* __restrict__ dst,
                                                                                int dst_fmt, int n_px) {
    const int ox = blockIdx.x * kTileX + threadIdx.x, oy = blockIdx.y * kTileY + threadIdx.y;
    if (ox >= n_px || oy >= n_px) return;
    const View ov = view_of(dst_fmt, n_px, n_px);
    for (int f = blockIdx.z; f < n_out; f += gridDim.z) {
        const int64_t* row = rows + (int64_t)f * CC_COLLATE_BOX_ROW;
        const int64_t kind = row[0], off = row[1], H = row[2], W = row[3], interp = row[9];
        uint8_t* out = dst + (int64_t)f * ov.sf;
        const bool ok = kind == 1 && H >= 4 && W >= 4 && H <= 8192 && W <= 8192 && off >= 0 && off <= src_bytes &&
                        cc_px::packed_frame_bytes<SRC>(yf, H, W) <= src_bytes - off && (interp == 0 || interp == 1) &&
                        !(cc_px::src_wide(SRC) && (off & 1));
        if (!ok) {
            uint8_t* q = out + (int64_t)oy * ov.sy + (int64_t)ox * ov.sx;
            q[0] = 0;
            q[ov.sc] = 0;
            q[2 * ov.sc] = 0;
            continue;
        }
        // a box value that is no int32 becomes -1, which crop_flip_pixel refuses (a zero frame) like any box outside the frame
        const auto i32 = [](int64_t v) { return v < INT32_MIN || v > INT32_MAX ? -1 : (int)v; };
        const int top = i32(row[4]), left = i32(row[5]), bh = i32(row[6]), bw = i32(row[7]);
        const PixelSource iv = SRC != kRgb ? cc_px::yuv_tight_source(yf, H, W, k) : rgb_source(fmt, H, W);
        const uint8_t* base = src + off;
        if (interp == 1)
            crop_flip_pixel<4, SRC>(base, iv, (int)H, (int)W, top, left, bh, bw, row[8] != 0, n_px, oy, ox, out, ov);
        else
            crop_flip_pixel<2, SRC>(base, iv, (int)H, (int)W, top, left, bh, bw, row[8] != 0, n_px, oy, ox, out, ov);
    }
}

// the launch of cc_resized_crop_flip_u8 / _yuv_u8 once the source is known to be sound
template <int SRC>
int crop_flip_launch(const void* src, const PixelSource& sv, int32_t F, int32_t H, int32_t W, int32_t frames_per_clip,
                     const int32_t* boxes_dev, int32_t n_px, int32_t interp, void* dst, int32_t dst_fmt, void* stream) {
    if (n_px < 1 || n_px > 1024 || H < 4 || W < 4 || H > 8192 || W > 8192) return CC_ERR_UNSUPPORTED;
    const int tiles_x = (n_px + kTileX - 1) / kTileX, tiles_y = (n_px + kTileY - 1) / kTileY;
    if ((int64_t)F * tiles_x * tiles_y > 0x7fffffffLL) return CC_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* in = static_cast<const uint8_t*>(src);
    uint8_t* out = static_cast<uint8_t*>(dst);
    const View dv = view_of(dst_fmt, n_px, n_px);
    const dim3 block(kTileX, kTileY);
    const unsigned grid = (unsigned)(F * tiles_x * tiles_y);
    if (interp == 0)
        resized_crop_flip_u8_kernel<2, SRC><<<grid, block, 0, st>>>(in, sv, H, W, frames_per_clip, boxes_dev, out, dv, n_px,
                                                                     tiles_x, tiles_y);
    else
        resized_crop_flip_u8_kernel<4, SRC><<<grid, block, 0, st>>>(in, sv, H, W, frames_per_clip, boxes_dev, out, dv, n_px,
                                                                     tiles_x, tiles_y);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

// the checks and the launch of cc_collate_crop_flip_u8 / _yuv_u8; fmt: the RGB format code, or yf: the tight YUV format
template <int SRC>
int collate_crop_flip_launch(const void* src, size_t src_bytes, int32_t fmt, const YuvFormat& yf, const YuvCoef& k,
                             const int64_t* clips_host,
                             int32_t n_clips, const int64_t* rows_dev, int32_t n_out, int32_t n_px, void* dst, int32_t dst_fmt,
                             void* stream) {
    for (int i = 0; i < n_clips; ++i) {
        const int64_t off = clips_host[4 * i], t = clips_host[4 * i + 1], H = clips_host[4 * i + 2], W = clips_host[4 * i + 3];
        if (off < 0 || t < 1 || H < 1 || W < 1 || H > 8192 || W > 8192 || t > (int64_t)1 << 31) return CC_ERR_INVALID;
        if (cc_px::src_wide(SRC) && (off & 1)) return CC_ERR_INVALID;
        const int64_t frame = cc_px::packed_frame_bytes<SRC>(yf, H, W);
        if ((uint64_t)off > src_bytes || (uint64_t)(t * frame) > src_bytes - (uint64_t)off) return CC_ERR_INVALID;
        if (H < 4 || W < 4) return CC_ERR_UNSUPPORTED;
    }
    if (n_px < 1 || n_px > 1024) return CC_ERR_UNSUPPORTED;
    const int tiles_x = (n_px + kTileX - 1) / kTileX, tiles_y = (n_px + kTileY - 1) / kTileY;
    int64_t planes = 0x7fffffffLL / ((int64_t)tiles_x * tiles_y * kTileX * kTileY);
    if (planes > CC_COLLATE_MAX_PLANES) planes = CC_COLLATE_MAX_PLANES;
    if (planes > n_out) planes = n_out;
    collate_crop_flip_u8_kernel<SRC><<<dim3(tiles_x, tiles_y, (unsigned)planes), dim3(kTileX, kTileY), 0,
                                       static_cast<hipStream_t>(stream)>>>(static_cast<const uint8_t*>(src), (int64_t)src_bytes,
                                                                           fmt, yf, k, rows_dev, n_out, static_cast<uint8_t*>(dst),
                                                                           dst_fmt, n_px);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // namespace

extern "C" {

int cc_resized_crop_flip_u8(const void* src, int32_t fmt, int32_t F, int32_t H, int32_t W, int32_t frames_per_clip,
                            const int32_t* boxes_dev, int32_t n_px, int32_t interp, void* dst, int32_t dst_fmt, void* stream) {
    if (!src || !dst || !boxes_dev || F <= 0 || frames_per_clip <= 0 || !u8_format(fmt) || !u8_format(dst_fmt) ||
        (interp != 0 && interp != 1))
        return CC_ERR_INVALID;
    return crop_flip_launch<kRgb>(src, rgb_source(fmt, H, W), F, H, W, frames_per_clip, boxes_dev, n_px, interp, dst, dst_fmt,
                                   stream);
}

int cc_resized_crop_flip_yuv_u8(const void* src, size_t src_bytes, const cc_yuv_layout* layout, int32_t F, int32_t H, int32_t W,
                                int32_t frames_per_clip, const int32_t* boxes_dev, int32_t n_px, int32_t interp, void* dst,
                                int32_t dst_fmt, void* stream) {
    if (!src || !dst || !boxes_dev || !layout || F <= 0 || frames_per_clip <= 0 || !u8_format(dst_fmt) ||
        (interp != 0 && interp != 1))
        return CC_ERR_INVALID;
    PixelSource sv;
    const int rc = cc_px::yuv_source(src, layout, src_bytes, F, H, W, &sv);
    if (rc != CC_OK) return rc;
    return cc_px::dispatch_yuv(layout->depth, layout->sub_x, layout->sub_y, [&](auto s) {
        return crop_flip_launch<decltype(s)::value>(src, sv, F, H, W, frames_per_clip, boxes_dev, n_px, interp, dst, dst_fmt, stream);
    });
}

int cc_resized_crop_flip_yuv420_u8(const void* src, size_t src_bytes, const cc_yuv420_layout* layout, int32_t F, int32_t H,
                                   int32_t W, int32_t frames_per_clip, const int32_t* boxes_dev, int32_t n_px, int32_t interp,
                                   void* dst, int32_t dst_fmt, void* stream) {
    if (!layout) return CC_ERR_INVALID;
    const cc_yuv_layout lay = cc_px::yuv420_layout(*layout);
    return cc_resized_crop_flip_yuv_u8(src, src_bytes, &lay, F, H, W, frames_per_clip, boxes_dev, n_px, interp, dst, dst_fmt,
                                       stream);
}

int cc_collate_crop_flip_u8(const void* src, size_t src_bytes, int32_t fmt, const int64_t* clips_host, int32_t n_clips,
                            const int64_t* rows_dev, int32_t n_out, int32_t n_px, void* dst, int32_t dst_fmt, void* stream) {
    if (!src || !dst || !rows_dev || !clips_host || n_out <= 0 || n_clips <= 0 || !u8_format(fmt) || !u8_format(dst_fmt))
        return CC_ERR_INVALID;
    return collate_crop_flip_launch<kRgb>(src, src_bytes, fmt, YuvFormat{}, YuvCoef{}, clips_host, n_clips, rows_dev, n_out, n_px, dst, dst_fmt,
                                           stream);
}

int cc_collate_crop_flip_yuv_u8(const void* src, size_t src_bytes, int32_t format, int32_t matrix, int32_t range,
                                const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out, int32_t n_px,
                                void* dst, int32_t dst_fmt, void* stream) {
    YuvCoef k;
    YuvFormat yf;
    if (!src || !dst || !rows_dev || !clips_host || n_out <= 0 || n_clips <= 0 || !u8_format(dst_fmt) ||
        !cc_px::yuv_format(format, &yf) || !cc_px::yuv_coefficients(matrix, range, yf.depth, &k))
        return CC_ERR_INVALID;
    if (yf.depth > 8 && ((uintptr_t)src & 1)) return CC_ERR_INVALID;
    return cc_px::dispatch_yuv(yf.depth, yf.sub_x, yf.sub_y, [&](auto s) {
        return collate_crop_flip_launch<decltype(s)::value>(src, src_bytes, 0, yf, k, clips_host, n_clips, rows_dev, n_out, n_px, dst,
                                                            dst_fmt, stream);
    });
}

int cc_collate_crop_flip_yuv420_u8(const void* src, size_t src_bytes, int32_t kind, int32_t matrix, int32_t range,
                                   const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out,
                                   int32_t n_px, void* dst, int32_t dst_fmt, void* stream) {
    if (kind != CC_YUV420_I420 && kind != CC_YUV420_NV12) return CC_ERR_INVALID;
    return cc_collate_crop_flip_yuv_u8(src, src_bytes, kind, matrix, range, clips_host, n_clips, rows_dev, n_out, n_px, dst,
                                       dst_fmt, stream);
}

}  // extern "C"
