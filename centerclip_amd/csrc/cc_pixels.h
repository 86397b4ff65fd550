// Pixel sources of the frame preprocessing (preprocess.hip, augment.hip): where a kernel's tap (row, column) of a source frame
// comes from.  Two sources, ONE fetch: interleaved / planar RGB bytes, and 8-bit YUV 4:2:0 planes converted to the three RGB
// bytes on the way in (include/centerclip_hip.h, "YUV 4:2:0 sources").  Everything behind the fetch - the
// resampling sums, the crops, the rounding - is the same code for both, so a kernel on a YUV source gives byte for byte what it
// gives on the converted frames.
#pragma once
#include <math.h>

#include "cc_common.h"

namespace cc_px {

// byte strides of (frame, channel, row, column) of a uint8 image batch
struct View {
    int64_t sf, sc, sy, sx;
};

__host__ __device__ inline View view_of(int fmt, int64_t rows, int64_t cols) {
    if (fmt == CC_FRAMES_U8_CHW) return View{3 * rows * cols, rows * cols, cols, 1};
    return View{3 * rows * cols, 1, 3 * cols, 3};
}

inline bool u8_format(int fmt) { return fmt == CC_FRAMES_U8_CHW || fmt == CC_FRAMES_U8_HWC; }

// the integer conversion of one (matrix, range): R = clamp((cy (Y - oy) + crv (Cr - 128) + 2^15) >> 16) and so on
struct YuvCoef {
    int32_t oy, cy, crv, cgu, cgv, cbu;
};

// A source of F frames.  RGB: the View of the frames (sf, sc, sy, sx).  YUV 4:2:0: sf = frame stride, sy = luma pitch, and the
// chroma sample of luma (y, x) at u_off / v_off + (y >> 1) c_pitch + (x >> 1) c_step from the frame's first byte.
struct PixelSource {
    int64_t sf, sc, sy, sx;
    int64_t u_off, v_off, c_pitch;
    int32_t c_step;
    YuvCoef k;
};

__host__ __device__ inline PixelSource rgb_source(int fmt, int64_t rows, int64_t cols) {
    const View v = view_of(fmt, rows, cols);
    PixelSource s{};
    s.sf = v.sf;
    s.sc = v.sc;
    s.sy = v.sy;
    s.sx = v.sx;
    return s;
}

__host__ __device__ inline int64_t yuv420_chroma(int64_t n) { return (n + 1) >> 1; }

// bytes of one tight 4:2:0 frame
__host__ __device__ inline int64_t yuv420_frame_bytes(int64_t H, int64_t W) {
    return H * W + 2 * yuv420_chroma(H) * yuv420_chroma(W);
}

// frames packed tight, one behind the other: kind CC_YUV420_I420 (Y, U, V planes) or CC_YUV420_NV12 (Y, interleaved UV)
__host__ __device__ inline PixelSource yuv420_tight_source(int kind, int64_t H, int64_t W, const YuvCoef& k) {
    const int64_t ch = yuv420_chroma(H), cw = yuv420_chroma(W);
    PixelSource s{};
    s.sf = yuv420_frame_bytes(H, W);
    s.sy = W;
    s.sx = 1;
    s.u_off = H * W;
    if (kind == CC_YUV420_NV12) {
        s.v_off = s.u_off + 1;
        s.c_pitch = 2 * cw;
        s.c_step = 2;
    } else {
        s.v_off = s.u_off + ch * cw;
        s.c_pitch = cw;
        s.c_step = 1;
    }
    s.k = k;
    return s;
}

__device__ __forceinline__ int clamp_byte(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// THE fetch: the three channel values, each in [0, 255], of pixel (y, x) of the frame that starts at `frame`
template <bool YUV>
__device__ __forceinline__ void fetch_pixel(const uint8_t* __restrict__ frame, const PixelSource& s, int y, int x, int& c0, int& c1,
                                            int& c2) {
    if (!YUV) {
        const uint8_t* p = frame + (int64_t)y * s.sy + (int64_t)x * s.sx;
        c0 = p[0];
        c1 = p[s.sc];
        c2 = p[2 * s.sc];
    } else {
        const uint8_t* c = frame + (int64_t)(y >> 1) * s.c_pitch + (int64_t)(x >> 1) * s.c_step;
        const int l = s.k.cy * ((int)frame[(int64_t)y * s.sy + x] - s.k.oy) + 32768;
        const int u = (int)c[s.u_off] - 128, v = (int)c[s.v_off] - 128;
        c0 = clamp_byte((l + s.k.crv * v) >> 16);                       // arithmetic shifts
        c1 = clamp_byte((l - s.k.cgu * u - s.k.cgv * v) >> 16);
        c2 = clamp_byte((l + s.k.cbu * u) >> 16);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the five coefficients as round(c 2^16) of the real ones, in double (both translation units that include this are compiled
// with -ffp-contract=off); false for a matrix / range outside {0, 1}
inline bool yuv_coefficients(int matrix, int range, YuvCoef* k) {
    if ((matrix != CC_YUV_BT601 && matrix != CC_YUV_BT709) || (range != CC_YUV_LIMITED && range != CC_YUV_FULL)) return false;
    const double kr = matrix == CC_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == CC_YUV_BT601 ? 0.114 : 0.0722;
    const double kg = 1.0 - kr - kb;
    const double sy = range == CC_YUV_LIMITED ? 255.0 / 219.0 : 1.0, sc = range == CC_YUV_LIMITED ? 255.0 / 224.0 : 1.0;
    const auto q = [](double c) { return (int32_t)floor(c * 65536.0 + 0.5); };
    k->oy = range == CC_YUV_LIMITED ? 16 : 0;
    k->cy = q(sy);
    k->crv = q(2.0 * (1.0 - kr) * sc);
    k->cgu = q(2.0 * kb * (1.0 - kb) / kg * sc);
    k->cgv = q(2.0 * kr * (1.0 - kr) / kg * sc);
    k->cbu = q(2.0 * (1.0 - kb) * sc);
    return true;
}

// The descriptor check every YUV entry point makes before any launch: CC_OK and the source, or the status.  Sizes outside
// 4 .. 8192 are CC_ERR_UNSUPPORTED as for the RGB entries; everything about the descriptor itself is CC_ERR_INVALID: a
// c_step outside {1, 2}, a matrix / range outside {0, 1}, a negative field, a pitch shorter than its row, and any address of
// (F, H, W) - luma or chroma - at or beyond src_bytes.
inline int yuv420_source(const cc_yuv420_layout* lay, size_t src_bytes, int64_t F, int64_t H, int64_t W, PixelSource* out) {
    if (!lay || F <= 0) return CC_ERR_INVALID;
    YuvCoef k;
    if (!yuv_coefficients(lay->matrix, lay->range, &k) || (lay->c_step != 1 && lay->c_step != 2)) return CC_ERR_INVALID;
    if (H < 4 || W < 4 || H > 8192 || W > 8192) return CC_ERR_UNSUPPORTED;
    const int64_t ch = yuv420_chroma(H), cw = yuv420_chroma(W), crow = (cw - 1) * lay->c_step + 1;
    if (lay->frame_stride < 0 || lay->u_offset < 0 || lay->v_offset < 0 || lay->y_pitch < W || lay->c_pitch < crow)
        return CC_ERR_INVALID;
    typedef unsigned __int128 u128;
    const u128 frames = (u128)(F - 1) * (u128)lay->frame_stride;
    const u128 luma = frames + (u128)(H - 1) * (u128)lay->y_pitch + (u128)W;                 // one past the last byte read
    const u128 chroma = frames + (u128)(ch - 1) * (u128)lay->c_pitch + (u128)crow;
    if (luma > src_bytes || chroma + (u128)lay->u_offset > src_bytes || chroma + (u128)lay->v_offset > src_bytes)
        return CC_ERR_INVALID;
    PixelSource s{};
    s.sf = lay->frame_stride;
    s.sy = lay->y_pitch;
    s.sx = 1;
    s.u_off = lay->u_offset;
    s.v_off = lay->v_offset;
    s.c_pitch = lay->c_pitch;
    s.c_step = lay->c_step;
    s.k = k;
    *out = s;
    return CC_OK;
}

}  // namespace cc_px
