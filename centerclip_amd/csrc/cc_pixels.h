// Pixel sources of the frame preprocessing (preprocess.hip, augment.hip): where a kernel's tap (row, column) of a source frame
// comes from.  Three sources, ONE fetch: interleaved / planar RGB bytes, and YUV planes of 8-bit or of 16-bit samples (4:2:0,
// 4:2:2 or 4:4:4, planar or semi-planar, depth 8 / 10 / 12 / 16) converted to the three RGB bytes on the way in
// (include/centerclip_hip.h, "YUV sources").  Everything behind the fetch - the resampling sums, the
// crops, the rounding - is the same code for all, so a kernel on a YUV source gives byte for byte what it gives on the
// converted frames.
//
// THE CONVERSION for depth d.  A sample is n = word >> shift: d = 8: word is a byte, shift 0; d in {10, 12, 16}: word is a
// little-endian 16-bit word, 0 <= shift <= 16 - d (P010: d 10, shift 6; yuv420p10le: d 10, shift 0; P016: d 16, shift 0); the
// bits below shift are discarded whatever they hold.  Real formula, Kr / Kb / Kg of BT.601 or BT.709: limited range
// oy = 16 2^(d-8), sy = 255 / (219 2^(d-8)), sc = 255 / (224 2^(d-8)); full range oy = 0, sy = sc = 255 / (2^d - 1); chroma
// centre 2^(d-1); R = sy (Y - oy) + 2 (1 - Kr) sc (V - centre), G = sy (Y - oy) - 2 Kb (1 - Kb) / Kg sc (U - centre)
// - 2 Kr (1 - Kr) / Kg sc (V - centre), B = sy (Y - oy) + 2 (1 - Kb) sc (U - centre).  Integer definition: C = floor(c 2^Q + 0.5)
// in double, Q = 16 for d = 8 and Q = 20 for d > 8; a channel is clamp((sum + 2^(Q-1)) >> Q, 0, 255) in int32, >> arithmetic;
// |sum| <= 5.8e8 < 2^31 for samples up to 2^d - 1 (a larger n, possible only where shift < 16 - d, is outside the definition:
// no address depends on it).  Chroma is replicated: luma (y, x) uses chroma (y >> sub_y, x >> sub_x).
// NOT built: BT.2020 and PQ / HLG tone mapping (10-bit frames are converted as the SDR signal their matrix describes); packed
// formats (YUYV, UYVY), big-endian words, 4:1:1, alpha planes; interpolated chroma siting, dithering.
#pragma once
#include <math.h>

#include <type_traits>

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

// What a kernel's fetch reads: the template argument SRC of every kernel of preprocess.hip / augment.hip.  kRgb, or a YUV source
// with the sample size (wide: 16-bit words) and the chroma subsampling in the code - as runtime fields of the source the two
// shifts cost the 8-bit 4:2:0 calls 0.7 - 1.4 % (profiles/yuv_formats.txt), more than their round-to-round spread.
constexpr int kRgb = 0;
constexpr int yuv_src(int wide, int sub_x, int sub_y) { return 1 | wide << 1 | sub_x << 2 | sub_y << 3; }
constexpr bool src_wide(int src) { return (src >> 1) & 1; }
constexpr int src_sub_x(int src) { return (src >> 2) & 1; }
constexpr int src_sub_y(int src) { return (src >> 3) & 1; }

// f(std::integral_constant<int, SRC>) for the YUV source of (depth, sub_x, sub_y), each already checked to be in range
template <class F>
int dispatch_yuv(int depth, int sub_x, int sub_y, F&& f) {
#define CC_PX_CASE(w, x, y) \
    case yuv_src(w, x, y): return f(std::integral_constant<int, yuv_src(w, x, y)>{})
    switch (yuv_src(depth > 8, sub_x, sub_y)) {
        CC_PX_CASE(0, 0, 0);
        CC_PX_CASE(0, 1, 0);
        CC_PX_CASE(0, 0, 1);
        CC_PX_CASE(0, 1, 1);
        CC_PX_CASE(1, 0, 0);
        CC_PX_CASE(1, 1, 0);
        CC_PX_CASE(1, 0, 1);
        CC_PX_CASE(1, 1, 1);
    }
#undef CC_PX_CASE
    return CC_ERR_INVALID;
}

// the integer conversion of one (matrix, range, depth): R = clamp((cy (Y - oy) + crv (Cr - centre) + 2^(Q-1)) >> Q) and so on
struct YuvCoef {
    int32_t oy, cy, crv, cgu, cgv, cbu;
    int32_t centre;                                 // 2^(depth - 1)
};

// A source of F frames.  RGB: the View of the frames (sf, sc, sy, sx).  YUV: sf = frame stride, sy = luma pitch, and the
// chroma sample of luma (y, x) at u_off / v_off + (y >> sub_y) c_pitch + (x >> sub_x) c_step from the frame's first byte
// (sub_x, sub_y: in SRC); 16-bit samples: n = word >> shift.  All in bytes.
struct PixelSource {
    int64_t sf, sc, sy, sx;
    int64_t u_off, v_off, c_pitch;
    int32_t c_step, shift;
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

// One named format (CC_YUV_I420 ... of the header): THE table of what a name means.
struct YuvFormat {
    int32_t sub_x, sub_y, depth, shift, interleaved;
};

__host__ __device__ inline int yuv_sample_bytes(int depth) { return depth > 8 ? 2 : 1; }

inline bool yuv_format(int format, YuvFormat* f) {
    static const YuvFormat table[CC_YUV_FORMATS] = {
        {1, 1, 8, 0, 0},  /* I420 */    {1, 1, 8, 0, 1},  /* NV12 */    {1, 0, 8, 0, 0},  /* I422 */    {0, 0, 8, 0, 0},  /* I444 */
        {1, 1, 10, 0, 0}, /* I420P10 */ {1, 0, 10, 0, 0}, /* I422P10 */ {0, 0, 10, 0, 0}, /* I444P10 */ {1, 1, 10, 6, 1}, /* P010 */
        {1, 1, 12, 0, 0}, /* I420P12 */ {1, 1, 12, 4, 1}, /* P012 */    {1, 1, 16, 0, 1}, /* P016 */    {0, 0, 16, 0, 0}, /* I444P16 */
    };
    if (format < 0 || format >= CC_YUV_FORMATS) return false;
    *f = table[format];
    return true;
}

__host__ __device__ inline int64_t yuv_chroma(int64_t n, int sub) { return (n + sub) >> sub; }

// bytes of one tight frame
__host__ __device__ inline int64_t yuv_frame_bytes(const YuvFormat& f, int64_t H, int64_t W) {
    return (H * W + 2 * yuv_chroma(H, f.sub_y) * yuv_chroma(W, f.sub_x)) * yuv_sample_bytes(f.depth);
}

// bytes of one frame of a packed buffer: [H, W, 3] / [3, H, W] RGB bytes, or a tight YUV frame of format f
template <int SRC>
__host__ __device__ inline int64_t packed_frame_bytes(const YuvFormat& f, int64_t H, int64_t W) {
    return SRC == kRgb ? 3 * H * W : yuv_frame_bytes(f, H, W);
}

// frames packed tight, one behind the other: Y, U, V planes, or Y and interleaved UV
__host__ __device__ inline PixelSource yuv_tight_source(const YuvFormat& f, int64_t H, int64_t W, const YuvCoef& k) {
    const int64_t ch = yuv_chroma(H, f.sub_y), cw = yuv_chroma(W, f.sub_x), b = yuv_sample_bytes(f.depth);
    PixelSource s{};
    s.sf = yuv_frame_bytes(f, H, W);
    s.sy = W * b;
    s.sx = b;
    s.u_off = H * W * b;
    if (f.interleaved) {
        s.v_off = s.u_off + b;
        s.c_pitch = 2 * cw * b;
        s.c_step = (int32_t)(2 * b);
    } else {
        s.v_off = s.u_off + ch * cw * b;
        s.c_pitch = cw * b;
        s.c_step = (int32_t)b;
    }
    s.shift = f.shift;
    s.k = k;
    return s;
}

__device__ __forceinline__ int clamp_byte(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int load_u16(const uint8_t* p) { return (int)*reinterpret_cast<const uint16_t*>(p); }   // p is even

// THE fetch: the three channel values, each in [0, 255], of pixel (y, x) of the frame that starts at `frame`
template <int SRC>
__device__ __forceinline__ void fetch_pixel(const uint8_t* __restrict__ frame, const PixelSource& s, int y, int x, int& c0, int& c1,
                                            int& c2) {
    if (SRC == kRgb) {
        const uint8_t* p = frame + (int64_t)y * s.sy + (int64_t)x * s.sx;
        c0 = p[0];
        c1 = p[s.sc];
        c2 = p[2 * s.sc];
    } else {
        const uint8_t* c = frame + (int64_t)(y >> src_sub_y(SRC)) * s.c_pitch + (int64_t)(x >> src_sub_x(SRC)) * s.c_step;
        constexpr int Q = src_wide(SRC) ? 20 : 16;
        int l, u, v;
        if (!src_wide(SRC)) {
            l = (int)frame[(int64_t)y * s.sy + x];
            u = (int)c[s.u_off] - 128;
            v = (int)c[s.v_off] - 128;
        } else {
            l = load_u16(frame + (int64_t)y * s.sy + 2 * (int64_t)x) >> s.shift;
            u = (load_u16(c + s.u_off) >> s.shift) - s.k.centre;
            v = (load_u16(c + s.v_off) >> s.shift) - s.k.centre;
        }
        l = s.k.cy * (l - s.k.oy) + (1 << (Q - 1));
        c0 = clamp_byte((l + s.k.crv * v) >> Q);                        // arithmetic shifts
        c1 = clamp_byte((l - s.k.cgu * u - s.k.cgv * v) >> Q);
        c2 = clamp_byte((l + s.k.cbu * u) >> Q);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the five coefficients as floor(c 2^Q + 0.5) of the real ones, in double (both translation units that include this are
// compiled with -ffp-contract=off); false for a matrix / range outside {0, 1} or a depth outside {8, 10, 12, 16}
inline bool yuv_coefficients(int matrix, int range, int depth, YuvCoef* k) {
    if ((matrix != CC_YUV_BT601 && matrix != CC_YUV_BT709) || (range != CC_YUV_LIMITED && range != CC_YUV_FULL)) return false;
    if (depth != 8 && depth != 10 && depth != 12 && depth != 16) return false;
    const double kr = matrix == CC_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == CC_YUV_BT601 ? 0.114 : 0.0722;
    const double kg = 1.0 - kr - kb;
    const double up = (double)(1 << (depth - 8)), top = (double)((1 << depth) - 1);
    // (depth 8: 255 / (219 * 1) and 255 / 255 are the same doubles as before)
    const double sy = range == CC_YUV_LIMITED ? 255.0 / (219.0 * up) : 255.0 / top;
    const double sc = range == CC_YUV_LIMITED ? 255.0 / (224.0 * up) : 255.0 / top;
    const double one = depth == 8 ? 65536.0 : 1048576.0;
    const auto q = [one](double c) { return (int32_t)floor(c * one + 0.5); };
    k->oy = range == CC_YUV_LIMITED ? 16 << (depth - 8) : 0;
    k->cy = q(sy);
    k->crv = q(2.0 * (1.0 - kr) * sc);
    k->cgu = q(2.0 * kb * (1.0 - kb) / kg * sc);
    k->cgv = q(2.0 * kr * (1.0 - kr) / kg * sc);
    k->cbu = q(2.0 * (1.0 - kb) * sc);
    k->centre = 1 << (depth - 1);
    return true;
}

// The descriptor check every YUV entry point makes before any launch: CC_OK and the source, or the status.  Everything about
// the descriptor itself is CC_ERR_INVALID: a depth outside {8, 10, 12, 16}, a shift outside 0 .. 16 - depth (nonzero at depth
// 8), sub_x / sub_y outside {0, 1}, a c_step other than one or two samples, a matrix / range outside {0, 1}; sizes outside
// 4 .. 8192 are then CC_ERR_UNSUPPORTED as for the RGB entries; then again CC_ERR_INVALID: a negative field, a pitch shorter
// than its row in bytes, for 16-bit samples an odd src address, offset, pitch or frame stride, and any address of (F, H, W) -
// luma or chroma - at or beyond src_bytes.
inline int yuv_source(const void* src, const cc_yuv_layout* lay, size_t src_bytes, int64_t F, int64_t H, int64_t W,
                      PixelSource* out) {
    if (!lay || F <= 0) return CC_ERR_INVALID;
    YuvCoef k;
    if (!yuv_coefficients(lay->matrix, lay->range, lay->depth, &k)) return CC_ERR_INVALID;
    const int64_t b = yuv_sample_bytes(lay->depth);
    if (lay->shift < 0 || lay->shift > (lay->depth == 8 ? 0 : 16 - lay->depth)) return CC_ERR_INVALID;
    if ((lay->sub_x != 0 && lay->sub_x != 1) || (lay->sub_y != 0 && lay->sub_y != 1)) return CC_ERR_INVALID;
    if (lay->c_step != b && lay->c_step != 2 * b) return CC_ERR_INVALID;
    if (H < 4 || W < 4 || H > 8192 || W > 8192) return CC_ERR_UNSUPPORTED;
    const int64_t ch = yuv_chroma(H, lay->sub_y), cw = yuv_chroma(W, lay->sub_x), crow = (cw - 1) * lay->c_step + b;
    if (lay->frame_stride < 0 || lay->u_offset < 0 || lay->v_offset < 0 || lay->y_pitch < W * b || lay->c_pitch < crow)
        return CC_ERR_INVALID;
    if (b == 2 && (((uintptr_t)src | (uintptr_t)lay->frame_stride | (uintptr_t)lay->y_pitch | (uintptr_t)lay->u_offset |
                    (uintptr_t)lay->v_offset | (uintptr_t)lay->c_pitch) & 1))
        return CC_ERR_INVALID;
    typedef unsigned __int128 u128;
    const u128 frames = (u128)(F - 1) * (u128)lay->frame_stride;
    const u128 luma = frames + (u128)(H - 1) * (u128)lay->y_pitch + (u128)(W * b);           // one past the last byte read
    const u128 chroma = frames + (u128)(ch - 1) * (u128)lay->c_pitch + (u128)crow;
    if (luma > src_bytes || chroma + (u128)lay->u_offset > src_bytes || chroma + (u128)lay->v_offset > src_bytes)
        return CC_ERR_INVALID;
    PixelSource s{};
    s.sf = lay->frame_stride;
    s.sy = lay->y_pitch;
    s.sx = b;
    s.u_off = lay->u_offset;
    s.v_off = lay->v_offset;
    s.c_pitch = lay->c_pitch;
    s.c_step = lay->c_step;
    s.shift = lay->shift;
    s.k = k;
    *out = s;
    return CC_OK;
}

// the 8-bit 4:2:0 descriptor of the cc_*_yuv420_u8 entries as the general one
inline cc_yuv_layout yuv420_layout(const cc_yuv420_layout& l) {
    cc_yuv_layout g{};
    g.frame_stride = l.frame_stride;
    g.y_pitch = l.y_pitch;
    g.u_offset = l.u_offset;
    g.v_offset = l.v_offset;
    g.c_pitch = l.c_pitch;
    g.c_step = l.c_step;
    g.sub_x = 1;
    g.sub_y = 1;
    g.depth = 8;
    g.shift = 0;
    g.matrix = l.matrix;
    g.range = l.range;
    return g;
}

}  // namespace cc_px
