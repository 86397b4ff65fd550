// Resize + centre crop of decoded uint8 frames on the device, byte for byte what CLIP's loader transform gives
// (dataloaders/rawvideo_util.py:16-23: Resize(n_px, BICUBIC) -> CenterCrop(n_px); the two operations behind them, ToTensor
// and Normalize, already run inside the uint8 patch gather).  Resize is Pillow's 8-bit resample: per axis a table of 22-bit
// integer coefficients computed in double, a horizontal pass rounded to bytes, then a vertical pass on those bytes.
//
// Host side (no GPU needed): cc_resize_plan_build fills the plan - geometry + the coefficient tables of the crop window's
// columns and rows.  THIS TRANSLATION UNIT IS COMPILED WITH -ffp-contract=off (build.py STRICT): the coefficients are IEEE
// double operations in source order.
// Device side: two launches of one kernel (horizontal pass into the workspace, vertical pass into dst); a pass whose axis
// keeps its size is not launched, and with neither the crop is a strided copy.  Only the window is computed: its n_px
// columns, and of the source rows only those the window's vertical taps read.  Every source sample is loaded as a single byte
// - a frame base and a row of 3 W bytes carry no alignment.
// A ragged batch (clips of mixed sizes and lengths packed back to back, cc_collate_resize_crop_u8): the same two passes as at
// most two launches for the whole batch, one table row per output frame; the per-pixel arithmetic is the same device function.
// YUV sources (the cc_*_yuv_u8 entries, and cc_*_yuv420_u8 as their 8-bit 4:2:0 case): the same kernels with the other pixel
// sources of cc_pixels.h (SRC = a yuv_src code) - the first pass that touches the source converts each tap in its fetch;
// cc_yuv_to_rgb_u8 is the crop kernel with the whole frame as window.
#include <math.h>

#include <vector>

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

constexpr int kPrecisionBits = 22;
constexpr int kMaxKsize = CC_RESIZE_MAX_TAPS;                     // taps per output sample the launches take: a shrink factor of 16
constexpr int32_t kMagic = 0x31504352;              // "RCP1"

struct Geometry {
    int oh, ow, top, left;                          // resized size, crop offsets in it
    int row0, row1;                                 // source rows [row0, row1) the window reads
    int ksize_h, ksize_v;                           // taps per output column / row; 0 = the pass is skipped
};

// torchvision CenterCrop: int(round((size - n_px) / 2.0)), round half to even
int crop_offset(int size, int n_px) { return (int)nearbyint((size - n_px) / 2.0); }

struct Axis {
    int in, out, ksize;
    double scale, support, ss;
};

Axis make_axis(int in, int out) {
    Axis a;
    a.in = in;
    a.out = out;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * fs;
    a.ss = 1.0 / fs;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}

double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// taps of output index xx: first source index, count, and (coef != NULL) the count integer coefficients, zeros behind;
// w: a.ksize doubles of scratch
void axis_taps(const Axis& a, int xx, int* first, int* count, int32_t* coef, double* w) {
    const double center = (xx + 0.5) * a.scale;
    int xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > a.in) xmax = a.in;
    const int n = xmax - xmin;
    *first = xmin;
    *count = n;
    if (!coef) return;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        w[x] = bicubic(((x + xmin) - center + 0.5) * a.ss);
        ww += w[x];
    }
    for (int x = 0; x < a.ksize; ++x) {
        if (x >= n) {
            coef[x] = 0;
            continue;
        }
        const double v = ww != 0.0 ? w[x] / ww : w[x];
        coef[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << kPrecisionBits)) : (int)(0.5 + v * (double)(1 << kPrecisionBits));
    }
}

// CC_OK and the geometry, or the status every entry point gives for these sizes.  max_ksize: the taps per output sample the
// caller takes (the plan builder: any; the launches and their workspace: kMaxKsize).
int geometry(int H, int W, int n_px, int resize, int max_ksize, Geometry* g) {
    if (resize != 0 && resize != 1) return CC_ERR_INVALID;
    if (n_px < 1 || n_px > 1024 || H < 4 || W < 4 || H > 8192 || W > 8192) return CC_ERR_UNSUPPORTED;
    g->oh = H;
    g->ow = W;
    if (resize) {
        // torchvision Resize(int): true division in double, then truncation; a short side that already is n_px: untouched
        if (W <= H) {
            if (W != n_px) {
                g->ow = n_px;
                g->oh = (int)((double)n_px * (double)H / (double)W);
            }
        } else if (H != n_px) {
            g->oh = n_px;
            g->ow = (int)((double)n_px * (double)W / (double)H);
        }
    }
    if (g->oh < n_px || g->ow < n_px) return CC_ERR_UNSUPPORTED;        // (the crop's zero padding is not built)
    g->top = crop_offset(g->oh, n_px);
    g->left = crop_offset(g->ow, n_px);
    g->ksize_h = g->ow != W ? make_axis(W, g->ow).ksize : 0;
    g->ksize_v = g->oh != H ? make_axis(H, g->oh).ksize : 0;
    if (g->ksize_h > max_ksize || g->ksize_v > max_ksize) return CC_ERR_UNSUPPORTED;
    g->row0 = g->top;
    g->row1 = g->top + n_px;
    if (g->ksize_v) {
        const Axis a = make_axis(H, g->oh);
        g->row0 = H;
        g->row1 = 0;
        for (int y = 0; y < n_px; ++y) {
            int first, count;
            axis_taps(a, g->top + y, &first, &count, nullptr, nullptr);
            if (first < g->row0) g->row0 = first;
            if (first + count > g->row1) g->row1 = first + count;
        }
    }
    return CC_OK;
}

size_t plan_ints(const Geometry& g, int n_px) { return CC_RESIZE_PLAN_HEADER + (size_t)n_px * (4 + g.ksize_h + g.ksize_v); }

// what the host believes the device plan was built for; a kernel handed another plan does nothing (its table entries are
// source indices - they are only followed when they belong to these sizes)
struct PlanKey {
    int32_t H, W, n_px, resize;
};

__device__ __forceinline__ bool plan_matches(const int32_t* plan, const PlanKey& k) {
    return plan[0] == kMagic && plan[1] == k.H && plan[2] == k.W && plan[3] == k.n_px && plan[4] == k.resize;
}

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> kPrecisionBits;                  // arithmetic shift
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

constexpr int kTileX = 64, kTileY = 4;

// One pass.  A thread owns output pixel (f, oy, ox) - ox along the lanes, so source, intermediate and output accesses of a wave
// run along a row - and its three channels.  HORIZONTAL: out(f, c, oy, ox) = sum_k in(f, c, row_base + oy, first[ox] + k) coef[ox][k];
// vertical: out(f, c, oy, ox) = sum_k in(f, c, row_base + first[oy] + k, col_base + ox) coef[oy][k] (the coefficients are then
// uniform over a wave).  row_base / col_base: the origin the row / column indices count from (the vertical pass reads the
// workspace, whose row 0 is source row row0: row_base = -row0 - or, no horizontal pass, the source itself from column `left`).
// resample_pixel is that thread's work, the one statement of the arithmetic: the per-size kernel below and the ragged-batch
// kernel behind it both call it.  SRC: what the fetch reads and converts (cc_pixels.h).
template <bool VERT, int SRC>
__device__ __forceinline__ void resample_pixel(const uint8_t* __restrict__ in, const PixelSource& iv, int row_base, int col_base,
                                               const int32_t* __restrict__ plan, int n_px, int f, int oy, int ox,
                                               uint8_t* __restrict__ out, const View& ov) {
    const int ksize = plan[VERT ? 12 : 11];
    const int32_t* tab = plan + plan[VERT ? 14 : 13];
    const int j = VERT ? oy : ox;
    const int first = tab[j], count = tab[n_px + j];
    const int32_t* coef = tab + 2 * n_px + (int64_t)j * ksize;
    const uint8_t* frame = in + (int64_t)f * iv.sf;
    int y = row_base + (VERT ? first : oy), x = col_base + (VERT ? ox : first);
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < count; ++k) {
        const int w = coef[k];
        int c0, c1, c2;
        fetch_pixel<SRC>(frame, iv, y, x, c0, c1, c2);
        a0 += c0 * w;
        a1 += c1 * w;
        a2 += c2 * w;
        if (VERT)
            ++y;
        else
            ++x;
    }
    uint8_t* q = out + (int64_t)f * ov.sf + (int64_t)oy * ov.sy + (int64_t)ox * ov.sx;
    q[0] = clip8(a0);
    q[ov.sc] = clip8(a1);
    q[2 * ov.sc] = clip8(a2);
}

// neither axis is resampled: out(f, c, oy, ox) = in(f, c, top + oy, left + ox)
template <int SRC>
__device__ __forceinline__ void crop_pixel(const uint8_t* __restrict__ in, const PixelSource& iv, int top, int left, int f, int oy,
                                           int ox, uint8_t* __restrict__ out, const View& ov) {
    int c0, c1, c2;
    fetch_pixel<SRC>(in + (int64_t)f * iv.sf, iv, top + oy, left + ox, c0, c1, c2);
    uint8_t* q = out + (int64_t)f * ov.sf + (int64_t)oy * ov.sy + (int64_t)ox * ov.sx;
    q[0] = (uint8_t)c0;
    q[ov.sc] = (uint8_t)c1;
    q[2 * ov.sc] = (uint8_t)c2;
}

template <bool VERT, int SRC>
__global__ __launch_bounds__(kTileX* kTileY) void resample_u8_kernel(const uint8_t* __restrict__ in, PixelSource iv, int row_base,
                                                                       int col_base, const int32_t* __restrict__ plan,
                                                                       PlanKey key, uint8_t* __restrict__ out, View ov,
                                                                       int out_rows, int tiles_x, int tiles_y) {
    if (!plan_matches(plan, key)) return;
    const int n_px = key.n_px;
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, f = blockIdx.x / (tiles_x * tiles_y);
    const int ox = bx * kTileX + threadIdx.x, oy = by * kTileY + threadIdx.y;
    if (ox >= n_px || oy >= out_rows) return;
    resample_pixel<VERT, SRC>(in, iv, row_base, col_base, plan, n_px, f, oy, ox, out, ov);
}

// the crop alone (n_px x n_px at (top, left)) and, with the whole frame as the window, the stand-alone conversion
template <int SRC>
__global__ __launch_bounds__(kTileX* kTileY) void crop_u8_kernel(const uint8_t* __restrict__ in, PixelSource iv, int top, int left,
                                                                   uint8_t* __restrict__ out, View ov, int rows, int cols,
                                                                   int tiles_x, int tiles_y) {
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, f = blockIdx.x / (tiles_x * tiles_y);
    const int ox = bx * kTileX + threadIdx.x, oy = by * kTileY + threadIdx.y;
    if (ox >= cols || oy >= rows) return;
    crop_pixel<SRC>(in, iv, top, left, f, oy, ox, out, ov);
}

// ---- a ragged batch: clips of mixed sizes and lengths packed back to back, one table row per OUTPUT frame ----------------
// (cc_collate_resize_crop_u8 in the header).  blockIdx.z runs over output frames, folded where there are more frames than
// planes; every workgroup reads its frame's row first - the same address in every lane, so plain loads.  The grid covers the
// largest frame of the call; a tile beyond its own frame's extent exits.  The host never reads the table, so nothing in a row
// becomes an address before it is checked against the sizes the host passed: a row that fails comes out as a zero frame.
struct CollateArgs {
    const uint8_t* src;
    int64_t src_bytes;
    const int64_t* rows;
    const int32_t* plans;
    int64_t plans_ints;
    uint8_t* ws;
    int64_t ws_bytes;
    uint8_t* dst;
    int32_t n_out, n_px, resize, fmt, dst_fmt;      // fmt: the RGB format code (SRC = kRgb only)
    YuvFormat yf;                                   // a YUV source: the packed frames' format and its conversion
    YuvCoef k;
};

struct CollateFrame {
    const uint8_t* src;                             // the frame's first byte
    const int32_t* plan;
    uint8_t* mid;                                   // both passes: the horizontal result [3, nrows, n_px]
    int H, W, top, left, row0, nrows, ksize_h, ksize_v;
};

// -> whether output frame f is a transform whose row holds up; false: a zero frame
template <int SRC>
__device__ __forceinline__ bool collate_frame(const CollateArgs& a, int f, CollateFrame* c) {
    const int64_t* row = a.rows + (int64_t)f * CC_COLLATE_ROW;
    const int64_t kind = row[0], off = row[1], H = row[2], W = row[3], plan_off = row[4], ws_off = row[5];
    if (kind != 1 || H < 4 || W < 4 || H > 8192 || W > 8192) return false;
    if (off < 0 || off > a.src_bytes || cc_px::packed_frame_bytes<SRC>(a.yf, H, W) > a.src_bytes - off) return false;
    if (cc_px::src_wide(SRC) && (off & 1)) return false;
    if (plan_off < 0 || plan_off > a.plans_ints - CC_RESIZE_PLAN_HEADER) return false;
    const int32_t* plan = a.plans + plan_off;
    if (!plan_matches(plan, PlanKey{(int32_t)H, (int32_t)W, a.n_px, a.resize})) return false;
    if (plan[15] < CC_RESIZE_PLAN_HEADER || plan[15] > a.plans_ints - plan_off) return false;
    c->src = a.src + off;
    c->plan = plan;
    c->H = (int)H;
    c->W = (int)W;
    c->top = plan[7];
    c->left = plan[8];
    c->row0 = plan[9];
    c->nrows = plan[10] - plan[9];
    c->ksize_h = plan[11];
    c->ksize_v = plan[12];
    c->mid = nullptr;
    if (c->ksize_h && c->ksize_v) {
        const int64_t need = (int64_t)3 * c->nrows * a.n_px;
        if (!a.ws || c->nrows < 1 || ws_off < 0 || ws_off > a.ws_bytes || need > a.ws_bytes - ws_off) return false;
        c->mid = a.ws + ws_off;
    }
    return true;
}

// FINAL = false: the horizontal pass of the frames that run both passes, into the workspace; nothing else is touched.
// FINAL = true: every output frame is written - zeros, the crop alone, the one pass its size needs, or the vertical pass over
// the workspace.
template <bool FINAL, int SRC>
__global__ __launch_bounds__(kTileX* kTileY) void collate_resample_u8_kernel(CollateArgs a) {
    const int ox = blockIdx.x * kTileX + threadIdx.x, oy = blockIdx.y * kTileY + threadIdx.y;
    if (ox >= a.n_px) return;
    const View dv = view_of(a.dst_fmt, a.n_px, a.n_px);
    for (int f = blockIdx.z; f < a.n_out; f += gridDim.z) {
        CollateFrame c;
        const bool ok = collate_frame<SRC>(a, f, &c);
        // (a frame that fails its checks has no sizes to build a source from)
        const PixelSource sv = !ok ? PixelSource{}
                                   : (SRC != kRgb ? cc_px::yuv_tight_source(a.yf, c.H, c.W, a.k) : rgb_source(a.fmt, c.H, c.W));
        if (!FINAL) {
            if (!ok || !c.mid || oy >= c.nrows) continue;
            resample_pixel<false, SRC>(c.src, sv, c.row0, 0, c.plan, a.n_px, 0, oy, ox, c.mid,
                                       view_of(CC_FRAMES_U8_CHW, c.nrows, a.n_px));
            continue;
        }
        if (oy >= a.n_px) return;
        uint8_t* out = a.dst + (int64_t)f * dv.sf;
        if (!ok) {
            uint8_t* q = out + (int64_t)oy * dv.sy + (int64_t)ox * dv.sx;
            q[0] = 0;
            q[dv.sc] = 0;
            q[2 * dv.sc] = 0;
            continue;
        }
        if (c.mid) {
            resample_pixel<true, kRgb>(c.mid, rgb_source(CC_FRAMES_U8_CHW, c.nrows, a.n_px), -c.row0, 0, c.plan, a.n_px, 0, oy, ox,
                                        out, dv);
        } else if (c.ksize_h) {
            resample_pixel<false, SRC>(c.src, sv, c.top, 0, c.plan, a.n_px, 0, oy, ox, out, dv);
        } else if (c.ksize_v) {
            resample_pixel<true, SRC>(c.src, sv, 0, c.left, c.plan, a.n_px, 0, oy, ox, out, dv);
        } else {
            crop_pixel<SRC>(c.src, sv, c.top, c.left, 0, oy, ox, out, dv);
        }
    }
}

// planes of blockIdx.z a launch of tiles_x x tiles_y workgroups per plane uses for n_out frames (the rest is folded)
int collate_planes(int n_out, int tiles_x, int tiles_y) {
    int64_t z = 0x7fffffffLL / ((int64_t)tiles_x * tiles_y * kTileX * kTileY);
    if (z > CC_COLLATE_MAX_PLANES) z = CC_COLLATE_MAX_PLANES;
    if (z > n_out) z = n_out;
    return z < 1 ? 1 : (int)z;
}

// the host's checks of a clip table [n_clips, 4] rows (byte offset, frames, H, W) against the packed buffer's size
template <int SRC>
int collate_check_clips(const int64_t* clips, int n_clips, size_t src_bytes, const YuvFormat& yf) {
    if (!clips || n_clips <= 0) return CC_ERR_INVALID;
    for (int i = 0; i < n_clips; ++i) {
        const int64_t off = clips[4 * i], t = clips[4 * i + 1], H = clips[4 * i + 2], W = clips[4 * i + 3];
        if (off < 0 || t < 1 || H < 1 || W < 1 || H > 8192 || W > 8192 || t > (int64_t)1 << 31) return CC_ERR_INVALID;
        if (cc_px::src_wide(SRC) && (off & 1)) return CC_ERR_INVALID;
        const int64_t frame = cc_px::packed_frame_bytes<SRC>(yf, H, W);
        if ((uint64_t)off > src_bytes || (uint64_t)(t * frame) > src_bytes - (uint64_t)off) return CC_ERR_INVALID;
    }
    return CC_OK;
}

// the launches of cc_resize_crop_u8 / cc_resize_crop_yuv_u8 once the source is known to be sound
template <int SRC>
int resize_crop_launch(const void* src, const PixelSource& sv, int32_t F, int32_t H, int32_t W, const void* plan_dev, int32_t n_px,
                       int32_t resize, void* dst, int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream) {
    Geometry g;
    const int rc = geometry(H, W, n_px, resize, kMaxKsize, &g);
    if (rc != CC_OK) return rc;
    const int nrows = g.row1 - g.row0;
    const int tiles_x = (n_px + kTileX - 1) / kTileX;
    const int tiles_mid = (nrows + kTileY - 1) / kTileY, tiles_out = (n_px + kTileY - 1) / kTileY;
    if ((int64_t)F * tiles_x * (tiles_mid > tiles_out ? tiles_mid : tiles_out) > 0x7fffffffLL) return CC_ERR_UNSUPPORTED;
    size_t need = 0;                                // (cc_resize_crop_workspace_bytes)
    if (g.ksize_h && g.ksize_v) need = (size_t)F * 3 * (size_t)nrows * (size_t)n_px;
    if (need && (!ws || ws_bytes < need)) return CC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* in = static_cast<const uint8_t*>(src);
    uint8_t* out = static_cast<uint8_t*>(dst);
    const int32_t* plan = static_cast<const int32_t*>(plan_dev);
    const View dv = view_of(dst_fmt, n_px, n_px);
    const PlanKey key{H, W, n_px, resize};
    const dim3 block(kTileX, kTileY);
    if (!g.ksize_h && !g.ksize_v) {
        crop_u8_kernel<SRC><<<(unsigned)(F * tiles_x * tiles_out), block, 0, st>>>(in, sv, g.top, g.left, out, dv, n_px, n_px,
                                                                                    tiles_x, tiles_out);
        CC_LAUNCH_CHECK();
        return CC_OK;
    }
    if (g.ksize_h && !g.ksize_v) {                  // rows keep their size: the horizontal pass writes the window's rows
        resample_u8_kernel<false, SRC><<<(unsigned)(F * tiles_x * tiles_out), block, 0, st>>>(in, sv, g.top, 0, plan, key, out,
                                                                                               dv, n_px, tiles_x, tiles_out);
        CC_LAUNCH_CHECK();
        return CC_OK;
    }
    if (!g.ksize_h) {                               // columns keep their size: the vertical pass reads the source from `left`
        resample_u8_kernel<true, SRC><<<(unsigned)(F * tiles_x * tiles_out), block, 0, st>>>(in, sv, 0, g.left, plan, key, out,
                                                                                              dv, n_px, tiles_x, tiles_out);
        CC_LAUNCH_CHECK();
        return CC_OK;
    }
    // both: the horizontal result of source rows [row0, row1), rounded to bytes, planar [F, 3, nrows, n_px] in the workspace
    uint8_t* mid = static_cast<uint8_t*>(ws);
    const View mv = view_of(CC_FRAMES_U8_CHW, nrows, n_px);
    resample_u8_kernel<false, SRC><<<(unsigned)(F * tiles_x * tiles_mid), block, 0, st>>>(in, sv, g.row0, 0, plan, key, mid, mv,
                                                                                           nrows, tiles_x, tiles_mid);
    CC_LAUNCH_CHECK();
    resample_u8_kernel<true, kRgb><<<(unsigned)(F * tiles_x * tiles_out), block, 0, st>>>(
        mid, rgb_source(CC_FRAMES_U8_CHW, nrows, n_px), -g.row0, 0, plan, key, out, dv, n_px, tiles_x, tiles_out);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

// the launch of cc_yuv_to_rgb_u8: the crop kernel with the whole frame as its window
template <int SRC>
int to_rgb_launch(const void* src, const PixelSource& sv, int32_t F, int32_t H, int32_t W, void* dst, int32_t dst_fmt,
                         void* stream) {
    const int tiles_x = (W + kTileX - 1) / kTileX, tiles_y = (H + kTileY - 1) / kTileY;
    if ((int64_t)F * tiles_x * tiles_y > 0x7fffffffLL) return CC_ERR_UNSUPPORTED;
    crop_u8_kernel<SRC><<<(unsigned)(F * tiles_x * tiles_y), dim3(kTileX, kTileY), 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const uint8_t*>(src), sv, 0, 0, static_cast<uint8_t*>(dst), view_of(dst_fmt, H, W), H, W, tiles_x, tiles_y);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // namespace

extern "C" {

size_t cc_resize_plan_bytes(int32_t H, int32_t W, int32_t n_px, int32_t resize) {
    Geometry g;
    if (geometry(H, W, n_px, resize, INT32_MAX, &g) != CC_OK) return 0;
    return plan_ints(g, n_px) * sizeof(int32_t);
}

int cc_resize_plan_build(int32_t H, int32_t W, int32_t n_px, int32_t resize, void* host_buf) {
    if (!host_buf) return CC_ERR_INVALID;
    Geometry g;
    const int rc = geometry(H, W, n_px, resize, INT32_MAX, &g);
    if (rc != CC_OK) return rc;
    std::vector<double> w((size_t)(g.ksize_h > g.ksize_v ? g.ksize_h : g.ksize_v) + 1);
    int32_t* plan = static_cast<int32_t*>(host_buf);
    const int off_h = CC_RESIZE_PLAN_HEADER, off_v = off_h + n_px * (2 + g.ksize_h);
    const int32_t header[CC_RESIZE_PLAN_HEADER] = {kMagic, H,         W,         n_px,  resize, g.oh,  g.ow,  g.top,
                                                    g.left, g.row0,    g.row1,    g.ksize_h, g.ksize_v, off_h, off_v,
                                                    (int32_t)plan_ints(g, n_px)};
    for (int i = 0; i < CC_RESIZE_PLAN_HEADER; ++i) plan[i] = header[i];
    for (int pass = 0; pass < 2; ++pass) {
        const int ksize = pass ? g.ksize_v : g.ksize_h, origin = pass ? g.top : g.left;
        int32_t* tab = plan + (pass ? off_v : off_h);
        const Axis a = ksize ? (pass ? make_axis(H, g.oh) : make_axis(W, g.ow)) : Axis{};
        for (int j = 0; j < n_px; ++j) {
            if (!ksize) {                           // a skipped pass: the window's own rows / columns, no taps
                tab[j] = origin + j;
                tab[n_px + j] = 0;
                continue;
            }
            axis_taps(a, origin + j, &tab[j], &tab[n_px + j], tab + 2 * n_px + (size_t)j * ksize, w.data());
        }
    }
    return CC_OK;
}

size_t cc_resize_crop_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t n_px, int32_t resize) {
    Geometry g;
    if (F <= 0 || geometry(H, W, n_px, resize, kMaxKsize, &g) != CC_OK) return 0;
    if (!g.ksize_h || !g.ksize_v) return 0;         // at most one pass: it writes dst itself
    return (size_t)F * 3 * (size_t)(g.row1 - g.row0) * (size_t)n_px;
}

int cc_resize_crop_u8(const void* src, int32_t fmt, int32_t F, int32_t H, int32_t W, const void* plan_dev, int32_t n_px,
                      int32_t resize, void* dst, int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream) {
    if (!src || !dst || !plan_dev || F <= 0 || !u8_format(fmt) || !u8_format(dst_fmt)) return CC_ERR_INVALID;
    return resize_crop_launch<kRgb>(src, rgb_source(fmt, H, W), F, H, W, plan_dev, n_px, resize, dst, dst_fmt, ws, ws_bytes, stream);
}

int cc_resize_crop_yuv_u8(const void* src, size_t src_bytes, const cc_yuv_layout* layout, int32_t F, int32_t H, int32_t W,
                          const void* plan_dev, int32_t n_px, int32_t resize, void* dst, int32_t dst_fmt, void* ws, size_t ws_bytes,
                          void* stream) {
    if (!src || !dst || !plan_dev || !layout || F <= 0 || !u8_format(dst_fmt)) return CC_ERR_INVALID;
    PixelSource sv;
    const int rc = cc_px::yuv_source(src, layout, src_bytes, F, H, W, &sv);
    if (rc != CC_OK) return rc;
    return cc_px::dispatch_yuv(layout->depth, layout->sub_x, layout->sub_y, [&](auto s) {
        return resize_crop_launch<decltype(s)::value>(src, sv, F, H, W, plan_dev, n_px, resize, dst, dst_fmt, ws, ws_bytes, stream);
    });
}

int cc_resize_crop_yuv420_u8(const void* src, size_t src_bytes, const cc_yuv420_layout* layout, int32_t F, int32_t H, int32_t W,
                             const void* plan_dev, int32_t n_px, int32_t resize, void* dst, int32_t dst_fmt, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!layout) return CC_ERR_INVALID;
    const cc_yuv_layout lay = cc_px::yuv420_layout(*layout);
    return cc_resize_crop_yuv_u8(src, src_bytes, &lay, F, H, W, plan_dev, n_px, resize, dst, dst_fmt, ws, ws_bytes, stream);
}

int cc_yuv_coefficients_depth(int32_t matrix, int32_t range, int32_t depth, int32_t* out5) {
    YuvCoef k;
    if (!out5 || !cc_px::yuv_coefficients(matrix, range, depth, &k)) return CC_ERR_INVALID;
    const int32_t v[5] = {k.cy, k.crv, k.cgu, k.cgv, k.cbu};
    for (int i = 0; i < 5; ++i) out5[i] = v[i];
    return CC_OK;
}

int cc_yuv_coefficients(int32_t matrix, int32_t range, int32_t* out5) { return cc_yuv_coefficients_depth(matrix, range, 8, out5); }

size_t cc_yuv_layout_tight(int32_t format, int32_t H, int32_t W, int32_t matrix, int32_t range, cc_yuv_layout* out) {
    YuvCoef k;
    YuvFormat f;
    if (!out || !cc_px::yuv_format(format, &f) || !cc_px::yuv_coefficients(matrix, range, f.depth, &k) || H < 1 || W < 1 ||
        H > 8192 || W > 8192)
        return 0;
    const PixelSource s = cc_px::yuv_tight_source(f, H, W, k);
    out->frame_stride = s.sf;
    out->y_pitch = s.sy;
    out->u_offset = s.u_off;
    out->v_offset = s.v_off;
    out->c_pitch = s.c_pitch;
    out->c_step = s.c_step;
    out->sub_x = f.sub_x;
    out->sub_y = f.sub_y;
    out->depth = f.depth;
    out->shift = f.shift;
    out->matrix = matrix;
    out->range = range;
    return (size_t)s.sf;
}

size_t cc_yuv420_layout_tight(int32_t kind, int32_t H, int32_t W, int32_t matrix, int32_t range, cc_yuv420_layout* out) {
    cc_yuv_layout g;
    if (!out || (kind != CC_YUV420_I420 && kind != CC_YUV420_NV12)) return 0;
    const size_t n = cc_yuv_layout_tight(kind, H, W, matrix, range, &g);       // (CC_YUV_I420 / _NV12 are the two kinds)
    if (!n) return 0;
    out->frame_stride = g.frame_stride;
    out->y_pitch = g.y_pitch;
    out->u_offset = g.u_offset;
    out->v_offset = g.v_offset;
    out->c_pitch = g.c_pitch;
    out->c_step = g.c_step;
    out->matrix = matrix;
    out->range = range;
    return n;
}

int cc_yuv_to_rgb_u8(const void* src, size_t src_bytes, const cc_yuv_layout* layout, int32_t F, int32_t H, int32_t W, void* dst,
                     int32_t dst_fmt, void* stream) {
    if (!src || !dst || !layout || F <= 0 || !u8_format(dst_fmt)) return CC_ERR_INVALID;
    PixelSource sv;
    const int rc = cc_px::yuv_source(src, layout, src_bytes, F, H, W, &sv);
    if (rc != CC_OK) return rc;
    return cc_px::dispatch_yuv(layout->depth, layout->sub_x, layout->sub_y, [&](auto s) {
        return to_rgb_launch<decltype(s)::value>(src, sv, F, H, W, dst, dst_fmt, stream);
    });
}

int cc_yuv420_to_rgb_u8(const void* src, size_t src_bytes, const cc_yuv420_layout* layout, int32_t F, int32_t H, int32_t W,
                        void* dst, int32_t dst_fmt, void* stream) {
    if (!layout) return CC_ERR_INVALID;
    const cc_yuv_layout lay = cc_px::yuv420_layout(*layout);
    return cc_yuv_to_rgb_u8(src, src_bytes, &lay, F, H, W, dst, dst_fmt, stream);
}

int cc_resize_crop_status(int32_t H, int32_t W, int32_t n_px, int32_t resize) {
    Geometry g;
    return geometry(H, W, n_px, resize, kMaxKsize, &g);
}

size_t cc_collate_resize_crop_workspace_bytes(const int64_t* clips_host, int32_t n_clips, int32_t n_out, int32_t n_px,
                                              int32_t resize) {
    if (!clips_host || n_clips <= 0 || n_out <= 0) return 0;
    size_t frame = 0;
    for (int i = 0; i < n_clips; ++i) {
        const size_t one = cc_resize_crop_workspace_bytes(1, (int32_t)clips_host[4 * i + 2], (int32_t)clips_host[4 * i + 3], n_px, resize);
        if (one > frame) frame = one;
    }
    return frame * (size_t)n_out;
}

}  // extern "C"

namespace {

// the checks and launches of cc_collate_resize_crop_u8 / _yuv_u8; fmt: the RGB format code, or yf: the tight YUV format
template <int SRC>
int collate_launch(const void* src, size_t src_bytes, int32_t fmt, const YuvFormat& yf, const YuvCoef& k, const int64_t* clips_host, int32_t n_clips,
                   const int64_t* rows_dev, int32_t n_out, const int32_t* plans_dev, size_t plans_ints, int32_t n_px,
                   int32_t resize, void* dst, int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream) {
    int rc = collate_check_clips<SRC>(clips_host, n_clips, src_bytes, yf);
    if (rc != CC_OK) return rc;
    int max_mid = 0;                                // rows of the largest horizontal result; 0: no clip runs both passes
    for (int i = 0; i < n_clips; ++i) {
        Geometry g;
        rc = geometry((int)clips_host[4 * i + 2], (int)clips_host[4 * i + 3], n_px, resize, kMaxKsize, &g);
        if (rc != CC_OK) return rc;
        if (g.ksize_h && g.ksize_v && g.row1 - g.row0 > max_mid) max_mid = g.row1 - g.row0;
    }
    if (max_mid && (!ws || ws_bytes < (size_t)3 * max_mid * n_px)) return CC_ERR_WORKSPACE;
    CollateArgs a;
    a.src = static_cast<const uint8_t*>(src);
    a.src_bytes = (int64_t)src_bytes;
    a.rows = rows_dev;
    a.plans = plans_dev;
    a.plans_ints = (int64_t)plans_ints;
    a.ws = static_cast<uint8_t*>(ws);
    a.ws_bytes = ws ? (int64_t)ws_bytes : 0;
    a.dst = static_cast<uint8_t*>(dst);
    a.n_out = n_out;
    a.n_px = n_px;
    a.resize = resize;
    a.fmt = fmt;
    a.dst_fmt = dst_fmt;
    a.yf = yf;
    a.k = k;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 block(kTileX, kTileY);
    const int tiles_x = (n_px + kTileX - 1) / kTileX, tiles_out = (n_px + kTileY - 1) / kTileY;
    if (max_mid) {
        const int tiles_mid = (max_mid + kTileY - 1) / kTileY;
        collate_resample_u8_kernel<false, SRC><<<dim3(tiles_x, tiles_mid, collate_planes(n_out, tiles_x, tiles_mid)), block, 0, st>>>(a);
        CC_LAUNCH_CHECK();
    }
    collate_resample_u8_kernel<true, SRC><<<dim3(tiles_x, tiles_out, collate_planes(n_out, tiles_x, tiles_out)), block, 0, st>>>(a);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // namespace

extern "C" {

int cc_collate_resize_crop_u8(const void* src, size_t src_bytes, int32_t fmt, const int64_t* clips_host, int32_t n_clips,
                              const int64_t* rows_dev, int32_t n_out, const int32_t* plans_dev, size_t plans_ints, int32_t n_px,
                              int32_t resize, void* dst, int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream) {
    if (!src || !dst || !rows_dev || !plans_dev || n_out <= 0 || !u8_format(fmt) || !u8_format(dst_fmt) ||
        plans_ints < CC_RESIZE_PLAN_HEADER)
        return CC_ERR_INVALID;
    return collate_launch<kRgb>(src, src_bytes, fmt, YuvFormat{}, YuvCoef{}, clips_host, n_clips, rows_dev, n_out, plans_dev, plans_ints, n_px,
                                 resize, dst, dst_fmt, ws, ws_bytes, stream);
}

int cc_collate_resize_crop_yuv_u8(const void* src, size_t src_bytes, int32_t format, int32_t matrix, int32_t range,
                                  const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out,
                                  const int32_t* plans_dev, size_t plans_ints, int32_t n_px, int32_t resize, void* dst,
                                  int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream) {
    YuvCoef k;
    YuvFormat yf;
    if (!src || !dst || !rows_dev || !plans_dev || n_out <= 0 || !cc_px::yuv_format(format, &yf) ||
        !cc_px::yuv_coefficients(matrix, range, yf.depth, &k) || !u8_format(dst_fmt) || plans_ints < CC_RESIZE_PLAN_HEADER)
        return CC_ERR_INVALID;
    if (yf.depth > 8 && ((uintptr_t)src & 1)) return CC_ERR_INVALID;
    return cc_px::dispatch_yuv(yf.depth, yf.sub_x, yf.sub_y, [&](auto s) {
        return collate_launch<decltype(s)::value>(src, src_bytes, 0, yf, k, clips_host, n_clips, rows_dev, n_out, plans_dev,
                                                  plans_ints, n_px, resize, dst, dst_fmt, ws, ws_bytes, stream);
    });
}

int cc_collate_resize_crop_yuv420_u8(const void* src, size_t src_bytes, int32_t kind, int32_t matrix, int32_t range,
                                     const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out,
                                     const int32_t* plans_dev, size_t plans_ints, int32_t n_px, int32_t resize, void* dst,
                                     int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream) {
    if (kind != CC_YUV420_I420 && kind != CC_YUV420_NV12) return CC_ERR_INVALID;
    return cc_collate_resize_crop_yuv_u8(src, src_bytes, kind, matrix, range, clips_host, n_clips, rows_dev, n_out, plans_dev,
                                         plans_ints, n_px, resize, dst, dst_fmt, ws, ws_bytes, stream);
}

}  // extern "C"
