// Host-side orchestration of the CLIP visual / text forward: one C call enqueues the whole
// encoder on a HIP stream (no host synchronisation, no allocation - the workspace is caller
// owned), so it can be captured into a hipGraph as is.
//
// Activations are frame-major ([frame, token, width], "NLD"): attention works on contiguous
// per-frame rows and the token-cluster op reads/writes the same buffer through strides.
// Reference call stack: CLIP.encode_image -> VisualTransformer.forward -> Transformer ->
// ResidualAttentionBlock.forward (modules/clip.py:460-469, 304-349, 256-269, 228-253).
#include "cc_kernels.h"
#include <cstdlib>
#include <cstdint>
#include <utility>

namespace {

struct TowerActs {         // one tower's activations
    float* h;              // residual stream (frame-major)
    _Float16* h16;         // fp16 copy of the residual stream (GEMM A operand; LayerNorm is folded into the GEMM)
    float *st0, *st1;      // partial (sum, sumsq) of the rows entering in_proj / c_fc  [M][CC_LN_MAX_SLOTS][2]
    float *sh0, *sh1;      // per-row constant the fp16 copy entering in_proj / c_fc was centred on  [M]
    _Float16 *qkv, *att, *u;
};

TowerActs carve_acts(Carver& c, size_t rows, size_t W) {
    TowerActs a{};
    a.h = c.take<float>(rows * W);
    a.h16 = c.take<_Float16>(rows * W);
    a.st0 = c.take<float>(rows * CC_LN_MAX_SLOTS * 2);
    a.st1 = c.take<float>(rows * CC_LN_MAX_SLOTS * 2);
    a.sh0 = c.take<float>(rows);
    a.sh1 = c.take<float>(rows);
    a.qkv = c.take<_Float16>(rows * 3 * W);
    a.att = c.take<_Float16>(rows * W);
    a.u = c.take<_Float16>(rows * 4 * W);
    return a;
}

// The cluster plan of a visual tower, block by block: which blocks run a token op in front of their attention and how the
// frame / token counts change along the layers.  Everything that needs the plan (scratch sizing, the forced-medoids
// count, the encoder itself) walks it through this one iterator.
enum ClusterKind { CK_MEDOIDS, CK_POOLING, CK_SPARSE, CK_SHIFT };   // k-medoids / spectral; pooling; sparse sampling (and ids the
                                                                    // cluster op itself refuses); temporal / token shift
const cc_cluster_variant kDefaultVariant{CC_CLUSTER_KMEDOIDS, CC_AGGREGATE_MEDOID};
struct ClusterStep {
    int block, kind;
    const cc_cluster_variant* var;     // the block's variant, or the default (k-medoids, medoid aggregation)
    int frames_in, tokens_in;
    int frames_out, tokens_out;        // as the plan states them (a shift block must state the incoming ones)
    bool ok;                           // frames_out divides frames_in (shift: both counts unchanged); the walk advances only then
};
struct ClusterPlan {
    const cc_vit_model* m;
    int frames, tokens;                // entering the next block
    // block i, called for i = 0, 1, ... in order: false = no token op in front of it
    bool step(int i, ClusterStep* s) {
        if (m->cluster_tokens[i] <= 0) return false;
        const cc_cluster_variant* var = m->cluster_variants ? &m->cluster_variants[i] : &kDefaultVariant;
        const int a = var->algorithm;
        const int kind = (a == CC_CLUSTER_TEMPORAL_SHIFT || a == CC_CLUSTER_TOKEN_SHIFT) ? CK_SHIFT
                         : (a == CC_CLUSTER_KMEDOIDS || a == CC_CLUSTER_SPECTRAL) ? CK_MEDOIDS
                         : a == CC_CLUSTER_POOLING ? CK_POOLING : CK_SPARSE;
        *s = ClusterStep{i, kind, var, frames, tokens, m->cluster_frames[i], m->cluster_tokens[i], false};
        s->ok = kind == CK_SHIFT ? (s->frames_out == frames && s->tokens_out == tokens)
                                 : (s->frames_out > 0 && frames % s->frames_out == 0);
        if (s->ok) { frames = s->frames_out; tokens = s->tokens_out; }
        return true;
    }
};

struct VitWs {
    _Float16* im2col;
    TowerActs a;
    float* h2;       // cluster output (ping-pong with a.h)
    void* cluster;
    size_t cluster_bytes, total;
};

VitWs carve_vit(const cc_vit_model* m, int B, int T, void* ws) {
    VitWs v{};
    Carver c(ws);
    const int g = m->resolution / m->patch, n = g * g, L0 = n + 1, W = m->width;
    const size_t F = (size_t)B * T, M0 = F * L0;
    v.im2col = c.take<_Float16>(F * n * (m->conv2_weight_f16 ? (size_t)9 * m->patch * m->patch : (size_t)cc_patch_cols(m->patch)));
    v.a = carve_acts(c, M0, W);
    v.h2 = c.take<float>(M0 * W);
    // cluster scratch: worst case over the plan (a block whose T_new does not divide the frame count is skipped)
    size_t cb = 0;
    ClusterPlan plan{m, T, n};
    ClusterStep s;
    for (int i = 0; i < m->layers; ++i) {
        if (!plan.step(i, &s) || s.kind == CK_SHIFT || !s.ok) continue;
        const int P = B * s.frames_out, N = (s.frames_in / s.frames_out) * s.tokens_in;
        size_t need = cc_cluster_workspace_bytes(P, N, W, m->cluster_pre_norm);
        if (s.var->algorithm == CC_CLUSTER_SPECTRAL) need += cc_spectral_workspace_bytes(P, N, s.tokens_out);
        cb = need > cb ? need : cb;
    }
    v.cluster_bytes = cb;
    v.cluster = c.take<char>(cb);
    v.total = c.off;
    return v;
}

struct BlockCtx {          // one tower's activations for the current block
    TowerActs a;           // (visual tower: a.h changes sides of the ping-pong behind a cluster step)
    int nseq, L, W, heads, causal;
    int slots0, slots1;    // partial-sum slots per row currently held in st0 / st1
    // compacted captions (text tower): device-side row count and per-caption (offset, length); null = dense [nseq, L]
    const int *m_dev, *seq_off, *seq_len;
    // Last block of a tower when nobody asked for the hidden state: only sel_rows rows feed the projection head (row
    // m -> sel_map ? sel_map[m] : m * sel_step), so everything after the attention runs on those rows in place
    int sel_rows, sel_step;
    const int* sel_map;
    // token_shift (clip.py:246-248): the CLS rows are shifted again between the out_proj residual and ln_2 - mode
    // CC_CLUSTER_TOKEN_SHIFT, segment, fold divisor; mid_shift 0 = none
    int mid_shift, mid_seg, mid_div;
    int act;               // CC_ACT_*: the activation behind c_fc (the model's)
};
// the c_fc epilogue of an activation
int c_fc_epi(int act) { return act == CC_ACT_GELU ? EPI_F16_GELU_ERF_LN : EPI_F16_GELU_LN; }
bool act_ok(int act) { return act == CC_ACT_QUICK_GELU || act == CC_ACT_GELU; }

// One set of row statistics of a tower: st0 / sh0 / slots0 (the rows entering in_proj) or st1 / sh1 / slots1 (entering c_fc)
struct RowStats { float* st; float* sh; int slots; };

// The GEMM of one phase of a block for one tower.  `in`: the statistics it consumes - a folded LayerNorm (in_proj, c_fc) reads
// the row sums, a residual phase (out_proj, c_proj) re-centres the fp16 copy on them; `out`: where a residual phase leaves
// those of the rows it writes.  The phases behind the attention run on every row, or on the rows the head will read
// (GemmArgs::row_step / row_map, the few-rows kernel).  fused (in_proj only): the attention of the sequences in the epilogue.
enum Phase { IN_PROJ, OUT_PROJ, C_FC, C_PROJ };
GemmArgs phase_args(const cc_block_weights& w, const BlockCtx& c, Phase ph, RowStats in, RowStats out, bool fused = false) {
    const int W = c.W;
    GemmArgs g{};
    g.M = c.nseq * c.L; g.m_dev = c.m_dev; g.ln_eps = 1e-5f;
    auto set = [&g](const _Float16* A, const void* Wt, const float* bias, const float* c1, void* C, int N, int K) {
        g.A = A; g.W = static_cast<const _Float16*>(Wt); g.bias = bias; g.ln_c1 = c1; g.C = C; g.N = g.ldc = N; g.K = K;
    };
    switch (ph) {
        case IN_PROJ: set(c.a.h16, w.in_proj_ln_weight_f16, w.in_proj_ln_c2, w.in_proj_ln_c1, c.a.qkv, 3 * W, W); break;
        case OUT_PROJ: set(c.a.att, w.out_proj_weight_f16, w.out_proj_bias, nullptr, c.a.h, W, W); break;
        case C_FC: set(c.a.h16, w.c_fc_ln_weight_f16, w.c_fc_ln_c2, w.c_fc_ln_c1, c.a.u, 4 * W, W); break;
        case C_PROJ: set(c.a.u, w.c_proj_weight_f16, w.c_proj_bias, nullptr, c.a.h, W, 4 * W); break;
    }
    if (ph == IN_PROJ || ph == C_FC) {
        g.ln_stats = in.st; g.ln_slots = in.slots;
    } else {
        g.c16 = c.a.h16; g.stats_out = out.st;
        g.shift_in = in.sh; g.shift_stats = in.st; g.shift_slots = in.slots; g.shift_out = out.sh;
    }
    if (ph != IN_PROJ && c.sel_rows > 0) { g.M = c.sel_rows; g.m_dev = nullptr; g.row_step = c.sel_step; g.row_map = c.sel_map; }
    if (fused) {
        g.C = c.a.att; g.ldc = W;
        g.att_L = c.L; g.att_nseq = c.nseq; g.att_causal = c.causal; g.att_seq_off = c.seq_off; g.att_seq_len = c.seq_len;
    }
    return g;
}

// One launch for up to two problems with the same epilogue: both tiled, or both on selected rows (rows0 / rows1: the few-rows
// kernel).  A tower whose partner is not in the same mode gets a launch of its own, problem 0 first; `apart` asks for that for a
// tiled pair too.  sl (optional, [2]): the slot counts the problems wrote, as cc_gemm_dispatch2 reports them.
int launch_pair(const GemmArgs& g0, const GemmArgs* g1, bool rows0, bool rows1, bool apart, int epi, hipStream_t st, int* sl) {
    if (!g1 || (rows0 == rows1 && (rows0 || !apart)))
        return rows0 ? cc_gemm_rows_dispatch2(g0, g1, epi, st, sl) : cc_gemm_dispatch2(g0, g1, epi, 0, st, sl);
    int a[2] = {0, 0}, b[2] = {0, 0};
    int r = launch_pair(g0, nullptr, rows0, false, false, epi, st, sl ? a : nullptr);
    if (r) return r;
    r = launch_pair(*g1, nullptr, rows1, false, false, epi, st, sl ? b : nullptr);
    if (sl) { sl[0] = a[0]; sl[1] = b[0]; }
    return r;
}

// One ResidualAttentionBlock for up to two towers at once (modules/clip.py:240,251).  Every phase is
// ONE launch covering both problems: the text tower (M = 16*32 rows, launch-latency bound on its own:
// 86 kernels of a few microseconds) rides inside the visual tower's launches and fills their tail round.
// LayerNorm never runs as a pass of its own: ln_1 / ln_2 are folded into in_proj / c_fc (the row statistics
// come out of the preceding residual epilogue), which removes two full reads of the fp32 residual stream
// and two launches per block.
int run_block_pair(const cc_block_weights* w0, BlockCtx* c0, const cc_block_weights* w1, BlockCtx* c1,
                   hipStream_t st) {
    if (!w0) { w0 = w1; c0 = c1; w1 = nullptr; c1 = nullptr; }
    int rc, slots[2];
    // experiment knob (development builds, -DCC_DEV_KNOBS): CC_UNPAIR bit mask (1 in_proj, 2 out_proj, 4 c_fc, 8 c_proj) - the clustered visual blocks launch
    // those phases separately for the two towers
#ifdef CC_DEV_KNOBS
    static const int unpair_mask = [] { const char* e = getenv("CC_UNPAIR"); return e ? atoi(e) : 0; }();
#else
    constexpr int unpair_mask = 0;
#endif
    const int unpair = (c1 && c0->nseq * c0->L < CC_BIG_CARRIER_ROWS) ? unpair_mask : 0;
    // The slot hand-over between the phases: set 0 (st0, sh0, slots0) describes the rows entering in_proj, set 1 (st1, sh1,
    // slots1) those entering c_fc; a residual phase reads one set and writes the other, its launch reports the new slot count
    auto set0 = [](const BlockCtx* c) { return RowStats{c->a.st0, c->a.sh0, c->slots0}; };
    auto set1 = [](const BlockCtx* c) { return RowStats{c->a.st1, c->a.sh1, c->slots1}; };
    auto none = [](const BlockCtx*) { return RowStats{}; };
    GemmArgs g0{}, g1{};
    auto build = [&](Phase ph, auto in, auto out, bool fused = false) {
        g0 = phase_args(*w0, *c0, ph, in(c0), out(c0), fused);
        if (c1) g1 = phase_args(*w1, *c1, ph, in(c1), out(c1), fused);
    };
    // the phases behind the attention, on the rows each tower selected (if any); bit: this phase's place in CC_UNPAIR
    auto tail_launch = [&](int epi, int bit, int* sl) {
        return launch_pair(g0, c1 ? &g1 : nullptr, c0->sel_rows > 0, c1 && c1->sel_rows > 0, unpair & bit, epi, st, sl);
    };
    // ---- q,k,v = in_proj(ln_1(x))   [LayerNorm folded]  and  attn = softmax(q k^T / 8) v      reads set 0
    // One launch where the sequences fit a row tile (L <= 56: the ViT-B/32 frames, every clustered block, the captions): a
    // workgroup owns whole sequences x one head and keeps their q, k, v in LDS (EPI_ATTN_LN); otherwise in_proj writes qkv
    // and the attention kernel reads it back.
    build(IN_PROJ, set0, none, true);
    if (!(unpair & 1) && c0->heads * 64 == c0->W && (!c1 || c1->heads * 64 == c1->W) && cc_gemm_attn_applies(g0, c1 ? &g1 : nullptr)) {
        rc = cc_gemm_attn_dispatch2(g0, c1 ? &g1 : nullptr, st);
        if (rc) return rc;
    } else {
        build(IN_PROJ, set0, none);
        rc = launch_pair(g0, c1 ? &g1 : nullptr, false, false, unpair & 1, EPI_F16_LN, st, nullptr);
        if (rc) return rc;
        auto att = [](const BlockCtx* c) {
            return AttArgs{c->a.qkv, c->a.att, c->nseq, c->L, c->heads, c->W, c->causal, 0, 0, c->seq_off, c->seq_len};
        };
        const AttArgs a0 = att(c0), a1 = c1 ? att(c1) : AttArgs{};
        rc = cc_launch_attention2(a0, c1 ? &a1 : nullptr, st);
        if (rc) return rc;
    }
    // ---- x = x + out_proj(attn)   [+ fp16 copy and row statistics for ln_2]      reads set 0, writes set 1
    build(OUT_PROJ, set0, set1);
    rc = tail_launch(EPI_F32_RESID_STATS, 2, slots);
    if (rc) return rc;
    c0->slots1 = slots[0];
    if (c1) c1->slots1 = slots[1];
    // ---- token_shift: x = S(x) on the CLS rows (the rows a last block with sel_rows computed), + their fp16 copy and
    // statistics for ln_2 in the slot layout out_proj left
    for (BlockCtx* c : {c0, c1}) {
        if (!c || !c->mid_shift) continue;
        rc = cc_token_shift_rows_f32(c->a.h, 1, c->L, c->nseq, c->L, c->W, c->mid_seg, c->mid_div, c->mid_shift, c->a.h16, c->a.st1,
                                     c->slots1, c->a.sh1, st);
        if (rc) return rc;
    }
    // ---- u = act(c_fc(ln_2(x)))   [LayerNorm folded]      reads set 1       act: QuickGELU, or the model's exact GELU
    // (the epilogue is a template argument of the launch: two towers with different activations launch apart)
    build(C_FC, set1, none);
    if (c1 && c0->act != c1->act) {
        rc = launch_pair(g0, nullptr, c0->sel_rows > 0, false, false, c_fc_epi(c0->act), st, nullptr);
        if (rc) return rc;
        rc = launch_pair(g1, nullptr, c1->sel_rows > 0, false, false, c_fc_epi(c1->act), st, nullptr);
    } else {
        rc = tail_launch(c_fc_epi(c0->act), 4, nullptr);
    }
    if (rc) return rc;
    // ---- x = x + c_proj(u)   [+ fp16 copy and row statistics for the next block's ln_1]      reads set 1, writes set 0
    build(C_PROJ, set1, set0);
    rc = tail_launch(EPI_F32_RESID_STATS, 8, slots);
    if (rc) return rc;
    c0->slots0 = slots[0];
    if (c1) c1->slots0 = slots[1];
    return CC_OK;
}

struct TextWs {
    TowerActs a;
    int* eot;
    int* seq_off;    // compacted captions: first row of caption b
    int* seq_len;    //                      its length (EOT position + 1)
    int* mcount;     //                      total number of kept rows
    size_t total;
};

TextWs carve_text(const cc_text_model* m, int Bt, int Lt, void* ws) {
    TextWs t{};
    Carver c(ws);
    t.a = carve_acts(c, (size_t)Bt * Lt, m->width);
    t.eot = c.take<int>(Bt);
    t.seq_off = c.take<int>(Bt);
    t.seq_len = c.take<int>(Bt);
    t.mcount = c.take<int>(1);
    t.total = c.off;
    return t;
}

bool vit_ok(const cc_vit_model* m) {
    if (m->layers <= 0 || m->layers > CC_MAX_LAYERS || m->width != m->heads * 64) return false;
    if (m->patch <= 0 || m->resolution % m->patch || (m->width % 64)) return false;
    return !(m->conv2_weight_f16 && (m->patch & 7));           // linear_patch '3d': the 8-wide gather only
}

bool text_ok(const cc_text_model* m, int Lt) {
    return m->layers > 0 && m->layers <= CC_MAX_LAYERS && m->width == m->heads * 64 && Lt <= m->context_length;
}

// What a call asks of a tower.  stop >= 0 (cc_*_encode_prefix*): the tower stops behind that many blocks and hands over its
// residual stream (hidden_out) - no projection head; the last block it runs computes every row, the caller reads them
struct VisualReq {
    const cc_vit_model* m; const cc_frames* frames; int B, T;
    float* features; float* hidden_out; int64_t* medoids_out; const int64_t* forced_medoids; int stop = -1;
};
struct TextReq {
    const cc_text_model* m; const int64_t* ids; int Bt, Lt;
    float* features; float* hidden_out; int stop = -1;
};

// patch embedding: conv1 as im2col GEMM, + positional embedding (the CLS row and ln_pre follow in the pre-stage; clip.py:324-338)
int patch_embed(const VisualReq& r, const VitWs& v, hipStream_t st) {
    const cc_vit_model* vm = r.m;
    const int g = vm->resolution / vm->patch, n = g * g, F = r.B * r.T;
    const bool patch3d = vm->conv2_weight_f16 != nullptr;      // linear_patch '3d' (clip.py:306-317)
    int rc = patch3d ? cc_launch_im2col3d(*r.frames, v.im2col, F, r.T, vm->resolution, vm->patch, st)
                     : cc_launch_im2col_any(*r.frames, v.im2col, F, vm->resolution, vm->patch, st);
    if (rc) return rc;
    GemmArgs ga{};
    ga.A = v.im2col;
    ga.W = static_cast<const _Float16*>(patch3d ? vm->conv2_weight_f16 : vm->conv1_weight_f16);
    ga.C = v.a.h;
    ga.pos = vm->positional_embedding;
    ga.M = F * n; ga.N = vm->width; ga.K = patch3d ? 9 * vm->patch * vm->patch : cc_patch_cols(vm->patch); ga.ldc = vm->width;
    ga.patch_n = n;
    return cc_gemm_dispatch(ga, EPI_F32_PATCH, 0, st);
}

// ln_pre in place (fp32; the CLS rows = class_embedding + positional_embedding[0] are formed inside) + fp16 copy +
// row statistics for block 1's folded ln_1, and the text embedding with the same by-products - one launch
int pre_stage(const VisualReq* vr, const VitWs& v, const BlockCtx& cv, const TextReq* tr, const TextWs& t, bool compact,
              hipStream_t st) {
    LnArgs a{};
    TextEmbedArgs te{};
    if (vr)
        a = LnArgs{v.a.h, cv.W, vr->m->ln_pre_weight, vr->m->ln_pre_bias, v.a.h, cv.W, cv.nseq * cv.L, cv.W, v.a.h16, v.a.st0,
                   v.a.sh0, vr->m->class_embedding, vr->m->positional_embedding, cv.L};
    if (tr)
        te = TextEmbedArgs{reinterpret_cast<const long long*>(tr->ids), tr->m->token_embedding, tr->m->positional_embedding,
                           t.a.h, t.eot, tr->Bt, tr->Lt, tr->m->width, t.a.h16, t.a.st0, t.a.sh0,
                           compact ? t.seq_off : nullptr, compact ? t.seq_len : nullptr, compact ? t.mcount : nullptr,
                           tr->m->vocab_size};
    return (vr && tr) ? cc_launch_pre_stage(a, te, 1e-5f, st)
                      : vr ? cc_launch_layernorm2(a, nullptr, 1e-5f, 0, st) : cc_launch_text_embed(te, st);
}

// The token op in front of a block's ln_1 (clip.py:236-242): a shift in place, or a cluster step into `spare`, which then
// becomes the residual stream (every launch also writes the fp16 copy + row statistics of the rows ln_1 will read).
// forced: the ids of this block (null = the block picks its own); medoids_out: where to leave them (may be null)
int token_op(const VisualReq& r, const VitWs& v, const ClusterStep& s, const int64_t* forced, int64_t* medoids_out, BlockCtx& cv,
             float*& spare, hipStream_t st) {
    const cc_vit_model* vm = r.m;
    const cc_cluster_variant* var = s.var;
    const int B = r.B, W = cv.W, frames = s.frames_in, tokens = s.tokens_in, Tn = s.frames_out, K = s.tokens_out;
    if (!s.ok) return CC_ERR_INVALID;
    int rc;
    if (s.kind == CK_SHIFT) {                 // temporal / token shift: frames and tokens stay
        if (var->shift_segment <= 0 || (B * frames) % var->shift_segment || var->shift_fold_div <= 0) return CC_ERR_INVALID;
        // temporal_shift rewrites every row's statistics (one slot); token_shift the CLS rows' in the current layout
        const bool temporal = var->algorithm == CC_CLUSTER_TEMPORAL_SHIFT;
        rc = cc_token_shift_rows_f32(cv.a.h, 1, tokens + 1, B * frames, tokens + 1, W, var->shift_segment, var->shift_fold_div,
                                     var->algorithm, cv.a.h16, cv.a.st0, temporal ? 1 : cv.slots0, cv.a.sh0, st);
        if (temporal) cv.slots0 = 1;
        else cv.mid_shift = CC_CLUSTER_TOKEN_SHIFT, cv.mid_seg = var->shift_segment, cv.mid_div = var->shift_fold_div;
        return rc;
    }
    if (s.kind == CK_POOLING && K != tokens) return CC_ERR_INVALID;
    TokenClusterReq rq{};
    rq.in = TokenIn{cv.a.h, W, (int64_t)(tokens + 1) * W};
    rq.out = TokenOut{spare, W, (int64_t)(K + 1) * W};
    rq.g = TokenGeom{B, frames, Tn, tokens, W, K};
    rq.h16 = cv.a.h16; rq.stats = cv.a.st0; rq.shift = cv.a.sh0;
    rq.metric = vm->cluster_metric; rq.norm_p = vm->cluster_norm_p; rq.threshold = vm->cluster_threshold;
    rq.iter_limit = vm->cluster_iter_limit; rq.split_size = vm->cluster_split_size; rq.pre_norm = vm->cluster_pre_norm;
    rq.var = var; rq.medoids = medoids_out;
    rq.ws = v.cluster; rq.ws_bytes = v.cluster_bytes;
    if (!forced)
        rc = cc_token_cluster_variant_rows(rq, st);
    else if (var->algorithm == CC_CLUSTER_KMEDOIDS && var->aggregation == CC_AGGREGATE_MEDOID && !var->cluster_embed &&
             !var->cls_multiplier)
        rc = cc_token_gather_rows(TokenGatherReq{rq, forced}, st);
    else
        rc = CC_ERR_UNSUPPORTED;
    if (rc) return rc;
    if (var->mean_residual) {
        // clip.py:239-242: x = res_x + attention(ln_1(x')) - ln_1 reads the clustered rows (their fp16 copy and
        // statistics are written), the fp32 residual stream restarts from the frame means of every token
        if (K != tokens) return CC_ERR_INVALID;                 // cluster.py:229
        cc_cluster_variant pool{};
        pool.algorithm = CC_CLUSTER_POOLING;
        rq.var = &pool; rq.medoids = nullptr;
        rq.h16 = nullptr; rq.stats = nullptr; rq.shift = nullptr;
        rc = cc_token_cluster_variant_rows(rq, st);
        if (rc) return rc;
    }
    std::swap(cv.a.h, spare);
    cv.nseq = B * Tn; cv.L = K + 1;
    cv.slots0 = 1;
    return CC_OK;
}

// Both towers, block i of the one paired with block i of the other (either may be absent).
int encode_towers(const VisualReq* vr, const TextReq* tr, void* ws, size_t ws_bytes, hipStream_t st) {
    const cc_vit_model* vm = vr ? vr->m : nullptr;
    const cc_text_model* tm = tr ? tr->m : nullptr;
    VitWs v{};
    TextWs t{};
    size_t off = 0;
    if (vr) { v = carve_vit(vm, vr->B, vr->T, ws); off = v.total; }
    if (tr) { t = carve_text(tm, tr->Bt, tr->Lt, static_cast<char*>(ws) + off); off += t.total; }
    if (!ws || ws_bytes < off) return CC_ERR_WORKSPACE;
    int rc = CC_OK;
    const int vl = vr ? (vr->stop >= 0 ? vr->stop : vm->layers) : 0, tl = tr ? (tr->stop >= 0 ? tr->stop : tm->layers) : 0;
    const bool prefix = (vr && vr->stop >= 0) || (tr && tr->stop >= 0);
    // Caption compaction (see TextEmbedArgs): the text tower runs on the rows up to each caption's EOT only - the launches
    // are sized for Bt * Lt rows, the kernels read the real count from the device, so nothing synchronises and a
    // captured graph stays valid for any batch.  Off when the caller wants the full hidden state.
    const bool compact = tr && !tr->hidden_out && tr->Bt <= 256 && !(tm->row_policy & CC_ROWS_ALL_TEXT);
    BlockCtx cv{}, ct{};
    cv.slots0 = ct.slots0 = 1;
    if (tr) {
        ct.a = t.a;
        ct.nseq = tr->Bt; ct.L = tr->Lt; ct.W = tm->width; ct.heads = tm->heads; ct.causal = 1; ct.act = tm->activation;
        if (compact) { ct.m_dev = t.mcount; ct.seq_off = t.seq_off; ct.seq_len = t.seq_len; }
    }
    float* spare = v.h2;           // the side of the visual ping-pong the next cluster step writes
    if (vr) {
        const int g = vm->resolution / vm->patch;
        cv.a = v.a;
        cv.nseq = vr->B * vr->T; cv.L = g * g + 1; cv.W = vm->width; cv.heads = vm->heads; cv.causal = 0; cv.act = vm->activation;
        rc = patch_embed(*vr, v, st);
        if (rc) return rc;
    }
    rc = pre_stage(vr, v, cv, tr, t, compact, st);
    if (rc) return rc;
    // medoids_out receives the ids of the LAST k-medoids block only (it is sized for that block); forced_medoids holds the id
    // tensors of ALL cluster blocks back to back, in block order ([B * T_new_i, K_i] int64 each: round 5 - one block before)
    ClusterPlan plan{vm, vr ? vr->T : 0, cv.L - 1}, scan = plan;
    ClusterStep s;
    int last_kmed = -1;
    for (int i = 0; i < vl; ++i)
        if (scan.step(i, &s) && s.kind == CK_MEDOIDS) last_kmed = i;
    size_t forced_off = 0;      // first id of the current cluster block inside forced_medoids
    int ti = 0;                 // next text block
    for (int i = 0; i < vl || ti < tl; ++i) {
        const bool hv = i < vl;
        if (hv) {
            cv.mid_shift = 0;
            if (plan.step(i, &s)) {
                rc = token_op(*vr, v, s, vr->forced_medoids ? vr->forced_medoids + forced_off : nullptr,
                              i == last_kmed ? vr->medoids_out : nullptr, cv, spare, st);
                if (rc) return rc;
                if (s.kind != CK_SHIFT) forced_off += (size_t)vr->B * s.frames_out * s.tokens_out;
            }
        }
        const bool ht = ti < tl;
        // last block, nobody wants the hidden state: everything behind the attention on the CLS / EOT rows only
        auto few_rows_ok = [](int Wd, int act) {
            return cc_gemm_rows_ok(Wd, Wd, EPI_F32_RESID_STATS) && cc_gemm_rows_ok(4 * Wd, Wd, c_fc_epi(act)) &&
                   cc_gemm_rows_ok(Wd, 4 * Wd, EPI_F32_RESID_STATS);
        };
        if (hv && i == vl - 1 && !vr->hidden_out && !(vm->row_policy & CC_ROWS_ALL_LAST_BLOCK) && cv.L > 1 && few_rows_ok(cv.W, cv.act)) {
            cv.sel_rows = cv.nseq;
            cv.sel_step = cv.L;
        }
        if (ht && ti == tl - 1 && compact && !(tm->row_policy & CC_ROWS_ALL_LAST_BLOCK) && few_rows_ok(tm->width, ct.act)) {
            ct.sel_rows = tr->Bt;
            ct.sel_map = t.eot;
        }
        rc = run_block_pair(hv ? &vm->blocks[i] : nullptr, hv ? &cv : nullptr, ht ? &tm->blocks[ti] : nullptr,
                            ht ? &ct : nullptr, st);
        if (rc) return rc;
        if (ht) ++ti;
    }
    // ln_post + proj on the CLS rows only (clip.py:463-464); ln_final + text_projection on the EOT rows only
    // (clip.py:480-484) - one launch for both heads
    if (!prefix) {
        HeadArgs hv{}, ht{};
        if (vr) hv = HeadArgs{cv.a.h, cv.L, nullptr, vm->ln_post_weight, vm->ln_post_bias, vm->proj, vr->features, cv.nseq, cv.W, vm->embed_dim};
        // (compacted captions: eot[b] is already the absolute row of the EOT token)
        if (tr) ht = HeadArgs{t.a.h, compact ? 0 : tr->Lt, t.eot, tm->ln_final_weight, tm->ln_final_bias, tm->text_projection, tr->features, tr->Bt, tm->width, tm->embed_dim};
        rc = cc_launch_head_project2(vr ? hv : ht, (vr && tr) ? &ht : nullptr, st);
        if (rc) return rc;
    }
    if (vr && vr->hidden_out && hipMemcpyAsync(vr->hidden_out, cv.a.h, (size_t)cv.nseq * cv.L * cv.W * sizeof(float),
                                               hipMemcpyDeviceToDevice, st) != hipSuccess)
        return CC_ERR_HIP;
    if (tr && tr->hidden_out && hipMemcpyAsync(tr->hidden_out, t.a.h, (size_t)tr->Bt * tr->Lt * tm->width * sizeof(float),
                                               hipMemcpyDeviceToDevice, st) != hipSuccess)
        return CC_ERR_HIP;
    return CC_OK;
}

}  // namespace

extern "C" {

size_t cc_vit_workspace_bytes(const cc_vit_model* m, int32_t B, int32_t T) {
    if (!m || B <= 0 || T <= 0 || m->patch <= 0 || m->resolution % m->patch) return 0;
    return carve_vit(m, B, T, nullptr).total;
}

int64_t cc_vit_forced_medoids_count(const cc_vit_model* m, int32_t B) {
    if (!m || B <= 0 || m->layers < 0 || m->layers > CC_MAX_LAYERS) return CC_ERR_INVALID;
    int64_t n = 0;
    ClusterPlan plan{m, 0, 0};          // the counts as the plan states them: nothing is validated here
    ClusterStep s;
    for (int i = 0; i < m->layers; ++i)
        if (plan.step(i, &s) && s.kind != CK_SHIFT) n += (int64_t)B * s.frames_out * s.tokens_out;
    return n;
}

int cc_vit_encode_frames(const cc_vit_model* m, const cc_frames* frames, int32_t B, int32_t T, float* features,
                         float* hidden_out, int64_t* medoids_out, const int64_t* forced_medoids, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!m || !frames || !frames->data || !features || !m->blocks || B <= 0 || T <= 0) return CC_ERR_INVALID;
    if (!act_ok(m->activation)) return CC_ERR_INVALID;
    if (!vit_ok(m)) return CC_ERR_UNSUPPORTED;
    const VisualReq vr{m, frames, B, T, features, hidden_out, medoids_out, forced_medoids};
    return encode_towers(&vr, nullptr, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

// The patch gathers read uint8 frames in 8-byte pieces and fp32 frames as float4: a base address off that grid is refused.
// A patch size off the 8-wide grid (im2col_any_kernel) loads sample by sample: any uint8 address, any float address.
static bool frames_base_ok(const cc_frames* fr, int patch = 8) {
    if (patch & 7) {
        if (fr->format == CC_FRAMES_U8_CHW || fr->format == CC_FRAMES_U8_HWC) return true;
        return fr->format == CC_FRAMES_F32_CHW && (reinterpret_cast<uintptr_t>(fr->data) & 3) == 0;
    }
    if (fr->format == CC_FRAMES_U8_CHW || fr->format == CC_FRAMES_U8_HWC) return (reinterpret_cast<uintptr_t>(fr->data) & 7) == 0;
    return fr->format == CC_FRAMES_F32_CHW && (reinterpret_cast<uintptr_t>(fr->data) & 15) == 0;
}

int cc_vit_encode_prefix_frames(const cc_vit_model* m, const cc_frames* frames, int32_t B, int32_t T, int32_t n_blocks,
                                float* hidden_out, const int64_t* forced_medoids, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !frames || !frames->data || !hidden_out || B <= 0 || T <= 0) return CC_ERR_INVALID;
    if (n_blocks < 0 || n_blocks > m->layers || (n_blocks > 0 && !m->blocks)) return CC_ERR_INVALID;
    if (!act_ok(m->activation)) return CC_ERR_INVALID;
    if (!vit_ok(m)) return CC_ERR_UNSUPPORTED;
    if (!frames_base_ok(frames, m->patch)) return CC_ERR_INVALID;
    const VisualReq vr{m, frames, B, T, nullptr, hidden_out, nullptr, forced_medoids, n_blocks};
    return encode_towers(&vr, nullptr, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int cc_patch_gather_f16(const cc_frames* frames, int32_t F, int32_t resolution, int32_t patch, void* out_f16, void* stream) {
    if (!frames || !frames->data || !out_f16 || F <= 0 || patch <= 0 || resolution <= 0) return CC_ERR_INVALID;
    if ((patch & 7) || resolution % patch || !frames_base_ok(frames)) return CC_ERR_INVALID;
    return cc_launch_im2col(*frames, static_cast<_Float16*>(out_f16), F, resolution, patch, static_cast<hipStream_t>(stream));
}

// The patch gather of the encoders for ANY patch size that divides the resolution: out [F * g * g][roundup(3 p^2, 64)] fp16,
// columns (c, kh, kw), columns >= 3 p^2 zero.  p % 8 == 0: cc_patch_gather_f16 itself (same kernels, same bits, same base
// alignment rule); otherwise frames may start at any element.
int cc_patch_gather_any_f16(const cc_frames* frames, int32_t F, int32_t resolution, int32_t patch, void* out_f16, void* stream) {
    if (!frames || !frames->data || !out_f16 || F <= 0 || patch <= 0 || resolution <= 0) return CC_ERR_INVALID;
    if (resolution % patch || !frames_base_ok(frames, patch)) return CC_ERR_INVALID;
    return cc_launch_im2col_any(*frames, static_cast<_Float16*>(out_f16), F, resolution, patch, static_cast<hipStream_t>(stream));
}

// linear_patch '3d': the gathers of the fused forward (im2col3d_f16_kernel, the P3D strip gather) on their own
int cc_patch_gather3d_f16(const cc_frames* frames, int32_t F, int32_t T, int32_t resolution, int32_t patch, void* out_f16,
                          void* stream) {
    if (!frames || !frames->data || !out_f16 || F <= 0 || T <= 0 || patch <= 0 || resolution <= 0) return CC_ERR_INVALID;
    if ((patch & 7) || resolution % patch || F % T || !frames_base_ok(frames)) return CC_ERR_INVALID;
    return cc_launch_im2col3d(*frames, static_cast<_Float16*>(out_f16), F, T, resolution, patch, static_cast<hipStream_t>(stream));
}

int cc_vit_encode(const cc_vit_model* m, const float* video, int32_t B, int32_t T, float* features,
                  float* hidden_out, int64_t* medoids_out, const int64_t* forced_medoids, void* ws, size_t ws_bytes,
                  void* stream) {
    cc_frames fr{};
    fr.data = video;
    fr.format = CC_FRAMES_F32_CHW;
    return cc_vit_encode_frames(m, &fr, B, T, features, hidden_out, medoids_out, forced_medoids, ws, ws_bytes, stream);
}

size_t cc_text_workspace_bytes(const cc_text_model* m, int32_t Bt, int32_t Lt) {
    if (!m || Bt <= 0 || Lt <= 0) return 0;
    return carve_text(m, Bt, Lt, nullptr).total;
}

int cc_text_encode_hidden(const cc_text_model* m, const int64_t* ids, int32_t Bt, int32_t Lt, float* features,
                          float* hidden_out, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !ids || !features || !m->blocks || Bt <= 0 || Lt <= 0) return CC_ERR_INVALID;
    if (Lt > m->context_length || !act_ok(m->activation)) return CC_ERR_INVALID;
    if (!text_ok(m, Lt)) return CC_ERR_UNSUPPORTED;
    const TextReq tr{m, ids, Bt, Lt, features, hidden_out};
    return encode_towers(nullptr, &tr, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int cc_text_encode_prefix(const cc_text_model* m, const int64_t* ids, int32_t Bt, int32_t Lt, int32_t n_blocks,
                          float* hidden_out, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !ids || !hidden_out || Bt <= 0 || Lt <= 0 || Lt > m->context_length) return CC_ERR_INVALID;
    if (n_blocks < 0 || n_blocks > m->layers || (n_blocks > 0 && !m->blocks) || !act_ok(m->activation)) return CC_ERR_INVALID;
    if (!text_ok(m, Lt)) return CC_ERR_UNSUPPORTED;
    const TextReq tr{m, ids, Bt, Lt, nullptr, hidden_out, n_blocks};
    return encode_towers(nullptr, &tr, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int cc_text_encode(const cc_text_model* m, const int64_t* ids, int32_t Bt, int32_t Lt, float* features, void* ws,
                   size_t ws_bytes, void* stream) {
    return cc_text_encode_hidden(m, ids, Bt, Lt, features, nullptr, ws, ws_bytes, stream);
}

int cc_head_project_f32(const float* h, int32_t row_mul, const int32_t* row_idx, const float* gamma, const float* beta,
                        const float* proj, float* out, int32_t R, int32_t W, int32_t E, void* stream) {
    if (!h || !gamma || !beta || !proj || !out || R <= 0 || W <= 0 || E <= 0 || row_mul <= 0) return CC_ERR_INVALID;
    return cc_launch_head_project(h, row_mul, row_idx, gamma, beta, proj, out, R, W, E, static_cast<hipStream_t>(stream));
}

size_t cc_clip_workspace_bytes(const cc_vit_model* vm, int32_t B, int32_t T, const cc_text_model* tm, int32_t Bt,
                               int32_t Lt) {
    return cc_vit_workspace_bytes(vm, B, T) + cc_text_workspace_bytes(tm, Bt, Lt);
}

int cc_clip_encode_frames(const cc_vit_model* vm, const cc_frames* frames, int32_t B, int32_t T,
                          float* visual_features, int64_t* medoids_out, const int64_t* forced_medoids,
                          const cc_text_model* tm, const int64_t* ids, int32_t Bt, int32_t Lt, float* text_features,
                          void* ws, size_t ws_bytes, void* stream) {
    if (!vm || !tm || !frames || !frames->data || !ids || !visual_features || !text_features || !vm->blocks ||
        !tm->blocks)
        return CC_ERR_INVALID;
    if (B <= 0 || T <= 0 || Bt <= 0 || Lt <= 0 || Lt > tm->context_length) return CC_ERR_INVALID;
    if (!act_ok(vm->activation) || !act_ok(tm->activation)) return CC_ERR_INVALID;
    if (!vit_ok(vm) || !text_ok(tm, Lt)) return CC_ERR_UNSUPPORTED;
    const VisualReq vr{vm, frames, B, T, visual_features, nullptr, medoids_out, forced_medoids};
    const TextReq tr{tm, ids, Bt, Lt, text_features, nullptr};
    return encode_towers(&vr, &tr, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int cc_clip_encode(const cc_vit_model* vm, const float* video, int32_t B, int32_t T, float* visual_features,
                   int64_t* medoids_out, const cc_text_model* tm, const int64_t* ids, int32_t Bt, int32_t Lt,
                   float* text_features, void* ws, size_t ws_bytes, void* stream) {
    cc_frames fr{};
    fr.data = video;
    fr.format = CC_FRAMES_F32_CHW;
    return cc_clip_encode_frames(vm, &fr, B, T, visual_features, medoids_out, nullptr, tm, ids, Bt, Lt, text_features,
                                 ws, ws_bytes, stream);
}

}  // extern "C"
