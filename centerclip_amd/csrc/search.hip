// Exact retrieval over cached similarity operands on gfx950 without the [Bq, Bg] matrix: the k best gallery rows (or groups of
// rows) per query row, the rank of a known row or group, and the dual-softmax statistics.  The operands are the split-fp16
// planes of similarity.hip; a score is what cc_scaled_dot_planes_products_f32 stores for the same pair, bit for bit: ONE fp32
// accumulator per (query, gallery row) fed by v_mfma_f32_16x16x32_f16 over the 32-wide k-slices in ascending order with the
// gallery fragment as the first operand (gemm.hip: mfma(bf, af, acc) for ks = 0, 1 of every k-step), then sc * acc with
// sc = mult * 2^-20.
//
// The structure, from the inside out:
//
// THE STREAM (tk_stream_tiles).  Grid (gallery slices) x (groups of 16 query rows), 4 waves; the 16 query rows are staged once
// in LDS (tk_stage_rows).  A wave multiplies whole 16-row gallery tiles: its fragments go from global memory straight to
// registers (16-byte loads; the two k-slices of a 128-byte line are requested back to back), two register buffers taking
// turns.  Which tiles a wave takes comes from a rule: TkEvery (all of them) or TkLive (under ONE row mask, the tiles with a
// selectable row: a dead tile is neither requested nor multiplied).  The request that overlaps a tile's last batch is
// unconditional - the rule only says WHICH tile - for the reason tk_stream_tiles gives.
//
// THE PRODUCER OF CANDIDATES (tk_candidates<DSL, GROUPED, MASK>), written once for every search and count.  It owns the split
// of a slice's tiles over the waves, the query row's statistics and the per-tile loads (gallery statistics, heads, mask word -
// all requested in before_last, in front of the load that overlaps the tile's last batch), the score, the selectable
// predicate, and in grouped mode the folding of rows into groups:
//   * the score is sc * acc; DSL: D = cc_dsl_value(n_total, S, m_x, s_x) - the expression dsl_apply_kernel evaluates, so the
//     bits cc_dsl_apply_f32 writes over the matrix op's entry - with x the gallery row or the query row;
//   * MASK: a bit per gallery row - one mask for all queries (1), or one per query row (2) - says whether the row may be
//     ranked; a row that may not is no candidate.  That is the whole rule in every DSL x GROUPED combination;
//   * rows mode hands the consumer, per tile, the lane's 4 scores, their row ids and whether each is selectable;
//   * GROUPED (the k best GROUPS of adjacent rows, each by its best row): a wave takes one contiguous row range between group
//     starts instead of interleaved tiles, and the consumer gets one candidate key per finished group (tk_group_tile) and, once,
//     the group open at the range's end - so every group lives in one wave.
// Two consumers:
//   * the LISTS (topk_stream_kernel).  Per query row every wave keeps a descending list of its k best in LDS and, in a
//     register, the row's k-th key.  After a tile the lanes compare their 4 keys with that threshold, a wave-wide ballot says
//     whether any survived, and the survivors of all 16 query rows are inserted side by side, 4 lanes a list (tk_insert_tile).
//     At the end the four waves' lists are folded into one per query row and written to the workspace: [Bq][k][slices] keys.
//     BOUND is this consumer's: a candidate is kept only if key < bound[q].
//   * the COUNTS (rank_stream_kernel).  Three integers a lane against a score t_q - candidates above it, equal to it, equal in
//     front - so LDS is the staged rows alone; plain float compares on the score the producer hands over.  COUNT (the bound
//     comes from the caller, not from a target) is this consumer's.
//
// THE KEY.  A (score, id) pair is ONE 64-bit key whose unsigned order is the result's order (larger score first, equal scores
// by smaller id; -0 and +0 equal), so ties never need a second look and the lists of any split merge to the same result.  Key
// 0 is the empty entry.
//
// THE MERGES.  No workgroup reads what another workgroup of the same launch wrote (the per-XCD L2s are not coherent, the kernel
// boundary is the hand-over), so every result takes a second launch:
//   * topk_merge_kernel, one wave per query row: the slices' lists -> the final k, decoded into scores / ids;
//   * rank_reduce_kernel adds the slices' partial counts.  Integers: any split of the gallery sums to the same result;
//   * topk_merge_lists_kernel merges the lists of a gallery split in shards (each shard one buffer, searched and counted on
//     its own; the results are those of the shards' concatenation), ties by smaller shard, then smaller local id - the order
//     the concatenated positions would give.
//
// Deep lists and cursors (more than TK_MAXK entries, or the entries behind a known one): a list is a chain of PAGES of at most
// TK_MAXK entries, each the list stream restricted to the keys BELOW a per-query bound - the last key of the page before, or
// the key of a (score, id) pair the caller holds.  Keys are unique and their unsigned order is the result's order, so "the
// keys below X" is exact and needs no state.  Bound 0 keeps nothing.  GROUPED applies the bound to the finished group's
// candidate, never to a row - a group whose best row lies at or above the bound was handed out before and must not return
// through its second-best row.  topk_merge_kernel writes a page at its column offset of the [Bq, k] result and its last key to
// bound[q] for the page after it: the pages of a call hand over on the device.  A list of at most TK_MAXK entries without a
// cursor is one page.
//
// The rank of a known row or group (where does THIS row stand for THIS query): three launches.  rank_target_kernel computes
// t_q, the score of every query row's target, with the MFMA sequence of the stream (so the bits are those of every other
// score); the count stream counts against it; rank_reduce_kernel adds up.  For a gallery split in shards rank_target_kernel
// behind an entry of its own gives the owner's t_q, and the COUNT mode counts a shard against that score and a `front`
// position the caller sets (the target's row on its owner, 0 on the shards behind it, 2^31 - 1 on those in front): the counts
// of the shards add up to the counts of the whole.
//
// The dual-softmax statistics (dsl_stats_stream_kernel): the pair (m, s) of every VIDEO row over many text rows on the same
// stream - the video rows take the place of the queries (16 staged in LDS), the text rows are streamed, and a running
// log-sum-exp pair is the consumer; with a mask, masked text rows are left out the way the producer leaves rows out (TkLive,
// the tile's mask word).
//     Summation tree of one video row (fixed; no atomics; it depends on Bt alone, never on Bv or on the row's place):
//       - the text tiles are cut into dsl_stats_slices(Bt) contiguous slices, a workgroup each; wave w takes tiles
//         t0 + w, t0 + w + 4, ... of its slice, and in a tile the lane group lg holds text rows 16 t + 4 lg + {0, 1, 2, 3};
//       - lane, per tile: mt = max(m, x0..x3);  s = (((share(s, m, mt) + e0) + e1) + e2) + e3,  e_r = expf(x_r - mt);  m = mt
//         (share(s, a, b) = s * expf(a - b), 0 for s == 0) - an old term passes 2 (expf) + 1 (mul) + 4 (add) = 7 roundings
//         per tile of its lane, ceil(ceil(tiles / slices) / 4) tiles at most;
//       - workgroup: the 16 pairs of a video row (wave-major, then lane group) under their maximum, shares added in that
//         order: 2 + 1 + 16 roundings;
//       - second launch (dsl.hip's merge): the slices' pairs under their maximum, added in slice order: 2 + 1 + slices.
//     The subtractions inside expf telescope: the partial maxima rise from x to m, so together they cost |x - m| U on the
//     exponent.  Longest chain of roundings: 7 * ceil(ceil(tiles / slices) / 4) + 19 + slices + 3.
//
// pack_row_mask_kernel turns byte flags into mask words.
#include <type_traits>

#include "cc_kernels.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

namespace {

constexpr int TK_WAVES = 4;            // waves of a streaming workgroup
constexpr int TK_QROWS = 16;           // query rows of a workgroup (one MFMA tile side)
constexpr int TK_MAXK = 128;             // entries of a list (of a page of a deep list) at most
constexpr int TK_QPAD = 8;             // halfs behind a staged query row: 16 rows 16 bytes apart mod 256 cover all LDS banks
constexpr int TK_TARGET_WGS = 512;     // streaming workgroups aimed at: the 256 CUs twice
constexpr int TK_MIN_TILES = 32;       // 16-row tiles a slice holds at least (8 per wave)
constexpr int TK_BATCH = 4;            // pairs of k-slices a lane requests at once (8 loads of 16 bytes)
constexpr int TK_MERGE_BATCH = 8;      // keys per lane the merge requests before it looks at any
constexpr size_t TK_LDS_LIMIT = 160 * 1024;
constexpr int DSL_MAX_SLICES = 512;    // text slices of the statistics pass at most (the 256 CUs twice for one group of videos)

// key = [ordered score bits : 32][~id, 31 bits][score was -0 : 1].  The score enters as score + 0.0f (so -0 orders as +0);
// the last bit only restores the sign of a zero on the way out - ids are unique, it never decides an order.  No finite or
// infinite score gives the high word 0: key 0 is the empty entry, decoded as (-inf, -1).
__device__ __forceinline__ u64 tk_key(float score, int id) {
    const unsigned negzero = __float_as_uint(score) == 0x80000000u ? 1u : 0u;
    const unsigned low = ((~(unsigned)id & 0x7FFFFFFFu) << 1) | negzero;
    return ((u64)cc_float_to_ordered_uint(score + 0.0f) << 32) | low;
}
__device__ __forceinline__ void tk_decode(u64 key, float& score, int& id) {
    if (key == 0) { score = -INFINITY; id = -1; return; }
    const unsigned o = (unsigned)(key >> 32), low = (unsigned)key;
    unsigned u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    if (low & 1u) u = 0x80000000u;
    score = __uint_as_float(u);
    id = (int)(~(low >> 1) & 0x7FFFFFFFu);
}

// LDS traffic between the lanes of one wave: the hardware runs a wave's LDS instructions in order, the compiler must not
// move them over this point
__device__ __forceinline__ void tk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// max over the 4 lanes l15 + 16 {0, 1, 2, 3} (the lanes that hold one query row's values), in all of them: the row swaps of
// cc_lane_xor16_pair / cc_lane_xor32_pair on both halves of the key
__device__ __forceinline__ u64 tk_group_max(u64 x) {
    {
        const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(x >> 32), (unsigned)(x >> 32), false, false);
        const u64 a = ((u64)hi[0] << 32) | lo[0], b = ((u64)hi[1] << 32) | lo[1];
        x = a > b ? a : b;
    }
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(x >> 32), (unsigned)(x >> 32), false, false);
    const u64 a = ((u64)hi[0] << 32) | lo[0], b = ((u64)hi[1] << 32) | lo[1];
    return a > b ? a : b;
}

// Candidates into the wave's 16 lists at once.  Lane (l15, lg) brings up to 4 keys (0 = none) for `list`, the descending list
// of query row l15 (k entries), and holds that list's k-th key in `thr`.  A round takes, per list, the largest candidate its 4
// lanes still hold above the threshold, and those 4 lanes shift it in, 16 entries a step (4 a lane) from the bottom up: a
// step writes entries [base, base + 15] from the old [base - 1, base + 14], every lane reading before any lane writes, and
// the entries later steps read lie above - nothing is read after it was overwritten.  `filled` (uniform) bounds the entries
// any of the wave's lists holds - a round adds at most one - so the steps start at the first empty entry, not at k; they end
// with the first one in which no list moved an entry (the lists descend: nothing above moves either).  The rounds end when no
// candidate is above its threshold: at most min(k, 16) of them, where inserting the survivors one at a time took up to
// 16 x 16 dependent LDS round trips.
__device__ __forceinline__ void tk_insert_tile(u64 (&key)[4], u64* list, int k, int lg, u64& thr, int& filled) {
    for (;;) {
        u64 m = key[0];
#pragma unroll
        for (int r = 1; r < 4; ++r) m = key[r] > m ? key[r] : m;
        m = m > thr ? m : 0;
        if (!__ballot(m != 0)) break;
        const u64 gm = tk_group_max(m);                      // 0: nothing for this list in this round
#pragma unroll
        for (int r = 0; r < 4; ++r) key[r] = key[r] == gm ? 0 : key[r];      // (ids are unique: one lane, one key)
        for (int base = min(filled, k - 1) & ~15; base >= 0; base -= 16) {
            const int i0 = base + 4 * lg;
            u64 v[5];                                        // old entries i0 - 1 .. i0 + 3; beyond the list: never moved
#pragma unroll
            for (int u = 0; u < 5; ++u) {                    // (clamped addresses: five loads in a row, no branch, one wait)
                const int i = i0 - 1 + u;
                const u64 raw = list[min(max(i, 0), k - 1)];
                v[u] = (gm != 0 && i >= 0 && i < k) ? raw : ~0ull;
            }
            tk_wave_sync();
            bool moved = false;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (v[u + 1] < gm) {
                    list[i0 + u] = v[u] > gm ? gm : v[u];
                    moved = true;
                }
            }
            tk_wave_sync();
            if (!__ballot(moved)) break;
        }
        filled = min(filled + 1, k);
        thr = list[k - 1];
    }
}

// The wave inserts `key` (uniform) into the descending list of k entries: entries below it move one place down, the last
// one leaves; a key below the last entry changes nothing.  Every lane reads before any lane writes.  (The merge launch.)
__device__ __forceinline__ void tk_insert(u64* list, int k, u64 key, int lane) {
    const bool in0 = lane < k, in1 = lane + 64 < k;
    const u64 r0 = list[min(lane, k - 1)], q0 = list[min(max(lane - 1, 0), k - 1)];      // (clamped: loads without a branch)
    const u64 v0 = in0 ? r0 : ~0ull, p0 = (in0 && lane) ? q0 : ~0ull;
    u64 v1 = ~0ull, p1 = ~0ull;
    if (k > 64) {
        const u64 r1 = list[min(lane + 64, k - 1)], q1 = list[min(lane + 63, k - 1)];
        v1 = in1 ? r1 : ~0ull;
        p1 = in1 ? q1 : ~0ull;
    }
    tk_wave_sync();
    if (v0 < key) list[lane] = p0 > key ? key : p0;
    if (v1 < key) list[lane + 64] = p1 > key ? key : p1;
    tk_wave_sync();
}

// 16 plane rows from `first` on (rows beyond `count`: clamped to the last one, their results are dropped) -> LDS [16][K + TK_QPAD]
__device__ __forceinline__ void tk_stage_rows(_Float16* qs, const _Float16* __restrict__ rows, int first, int count, int ld, int K) {
    const int QS = K + TK_QPAD, chunks = K >> 3;
    for (int c = threadIdx.x; c < TK_QROWS * chunks; c += 256) {
        const int r = c / chunks, cc = c - r * chunks;
        const int qr = min(first + r, count - 1);
        *reinterpret_cast<h8*>(qs + r * QS + cc * 8) = *reinterpret_cast<const h8*>(rows + (int64_t)qr * ld + cc * 8);
    }
}

// Which tiles a wave streams, in which order: the "next tile" rule of tk_stream_tiles.
// TkEvery: the tiles first, first + stride, ... < t1.  It only names them: tk_stream_tiles does their arithmetic (count, last
// tile, t + stride) in place, with no state to carry.
struct TkEvery {
    int first, stride, t1;
};

// TkLive: of TkEvery's tiles the LIVE ones under one row mask shared by all staged rows (bit b of word w = row 32 w + b): the
// 16 bits of tile t are halfword t of the mask, and a tile whose halfword is 0 is neither requested nor multiplied.  The flags
// of 64 candidate tiles are one load and one ballot (`bits`, wave-uniform; refilled every 64 candidates), so finding the next
// live tile puts no memory round trip in front of a tile's request.  All lanes of the wave call every member together.
// count(): how many tiles; start(): the first; request(t), asked once per tile in front of the request that overlaps tile t's
// last batch: the tile whose first batch that request fetches - behind the wave's last tile a tile already read (a cache hit
// that nobody multiplies: the request stays unconditional); advance(t), asked once behind request(t): the tile after t.
struct TkLive {
    const int* __restrict__ mask;
    int first, stride, t1, lane, tiles, base, next;
    u64 bits;                                                                          // bit i: tile base + i * stride is live and not yet taken
    __device__ __forceinline__ u64 flags(int b) const {
        const int t = b + lane * stride, tc = max(min(t, t1 - 1), 0);                 // (words behind the last tile are never read)
        const int w = mask[tc >> 1];
        return __ballot(t < t1 && ((w >> (16 * (tc & 1))) & 0xFFFF) != 0);
    }
    __device__ __forceinline__ TkLive(const int* __restrict__ mask_, int first_, int stride_, int t1_, int lane_)
        : mask(mask_), first(__builtin_amdgcn_readfirstlane(first_)), stride(stride_), t1(__builtin_amdgcn_readfirstlane(t1_)),
          lane(lane_), tiles(0), base(first), next(t1), bits(0) {                      // (the ends are the same in all lanes: scalars)
        for (int b = first; b < t1; b += 64 * stride) tiles += __builtin_popcountll(flags(b));
        if (first < t1) bits = flags(first);
    }
    __device__ __forceinline__ int take() {                                            // the next live tile; t1: none left
        while (!bits) {
            base += 64 * stride;
            if (base >= t1) return t1;
            bits = flags(base);
        }
        const int i = __builtin_ctzll(bits);
        bits &= bits - 1;
        return base + i * stride;
    }
    __device__ __forceinline__ int count() const { return tiles; }
    __device__ __forceinline__ int start() { return take(); }
    __device__ __forceinline__ int request(int t) { return (next = take()) < t1 ? next : t; }
    __device__ __forceinline__ int advance(int) const { return next; }
};

// The stream of one wave: the 16-row tiles `rule` names (TkEvery: first, first + stride, ... < t1; TkLive: of those the ones
// with a selectable row) of `gallery` (Bg rows, `ld` halfs apart, the first K multiplied) against the 16 staged rows
// (`qrow`: the lane's fragments of staged row l15).  Behind a tile's last k-slice
// on_tile(t, acc) gets the 16 x 16 products: the lane holds streamed rows t * 16 + 4 lg + r (r = 0..3) of staged row l15, each
// ONE fp32 accumulator over the k-slices in ascending order, the streamed fragment as the first operand.  before_last(t) runs
// in front of the request that overlaps tile t's last batch: what it requests arrives before that batch (loads return in
// order), so on_tile waits for the tile, not for the next one.
// A batch = TK_BATCH pairs of k-slices of one tile (2 TK_BATCH 16-byte loads a lane).  Two register buffers take turns:
// while one batch is multiplied - and, behind a tile's last batch, consumed by on_tile - the next one (the tile's next, or the
// first of the wave's next tile) is in flight.  Pairs beyond the row's end are clamped to its last pair (read again, not
// multiplied).
template <class Rule, class Before, class Tile>
__device__ __forceinline__ void tk_stream_tiles(const _Float16* __restrict__ gallery, int Bg, int ld, int K, const _Float16* qrow,
                                                Rule&& rule, int l15, int lg, Before&& before_last, Tile&& on_tile) {
    const int nk2 = K >> 6;                                                            // pairs of k-slices: one 128-byte line per row
    auto load_batch = [&](h8 (&b)[2 * TK_BATCH], int t, int s0) {
        const int grow = min(t * 16 + l15, Bg - 1);                                    // rows at Bg or above are never read
        const _Float16* gp = gallery + (int64_t)grow * ld + lg * 8;
#pragma unroll
        for (int u = 0; u < TK_BATCH; ++u) {
            const int s = min(s0 + u, nk2 - 1);
            b[2 * u] = *reinterpret_cast<const h8*>(gp + s * 64);
            b[2 * u + 1] = *reinterpret_cast<const h8*>(gp + s * 64 + 32);
        }
    };
    const int nb = (nk2 + TK_BATCH - 1) / TK_BATCH;                                    // batches of a tile
    constexpr bool every = std::is_same<std::decay_t<Rule>, TkEvery>::value;
    const int first = rule.first, stride = rule.stride, t1 = rule.t1;
    const int my_tiles = [&] {
        if constexpr (every) return first < t1 ? (t1 - first + stride - 1) / stride : 0;
        else return rule.count();
    }();
    const int total = my_tiles * nb, t_last = first + (my_tiles - 1) * stride;         // (t_last: TkEvery's last tile)
    int t = first, b = 0;                                                              // the batch about to be multiplied
    if constexpr (!every) t = rule.start();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    auto step = [&](const h8 (&cur)[2 * TK_BATCH], h8 (&nxt)[2 * TK_BATCH]) {
        // (the request is unconditional - behind the wave's last batch it repeats the last tile's first, a cache hit that
        // nobody multiplies: under a condition the compiler's wait for `cur` has to cover the path without the request,
        // and on the other path it then waits for the batch just requested.  The rule only says WHICH tile.)
        const bool last = b + 1 == nb;
        if (last) before_last(t);
        if constexpr (every) {
            load_batch(nxt, last ? min(t + stride, t_last) : t, last ? 0 : (b + 1) * TK_BATCH);
        } else {
            load_batch(nxt, last ? rule.request(t) : t, last ? 0 : (b + 1) * TK_BATCH);
        }
#pragma unroll
        for (int u = 0; u < TK_BATCH; ++u) {
            const int s = b * TK_BATCH + u;
            if (s < nk2) {
                const h8 a0 = *reinterpret_cast<const h8*>(qrow + s * 64);
                const h8 a1 = *reinterpret_cast<const h8*>(qrow + s * 64 + 32);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[2 * u], a0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[2 * u + 1], a1, acc, 0, 0, 0);
            }
        }
        if (!last) { ++b; return; }
        on_tile(t, acc);
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (every) t += stride;
        else t = rule.advance(t);
        b = 0;
    };
    h8 buf0[2 * TK_BATCH], buf1[2 * TK_BATCH];
    if (total) load_batch(buf0, t, 0);
    for (int g = 0; g < total; g += 2) {
        step(buf0, buf1);
        if (g + 1 < total) step(buf1, buf0);
    }
}

// Grouped search, one tile of a wave's row range: key[r] (in) is the key of streamed row 4 lg + r of the tile for query row
// l15, 0 for a row outside the range; head[r] says that the row is the first of its group (the same in all 16 query rows).
// The rows of a range arrive in ascending order, so a group's rows arrive one after the other: `carry` - the same value in
// the 4 lanes of a query row - is the best key of the group still open in front of the tile.  A segmented maximum over the
// 16 rows in row order, started from the carry, replaces the keys: key[r] (out) = the best key of the group that ENDS in
// front of row 4 lg + r (head[r]; 0 otherwise), at most one candidate a row, and the group open behind row 15 is the new
// carry.  Keys are unique and 0 is the empty key: the maximum of keys is "best score, smallest id", and max with 0 changes
// nothing.  Across the 4 lanes: every lane gets the 4 lanes' tails (the open group's best behind the lane's 4 rows, started
// from nothing) by three row swaps, and a ballot tells which lanes saw a head.
__device__ __forceinline__ void tk_group_tile(u64 (&key)[4], const bool (&head)[4], int lg, u64& carry) {
    u64 tail = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) tail = (head[r] || key[r] > tail) ? key[r] : tail;
    const u64 any = __ballot(head[0] || head[1] || head[2] || head[3]);               // bit 16 g: lane group g saw a head
    u64 tails[4];
    {
        const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)tail, (unsigned)tail, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(tail >> 32), (unsigned)(tail >> 32), false, false);
        const unsigned elo = lo[0], olo = lo[1], ehi = hi[0], ohi = hi[1];             // of the even / odd lane group of the pair
        const auto el = __builtin_amdgcn_permlane32_swap(elo, elo, false, false);
        const auto eh = __builtin_amdgcn_permlane32_swap(ehi, ehi, false, false);
        const auto ol = __builtin_amdgcn_permlane32_swap(olo, olo, false, false);
        const auto oh = __builtin_amdgcn_permlane32_swap(ohi, ohi, false, false);
        tails[0] = ((u64)eh[0] << 32) | el[0];
        tails[1] = ((u64)oh[0] << 32) | ol[0];
        tails[2] = ((u64)eh[1] << 32) | el[1];
        tails[3] = ((u64)oh[1] << 32) | ol[1];
    }
    u64 run = carry, in = carry;                                                       // in: the open group in front of this lane's rows
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        run = ((any >> (16 * g)) & 1) ? tails[g] : (tails[g] > run ? tails[g] : run);
        if (g < 3) in = lg > g ? run : in;
    }
    carry = run;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u64 x = key[r];
        key[r] = head[r] ? in : 0;
        in = (head[r] || x > in) ? x : in;
    }
}

// The contiguous share of the 16-row tiles of `rows` rows that slice `slice` of `slices` takes: [t0, t1).  -> all tiles.
__device__ __forceinline__ int tk_slice_tiles(int rows, int slice, int slices, int& t0, int& t1) {
    const int tiles = (rows + 15) >> 4;
    t0 = (int)((int64_t)tiles * slice / slices);
    t1 = (int)((int64_t)tiles * (slice + 1) / slices);
    return tiles;
}

// The bit of row 4 lg + r of tile t in `word`, the mask word that holds the tile's 16 bits (word t >> 1 of the mask row).
__device__ __forceinline__ bool tk_mask_bit(int word, int t, int lg, int r) { return (word >> ((t & 1) * 16 + lg * 4 + r)) & 1; }

// tk_stream_tiles over the tiles first, first + stride, ... < t1 - LIVE: of those the live ones under the one mask row `mask`
template <bool LIVE, class Before, class Tile>
__device__ __forceinline__ void tk_stream_rule(const _Float16* __restrict__ gallery, int Bg, int ld, int K, const _Float16* qrow,
                                               const int* __restrict__ mask, int first, int stride, int t1, Before&& before_last,
                                               Tile&& on_tile) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    if constexpr (LIVE) tk_stream_tiles(gallery, Bg, ld, K, qrow, TkLive(mask, first, stride, t1, lane), l15, lg, before_last, on_tile);
    else tk_stream_tiles(gallery, Bg, ld, K, qrow, TkEvery{first, stride, t1}, l15, lg, before_last, on_tile);
}

// What the producer of candidates reads: the gallery side of a search or count kernel's arguments and the block's slice.
// gallery: plane rows `ld` halfs apart, the first K of them multiplied.  DSL: the score is cc_dsl_value(nt, S, m, s) with the
// pair of the gallery row (on_gallery) or of the query row; without DSL those four are not read.  GROUPED: group_head[r] = the
// first row of r's group (the rows of a group are adjacent).  MASK: 0 every row may be ranked (row_mask, mask_words are not
// read), 1 row_mask is ONE mask row for all queries, 2 one per query row, mask_words apart (bit b of word w = row 32 w + b;
// bits at Bg or above are ignored).
struct TkSource {
    const _Float16* __restrict__ gallery;
    int Bg, ld, K;
    float sc;
    int slice, slices;
    const float* __restrict__ stat_m;
    const float* __restrict__ stat_s;
    int on_gallery;
    float nt;
    const int* __restrict__ group_head;
    const int* __restrict__ row_mask;
    int mask_words;
};

// The candidates of one wave for the 16 rows staged in `qs` ([16][K + TK_QPAD]); the lane works for staged row l15, query row
// `qr` (clamped into [0, Bq): its statistics and its mask row), and `qvalid` says whether that row has candidates at all.
// Rows mode: the wave streams the tiles t0 + wave, t0 + wave + 4, ... of its slice and on_rows(x, id, in) gets, per tile, the
// lane's 4 scores x[r] of gallery rows id[r] and in[r]: the row is a candidate (qvalid, below Bg, its mask bit set).
// GROUPED: instead of the interleaved tiles a wave takes ONE contiguous row range whose ends are group starts: the
// 4 * slices + 1 even shares of the tiles, each planned row b snapped down to group_head[b] (monotone; a range may be empty; a
// group longer than a share belongs wholly to the range that starts at its head).  A row outside the range or not selectable
// gets key 0, the empty key; on_groups(key) gets what tk_group_tile hands out - at most one candidate a row, the best key of
// the group that ends in front of it - and once, behind the range, the group still open in key[0] of lane group 0.  Every
// group lives in one wave.  Only the snapping indexes with a value of group_head, and clamps it to [0, b].
// Statistics and heads are indexed as without a mask.  MASK == 1 streams the live tiles only (TkLive); MASK == 2 skips nothing.
template <bool DSL, bool GROUPED, int MASK, class Rows, class Groups>
__device__ __forceinline__ void tk_candidates(const TkSource& a, const _Float16* qs, int qr, bool qvalid, Rows&& on_rows,
                                              Groups&& on_groups) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
    const int Bg = a.Bg;
    int t0, t1;
    const int tiles = tk_slice_tiles(Bg, a.slice, a.slices, t0, t1);
    // DSL: the statistics of the lane's 4 gallery rows (requested per tile) or of its query row (once)
    float dm[4] = {0.f, 0.f, 0.f, 0.f}, ds[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (DSL) {
        if (!a.on_gallery) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { dm[r] = a.stat_m[qr]; ds[r] = a.stat_s[qr]; }
        }
    }
    // GROUPED: the wave's row range [r0, r1) and the open group's best key (tk_group_tile); the lane's 4 heads come per tile
    int first = t0 + wave, last = t1, r0 = 0, r1 = Bg;
    u64 carry = 0;
    int gh[4] = {0, 0, 0, 0};
    if constexpr (GROUPED) {
        auto bound = [&](int j) {
            if (j <= 0) return 0;
            if (j >= TK_WAVES * a.slices) return Bg;
            const int b = min((int)((int64_t)tiles * j / (TK_WAVES * a.slices)) * 16, Bg - 1);
            return min(max(a.group_head[b], 0), b);                                    // (a malformed head stays inside the rows)
        };
        r0 = bound(TK_WAVES * a.slice + wave);
        r1 = bound(TK_WAVES * a.slice + wave + 1);
        first = r0 >> 4;
        last = r1 > r0 ? (r1 + 15) >> 4 : first;                                       // the tile at a boundary: both neighbours' work
    }
    // MASK: the mask word that holds the tile's 16 bits comes per tile, from the one mask row or from query row qr's.
    // GROUPED, MASK == 1: the tile streamed before this one, and the head of the row in front of this one (per tile)
    const int* mrow = a.row_mask;
    if constexpr (MASK == 2) mrow += (int64_t)qr * a.mask_words;
    int word = 0, prev = first - 1, gap_head = 0;
    auto before_last = [&](int t) {
        if constexpr (MASK != 0) word = mrow[t >> 1];                                  // (t < tiles: inside ceil(Bg / 32) words)
        if constexpr (GROUPED && MASK == 1) gap_head = a.group_head[min(max(t * 16 - 1, 0), Bg - 1)];
        if constexpr (DSL) {
            if (a.on_gallery) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int id = min(t * 16 + lg * 4 + r, Bg - 1);                   // statistics at Bg or above are never read
                    dm[r] = a.stat_m[id];
                    ds[r] = a.stat_s[id];
                }
            }
        }
        if constexpr (GROUPED) {
#pragma unroll
            for (int r = 0; r < 4; ++r) gh[r] = a.group_head[min(t * 16 + lg * 4 + r, Bg - 1)];    // nor heads
        }
    };
    auto on_tile = [&](int t, const f32x4& acc) {
        // the lane holds gallery rows t * 16 + 4 lg + r (r = 0..3) of staged row l15
        float x[4];
        int id[4];
        bool in[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            id[r] = t * 16 + lg * 4 + r;
            x[r] = a.sc * acc[r];
            if constexpr (DSL) x[r] = cc_dsl_value(a.nt, x[r], dm[r], ds[r]);
            in[r] = qvalid && (GROUPED ? (id[r] >= r0 && id[r] < r1) : id[r] < Bg);
            if constexpr (MASK != 0) in[r] = in[r] && tk_mask_bit(word, t, lg, r);
        }
        if constexpr (GROUPED) {
            u64 key[4];
            bool head[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                key[r] = in[r] ? tk_key(x[r], id[r]) : 0;
                head[r] = gh[r] == id[r];
            }
            if constexpr (MASK == 1) {
                // Dead tiles between the tile streamed before and this one were skipped, heads included.  If a group starts in
                // them (the head of the row in front of this tile lies behind the tile streamed before), the group open in front
                // of them ends there, and this tile's rows up to its first head belong to a group whose earlier rows are all
                // unselectable: both are what a head at the tile's first row says.  (A gap lies inside the wave's range; a group
                // none of whose rows is selectable only ever holds key 0 and never becomes a candidate.)
                if (lg == 0 && t > prev + 1 && gap_head >= (prev + 1) * 16) head[0] = true;
                prev = t;
            }
            tk_group_tile(key, head, lg, carry);
            on_groups(key);
        } else {
            on_rows(x, id, in);
        }
    };
    tk_stream_rule<MASK == 1>(a.gallery, Bg, a.ld, a.K, qs + l15 * (a.K + TK_QPAD) + lg * 8, a.row_mask, first,
                              GROUPED ? 1 : TK_WAVES, last, before_last, on_tile);
    if constexpr (GROUPED) {
        u64 key[4] = {lg == 0 ? carry : 0, 0, 0, 0};                                   // the group open at the range's end
        on_groups(key);
    }
}

// The lists: stage the query rows, clear the lists, insert what the producer hands over, fold, write.  query: plane rows as
// the gallery's.  ws [Bq][k][slices] keys.  The fold, the workspace and the merge launch never know the mode: a row that may
// not be ranked is no candidate, and with GROUPED the lists hold groups that are disjoint between the waves.
// BOUND: a candidate of query row q is kept only if its key is below bound[q] (0: nothing is kept); without GROUPED a
// candidate is a row, with it the finished group the producer hands over (and the one open at the range's end), so the rows
// of a group are folded before the bound looks at it.  Without BOUND `bound` is not read.
template <bool DSL, bool GROUPED, int MASK, bool BOUND>
__global__ __launch_bounds__(256) void topk_stream_kernel(const _Float16* __restrict__ query, const _Float16* __restrict__ gallery,
                                                          int Bq, int Bg, int ld, int K, float sc, int k, int slices,
                                                          u64* __restrict__ ws, const float* __restrict__ stat_m,
                                                          const float* __restrict__ stat_s, int on_gallery, float nt,
                                                          const int* __restrict__ group_head, const int* __restrict__ row_mask,
                                                          int mask_words, const u64* __restrict__ bound) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
    const int slice = blockIdx.x, q0 = blockIdx.y * TK_QROWS;
    _Float16* qs = reinterpret_cast<_Float16*>(tk_smem);                               // [16][K + TK_QPAD]
    u64* lists = reinterpret_cast<u64*>(tk_smem + (size_t)TK_QROWS * (K + TK_QPAD) * 2);     // [wave][16][k]
    tk_stage_rows(qs, query, q0, Bq, ld, K);
    for (int i = threadIdx.x; i < TK_WAVES * TK_QROWS * k; i += 256) lists[i] = 0;
    __syncthreads();

    u64* mine = lists + ((size_t)wave * TK_QROWS + l15) * k;                           // this wave's list of query row l15
    const int qr = min(q0 + l15, Bq - 1);
    u64 thr = 0;                                                                       // the k-th key of `mine`
    int filled = 0;                                                                    // entries any of the wave's lists holds, at most
    u64 below = 0;                                                                     // BOUND: query row l15's bound
    if constexpr (BOUND) below = bound[qr];
    auto keep = [&](u64 key) {                                                         // a candidate that passes the bound, or 0
        if constexpr (BOUND) return key < below ? key : 0;
        else return key;
    };
    const TkSource src{gallery, Bg, ld, K, sc, slice, slices, stat_m, stat_s, on_gallery, nt, group_head, row_mask, mask_words};
    tk_candidates<DSL, GROUPED, MASK>(
        src, qs, qr, q0 + l15 < Bq,
        [&](const float (&x)[4], const int (&id)[4], const bool (&in)[4]) {
            u64 key[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) key[r] = keep(in[r] ? tk_key(x[r], id[r]) : 0);
            tk_insert_tile(key, mine, k, lg, thr, filled);
        },
        [&](u64 (&key)[4]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) key[r] = keep(key[r]);                         // the finished groups, not their rows
            tk_insert_tile(key, mine, k, lg, thr, filled);
        });
    // the four waves' lists -> wave 0's, as a tree: the other wave's entries are the candidates, 16 a list at a time
    auto fold = [&](int from) {
        const u64* other = lists + ((size_t)from * TK_QROWS + l15) * k;
        u64 th = mine[k - 1];
        for (int c0 = 0; c0 < k; c0 += 16) {
            u64 key[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = c0 + lg * 4 + r;
                key[r] = i < k ? other[i] : 0;
            }
            tk_insert_tile(key, mine, k, lg, th, filled);
        }
    };
    __syncthreads();
    if (wave == 0 || wave == 2) fold(wave + 1);
    __syncthreads();
    if (wave == 0) fold(2);
    __syncthreads();
    for (int e = threadIdx.x; e < TK_QROWS * k; e += 256) {
        const int ql = e / k;
        if (q0 + ql < Bq) ws[((int64_t)(q0 + ql) * k + (e - ql * k)) * slices + slice] = lists[e];     // [query][rank][slice]
    }
}

// ws [Bq][k][slices]: rank by rank, the best entry of every slice first.  A rank none of whose entries passes the threshold
// ends the merge: every list descends, so no deeper entry passes either - for k well below the gallery the result comes from
// the first few ranks.  scores / ids: rows out_ld entries apart (a page of a deep list lands at its column offset of the whole
// result).  last != nullptr: last[q] = the list's k-th key (0: the list is not full) - the bound of the page behind this one.
__global__ __launch_bounds__(64) void topk_merge_kernel(const u64* __restrict__ ws, int slices, int k, float* __restrict__ scores,
                                                        int* __restrict__ ids, int out_ld, u64* __restrict__ last) {
    __shared__ u64 list[TK_MAXK];
    const int q = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < k; i += 64) list[i] = 0;
    tk_wave_sync();
    u64 thr = 0;                                                           // list[k - 1]
    for (int rank = 0; rank < k; ++rank) {
        const u64* src = ws + ((int64_t)q * k + rank) * slices;
        bool any = false;
        for (int i0 = 0; i0 < slices; i0 += 64 * TK_MERGE_BATCH) {
            u64 c[TK_MERGE_BATCH];
#pragma unroll
            for (int u = 0; u < TK_MERGE_BATCH; ++u) {
                const int i = i0 + u * 64 + lane;
                c[u] = i < slices ? src[i] : 0;
            }
#pragma unroll
            for (int u = 0; u < TK_MERGE_BATCH; ++u) {
                u64 mask = __ballot(c[u] > thr);
                any |= mask != 0;
                while (mask) {                                             // (a survivor of a threshold raised since: no change)
                    const int from = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const unsigned lo = __builtin_amdgcn_readlane((unsigned)c[u], from);
                    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(c[u] >> 32), from);
                    tk_insert(list, k, ((u64)hi << 32) | lo, lane);
                    thr = list[k - 1];
                }
            }
        }
        if (!any) break;
    }
    for (int i = lane; i < k; i += 64) {
        float s;
        int id;
        tk_decode(list[i], s, id);
        scores[(int64_t)q * out_ld + i] = s;
        ids[(int64_t)q * out_ld + i] = id;
    }
    if (last && lane == 0) last[q] = list[k - 1];
}

// The bound of a search that continues behind a known entry: bound[q] = tk_key(after_scores[q], after_ids[q]), the key that
// entry has in every list; an id < 0 (the fill: nothing lies behind it) gives 0, which keeps nothing.
__global__ __launch_bounds__(256) void topk_cursor_kernel(const float* __restrict__ after_scores, const int* __restrict__ after_ids,
                                                          int Bq, u64* __restrict__ bound) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < Bq) bound[q] = after_ids[q] < 0 ? 0 : tk_key(after_scores[q], after_ids[q]);
}

// ---------------------------------------------------------------------------- rank of a known row or group
// First launch of the rank: t_q, the score of query row q's target, one wave per query row (4 a workgroup).  The wave
// multiplies the 16-row tiles that cover the target - rows mode: the one tile of row target[q]; GROUPED: the tiles of
// [head, end), head = group_head[target[q]] and end the next group start, found by walking group_head forward 64 rows a step -
// with the query row in all 16 columns of the second operand: the k-slices in ascending order, the gallery fragment first, one
// fp32 accumulator, then sc * acc (and cc_dsl_value) - the instruction sequence of tk_stream_tiles, so t_q has the bits the
// counting pass computes for the same pair and its `==` finds the target itself.  Rows mode never looks at the target's own
// mask bit; GROUPED takes the best key (tk_key: best score, smallest row) of the group's selectable rows, as the searches do,
// and decodes it: -inf without one.  row_mask == nullptr: every row is selectable; mask_step: words between the mask rows of
// two query rows (0: one mask for all).  A target outside [0, Bg): -inf.
template <bool DSL, bool GROUPED>
__global__ __launch_bounds__(256) void rank_target_kernel(const _Float16* __restrict__ query, const _Float16* __restrict__ gallery,
                                                          int Bq, int Bg, int ld, int K, float sc, const int* __restrict__ target,
                                                          float* __restrict__ tscore, const float* __restrict__ stat_m,
                                                          const float* __restrict__ stat_s, int on_gallery, float nt,
                                                          const int* __restrict__ group_head, const int* __restrict__ row_mask,
                                                          int mask_step) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    const int q = blockIdx.x * TK_WAVES + (threadIdx.x >> 6);
    if (q >= Bq) return;                                                               // (a whole wave; no barrier below)
    const int tg = target[q];
    if (tg < 0 || tg >= Bg) {
        if (lane == 0) tscore[q] = -INFINITY;
        return;
    }
    int h = tg, e = tg + 1;                                                            // the rows of the target: [h, e)
    if constexpr (GROUPED) {
        h = min(max(group_head[tg], 0), tg);                                           // (a malformed head stays inside the rows)
        for (int base = tg + 1;; base += 64) {
            const int r = base + lane;
            const u64 heads = __ballot(r < Bg && group_head[min(r, Bg - 1)] == r);
            if (heads) { e = base + __builtin_ctzll(heads); break; }
            if (base + 64 >= Bg) { e = Bg; break; }
        }
    }
    const int nk2 = K >> 6;
    const _Float16* qp = query + (int64_t)q * ld + lg * 8;
    const int* mrow = row_mask ? row_mask + (int64_t)q * mask_step : nullptr;
    float qm = 0.f, qs = 1.f;
    if constexpr (DSL) {
        if (!on_gallery) { qm = stat_m[q]; qs = stat_s[q]; }
    }
    u64 best = 0;                                                                      // GROUPED: the group's best key so far
    float xt = 0.f;                                                                    // rows mode: the target's score (one lane group)
    for (int t = h >> 4; t <= (e - 1) >> 4; ++t) {
        const _Float16* gp = gallery + (int64_t)min(t * 16 + l15, Bg - 1) * ld + lg * 8;     // rows at Bg or above are never read
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < nk2; s0 += TK_BATCH) {                                   // TK_BATCH pairs of k-slices requested at once
            h8 b[2 * TK_BATCH], a[2 * TK_BATCH];
#pragma unroll
            for (int u = 0; u < TK_BATCH; ++u) {
                const int s = min(s0 + u, nk2 - 1);                                    // (beyond the row's end: read again, not multiplied)
                b[2 * u] = *reinterpret_cast<const h8*>(gp + s * 64);
                b[2 * u + 1] = *reinterpret_cast<const h8*>(gp + s * 64 + 32);
                a[2 * u] = *reinterpret_cast<const h8*>(qp + s * 64);
                a[2 * u + 1] = *reinterpret_cast<const h8*>(qp + s * 64 + 32);
            }
#pragma unroll
            for (int u = 0; u < TK_BATCH; ++u) {
                if (s0 + u < nk2) {
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[2 * u], a[2 * u], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[2 * u + 1], a[2 * u + 1], acc, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int id = t * 16 + lg * 4 + r, idc = min(id, Bg - 1);
            float x = sc * acc[r];
            if constexpr (DSL) x = on_gallery ? cc_dsl_value(nt, x, stat_m[idc], stat_s[idc]) : cc_dsl_value(nt, x, qm, qs);
            if constexpr (GROUPED) {
                bool sel = id >= h && id < e;
                if (mrow) sel = sel && ((mrow[idc >> 5] >> (idc & 31)) & 1);
                const u64 key = sel ? tk_key(x, id) : 0;
                best = key > best ? key : best;
            } else {
                xt = id == tg ? x : xt;
            }
        }
    }
    if constexpr (GROUPED) {
        best = tk_group_max(best);                                                     // (all 16 columns hold the same values)
        int id;
        tk_decode(best, xt, id);
        if (lane == 0) tscore[q] = xt;
    } else {
        if (l15 == 0 && lg == ((tg & 15) >> 2)) tscore[q] = xt;
    }
}

// Second launch: the counts, on topk_stream_kernel's grid: stage the query rows, count what the producer hands over, reduce,
// write.  Every lane keeps three integers for query row l15 against t = tscore[q]: candidates with x > t, with x == t, and with
// x == t in front of the target (rows mode: a candidate is a selectable row < Bg, in front = its index below target[q];
// GROUPED: a candidate is a key the producer hands over - the best key of a finished group, 0 for one without a selectable
// row - in front = its row below the target group's head).  Plain float compares, as rank_counts_kernel: -0 == +0, a NaN is
// neither greater nor equal; in rows mode the score never passes through a key.  A query row whose target is outside [0, Bg)
// counts nothing.  At the end the 4 lanes of a query row and the 4 waves are added: part [Bq][3][slices].
// COUNT: the bound comes from the caller instead of a target (cc_similarity_count_planes_f32): `tscore` holds the bound's score
// and `target` the position in front of which an equal candidate counts as "in front", taken as it is (no group_head look-up,
// no upper limit: a position at Bg or above puts every equal candidate in front; a negative one makes the query row count
// nothing).
template <bool DSL, bool GROUPED, int MASK, bool COUNT>
__global__ __launch_bounds__(256) void rank_stream_kernel(const _Float16* __restrict__ query, const _Float16* __restrict__ gallery,
                                                          int Bq, int Bg, int ld, int K, float sc, int slices,
                                                          const int* __restrict__ target, const float* __restrict__ tscore,
                                                          int* __restrict__ part, const float* __restrict__ stat_m,
                                                          const float* __restrict__ stat_s, int on_gallery, float nt,
                                                          const int* __restrict__ group_head, const int* __restrict__ row_mask,
                                                          int mask_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
    __shared__ int pc[TK_WAVES][3][TK_QROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
    const int slice = blockIdx.x, q0 = blockIdx.y * TK_QROWS;
    _Float16* qs = reinterpret_cast<_Float16*>(tk_smem);                               // [16][K + TK_QPAD]
    tk_stage_rows(qs, query, q0, Bq, ld, K);
    __syncthreads();

    const int qr = min(q0 + l15, Bq - 1);
    const int tg = target[qr];
    const bool qvalid = q0 + l15 < Bq && tg >= 0 && (COUNT || tg < Bg);
    const float tq = tscore[qr];
    int front = tg;                                                                    // a candidate row below it lies in front
    if constexpr (GROUPED && !COUNT) front = min(max(group_head[min(max(tg, 0), Bg - 1)], 0), tg);
    int gt = 0, eq = 0, before = 0;
    auto count = [&](bool in, float x, int id) {
        gt += (in && x > tq) ? 1 : 0;
        eq += (in && x == tq) ? 1 : 0;
        before += (in && x == tq && id < front) ? 1 : 0;
    };
    const TkSource src{gallery, Bg, ld, K, sc, slice, slices, stat_m, stat_s, on_gallery, nt, group_head, row_mask, mask_words};
    tk_candidates<DSL, GROUPED, MASK>(
        src, qs, qr, qvalid,
        [&](const float (&x)[4], const int (&id)[4], const bool (&in)[4]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) count(in[r], x[r], id[r]);
        },
        [&](u64 (&key)[4]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x;
                int id;
                tk_decode(key[r], x, id);
                count(key[r] != 0, x, id);
            }
        });
    int c[3] = {gt, eq, before};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] += __shfl_xor(c[i], 16, CC_WAVE);
        c[i] += __shfl_xor(c[i], 32, CC_WAVE);
        if (lg == 0) pc[wave][i][l15] = c[i];
    }
    __syncthreads();
    if (threadIdx.x < 3 * TK_QROWS) {
        const int i = threadIdx.x >> 4, l = threadIdx.x & 15;
        if (q0 + l < Bq) part[((int64_t)(q0 + l) * 3 + i) * slices + slice] = pc[0][i][l] + pc[1][i][l] + pc[2][i][l] + pc[3][i][l];
    }
}

// Third launch: part [n][slices] -> counts [n] (n = 3 Bq), one wave per count: the lanes take the slices 64 apart, then the
// wave adds up.  Integers: the order does not matter.
__global__ __launch_bounds__(256) void rank_reduce_kernel(const int* __restrict__ part, int slices, int n, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * TK_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    int a = 0;
    for (int s = lane; s < slices; s += 64) a += part[(int64_t)i * slices + s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, CC_WAVE);
    if (lane == 0) counts[i] = a;
}

// ---------------------------------------------------------------------------- the lists of several shards -> one list
// S descending lists of k entries per query row (scores / ids [S][Bq][k]; id < 0: a fill, whatever its score) -> the first k of
// their union.  An entry's place in the union's order is decided by (fills last; tk_key's score part: the ordered bits of
// score + 0.0f, larger first; smaller shard; smaller local id - a fill: smaller index in its list), a strict total order over
// all S k entries.  Every list is in that order already (the caller's precondition), so the entries of list t in front of an
// entry form a prefix of t, a binary search finds its length, and the entry's output slot is its own index plus those
// lengths over the other lists.  Slots are distinct and cover [0, S k): every slot below k has exactly one writer - no atomics,
// no initialisation pass, no LDS.  One lane per entry, grid (query rows) x (blocks of 256 entries): one query row already
// spreads over S k / 256 workgroups; a lane stops as soon as its slot reaches k (slots only grow), which is where most lanes
// of a deep list end.  The score is written with the bits it came with (the sign of a zero included).
struct TmEntry {
    u64 major;                                                                         // 0: a fill; else 2^32 | ordered score bits
    u64 minor;                                                                         // shard : 32 | local id (a fill: its index)
};
__device__ __forceinline__ TmEntry tm_entry(const float* __restrict__ scores, const int* __restrict__ ids, int64_t base, int s, int i) {
    const int id = ids[base + i];
    TmEntry e;
    e.major = id < 0 ? 0 : ((u64)1 << 32) | cc_float_to_ordered_uint(scores[base + i] + 0.0f);
    e.minor = ((u64)(unsigned)s << 32) | (unsigned)(id < 0 ? i : id);
    return e;
}
__device__ __forceinline__ bool tm_in_front(const TmEntry& a, const TmEntry& b) {
    return a.major > b.major || (a.major == b.major && a.minor < b.minor);
}

__global__ __launch_bounds__(256) void topk_merge_lists_kernel(const float* __restrict__ scores, const int* __restrict__ ids, int S, int Bq,
                                                               int k, float* __restrict__ out_scores, long long* __restrict__ out_ids,
                                                               int* __restrict__ out_src) {
    const int q = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    if (e >= S * k) return;                                                            // (no barrier below)
    const int s = e / k, i = e - s * k;
    const TmEntry mine = tm_entry(scores, ids, ((int64_t)s * Bq + q) * k, s, i);
    int slot = i;
    for (int t = 0; t < S && slot < k; ++t) {
        if (t == s) continue;
        const int64_t base = ((int64_t)t * Bq + q) * k;
        int lo = 0, hi = k;                                                            // entries [0, lo) of list t lie in front
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;                                            // (< k: inside the list)
            if (tm_in_front(tm_entry(scores, ids, base, t, mid), mine)) lo = mid + 1;
            else hi = mid;
        }
        slot += lo;
    }
    if (slot >= k) return;
    const int64_t o = (int64_t)q * k + slot, from = ((int64_t)s * Bq + q) * k + i;
    const int id = ids[from];
    out_scores[o] = id < 0 ? -INFINITY : scores[from];
    out_ids[o] = id < 0 ? -1ll : (long long)(((u64)(unsigned)s << 32) | (unsigned)id);
    out_src[o] = id < 0 ? -1 : e;
}

// The (m, s) pairs of the 16 video rows from blockIdx.y * 16 on over the text tiles of slice blockIdx.x (the tree: the file's
// head).  part [slices][Bv] pairs.  The split of the text rows uses Bt alone.  MASKED: text_mask is one mask row over the text
// rows (topk_stream_kernel's format); a row whose bit is 0 is treated as a row at Bt or above - neither its maximum nor its
// expf term enters - and a tile without a selectable row is skipped (TkLive), which leaves the lane's pair as it is: the pair
// of a video row is the unmasked tree with those terms left out, (-inf, 0) without any.
template <bool MASKED>
__global__ __launch_bounds__(256) void dsl_stats_stream_kernel(const _Float16* __restrict__ video, const _Float16* __restrict__ text,
                                                               int Bv, int Bt, int ld, int K, float sc, int slices,
                                                               float* __restrict__ part, const int* __restrict__ text_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
    __shared__ float pm[TK_WAVES][4][TK_QROWS], ps[TK_WAVES][4][TK_QROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
    const int slice = blockIdx.x, v0 = blockIdx.y * TK_QROWS;
    _Float16* vs = reinterpret_cast<_Float16*>(tk_smem);                               // [16][K + TK_QPAD]
    tk_stage_rows(vs, video, v0, Bv, ld, K);
    __syncthreads();
    int t0, t1;
    tk_slice_tiles(Bt, slice, slices, t0, t1);
    float m = -INFINITY, s = 0.f;                                                      // of video row l15 over the lane's text rows
    int mw = 0;                                                                        // MASKED: the mask word of the tile's 16 bits
    auto before_last = [&](int t) {
        if constexpr (MASKED) mw = text_mask[t >> 1];
    };
    auto on_tile = [&](int t, const f32x4& acc) {
        float x[4], mt = m;
        bool in[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool sel = MASKED ? tk_mask_bit(mw, t, lg, r) : true;
            in[r] = sel && t * 16 + lg * 4 + r < Bt;
            x[r] = sc * acc[r];
            mt = in[r] ? fmaxf(mt, x[r]) : mt;
        }
        float a = cc_dsl_share(s, m, mt);
#pragma unroll
        for (int r = 0; r < 4; ++r) a += in[r] ? expf(x[r] - mt) : 0.f;
        s = a;
        m = mt;
    };
    tk_stream_rule<MASKED>(text, Bt, ld, K, vs + l15 * (K + TK_QPAD) + lg * 8, text_mask, t0 + wave, TK_WAVES, t1, before_last,
                           on_tile);
    pm[wave][lg][l15] = m;
    ps[wave][lg][l15] = s;
    __syncthreads();
    if (threadIdx.x < TK_QROWS && v0 + threadIdx.x < Bv) {
        const int v = threadIdx.x;
        float mm = -INFINITY;
#pragma unroll
        for (int i = 0; i < TK_WAVES * 4; ++i) mm = fmaxf(mm, pm[i >> 2][i & 3][v]);
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < TK_WAVES * 4; ++i) a += cc_dsl_share(ps[i >> 2][i & 3][v], pm[i >> 2][i & 3][v], mm);
        float* p = part + ((int64_t)slice * Bv + v0 + v) * 2;
        p[0] = mm;
        p[1] = a;
    }
}

// flags [R][n] bytes (non-zero = 1) -> out [R][W] mask words: a wave packs 64 flags with one ballot and two of its lanes store
// the two words (W >= ceil(n / 32); flags at n or above count as 0).  grid: (ceil(32 W / 256), rows, strided over R).
__global__ __launch_bounds__(256) void pack_row_mask_kernel(const uint8_t* __restrict__ flags, int R, int n, int* __restrict__ out,
                                                            int W) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;                         // the flag of this lane
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        const u64 b = __ballot(i < n && flags[(int64_t)r * n + min(i, (int64_t)n - 1)] != 0);
        const int64_t w = i >> 5;
        if ((lane & 31) == 0 && w < W) out[(int64_t)r * W + w] = (int)(unsigned)(lane ? b >> 32 : b);
    }
}

int tk_slices(int Bq, int Bg) {
    const int groups = (max(Bq, 1) + TK_QROWS - 1) / TK_QROWS, tiles = (max(Bg, 1) + 15) / 16;
    const int want = (TK_TARGET_WGS + groups - 1) / groups, cap = tiles / TK_MIN_TILES;
    return max(1, min(want, cap));
}
// text slices of the statistics pass: a function of Bt ALONE (a video row's pair must not depend on the rows it shares a call
// with), at least TK_MIN_TILES tiles a slice
int dsl_stats_slices(int Bt) { return max(1, min(DSL_MAX_SLICES, (max(Bt, 1) + 15) / 16 / TK_MIN_TILES)); }
size_t tk_stream_lds(int K, int k) { return (size_t)TK_QROWS * (K + TK_QPAD) * 2 + (size_t)TK_WAVES * TK_QROWS * k * sizeof(u64); }
// the longest list (page) the stream's LDS holds next to 16 staged rows of K halfs: TK_MAXK, 127 for K = 3072
int tk_page_len(int K) {
    int page = TK_MAXK;
    while (page > 1 && tk_stream_lds(K, page) > TK_LDS_LIMIT) --page;
    return page;
}
// sc of a score: mult * 2^-20, as the matrix GEMM's epilogue
float tk_scale(float mult) { return mult * 9.5367431640625e-07f; }
int tk_row_groups(int Bq) { return (Bq + TK_QROWS - 1) / TK_QROWS; }

// A search request: what every list, rank and count entry is asked over.  dsl / grouped / masked say which of the optional
// parts the ENTRY asks for (the plain entries by their name, the others by the pointers they got), so a part that is asked
// for and missing is refused.  Without dsl, on_gallery and n_total are 0 whatever the caller passed.
struct TkRequest {
    const _Float16* query;
    const _Float16* gallery;
    int Bq, Bg, E;
    float mult;
    int products;
    bool dsl;
    const float* m;
    const float* s;
    int on_gallery, n_total;
    bool grouped;
    const int* group_head;
    bool masked;
    const int* row_mask;
    int mask_rows, mask_words;
    int K() const { return products * E; }
    int mask_mode() const { return !masked ? 0 : mask_rows == 1 ? 1 : 2; }            // one mask row also when Bq == 1
    dim3 grid() const { return dim3(tk_slices(Bq, Bg), tk_row_groups(Bq)); }
};
TkRequest tk_request(const void* query, const void* gallery, int Bq, int Bg, int E, float mult, int products, bool dsl, const float* m,
                     const float* s, int on_gallery, int n_total, bool grouped, const int* group_head, bool masked,
                     const int* row_mask, int mask_rows, int mask_words) {
    return TkRequest{static_cast<const _Float16*>(query), static_cast<const _Float16*>(gallery), Bq, Bg, E, mult, products, dsl, m, s,
                     dsl ? on_gallery : 0, dsl ? n_total : 0, grouped, group_head, masked, row_mask, mask_rows, mask_words};
}
// m, s, group_head and row_mask all optional, each part asked for by its pointer (the deep, rank, target-score and count
// entries; exactly one of m, s: refused as a dsl request)
TkRequest tk_request(const void* query, const void* gallery, int Bq, int Bg, int E, float mult, int products, const int* row_mask,
                     int mask_rows, int mask_words, const float* m, const float* s, int on_gallery, int n_total,
                     const int* group_head) {
    return tk_request(query, gallery, Bq, Bg, E, mult, products, m || s, m, s, on_gallery, n_total, group_head != nullptr, group_head,
                      row_mask != nullptr, row_mask, mask_rows, mask_words);
}

// The refusals all entries share.  Every entry refuses what is invalid before what is unsupported, and the workspace last:
// an entry passes its own invalid / unsupported conditions (missing outputs, k, the cursor pair) and checks its workspace
// behind this.  stream_grid: the entry launches on the stream's grid (grid.y: a million query rows a call).
int tk_check(const TkRequest& r, bool own_invalid, bool own_unsupported, bool stream_grid = true) {
    if (!r.query || !r.gallery || r.Bq <= 0 || r.Bg <= 0 || r.E <= 0 || own_invalid) return CC_ERR_INVALID;
    if (r.dsl && (!r.m || !r.s || r.n_total < 0 || (r.on_gallery != 0 && r.on_gallery != 1))) return CC_ERR_INVALID;
    if (r.grouped && !r.group_head) return CC_ERR_INVALID;
    if (r.masked && (!r.row_mask || (r.mask_rows != 1 && r.mask_rows != r.Bq) || r.mask_words < (r.Bg - 1) / 32 + 1))
        return CC_ERR_INVALID;
    if (own_unsupported || r.products < 1 || r.products > 3 || (r.E & 63) || r.E > 1024) return CC_ERR_UNSUPPORTED;
    if (stream_grid && tk_row_groups(r.Bq) > 65535) return CC_ERR_UNSUPPORTED;
    return CC_OK;
}

template <int MASK, bool BOUND>
auto tk_stream_kernel_of(bool dsl, bool grouped) {
    return grouped ? (dsl ? topk_stream_kernel<true, true, MASK, BOUND> : topk_stream_kernel<false, true, MASK, BOUND>)
                   : (dsl ? topk_stream_kernel<true, false, MASK, BOUND> : topk_stream_kernel<false, false, MASK, BOUND>);
}
template <bool BOUND>
auto tk_stream_kernel_of(const TkRequest& r) {
    return r.mask_mode() == 0   ? tk_stream_kernel_of<0, BOUND>(r.dsl, r.grouped)
           : r.mask_mode() == 1 ? tk_stream_kernel_of<1, BOUND>(r.dsl, r.grouped)
                                : tk_stream_kernel_of<2, BOUND>(r.dsl, r.grouped);
}
template <int MASK, bool COUNT>
auto rank_stream_kernel_of(bool dsl, bool grouped) {
    return grouped ? (dsl ? rank_stream_kernel<true, true, MASK, COUNT> : rank_stream_kernel<false, true, MASK, COUNT>)
                   : (dsl ? rank_stream_kernel<true, false, MASK, COUNT> : rank_stream_kernel<false, false, MASK, COUNT>);
}
template <bool COUNT>
auto rank_stream_kernel_of(const TkRequest& r) {
    return r.mask_mode() == 0   ? rank_stream_kernel_of<0, COUNT>(r.dsl, r.grouped)
           : r.mask_mode() == 1 ? rank_stream_kernel_of<1, COUNT>(r.dsl, r.grouped)
                                : rank_stream_kernel_of<2, COUNT>(r.dsl, r.grouped);
}

// The pages of a list of k entries, `page` entries each (the last one what is left): per page the list stream and the merge,
// which writes the page at its column offset of scores / ids [Bq, k] and - if a page follows - its last key to `cursor`.
// bounded: the first page already lies below `cursor`; every page behind the first does.  One page, not bounded, no cursor
// buffer: the two launches of a plain list.
int tk_launch_pages(const TkRequest& r, int k, int page, bool bounded, u64* lists, u64* cursor, float* scores, int32_t* ids,
                    hipStream_t st) {
    const int K = r.K(), slices = tk_slices(r.Bq, r.Bg);
    for (int done = 0; done < k; done += page, bounded = true) {
        const int kp = min(page, k - done);
        const size_t smem = tk_stream_lds(K, kp);
        const auto kernel = bounded ? tk_stream_kernel_of<true>(r) : tk_stream_kernel_of<false>(r);
        if (cc_allow_dynamic_lds(reinterpret_cast<const void*>(kernel), smem) != CC_OK) return CC_ERR_HIP;
        hipLaunchKernelGGL(kernel, r.grid(), dim3(256), smem, st, r.query, r.gallery, r.Bq, r.Bg, 3 * r.E, K, tk_scale(r.mult), kp,
                           slices, lists, r.m, r.s, r.on_gallery, (float)r.n_total, r.group_head, r.row_mask, r.mask_words,
                           static_cast<const u64*>(cursor));
        CC_LAUNCH_CHECK();
        hipLaunchKernelGGL(topk_merge_kernel, dim3(r.Bq), dim3(64), 0, st, static_cast<const u64*>(lists), slices, kp, scores + done,
                           ids + done, k, done + kp < k ? cursor : static_cast<u64*>(nullptr));
        CC_LAUNCH_CHECK();
    }
    return CC_OK;
}

// t_q of every query row's target -> score (rank_target_kernel)
int tk_launch_target(const TkRequest& r, const int32_t* target, float* score, hipStream_t st) {
    const auto kernel = r.grouped ? (r.dsl ? rank_target_kernel<true, true> : rank_target_kernel<false, true>)
                                  : (r.dsl ? rank_target_kernel<true, false> : rank_target_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((r.Bq + TK_WAVES - 1) / TK_WAVES), dim3(256), 0, st, r.query, r.gallery, r.Bq, r.Bg, 3 * r.E, r.K(),
                       tk_scale(r.mult), target, score, r.m, r.s, r.on_gallery, (float)r.n_total, r.group_head, r.row_mask,
                       r.mask_rows == 1 ? 0 : r.mask_words);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

// the count stream against tscore and target (bound: the caller's bound and front position, rank_stream_kernel's COUNT mode),
// then the reduce: part [Bq][3][slices] -> counts [Bq][3]
int tk_launch_count(const TkRequest& r, bool bound, const int32_t* target, const float* tscore, int* part, int32_t* counts,
                    hipStream_t st) {
    const int K = r.K(), slices = tk_slices(r.Bq, r.Bg);
    const size_t smem = tk_stream_lds(K, 0);                                // the staged rows: no lists, no (E, products) exclusion
    const auto kernel = bound ? rank_stream_kernel_of<true>(r) : rank_stream_kernel_of<false>(r);
    if (cc_allow_dynamic_lds(reinterpret_cast<const void*>(kernel), smem) != CC_OK) return CC_ERR_HIP;
    hipLaunchKernelGGL(kernel, r.grid(), dim3(256), smem, st, r.query, r.gallery, r.Bq, r.Bg, 3 * r.E, K, tk_scale(r.mult), slices, target,
                       tscore, part, r.m, r.s, r.on_gallery, (float)r.n_total, r.group_head, r.row_mask, r.mask_words);
    CC_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_reduce_kernel, dim3((3 * r.Bq + TK_WAVES - 1) / TK_WAVES), dim3(256), 0, st, static_cast<const int*>(part),
                       slices, 3 * r.Bq, counts);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

}  // namespace

extern "C" {

int32_t cc_similarity_topk_slices(int32_t Bq, int32_t Bg, int32_t k) {
    (void)k;                                    // the split follows the grid alone; k only sizes a list
    return tk_slices(Bq, Bg);
}

size_t cc_similarity_topk_workspace_bytes(int32_t Bq, int32_t Bg, int32_t k) {
    if (Bq <= 0 || Bg <= 0 || k <= 0) return 0;
    return cc_align_up((size_t)Bq * tk_slices(Bq, Bg) * k * sizeof(u64), 256);
}

// the plain / dsl / grouped / masked entries: a list of at most TK_MAXK entries that the stream's LDS holds, as one page
static int tk_launch(const TkRequest& r, int32_t k, float* scores, int32_t* ids, void* ws, size_t ws_bytes, void* stream) {
    if (const int rc = tk_check(r, !scores || !ids, k < 1 || k > TK_MAXK)) return rc;
    if (tk_stream_lds(r.K(), k) > TK_LDS_LIMIT) return CC_ERR_UNSUPPORTED;  // products * E = 3072 with k = 128 only
    if (!ws || ws_bytes < cc_similarity_topk_workspace_bytes(r.Bq, r.Bg, k)) return CC_ERR_WORKSPACE;
    return tk_launch_pages(r, k, k, false, static_cast<u64*>(ws), nullptr, scores, ids, static_cast<hipStream_t>(stream));
}

int cc_similarity_topk_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                  float mult, int32_t products, int32_t k, float* scores, int32_t* ids, void* ws,
                                  size_t ws_bytes, void* stream) {
    return tk_launch(tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, false, nullptr, nullptr, 0, 0, false, nullptr,
                                false, nullptr, 0, 0), k, scores, ids, ws, ws_bytes, stream);
}

int cc_similarity_topk_dsl_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                      float mult, int32_t products, int32_t k, const float* m, const float* s,
                                      int32_t stats_on_gallery, int32_t n_total, float* scores, int32_t* ids, void* ws,
                                      size_t ws_bytes, void* stream) {
    return tk_launch(tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, true, m, s, stats_on_gallery, n_total, false,
                                nullptr, false, nullptr, 0, 0), k, scores, ids, ws, ws_bytes, stream);
}

int cc_similarity_topk_grouped_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                          float mult, int32_t products, int32_t k, const int32_t* group_head, float* scores,
                                          int32_t* ids, void* ws, size_t ws_bytes, void* stream) {
    return tk_launch(tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, false, nullptr, nullptr, 0, 0, true, group_head,
                                false, nullptr, 0, 0), k, scores, ids, ws, ws_bytes, stream);
}

int cc_similarity_topk_grouped_dsl_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg,
                                              int32_t E, float mult, int32_t products, int32_t k, const float* m, const float* s,
                                              int32_t stats_on_gallery, int32_t n_total, const int32_t* group_head, float* scores,
                                              int32_t* ids, void* ws, size_t ws_bytes, void* stream) {
    return tk_launch(tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, true, m, s, stats_on_gallery, n_total, true,
                                group_head, false, nullptr, 0, 0), k, scores, ids, ws, ws_bytes, stream);
}

int cc_similarity_topk_masked_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                         float mult, int32_t products, int32_t k, const int32_t* row_mask, int32_t mask_rows,
                                         int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery,
                                         int32_t n_total, const int32_t* group_head, float* scores, int32_t* ids, void* ws,
                                         size_t ws_bytes, void* stream) {
    return tk_launch(tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, m || s, m, s, stats_on_gallery, n_total,
                                group_head != nullptr, group_head, true, row_mask, mask_rows, mask_words),      // (a mask it must have)
                     k, scores, ids, ws, ws_bytes, stream);
}

// one page's workspace (the plain entry's at the page length), then the cursor buffer: u64 [Bq]
size_t cc_similarity_topk_deep_workspace_bytes(int32_t Bq, int32_t Bg, int32_t E, int32_t products, int32_t k) {
    if (Bq <= 0 || Bg <= 0 || E <= 0 || k < 1 || k > CC_TOPK_DEEP_MAXK) return 0;
    if (products < 1 || products > 3 || (E & 63) || E > 1024) return 0;
    return cc_similarity_topk_workspace_bytes(Bq, Bg, min(k, tk_page_len(products * E)))
           + cc_align_up((size_t)Bq * sizeof(u64), 256);
}

int cc_similarity_topk_deep_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                       float mult, int32_t products, int32_t k, const int32_t* row_mask, int32_t mask_rows,
                                       int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery, int32_t n_total,
                                       const int32_t* group_head, const float* after_scores, const int32_t* after_ids, float* scores,
                                       int32_t* ids, void* ws, size_t ws_bytes, void* stream) {
    const TkRequest r = tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, row_mask, mask_rows, mask_words, m, s,
                                   stats_on_gallery, n_total, group_head);
    if (const int rc = tk_check(r, !scores || !ids || k < 1 || !after_scores != !after_ids, k > CC_TOPK_DEEP_MAXK)) return rc;
    if (!ws || ws_bytes < cc_similarity_topk_deep_workspace_bytes(Bq, Bg, E, products, k)) return CC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int page = min(k, tk_page_len(r.K()));
    u64* cursor = reinterpret_cast<u64*>(static_cast<char*>(ws) + cc_similarity_topk_workspace_bytes(Bq, Bg, page));
    if (after_scores) {
        hipLaunchKernelGGL(topk_cursor_kernel, dim3((Bq + 255) / 256), dim3(256), 0, st, after_scores, after_ids, Bq, cursor);
        CC_LAUNCH_CHECK();
    }
    return tk_launch_pages(r, k, page, after_scores != nullptr, static_cast<u64*>(ws), cursor, scores, ids, st);
}

size_t cc_similarity_rank_workspace_bytes(int32_t Bq, int32_t Bg) {
    if (Bq <= 0 || Bg <= 0) return 0;
    return cc_align_up((size_t)tk_slices(Bq, Bg) * Bq * 3 * sizeof(int32_t), 256);
}

int cc_similarity_rank_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E, float mult,
                                  int32_t products, const int32_t* target, const int32_t* row_mask, int32_t mask_rows,
                                  int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery, int32_t n_total,
                                  const int32_t* group_head, int32_t* counts, float* score, void* ws, size_t ws_bytes, void* stream) {
    const TkRequest r = tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, row_mask, mask_rows, mask_words, m, s,
                                   stats_on_gallery, n_total, group_head);
    if (const int rc = tk_check(r, !target || !counts || !score, false)) return rc;
    if (!ws || ws_bytes < cc_similarity_rank_workspace_bytes(Bq, Bg)) return CC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = tk_launch_target(r, target, score, st)) return rc;
    return tk_launch_count(r, false, target, score, static_cast<int*>(ws), counts, st);
}

int cc_topk_merge_lists_f32(const float* scores, const int32_t* ids, int32_t S, int32_t Bq, int32_t k, float* out_scores,
                            int64_t* out_ids, int32_t* out_src, void* stream) {
    if (!scores || !ids || !out_scores || !out_ids || !out_src || S < 1 || Bq <= 0 || k < 1) return CC_ERR_INVALID;
    if (S > CC_TOPK_MERGE_MAX_LISTS || k > CC_TOPK_DEEP_MAXK) return CC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(topk_merge_lists_kernel, dim3(Bq, (S * k + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), scores, ids,
                       S, Bq, k, out_scores, reinterpret_cast<long long*>(out_ids), out_src);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

// the first launch of cc_similarity_rank_planes_f32 on its own: its checks but the grid's and the workspace's
int cc_similarity_target_score_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                          float mult, int32_t products, const int32_t* target, const int32_t* row_mask,
                                          int32_t mask_rows, int32_t mask_words, const float* m, const float* s,
                                          int32_t stats_on_gallery, int32_t n_total, const int32_t* group_head, float* score,
                                          void* stream) {
    const TkRequest r = tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, row_mask, mask_rows, mask_words, m, s,
                                   stats_on_gallery, n_total, group_head);
    if (const int rc = tk_check(r, !target || !score, false, false)) return rc;
    return tk_launch_target(r, target, score, static_cast<hipStream_t>(stream));
}

size_t cc_similarity_count_workspace_bytes(int32_t Bq, int32_t Bg) { return cc_similarity_rank_workspace_bytes(Bq, Bg); }

// the counting pass and the reduce of cc_similarity_rank_planes_f32 against a bound the caller holds
int cc_similarity_count_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E, float mult,
                                   int32_t products, const float* bound_scores, const int32_t* bound_front, const int32_t* row_mask,
                                   int32_t mask_rows, int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery,
                                   int32_t n_total, const int32_t* group_head, int32_t* counts, void* ws, size_t ws_bytes,
                                   void* stream) {
    const TkRequest r = tk_request(query_planes, gallery_planes, Bq, Bg, E, mult, products, row_mask, mask_rows, mask_words, m, s,
                                   stats_on_gallery, n_total, group_head);
    if (const int rc = tk_check(r, !bound_scores || !bound_front || !counts, false)) return rc;
    if (!ws || ws_bytes < cc_similarity_count_workspace_bytes(Bq, Bg)) return CC_ERR_WORKSPACE;
    return tk_launch_count(r, true, bound_front, bound_scores, static_cast<int*>(ws), counts, static_cast<hipStream_t>(stream));
}

int cc_pack_row_mask_u8(const uint8_t* flags, int32_t rows, int32_t n, int32_t* out_words, int32_t words_per_row, void* stream) {
    if (!flags || !out_words || rows <= 0 || n <= 0 || words_per_row < (n - 1) / 32 + 1) return CC_ERR_INVALID;
    hipLaunchKernelGGL(pack_row_mask_kernel, dim3((words_per_row + 7) / 8, min(rows, 65535)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), flags, rows, n, out_words, words_per_row);
    CC_LAUNCH_CHECK();
    return CC_OK;
}

int32_t cc_dsl_col_stats_planes_slices(int32_t Bt) { return Bt > 0 ? dsl_stats_slices(Bt) : 0; }

size_t cc_dsl_col_stats_planes_workspace_bytes(int32_t Bt, int32_t Bv) {
    if (Bt <= 0 || Bv <= 0) return 0;
    return cc_align_up((size_t)dsl_stats_slices(Bt) * Bv * 2 * sizeof(float), 256);
}

// the checks and the two launches of both statistics entries
static int dsl_stats_launch(bool masked, const void* text_planes, const void* video_planes, int32_t Bt, int32_t Bv, int32_t E,
                            float mult, int32_t products, const int32_t* text_mask, float* m, float* s, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!video_planes || !m || !s || Bt < 0 || Bv <= 0 || E <= 0 || (Bt > 0 && !text_planes)) return CC_ERR_INVALID;
    if (masked && Bt > 0 && !text_mask) return CC_ERR_INVALID;
    if (products < 1 || products > 3 || (E & 63) || E > 1024) return CC_ERR_UNSUPPORTED;
    const int K = products * E;
    const size_t smem = tk_stream_lds(K, 0);
    if (smem > TK_LDS_LIMIT) return CC_ERR_UNSUPPORTED;                   // (never with E <= 1024: 96 KB at most)
    if ((Bv + TK_QROWS - 1) / TK_QROWS > 65535) return CC_ERR_UNSUPPORTED;  // (grid.y: a million video rows a call)
    if (Bt > 0 && (!ws || ws_bytes < cc_dsl_col_stats_planes_workspace_bytes(Bt, Bv))) return CC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int slices = Bt > 0 ? dsl_stats_slices(Bt) : 0;
    if (slices > 0) {
        const auto kernel = masked ? dsl_stats_stream_kernel<true> : dsl_stats_stream_kernel<false>;
        if (cc_allow_dynamic_lds(reinterpret_cast<const void*>(kernel), smem) != CC_OK) return CC_ERR_HIP;
        hipLaunchKernelGGL(kernel, dim3(slices, (Bv + TK_QROWS - 1) / TK_QROWS), dim3(256), smem, st,
                           static_cast<const _Float16*>(video_planes), static_cast<const _Float16*>(text_planes), Bv, Bt, 3 * E, K,
                           tk_scale(mult), slices, static_cast<float*>(ws), text_mask);
        CC_LAUNCH_CHECK();
    }
    return cc_launch_dsl_col_merge(static_cast<const float*>(ws), slices, Bv, m, s, st);      // no slice: (-inf, 0)
}

int cc_dsl_col_stats_planes_f32(const void* text_planes, const void* video_planes, int32_t Bt, int32_t Bv, int32_t E, float mult,
                                int32_t products, float* m, float* s, void* ws, size_t ws_bytes, void* stream) {
    return dsl_stats_launch(false, text_planes, video_planes, Bt, Bv, E, mult, products, nullptr, m, s, ws, ws_bytes, stream);
}

int cc_dsl_col_stats_planes_masked_f32(const void* text_planes, const void* video_planes, int32_t Bt, int32_t Bv, int32_t E,
                                       float mult, int32_t products, const int32_t* text_mask, float* m, float* s, void* ws,
                                       size_t ws_bytes, void* stream) {
    return dsl_stats_launch(true, text_planes, video_planes, Bt, Bv, E, mult, products, text_mask, m, s, ws, ws_bytes, stream);
}

}  // extern "C"
