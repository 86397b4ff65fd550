/*
 * centerclip_hip.h - C ABI of libcenterclip_hip.so (gfx950 / MI355X).
 *
 * The reference (mzhaoshuai/CenterCLIP) is pure Python/PyTorch: it has no FFI or
 * operator registry, its boundary is a set of Python call signatures (SURVEY.md
 * §8b).  This header declares the C entry points a maintainer of the reference
 * binds (ctypes stub in INTEGRATION.md) to replace those call sites.  Every
 * declaration cites the reference interface it replaces (paths relative to the
 * reference repository root).
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless the
 *     name ends in _host; `stream` is a hipStream_t passed as void* (NULL = the
 *     null stream); nothing in here allocates, synchronises the device or
 *     throws: workspace is caller-owned (size it with the *_workspace_bytes
 *     query), every call only enqueues kernels on `stream`;
 *   - return value: CC_OK or a negative cc_status; cc_status_string() names it;
 *   - fp32 tensors are IEEE binary32, index outputs are int64 (torch.long), as
 *     the reference returns them;
 *   - re-entrant: no global state besides per-kernel function attributes.
 */
#ifndef CENTERCLIP_HIP_H
#define CENTERCLIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cc_status {
    CC_OK = 0,
    CC_ERR_INVALID = -1,      /* bad argument (NULL pointer, K > N, non-positive size ...)      */
    CC_ERR_UNSUPPORTED = -2,  /* legal in the reference but not built here      */
    CC_ERR_WORKSPACE = -3,    /* workspace too small / NULL                                      */
    CC_ERR_HIP = -4           /* a HIP runtime call failed (hipGetLastError after a launch ...)  */
} cc_status;

/* Largest `threshold` for which the k-medoids entry points run the whole selection in ONE launch (reference default 1e-5,
 * fast_kmeans.py:14; the shipped scripts pass 1e-6): every problem iterates to its fixed point, which is the final state of
 * the reference's chunk-mean stop test (fast_kmeans.py:85-88) for any threshold below the distance between two distinct
 * tokens.  A looser threshold ends the reference's loop earlier, at a step that depends on all problems of the split chunk:
 * the entry points then run the literal loop (one iteration of every problem per launch + the chunk's center_shift in
 * ATen's summation order, 2 * iter_limit + 2 launches, split_size <= 1024); a NaN threshold is CC_ERR_INVALID. */
#define CC_KMEDOIDS_MAX_THRESHOLD 1e-5f

/* metric: reference strings 'euclidean' / 'cosine' (modules/cluster/cluster_utils.py:21-33) */
#define CC_METRIC_EUCLIDEAN 0
#define CC_METRIC_COSINE 1

const char* cc_version(void);
const char* cc_status_string(int status);

/* ------------------------------------------------------------------------------------------
 * Token addressing shared by the cluster entry points.
 *
 * A clustering problem p = s*B + b (segment-major, modules/cluster/cluster.py:247-250) has
 * N = fd*n tokens; token j = f*n + i (frame-in-segment major).  Its W floats start at
 *     x + b*stride_b + s*stride_s + f*stride_f + i*stride_i          (strides in floats)
 * which covers
 *   - a contiguous [P,N,W] batch (the argument of batch_fast_kmedoids_with_split):
 *         B=P, S=1, fd=1, n=N, stride_b=N*W, stride_i=W;
 *   - the [L=1+n, B*T, W] (LND) activation TokenClusterInter.forward receives, patch rows
 *     only: x += B*T*W, stride_b=T*W, stride_s=fd*W, stride_f=W, stride_i=B*T*W;
 *   - the same activation stored frame-major ([B*T, L, W], NLD): x += W,
 *     stride_b=T*L*W, stride_s=fd*L*W, stride_f=L*W, stride_i=W.
 * ------------------------------------------------------------------------------------------ */
typedef struct cc_token_layout {
    int32_t B;          /* clips (problems per segment)                      */
    int32_t S;          /* segments per clip (T_new); P = S*B                */
    int32_t fd;         /* frames per segment                                */
    int32_t n;          /* tokens per frame; N = fd*n                        */
    int64_t stride_b, stride_s, stride_f, stride_i;
} cc_token_layout;

/* Bytes of scratch the cluster entry points need for P problems of N tokens. */
size_t cc_cluster_workspace_bytes(int32_t P, int32_t N, int32_t W, int32_t pre_norm);

/* L2 norm of every token, norms [P,N] - replaces torch.norm(X, dim=-1) in KKZ_init
 * (modules/cluster/cluster_utils.py:93). */
int cc_token_norms_f32(const float* x, const cc_token_layout* lay, int32_t W, float* norms,
                       void* ws, size_t ws_bytes, void* stream);

/*
 * C3 - replaces pairwise_distance(data, data, metric, self_nearest, all_negative, p)
 *      modules/cluster/cluster_utils.py:8-43 for the self-distance case the hot path uses
 *      (fast_kmeans.py:61-62).  dist [P,N,N] fp32.  `chunk` = number of consecutive
 *      problems that share one max in the all_negative shift (the reference takes the max
 *      of the whole tensor it is handed = one split chunk; pass P for a single call).
 *      norms_out (optional) [P,N] = L2 norm of every token (cluster_utils.py:93).
 */
/* The same function for two DIFFERENT token sets: x1 [P,N1,W], x2 [P,N2,W] contiguous -> dist [P,N1,N2]; the all_negative
 * shift uses the maximum of the whole tensor (cluster_utils.py:35-36), self_nearest lowers dist[.., j, j] for j < N2 (needs
 * N2 <= N1, as the reference's indexing does).  Not on the retrieval path (the k-medoids only ever passes one set).
 * ws: at least 4 bytes when all_negative. */
int cc_pairwise_distance_cross_f32(const float* x1, const float* x2, int32_t P, int32_t N1, int32_t N2, int32_t W,
                                   int32_t metric, float p, int32_t all_negative, int32_t self_nearest, float* dist,
                                   void* ws, size_t ws_bytes, void* stream);
int cc_pairwise_distance_f32(const float* x, const cc_token_layout* lay, int32_t W,
                             int32_t metric, float p, int32_t all_negative, int32_t self_nearest,
                             int32_t chunk, float* dist, float* norms_out,
                             void* ws, size_t ws_bytes, void* stream);

/*
 * C4+C5 from a finished distance tensor (parity level P0): KKZ init
 * (cluster_utils.py:93,106-118), assignment/update iterations, ascending sort and final
 * re-assignment (fast_kmeans.py:65-97).  dist [P,N,N] is used exactly as given (no shift);
 * norms [P,N] selects the first KKZ medoid (first argmax).  Each problem iterates until
 * its medoid vector is unchanged or iter_limit is reached (equivalence 4 in SURVEY §8a).
 * Outputs: medoids [P,K] int64 (ascending if id_sort), assign [P,N] int64 (may be NULL),
 * iters [P] int32 (may be NULL).
 */
int cc_kmedoids_from_dist_f32(const float* dist, const float* norms, int32_t P, int32_t N, int32_t K,
                              int32_t iter_limit, int32_t id_sort,
                              int64_t* medoids, int64_t* assign, int32_t* iters,
                              void* ws, size_t ws_bytes, void* stream);

/*
 * C2..C5 - replaces batch_fast_kmedoids_with_split(X, K, distance, threshold, iter_limit,
 *      id_sort, norm_p, split_size, pre_norm)  modules/cluster/fast_kmeans.py:14-40 and
 *      batch_fast_kmedoids (:45-97; pass split_size >= P).  The stop test: see CC_KMEDOIDS_MAX_THRESHOLD above (fixed point in
 *      one launch up to it, the reference's literal chunk-mean test above it).
 */
int cc_batch_kmedoids_f32(const float* x, const cc_token_layout* lay, int32_t W, int32_t K,
                          int32_t metric, float norm_p, float threshold, int32_t iter_limit,
                          int32_t id_sort, int32_t split_size, int32_t pre_norm,
                          int64_t* medoids, int64_t* assign, int32_t* iters,
                          void* ws, size_t ws_bytes, void* stream);

/*
 * C1..C6 - replaces TokenClusterInter.forward (kmediods++ branch, aggregation=None)
 *      modules/cluster/cluster.py:206-216,239-260,287-289,303-310,350-352.
 * Input: activation with 1+n tokens per frame, B*T frames, W floats per token; token l of
 * frame c starts at x + l*in_tok_stride + c*in_frame_stride (LND: tok=B*T*W, frame=W;
 * frame-major: tok=W, frame=(1+n)*W).  Output: 1+K tokens per segment, B*T_new segments,
 * same addressing with out_*_stride; out token 0 = mean of the segment's fd CLS tokens
 * (cluster.py:307-308), out token 1+k = the k-th medoid token (ascending ids).
 * medoids [T_new*B, K] int64 in the reference's problem order p = s*B + b; assign / iters
 * optional as above.
 */
int cc_token_cluster_f32(const float* x, int64_t in_tok_stride, int64_t in_frame_stride,
                         int32_t B, int32_t T, int32_t T_new, int32_t n, int32_t W, int32_t K,
                         int32_t metric, float norm_p, float threshold, int32_t iter_limit,
                         int32_t split_size, int32_t pre_norm,
                         float* out, int64_t out_tok_stride, int64_t out_frame_stride,
                         int64_t* medoids, int64_t* assign, int32_t* iters,
                         void* ws, size_t ws_bytes, void* stream);

/* The other TokenClusterInter variants that share this data layout, modules/cluster/cluster.py:
 *   algorithm CC_CLUSTER_KMEDOIDS + aggregation CC_AGGREGATE_MEDOID  the shipped path (:289), = cc_token_cluster_f32
 *   algorithm CC_CLUSTER_KMEDOIDS + aggregation CC_AGGREGATE_MEAN    output token k = mean of the tokens assigned to
 *                                medoid k (:291-301; an empty cluster yields NaN, as 0/0 does in the reference)
 *   algorithm CC_CLUSTER_POOLING  every token, CLS included, = mean over the segment's frames (:319-324);
 *                                K and the k-medoids arguments are ignored, out is [1+n, B*T_new, W]
 *   cluster_embed  [K, W] fp32 or NULL: learnt embedding added to output tokens 1..K (:304-305)
 *   cls_multiplier [T] fp32 or NULL: per-frame scale of the CLS token before the segment mean (adaptive_cls, :244-245)
 * Sums follow the association of the reference's torch.sum / mean over a non-innermost dimension (running sum
 * folded into a second level every 16 rows), so the outputs are bit-identical to the reference's CPU path.
 *   algorithm CC_CLUSTER_SPARSE_SAMPLING  eval-mode 'sparse_sampling' (:326-343): fixed_ids [K] int64 (device) are the
 *                                ids of token_sparse_sampling(K, fd*n, random_shift=False) (cluster_utils.py:136-170),
 *                                the same for every segment; gather + CLS mean as for medoids */
#define CC_CLUSTER_KMEDOIDS 0
#define CC_CLUSTER_POOLING  1
#define CC_CLUSTER_SPECTRAL 3          /* spectral clustering picks the medoids / the assignment (cluster_algo 'spectral') */
#define CC_CLUSTER_SPARSE_SAMPLING 2   /* fixed_ids [K]: token_sparse_sampling(K, fd*n, random_shift=False) */
#define CC_CLUSTER_TEMPORAL_SHIFT 4    /* temporal_shift_wo_cls (shift.py:15-37), see cc_token_shift_f32 */
#define CC_CLUSTER_TOKEN_SHIFT 5       /* token_shift (shift.py:40-61): the CLS rows only */
#define CC_AGGREGATE_MEDOID 0
#define CC_AGGREGATE_MEAN   1
typedef struct cc_cluster_variant {
    int32_t algorithm;
    int32_t aggregation;
    const float* cluster_embed;
    const float* cls_multiplier;
    const int64_t* fixed_ids;
    /* CC_CLUSTER_SPECTRAL (cluster.py:262-272 -> spectral.py:17-75): the selection is made by spectral clustering of the
     * segment's tokens (graph mode CC_GRAPH_*, sigma, knn_k, optional [N,N] uint8 spatial-temporal mask, sign correction),
     * the k-medoids tail runs on the row-normalised eigenvectors with the call's metric / norm_p / threshold / iter_limit /
     * split_size; gather / cluster means / CLS mean as for CC_CLUSTER_KMEDOIDS.  Needs cc_spectral_workspace_bytes more
     * scratch behind cc_cluster_workspace_bytes. */
    float spectral_sigma;
    int32_t spectral_graph_mode;
    int32_t spectral_knn_k;
    int32_t spectral_correct_sign;
    const uint8_t* spectral_graph;
    /* mean_residual (cluster.py:228-235, clip.py:239-242) - read by the fused encoders only: the block's residual stream
     * restarts from the frame means of every token (the 'pooling' reduction of the block's input) while ln_1 / the attention
     * read the clustered tokens.  Needs an unchanged token count (cluster_tokens[i] == incoming tokens, the reference's
     * assert).  The module-level entry points return the clustered tokens only; their caller forms the means with
     * algorithm = CC_CLUSTER_POOLING on the same input. */
    int32_t mean_residual;
    /* CC_CLUSTER_TEMPORAL_SHIFT / CC_CLUSTER_TOKEN_SHIFT - read by the fused encoders: fold = W / shift_fold_div (the
     * reference's 8), frames shifted within segments of shift_segment consecutive frames of the batch (original_frame =
     * max_frames).  The block keeps its frame and token counts (cluster_frames[i] / cluster_tokens[i] must equal the incoming
     * ones); the shift runs in place before ln_1 and, for token_shift, again between the out_proj residual and ln_2
     * (clip.py:236-248).  Shift blocks take no forced_medoids ids. */
    int32_t shift_fold_div;
    int32_t shift_segment;
} cc_cluster_variant;

/* cluster_algo 'temporal_shift' / 'token_shift' (modules/cluster/shift.py, cluster.py:343-347) on F frames of L tokens
 * (token 0 = CLS) of width W, element (f, j, c) at f * frame_stride + j * tok_stride + c: within each segment of `segment`
 * consecutive frames, channels [0, fold) of a shifted row take the next frame's value (zero in the segment's last frame),
 * channels [fold, 2 fold) the previous frame's (zero in the first), channels >= 2 fold are copied; fold = W / fold_div
 * (fold 0 = a copy).  mode CC_CLUSTER_TEMPORAL_SHIFT shifts tokens 1..L-1, CC_CLUSTER_TOKEN_SHIFT token 0; the other rows
 * are copied.  adjoint = 1 applies the transpose (the backward: the two directions swapped, zero fill).  Bit exact.
 * out == x with the same strides runs in place (only the shifted channels of the shifted rows are read and written);
 * otherwise out must not overlap x.  Both layouts must be alias free (LND [L, N, W]: tok_stride = N W, frame_stride = W;
 * frame-major [N, L, W]: tok_stride = W, frame_stride = L W).  CC_ERR_INVALID for F % segment != 0 or bad strides / sizes. */
int cc_token_shift_f32(const float* x, int64_t tok_stride, int64_t frame_stride, int32_t F, int32_t L, int32_t W,
                       int32_t segment, int32_t fold_div, int32_t mode, int32_t adjoint, float* out,
                       int64_t out_tok_stride, int64_t out_frame_stride, void* stream);

/* The forward shift in place on contiguous fp32 rows h [*, W] (row of frame f, token j = f * frame_rows + j * tok_rows),
 * with what the next LayerNorm-folded GEMM reads for every row it rewrites: h16 [*, W] fp16 = h - c (c = the row mean,
 * written to shift[row]), stats [row][slots][2] = (sum, sum of squares) of that copy in slot 0 and zeros in the other
 * slots.  token_shift rewrites the F CLS rows only (the others keep their statistics in any slot layout); temporal_shift
 * rewrites every row, CLS rows included, so the caller may pass slots = 1.  W % 4 == 0, W <= 1024, slots <= 32,
 * segment * min(2 fold, W) * 4 bytes <= 64 KiB (else CC_ERR_UNSUPPORTED).  One launch. */
int cc_token_shift_rows_f32(float* h, int64_t tok_rows, int64_t frame_rows, int32_t F, int32_t L, int32_t W,
                            int32_t segment, int32_t fold_div, int32_t mode, void* h16, float* stats, int32_t slots,
                            float* shift, void* stream);
size_t cc_token_shift_rows_lds_bytes(int32_t segment, int32_t W, int32_t fold_div);
/* The aggregation step of CC_AGGREGATE_MEAN alone, from a given assignment [T_new*B, fd*n] int64 (values 0..K-1;
 * problem p = s*B + b as everywhere) - the counterpart of cc_token_gather_f32 for cluster means
 * (cluster.py:291-310).  variant may be NULL; only its cluster_embed / cls_multiplier are used. */
int cc_token_aggregate_f32(const float* x, int64_t in_tok_stride, int64_t in_frame_stride,
                           int32_t B, int32_t T, int32_t T_new, int32_t n, int32_t W, int32_t K,
                           const int64_t* assign, const cc_cluster_variant* variant,
                           float* out, int64_t out_tok_stride, int64_t out_frame_stride, void* stream);

/* The same step for a selection made elsewhere (cluster_algo 'spectral', cluster.py:262-272 + :287-310): medoids
 * [T_new*B, K] (aggregation None) or assign [T_new*B, fd*n] (cluster means), + the variant's cluster_embed / cls_multiplier. */
int cc_token_apply_selection_f32(const float* x, int64_t in_tok_stride, int64_t in_frame_stride,
                                 int32_t B, int32_t T, int32_t T_new, int32_t n, int32_t W, int32_t K,
                                 const cc_cluster_variant* variant, const int64_t* medoids, const int64_t* assign,
                                 float* out, int64_t out_tok_stride, int64_t out_frame_stride, void* stream);

int cc_token_cluster_variant_f32(const float* x, int64_t in_tok_stride, int64_t in_frame_stride,
                                 int32_t B, int32_t T, int32_t T_new, int32_t n, int32_t W, int32_t K,
                                 int32_t metric, float norm_p, float threshold, int32_t iter_limit,
                                 int32_t split_size, int32_t pre_norm, const cc_cluster_variant* variant,
                                 float* out, int64_t out_tok_stride, int64_t out_frame_stride,
                                 int64_t* medoids, int64_t* assign, int32_t* iters,
                                 void* ws, size_t ws_bytes, void* stream);

/*
 * N4 (training support): gradient of TokenClusterInter.forward (modules/cluster/cluster.py:239-310,319-343) with respect to
 * its input and parameters for a FIXED selection - the reference selects under no_grad (fast_kmeans.py:13,44), so the
 * medoid ids / assignment are constants of the backward pass, exactly what torch.autograd does with the reference module:
 *   medoid gather (:289)            grad_x[token medoid_k] = grad_out[1 + k]
 *   cluster means (:291-301)        grad_x[j] = grad_out[1 + assign_j] / |cluster(assign_j)|     (assign [T_new*B, fd*n])
 *   cluster_embed (:304-305)        grad_cluster_embed[k] = sum over segments of grad_out[1 + k]            ([K, W] or NULL)
 *   CLS mean (* cls_multiplier, :244-245,307-308)   grad_x[cls, frame t] = grad_out[0] / fd (* m_t);
 *                                   grad_cls_mult[t] = sum_{b,w} grad_out[0] / fd * x[cls, frame t]         ([T] or NULL; needs x)
 *   pooling (:319-324)              grad_x[token] = grad_out[token] / fd
 *   sparse_sampling (:326-343)      gather with variant->fixed_ids
 * Every row of grad_x ([1+n, B*T, W] through the strides) is written exactly once, zeros included: no memset, no atomics.
 * medoids [T_new*B, K] as returned by cc_token_cluster_variant_f32 (ignored for mean / pooling / sparse_sampling).
 */
int cc_token_cluster_backward_f32(const float* grad_out, int64_t go_tok_stride, int64_t go_frame_stride,
                                  int32_t B, int32_t T, int32_t T_new, int32_t n, int32_t W, int32_t K,
                                  const cc_cluster_variant* variant, const int64_t* medoids, const int64_t* assign,
                                  const float* x, int64_t x_tok_stride, int64_t x_frame_stride,
                                  float* grad_x, int64_t gx_tok_stride, int64_t gx_frame_stride,
                                  float* grad_cluster_embed, float* grad_cls_mult, void* stream);


/*
 * N4: cluster_algo 'spectral' (modules/cluster/spectral.py:17-165), step by step; the whole selection also runs inside
 * cc_token_cluster_variant_f32 / the fused encoders through cc_cluster_variant.algorithm = CC_CLUSTER_SPECTRAL:
 *   cc_spectral_laplacian_f32  W = exp(-|x_i - x_j|^2 / (2 sigma^2)) (constructW 'HeatKernel', spectral.py:79-88, squared
 *                              distances as batched_cdist_l2, cluster_utils.py:121-133), optionally * graph [N,N] uint8
 *                              (spatial_temporal_graph, :139-165); D = diag(W 1); laplacian [P,N,N] = D^-1/2 (D - W) D^-1/2
 *                              (:44-52).  affinity_out [P,N,N] / degree_out [P,N] optional.  ws: cc_cluster_workspace_bytes.
 *   cc_svd_sign_flip_f32       batch_sign_flip_rasmus_bro (:110-137), in place on U [P,M,K] given S [P,K], VT [P,K,N].
 */
int cc_spectral_laplacian_f32(const float* x, const cc_token_layout* lay, int32_t W, float sigma,
                              const uint8_t* graph, float* laplacian, float* affinity_out, float* degree_out,
                              void* ws, size_t ws_bytes, void* stream);
/* constructW graph modes (spectral.py:86-100): heat kernel, or the heat kernel kept where j is among the knn_k largest entries
 * of row i or i among those of row j (mutual: and).  The spatial-temporal mask is applied after either (:104-105). */
#define CC_GRAPH_HEAT_KERNEL 0
#define CC_GRAPH_KNN         1
int cc_spectral_graph_laplacian_f32(const float* x, const cc_token_layout* lay, int32_t W, float sigma, int32_t mode,
                                    int32_t knn_k, int32_t mutual, const uint8_t* graph, float* laplacian,
                                    float* affinity_out, float* degree_out, void* ws, size_t ws_bytes, void* stream);
/*
 * The decomposition of batch_spectral_clustering (spectral.py:54-61): Q [P, N, ldq] (columns 0..K-1, the rest zeroed) = the
 * K eigenvectors of the symmetric positive semi-definite laplacian [P,N,N] with the smallest eigenvalues, in the reference's
 * column order (U[:, :, -K:] of torch.linalg.svd: eigenvalue descending), eigenvalues [P,K] optional, sweeps_out [P]
 * optional (Jacobi sweeps; 0 from the direct solver).  One workgroup per problem.  Direct solver (eig.hip) - Householder
 * tridiagonalisation (fp32), Sturm multi-section and inverse iteration (fp64), back-transformation: N <= 196 with the matrix
 * and then the packed reflectors + K vectors in LDS (K <= 49 at N = 196, K <= 64), 196 < N <= 832 with K <= 192 from a global
 * scratch in ws (ViT-B/16 ships N = 784, K = 160, scripts/activitynet.sh:104-122).  Remaining shapes up to N = 640: batched
 * one-sided Jacobi on 2I - L.
 * correct_sign: batch_sign_flip_rasmus_bro (:110-137) applied (for a symmetric matrix it depends on the vector alone).
 * Parity: eigenpairs to fp32 working precision, the eigenvalues equal the reference's singular values to 1e-5; the vectors
 * equal the reference's up to sign and, where eigenvalues coincide to rounding, up to a rotation inside that eigenspace -
 * which no solver pins.  Row distances of Q, which is all the k-medoids tail uses, are invariant to both
 * as long as the K-th and (K+1)-th eigenvalue are separated.  ws: cc_spectral_embedding_workspace_bytes.
 */
size_t cc_spectral_embedding_workspace_bytes(int32_t P, int32_t N);
/* Extra scratch of a CC_CLUSTER_SPECTRAL token-cluster call, appended to cc_cluster_workspace_bytes(P, N, W, pre_norm). */
size_t cc_spectral_workspace_bytes(int32_t P, int32_t N, int32_t K);
int cc_spectral_embedding_f32(const float* laplacian, int32_t P, int32_t N, int32_t K, int32_t correct_sign,
                              float* Q, int32_t ldq, float* eigenvalues, int32_t* sweeps_out, void* ws, size_t ws_bytes,
                              void* stream);
/* The same with the solver named: CC_EIG_AUTO = the direct solver wherever it applies (cc_spectral_embedding_f32),
 * CC_EIG_JACOBI = the one-sided Jacobi kernel for every shape (what shapes outside the direct solver's scope run; the
 * tests hold both against float64). */
#define CC_EIG_AUTO   0
#define CC_EIG_JACOBI 1
int cc_spectral_embedding_solver_f32(const float* laplacian, int32_t P, int32_t N, int32_t K, int32_t correct_sign,
                                     float* Q, int32_t ldq, float* eigenvalues, int32_t* sweeps_out, int32_t solver,
                                     void* ws, size_t ws_bytes, void* stream);
int cc_svd_sign_flip_f32(float* U, const float* S, const float* VT, int32_t P, int32_t M, int32_t K, int32_t N,
                         void* stream);

/*
 * C6 alone - the gather half of TokenClusterInter.forward for given medoid ids:
 *      x_tmp = res_tmp[batch_index, mediods_ids] (modules/cluster/cluster.py:289), the per-segment
 *      CLS mean (:307-308) and the restack (:303,310).  medoids [T_new*B, K] int64, p = s*B + b.
 */
int cc_token_gather_f32(const float* x, int64_t in_tok_stride, int64_t in_frame_stride,
                        int32_t B, int32_t T, int32_t T_new, int32_t n, int32_t W, int32_t K,
                        const int64_t* medoids, float* out, int64_t out_tok_stride,
                        int64_t out_frame_stride, void* stream);

/* ==========================================================================================
 * CLIP forward path.  fp16 MFMA operands, fp32 accumulate,
 * fp32 residual stream / LayerNorm / softmax (modules/clip.py:183-189 keeps LN in fp32; the
 * reference runs fp16 weights on GPU via convert_weights, clip.py:515-536).
 * Weight tensors keep the reference's state-dict layouts: Linear / in_proj
 * weights [out, in] row-major, conv1 weight [W, 3, p, p] == [W, 3*p*p]; "f16" pointers are IEEE
 * binary16 copies of those tensors, everything else fp32.
 * ========================================================================================== */

/* epilogue ids of cc_linear_f16 */
#define CC_EPI_F16 0        /* C(fp16) = A W^T + b                                           */
#define CC_EPI_F16_GELU 1   /* C(fp16) = QuickGELU(A W^T + b)         modules/clip.py:192-194 */
#define CC_EPI_F32_RESID 2  /* C(fp32) += A W^T + b   (residual add)  modules/clip.py:240,251 */
#define CC_EPI_F32 4        /* C(fp32) = A W^T + b                                           */
#define CC_EPI_F16_GELU_ERF 9   /* C(fp16) = GELU(A W^T + b), the exact x Phi(x) of nn.GELU() (OpenCLIP checkpoints) */

/* nn.Linear forward, y = x W^T + b  (c_fc / c_proj / out_proj: modules/clip.py:207-211; the
 * packed in_proj of nn.MultiheadAttention: clip.py:205).  a [M,K] fp16, w [N,K] fp16, bias
 * [N] fp32 or NULL, c row stride ldc elements.  K % 64 == 0, N % 64 == 0.  tile: 0 = auto. */
int cc_linear_f16(const void* a_f16, const void* w_f16, const float* bias, void* c,
                  int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t epilogue, int32_t tile,
                  void* stream);
/* out [M, N] fp32 = resid [M, N] + a w^T + bias (the "f32_resid" epilogue with a separate source of the rows that are added;
 * resid == out is cc_linear_f16's in-place form). */
int cc_linear_resid_f16(const void* a_f16, const void* w_f16, const float* bias, const float* resid, float* out, int32_t M,
                        int32_t N, int32_t K, int32_t tile, void* stream);
/* LayerNorm over the last dim (fp32 statistics, eps as given) - modules/clip.py:183-189.
 * Row r is read at in + r*in_stride and written at out + r*out_stride (elements); out is fp16
 * when out_f16 != 0, else fp32 (may alias in). */
int cc_layernorm_f32(const float* in, int64_t in_stride, const float* gamma, const float* beta,
                     void* out, int64_t out_stride, int32_t rows, int32_t W, float eps,
                     int32_t out_f16, void* stream);

/* The three pieces of the folded-LayerNorm pipeline the encoders use instead of stand-alone LayerNorm passes
 * (replaces ln_1 -> in_proj and ln_2 -> c_fc of modules/clip.py:240,251):
 *   cc_row_stats_f16          h [rows,W] fp32 -> h16 = fp16(h - c), stats [rows][1][2] = (sum, sum of squares) of h16,
 *                             c = the row mean, written to shift_out [rows] (shift_out NULL: c = 0).
 *   cc_linear_ln_f16          out(fp16) = [act](LN(h) W^T + b), from h16, the folded weight and the stats; gelu: 0 no
 *                             activation, 1 QuickGELU, 2 the exact GELU x Phi(x) (anything else: CC_ERR_INVALID)
 *                             (LayerNorm is invariant to the per-row shift c, so the consumer never sees it)
 *   cc_linear_resid_stats_f16 h += a W^T + b (residual), h16 = fp16(h - c), stats [M][*slots_out][2] (one slot per
 *                             tile column x wave column; stats buffers must hold 32 slots per row).  c = the row mean
 *                             before this update = shift_in[m] + mean of the centred copy the previous stage wrote
 *                             (stats_in [M][slots_in][2]); written to shift_out [M].  stats_in NULL: c = 0.
 * Centring keeps the rounding error of the fp16 copy relative to the row's spread, not to its mean (rows of real
 * checkpoints can have |mean| >> sigma). */
int cc_row_stats_f16(const float* h, void* h16_out, float* stats_out, float* shift_out, int32_t rows, int32_t W,
                     void* stream);
int cc_linear_ln_f16(const void* h_f16, const void* w_ln_f16, const float* c1, const float* c2,
                     const float* stats, int32_t slots, float eps, void* out_f16,
                     int32_t M, int32_t N, int32_t K, int32_t gelu, int32_t tile, void* stream);
/* in_proj with the LayerNorm folded + the multi-head attention core in ONE launch (modules/clip.py:210-214, the ln_1 ->
 * nn.MultiheadAttention path of ResidualAttentionBlock.attention): att [M, W] fp16 = softmax(q k^T / 8 [causal]) v per
 * (sequence, head) with q | k | v = LN(h) Wqkv^T + b evaluated as in cc_linear_ln_f16 (w_ln_f16 [3W, W], c1 / c2 [3W], stats
 * [M][slots][2]).  A workgroup owns whole sequences x one head and keeps their q, k, v in LDS - they never reach HBM.  Rows:
 * nseq sequences of L tokens (row = s * L + t), or - seq_off / seq_len both non-null (device arrays) - seq_len[s] <= L tokens
 * from row seq_off[s], packed back to back; m_dev (device, may be null) = count of valid rows.  W = heads * 64, L <= 256.
 * L <= 56: every operand of a (sequence, 16-query tile) item in registers, bit-identical to cc_linear_ln_f16 followed by
 * cc_attention_f16.  56 < L <= 256 (round 5: ViT-B/16's 197-token frames, its 101 / 161-token clustered blocks, CLIP's
 * 77-token captions): scores and P stay in registers, the PV contraction takes the keys of a 32-key block in the accumulator's
 * own order - equal to the two launches to the rounding of the fp16 output.  CC_ERR_UNSUPPORTED outside that range. */
int cc_inproj_attention_f16(const void* h_f16, const void* w_ln_f16, const float* c1, const float* c2, const float* stats,
                            int32_t slots, float eps, void* att_f16, int32_t nseq, int32_t L, int32_t heads, int32_t causal,
                            const int32_t* seq_off, const int32_t* seq_len, const int32_t* m_dev, void* stream);
/* host-side query: the tile (1 = 128x128, 2 = 128x64, 3 = 64x128, 4 = 64x64, 5 = 256x256, 6 = 256x128, 7 = 256x192, 8 = 64x64 with
 * 128-deep k-steps, 10 = 128x256) the dispatcher picks for this shape / epilogue id (CC_EPI_*; 5, 6 =
 * LN-folded f16 without / with QuickGELU, 7 = residual + statistics, 9 / 10 = 1 / 6 with the exact GELU); <= 0: unsupported */
int cc_linear_tile_for(int32_t M, int32_t N, int32_t K, int32_t epilogue);
/* host-side query: slots per row cc_linear_resid_stats_f16 will write for this shape (tile 0 = auto); <= 0: unsupported */
int cc_linear_resid_stats_slots(int32_t M, int32_t N, int32_t K, int32_t tile);
int cc_linear_resid_stats_f16(const void* a_f16, const void* w_f16, const float* bias, float* h,
                              void* h16_out, float* stats_out, int32_t* slots_out, const float* shift_in,
                              const float* stats_in, int32_t slots_in, float* shift_out,
                              int32_t M, int32_t N, int32_t K, int32_t tile, void* stream);

/* The launch forms the fused encoders use, one op at a time: up to TWO independent problems with the same epilogue in one
 * launch (the text tower's tiles ride in the ViT's grid), the few-rows kernel of the last block, and every per-problem
 * option of the entries above.  A problem is described by one struct; fields an epilogue does not read stay zero.
 *   a / w / bias / c / resid, M N K ldc   as cc_linear_f16 (ldc >= N; resid NULL = c, the in-place residual add)
 *   ln_stats [M][ln_slots][2], ln_c1 [N], ln_eps           LN-folded epilogues (5, 6): as cc_linear_ln_f16, c2 in `bias`
 *   stats_out [M][slots][2], c16 [M][ldc] fp16             residual + statistics (7): as cc_linear_resid_stats_f16
 *   shift_in [M], shift_stats [M][shift_slots][2], shift_out [M]     its row centring (shift_stats NULL: c = 0)
 *   m_dev        device int32, may be NULL: the number of valid rows (<= M, which sizes the grid); rows behind it are
 *                neither computed nor stored
 *   row_step / row_map [M] (device int32)   cc_linear_rows_pair_f16 only: logical row m lives at physical row
 *                row_map ? row_map[m] : m * row_step (0 = 1) of a / c / c16 / resid and of every per-row side array
 *   pos [1 + patch_n][N], patch_n           CC_EPI_F32_PATCH: out row of patch row m = f * (patch_n + 1) + 1 + i with
 *                f = m / patch_n, i = m % patch_n, value = a w^T + bias + pos[1 + i] (the class-token rows are not written)
 *   att_*        cc_inproj_attention_pair_f16: as nseq / L / causal / seq_off / seq_len of cc_inproj_attention_f16
 *                (N = 3 K, K = heads * 64, ldc = K, M = nseq * L, c = the attention output) */
typedef struct cc_linear_problem {
    const void* a;            /* [M, K] fp16 */
    const void* w;            /* [N, K] fp16 */
    const float* bias;
    void* c;
    const float* resid;
    int32_t M, N, K, ldc;
    const float* ln_stats;
    int32_t ln_slots;
    const float* ln_c1;
    float ln_eps;
    float* stats_out;
    void* c16;
    const float* shift_in;
    const float* shift_stats;
    int32_t shift_slots;
    float* shift_out;
    const int32_t* m_dev;
    int32_t row_step;
    const int32_t* row_map;
    const float* pos;
    int32_t patch_n;
    int32_t att_L, att_nseq, att_causal;
    const int32_t* att_seq_off;
    const int32_t* att_seq_len;
} cc_linear_problem;
#define CC_EPI_F32_PATCH 3        /* patch embedding, see cc_linear_problem::pos */
#define CC_EPI_F16_LN 5           /* C(fp16) = LN(h) W^T + b from the centred copy and its statistics */
#define CC_EPI_F16_GELU_LN 6      /* ... with QuickGELU */
#define CC_EPI_F32_RESID_STATS 7  /* C(fp32) += A W^T + b, + fp16 copy + partial row statistics */
#define CC_EPI_F16_GELU_ERF_LN 10 /* as 6 with the exact GELU x Phi(x) in place of QuickGELU (id 8 is internal) */
/* sizeof(cc_linear_problem) as the library was built (a binding checks its own layout against it) */
size_t cc_linear_problem_size(void);
/* p0 and, if non-NULL, p1 through the tile kernel in one launch; epilogue 0..7, 9 or 10, tile as cc_linear_f16 (a forced tile must
 * divide both problems; 0 = the choice for p0, narrowed until it divides p1).  slots_out [2] (required for epilogue 7,
 * else may be NULL): statistics slots per row each problem wrote.  CC_ERR_INVALID - before anything is enqueued - for a
 * NULL operand, an operand its epilogue needs, row_step / row_map, or a tile that does not divide a problem. */
int cc_linear_pair_f16(const cc_linear_problem* p0, const cc_linear_problem* p1, int32_t epilogue, int32_t tile,
                       int32_t* slots_out, void* stream);
/* The same product for a FEW selected rows (row_step / row_map), in place on the physical rows: epilogues 6, 10, 2 and 7;
 * N % 32 == 0, K % 32 == 0 and, with statistics, N <= 1024 (N / 32 slots per row) - else CC_ERR_UNSUPPORTED. */
int cc_linear_rows_pair_f16(const cc_linear_problem* p0, const cc_linear_problem* p1, int32_t epilogue,
                            int32_t* slots_out, void* stream);
/* cc_inproj_attention_f16 for one or two problems in one launch (the row-tile height is chosen over both);
 * CC_ERR_UNSUPPORTED outside the one-launch form's range. */
int cc_inproj_attention_pair_f16(const cc_linear_problem* p0, const cc_linear_problem* p1, void* stream);

/* Multi-head self-attention core of nn.MultiheadAttention (modules/clip.py:220-226):
 * qkv [nseq*L, 3W] fp16 (row = seq*L + token; q | k | v, heads = contiguous 64-wide slices),
 * out [nseq*L, W] fp16 = softmax(q k^T / 8 + mask) v; causal != 0 adds the strict upper
 * triangular -inf mask of clip.py:448-454.  head_dim is 64 (W == 64*heads).  L <= 256: K and V^T of a (sequence, head)
 * resident in LDS; 256 < L <= 640 (ViT-L/14: 257 tokens at 224 px, 577 at 336 px): 64-key tiles streamed through LDS with
 * an online softmax (attention_long.hip); L > 640: CC_ERR_UNSUPPORTED. */
int cc_attention_f16(const void* qkv_f16, void* out_f16, int32_t nseq, int32_t L, int32_t heads,
                     int32_t W, int32_t causal, void* stream);
/* The same for other row orders: token t of sequence s is row s*seq_rows + t*tok_rows of qkv / out.  The LND
 * activations ResidualAttentionBlock.forward receives (modules/clip.py:228-253: x [L, N, W]) are seq_rows = 1,
 * tok_rows = N; cc_attention_f16 is seq_rows = L, tok_rows = 1. */
int cc_attention_strided_f16(const void* qkv_f16, void* out_f16, int32_t nseq, int32_t L, int32_t heads,
                             int32_t W, int32_t causal, int64_t seq_rows, int64_t tok_rows, void* stream);

/* The same for sequences of different lengths packed back to back (the text tower's compacted captions): sequence s has
 * seq_len[s] <= L_max tokens (device int32 [nseq], each >= 1) starting at row seq_off[s] of qkv / out; rows are W-strided as
 * in cc_attention_f16.  L_max sizes the launch and picks the kernel (<= 640). */
int cc_attention_varlen_f16(const void* qkv_f16, void* out_f16, int32_t nseq, int32_t L_max, int32_t heads, int32_t W,
                            int32_t causal, const int32_t* seq_off, const int32_t* seq_len, void* stream);

/* One ResidualAttentionBlock (state-dict keys resblocks.{i}.*) */
typedef struct cc_block_weights {
    const float* ln_1_weight;  const float* ln_1_bias;
    const void* in_proj_weight_f16;   /* [3W, W] */   const float* in_proj_bias;    /* [3W] */
    const void* out_proj_weight_f16;  /* [W, W]  */   const float* out_proj_bias;   /* [W]  */
    const float* ln_2_weight;  const float* ln_2_bias;
    const void* c_fc_weight_f16;      /* [4W, W] */   const float* c_fc_bias;       /* [4W] */
    const void* c_proj_weight_f16;    /* [W, 4W] */   const float* c_proj_bias;     /* [W]  */
    /* ln_1 / ln_2 folded into the Linear layer that consumes them (cc_fold_layernorm_linear_f32):
     *   LN(h) W^T + b = rstd (h (W*gamma)^T - mu c1) + c2
     * so the encoders never run a stand-alone LayerNorm pass over the residual stream.           */
    const void* in_proj_ln_weight_f16; /* fp16(in_proj_weight * ln_1.weight)  [3W, W] */
    const float* in_proj_ln_c1;        /* [3W] row sums of the folded weight          */
    const float* in_proj_ln_c2;        /* [3W] in_proj_weight ln_1.bias + in_proj_bias */
    const void* c_fc_ln_weight_f16;    /* fp16(c_fc.weight * ln_2.weight)     [4W, W] */
    const float* c_fc_ln_c1;           /* [4W] */
    const float* c_fc_ln_c2;           /* [4W] */
} cc_block_weights;

/* Fold a LayerNorm (gamma, beta over K) into the Linear layer y = LN(x) W^T + b that consumes it:
 * w_f16_out[n,k] = fp16(W[n,k] * gamma[k]); c1_out[n] = sum_k w_f16_out[n,k]; c2_out[n] = sum_k beta[k] W[n,k] + b[n].
 * weight [N,K] fp32, bias [N] fp32 or NULL.  Fills the *_ln_* fields of cc_block_weights. */
int cc_fold_layernorm_linear_f32(const float* weight, const float* bias, const float* gamma, const float* beta,
                                 int32_t N, int32_t K, void* w_f16_out, float* c1_out, float* c2_out, void* stream);

#define CC_MAX_LAYERS 32

/* cc_vit_model.activation / cc_text_model.activation: the MLP activation of the tower's blocks.  0 (a zero-filled struct) is the
 * reference's model; the OpenCLIP / LAION checkpoints of the same architecture use nn.GELU().  Any other value: CC_ERR_INVALID
 * before anything is launched.  (The seqTransf head is CLIP4Clip's own transformer: QuickGELU whatever the towers use.) */
#define CC_ACT_QUICK_GELU 0   /* x sigmoid(1.702 x), modules/clip.py:192-194 */
#define CC_ACT_GELU       1   /* x Phi(x), evaluated as x erfc(-x / sqrt 2) / 2 in fp32 */

/* cc_vit_model.row_policy / cc_text_model.row_policy: compute rows whose values nothing downstream reads, exactly as the
 * reference does (bench.py and the tests time / compare both forms; results agree bit for bit for the text rows and to the
 * rounding of the fp16 intermediates for the last block). */
#define CC_ROWS_ALL_TEXT        1   /* text tower: every token row, not only those up to each caption's EOT            */
#define CC_ROWS_ALL_LAST_BLOCK  2   /* last block of the tower: every row behind the attention, not only CLS / EOT rows */

/* VisualTransformer + the ln_post/proj tail of CLIP.encode_image (modules/clip.py:272-349,460-469) */
typedef struct cc_vit_model {
    int32_t layers, width, heads, patch, resolution, embed_dim;
    const void* conv1_weight_f16;         /* [W, 3*p*p]                         */
    const float* class_embedding;         /* [W]                                */
    const float* positional_embedding;    /* [1 + (res/p)^2, W]                 */
    const float* ln_pre_weight;  const float* ln_pre_bias;
    const float* ln_post_weight; const float* ln_post_bias;
    const float* proj;                    /* [W, embed_dim] fp32                */
    const cc_block_weights* blocks;       /* HOST array [layers]                */
    /* token-cluster plan, one entry per block (the per-block decision of get_cluster_inter,
     * modules/cluster/cluster.py:15-37): cluster_tokens[i] > 0 => before the attention of block i
     * (0-based) the clip's frames are cut to cluster_frames[i] segments of cluster_tokens[i]
     * medoid tokens (clip.py:236-242). */
    int32_t cluster_frames[CC_MAX_LAYERS];
    int32_t cluster_tokens[CC_MAX_LAYERS];
    int32_t cluster_metric;   float cluster_norm_p;   float cluster_threshold;
    int32_t cluster_iter_limit, cluster_split_size, cluster_pre_norm;
    /* optional HOST array [layers]: the TokenClusterInter variant of block i (N2); NULL = medoid gather
     * everywhere.  For CC_CLUSTER_POOLING cluster_tokens[i] must equal the incoming token count. */
    const struct cc_cluster_variant* cluster_variants;
    /* CC_ROWS_* bits; 0 = the shipped policy (the last block computes out_proj / c_fc / c_proj for the rows the
     * projection head reads).  Per model, not process state: two models with different policies can run side by side. */
    int32_t row_policy;
    /* linear_patch = '3d' (modules/clip.py:296-317): the patch embedding is a Conv3d over (t, h, w) with kernel (3, p, p),
     * stride (1, p, p) and zero padding 1 along t - frame t of a clip sees frames t-1, t, t+1 of the SAME clip.
     * conv2_weight_f16 [W, 3*3*p*p] = the Conv3d weight [W, 3(c), 3(t), p, p] flattened; NULL = '2d' (conv1). */
    const void* conv2_weight_f16;
    int32_t activation;                   /* CC_ACT_*; 0 = QuickGELU */
} cc_vit_model;

/* Frame input descriptor for the *_frames entry points.  The reference's evaluation
 * loader turns a decoded uint8 frame into the float tensor the ViT eats with three fp32 ops -
 * x = u8 / 255 (dataloaders/transforms.py:166, GroupToTensorBCHW(div=True)), then x = (x - mean) / std
 * (transforms.py:19-34 -> torchvision normalize: sub_, div_) with the constants of dataloaders/decode.py:43-48.
 * Handing over the uint8 frames lets the patch gather do exactly these three IEEE fp32 operations itself
 * (bit-identical patches), reading 1 byte per sample from HBM (and over PCIe) instead of 4. */
#define CC_FRAMES_F32_CHW 0   /* [F, 3, res, res] fp32, already normalised (what CLIP.encode_image takes)   */
#define CC_FRAMES_U8_CHW  1   /* [F, 3, res, res] uint8                                                   */
#define CC_FRAMES_U8_HWC  2   /* [F, res, res, 3] uint8 (decoder layout, before transforms.py:157 permutes) */
typedef struct cc_frames {
    const void* data;
    int32_t format;           /* CC_FRAMES_*                                         */
    float mean[3], std[3];    /* per channel; used by the uint8 formats only         */
} cc_frames;

size_t cc_vit_workspace_bytes(const cc_vit_model* m, int32_t B, int32_t T);

/* Number of int64 ids the forced_medoids argument of cc_vit_encode* / cc_clip_encode* must hold for a batch of B clips: the
 * sum over the tower's cluster blocks of B x cluster_frames[i] x cluster_tokens[i] (0: no cluster block, < 0: bad arguments).
 * Shift blocks (CC_CLUSTER_TEMPORAL_SHIFT / CC_CLUSTER_TOKEN_SHIFT) take no ids and are not counted.
 * The pointer carries no length - a host-side caller checks its buffer against this before the call. */
int64_t cc_vit_forced_medoids_count(const cc_vit_model* m, int32_t B);

/* CLIP.encode_image(image, video_frame=T) (modules/clip.py:460-469): video [B*T, 3, res, res]
 * fp32 -> features [B*T_final, embed_dim] fp32 (CLS row of ln_post(hidden) @ proj; only the
 * CLS row is projected - identical values).  hidden_out (optional):
 * the final hidden state [B*T_final, L_final, W] fp32 before ln_post (VisualTransformer.forward
 * output, clip.py:304-349).  medoids_out (optional): int64 [T_new*B, K] of the LAST k-medoids block of the
 * plan (T_new, K of THAT block; earlier cluster blocks do not write it).
 * forced_medoids (optional, test hook for "embeddings given identical medoid sets"):
 * int64 [T_new*B, K] per cluster block, the blocks' tensors back to back in block order; when non-NULL every cluster block
 * (shipped variant: k-medoids, medoid aggregation) skips the selection and gathers these ids instead. */
int cc_vit_encode(const cc_vit_model* m, const float* video, int32_t B, int32_t T,
                  float* features, float* hidden_out, int64_t* medoids_out,
                  const int64_t* forced_medoids, void* ws, size_t ws_bytes, void* stream);

/* Text transformer + ln_final/text_projection tail of CLIP.encode_text (modules/clip.py:471-496) */
typedef struct cc_text_model {
    int32_t layers, width, heads, context_length, vocab_size, embed_dim;
    const float* token_embedding;         /* [vocab, W]        */
    const float* positional_embedding;    /* [context, W]      */
    const float* ln_final_weight; const float* ln_final_bias;
    const float* text_projection;         /* [W, embed_dim]    */
    const cc_block_weights* blocks;       /* HOST array [layers] */
    int32_t row_policy;                   /* CC_ROWS_* bits; 0 = shipped policy */
    int32_t activation;                   /* CC_ACT_*; 0 = QuickGELU */
} cc_text_model;

size_t cc_text_workspace_bytes(const cc_text_model* m, int32_t Bt, int32_t Lt);

/* ids [Bt, Lt] int64 -> features [Bt, embed_dim] fp32: row at the first argmax of the ids
 * (EOT has the largest id, clip.py:484) of ln_final(x) @ text_projection.
 * Caption compaction: the attention mask is causal (clip.py:448-454) and only the EOT row is projected, so tokens behind
 * a caption's EOT cannot reach its feature.  The tower therefore runs on the rows up to each caption's EOT only, packed
 * back to back (positions found on the device, launches sized for Bt*Lt rows, no host synchronisation) - the features
 * are bit-identical to running all Bt*Lt rows.  cc_text_encode_hidden with hidden_out != NULL runs every row. */
int cc_text_encode(const cc_text_model* m, const int64_t* ids, int32_t Bt, int32_t Lt,
                   float* features, void* ws, size_t ws_bytes, void* stream);
/* ... also returning the final hidden state [Bt, Lt, W] fp32 before ln_final (hidden_out may be NULL) */
int cc_text_encode_hidden(const cc_text_model* m, const int64_t* ids, int32_t Bt, int32_t Lt,
                          float* features, float* hidden_out, void* ws, size_t ws_bytes, void* stream);

/* out[r] = LayerNorm(h[r*row_mul + (row_idx ? row_idx[r] : 0)]) @ proj   (fp32 throughout; h rows of W floats,
 * proj [W, E], out [R, E]).  The ln_post @ proj / ln_final @ text_projection tail of CLIP.encode_image / encode_text
 * (modules/clip.py:463,480) for any set of rows: row_mul = 1, row_idx = NULL projects every token
 * (return_hidden=True, clip.py:466-467,491-492).  W <= 1024, E % 4 == 0, R <= 65535. */
int cc_head_project_f32(const float* h, int32_t row_mul, const int32_t* row_idx, const float* gamma,
                        const float* beta, const float* proj, float* out, int32_t R, int32_t W, int32_t E,
                        void* stream);

/* Both encoders of one CLIP4Clip.forward call (modules/clip4clip.py:199-243: get_sequence_output
 * + get_visual_output) in one enqueue.  Block i of the text tower shares every launch with block i
 * of the ViT (horizontal fusion): same results as cc_vit_encode + cc_text_encode, fewer and fuller
 * launches.  ws: cc_clip_workspace_bytes. */
size_t cc_clip_workspace_bytes(const cc_vit_model* vm, int32_t B, int32_t T,
                               const cc_text_model* tm, int32_t Bt, int32_t Lt);
int cc_clip_encode(const cc_vit_model* vm, const float* video, int32_t B, int32_t T,
                   float* visual_features, int64_t* medoids_out,
                   const cc_text_model* tm, const int64_t* ids, int32_t Bt, int32_t Lt,
                   float* text_features, void* ws, size_t ws_bytes, void* stream);

/* cc_vit_encode / cc_clip_encode with the frames given through a cc_frames descriptor (N3): for
 * CC_FRAMES_F32_CHW identical to the calls above; for the uint8 formats the normalisation of
 * dataloaders/transforms.py is fused into the patch gather.  Same outputs, same workspace. */
int cc_vit_encode_frames(const cc_vit_model* m, const cc_frames* frames, int32_t B, int32_t T,
                         float* features, float* hidden_out, int64_t* medoids_out,
                         const int64_t* forced_medoids, void* ws, size_t ws_bytes, void* stream);
int cc_clip_encode_frames(const cc_vit_model* vm, const cc_frames* frames, int32_t B, int32_t T,
                          float* visual_features, int64_t* medoids_out, const int64_t* forced_medoids,
                          const cc_text_model* tm, const int64_t* ids, int32_t Bt, int32_t Lt,
                          float* text_features, void* ws, size_t ws_bytes, void* stream);

/* The frozen prefix of a tower in training (main.py:102 freeze_cip_layers: every shipped launcher freezes at least the
 * patch embedding and the token embedding): the launch sequence of cc_vit_encode_frames / cc_text_encode_hidden stopped
 * behind n_blocks blocks, 0 <= n_blocks <= layers, returning the residual stream at that point and no projection head.
 *   visual: hidden_out [B*T_n, L_n, W] fp32 frame-major (T_n segments and L_n tokens incl. CLS behind the cluster blocks among
 *           the first n_blocks); n_blocks = 0 is gather -> patch GEMM with the position-embedding epilogue -> ln_pre.
 *           forced_medoids: as cc_vit_encode, the ids of the cluster blocks among the first n_blocks only.
 *   text:   hidden_out [Bt, Lt, W] fp32, every row (no caption compaction); n_blocks = 0 is token + position embedding.
 * The last block run computes every row (the next block reads them all).  Only the first n_blocks entries of m->blocks, the
 * front-end fields and the cluster plan are read: ln_post / proj / ln_final / text_projection may be NULL.
 * Workspace: cc_vit_workspace_bytes / cc_text_workspace_bytes.  Errors, all found before anything is enqueued:
 * CC_ERR_INVALID for n_blocks outside [0, layers], a NULL argument or a frame base off the gathers' read grid (uint8 frames
 * are read in 8-byte pieces, fp32 frames as float4: 8- and 16-byte aligned); CC_ERR_WORKSPACE for a workspace that is too
 * small. */
int cc_vit_encode_prefix_frames(const cc_vit_model* m, const cc_frames* frames, int32_t B, int32_t T, int32_t n_blocks,
                                float* hidden_out, const int64_t* forced_medoids, void* ws, size_t ws_bytes,
                                void* stream);
int cc_text_encode_prefix(const cc_text_model* m, const int64_t* ids, int32_t Bt, int32_t Lt, int32_t n_blocks,
                          float* hidden_out, void* ws, size_t ws_bytes, void* stream);

/* The patch gather of the encoders on its own (training with a trainable conv1): frames (cc_frames, F frames of
 * resolution x resolution) -> out_f16 [F * (resolution/patch)^2, 3 * patch^2] fp16, rows (c, kh, kw) as conv1.weight is
 * flattened; uint8 frames get the loader's three fp32 operations (see cc_frames).  patch % 8 == 0, resolution % patch == 0
 * (uint8: resolution % 8 == 0; a power-of-two patch takes the strip kernel, any other the general gather), a uint8 base
 * 8-byte aligned, an fp32 base 16-byte aligned - else CC_ERR_INVALID before any launch. */
int cc_patch_gather_f16(const cc_frames* frames, int32_t F, int32_t resolution, int32_t patch, void* out_f16,
                        void* stream);

/* The same for ANY patch size that divides the resolution (ViT-L/14: patch 14): out_f16 [F * (resolution/patch)^2, Kp] fp16
 * with Kp = roundup(3 * patch^2, 64); columns (c, kh, kw), columns >= 3 * patch^2 exact zeros - the conv1 weight is packed with
 * the same zero columns and the GEMM sees an ordinary K.  patch % 8 == 0 (Kp = 3 * patch^2): cc_patch_gather_f16 itself, same
 * bits, same alignment rule.  Otherwise every sample is loaded on its own: a uint8 base may be any address, an fp32 base any
 * float address.  resolution % patch != 0: CC_ERR_INVALID. */
int cc_patch_gather_any_f16(const cc_frames* frames, int32_t F, int32_t resolution, int32_t patch, void* out_f16,
                            void* stream);

/* The same for linear_patch '3d' (training with conv2, modules/clip.py:296-317: Conv3d kernel (3, patch, patch), stride
 * (1, patch, patch), padding (1, 0, 0) over clips of T frames): frames (F frames, F % T == 0, clip b = frames b*T .. b*T + T - 1)
 * -> out_f16 [F * (resolution/patch)^2, 9 * patch^2] fp16, columns (c, kt, kh, kw) as conv2.weight is flattened.  Tap kt of
 * frame f holds frame f + kt - 1 of the same clip, exact zeros where that frame lies outside the clip.  uint8 frames get the
 * loader's three fp32 operations as above.  These are the gathers of the fused forward.  No allocation, no synchronisation.
 * patch % 8 == 0, resolution % patch == 0, F % T == 0, a uint8 base 8-byte aligned, an fp32 base 16-byte aligned - else
 * CC_ERR_INVALID before any launch; uint8 frames with a patch that is no power of two: CC_ERR_UNSUPPORTED. */
int cc_patch_gather3d_f16(const cc_frames* frames, int32_t F, int32_t T, int32_t resolution, int32_t patch, void* out_f16,
                          void* stream);

/* The loader transform in front of the patch gather: decoded uint8 frames of any size H x W -> the n_px x n_px uint8 frames the
 * uint8 formats of cc_frames take, byte for byte what CLIP's transform (dataloaders/rawvideo_util.py:16-23: Resize(n_px,
 * BICUBIC) -> CenterCrop(n_px)) produces before ToTensor / Normalize - Pillow's 8-bit bicubic resample (double coefficients
 * rounded to 22-bit integers; a horizontal pass rounded to bytes, then a vertical pass on those bytes; a pass whose axis
 * keeps its size is skipped) and torchvision's sizes (the short side becomes n_px, the long side int(n_px * long / short); a
 * short side that already is n_px leaves the frame as it is; crop offsets round((size - n_px) / 2.0), half to even).
 * resize = 0 is the crop alone (dataloaders/decode.py:37,46 on videos that preprocess/compress_video.py already shrank).
 * Range: 1 <= n_px <= 1024, 4 <= H, W <= 8192 and a resized frame no smaller than the crop (torchvision's zero padding is
 * not built); for cc_resize_crop_u8 and its workspace also at most 65 taps per output sample on either axis (ksize =
 * 2 ceil(2 in / out) + 1 <= 65: a shrink factor of 16; the plan builder itself takes any) - else CC_ERR_UNSUPPORTED; resize
 * other than 0 / 1: CC_ERR_INVALID.  DESIGN.md, "Resize and centre crop".
 *
 * The plan is a flat int32 table, built on the host without a GPU and uploaded by the caller once per (H, W, n_px, resize):
 *   [0] magic  [1] H  [2] W  [3] n_px  [4] resize  [5] oh  [6] ow (resized size)  [7] top  [8] left (crop offsets in it)
 *   [9] row0  [10] row1 (the source rows [row0, row1) the window reads)  [11] ksize_h  [12] ksize_v (taps per output column /
 *   row; 0 = that pass is skipped)  [13] off_h  [14] off_v (int32 offsets of the two tables)  [15] total int32 count
 *   table at off_h: first[n_px] (first source column of window column j), count[n_px], coef[n_px][ksize_h] (zeros behind
 *   count[j]); table at off_v: the same for the window's rows.  A skipped pass: first[j] = left + j (top + j), count[j] = 0.
 *   One pass over an axis: out = clamp((2^21 + sum_k in[first[j] + k] * coef[j][k]) >> 22, 0, 255) in int32. */
#define CC_RESIZE_PLAN_HEADER 16
/* bytes of the plan; 0 for sizes cc_resize_plan_build refuses */
size_t cc_resize_plan_bytes(int32_t H, int32_t W, int32_t n_px, int32_t resize);
int cc_resize_plan_build(int32_t H, int32_t W, int32_t n_px, int32_t resize, void* host_buf);
/* bytes of the horizontal pass' result (F x 3 x (row1 - row0) x n_px); 0 when at most one pass runs or the launch is refused */
size_t cc_resize_crop_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t n_px, int32_t resize);
/* src: F frames [H, W, 3] (fmt = CC_FRAMES_U8_HWC) or [3, H, W] (CC_FRAMES_U8_CHW) at ANY byte address; plan_dev: the plan of
 * (H, W, n_px, resize) in device memory - the host decides the launches from these four arguments and never reads the plan;
 * the kernels follow its tables only when its header names the same four values, a plan built for anything else leaves dst
 * unwritten; dst: [F, n_px, n_px, 3] or [F, 3, n_px, n_px] (dst_fmt).  At most two launches, no upload, no synchronisation
 * (capturable).  CC_ERR_INVALID for a NULL src / dst / plan, F <= 0 or a format other than the two uint8 codes;
 * CC_ERR_WORKSPACE for a NULL or short workspace where cc_resize_crop_workspace_bytes is not 0; all before any launch. */
int cc_resize_crop_u8(const void* src, int32_t fmt, int32_t F, int32_t H, int32_t W, const void* plan_dev, int32_t n_px,
                      int32_t resize, void* dst, int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream);

/* Train-time augmentation of decoded uint8 frames: per clip one crop box resized to n_px x n_px and one horizontal flip - the
 * reference's TensorMultiScaleCrop / RandomResizedCrop and TensorRandomHorizontalFlip (dataloaders/decode.py:32-41,
 * dataloaders/transforms.py:37-134, 168-196) once the box and the flip are drawn; the drawing is the caller's.
 * src: F frames [H, W, 3] (fmt = CC_FRAMES_U8_HWC) or [3, H, W] (CC_FRAMES_U8_CHW) at ANY byte address; dst: F frames
 * [n_px, n_px, 3] or [3, n_px, n_px] (dst_fmt).  boxes_dev: int32 [ceil(F / frames_per_clip), 5] in device memory, rows
 * (top, left, height, width, flip); frame f uses row f / frames_per_clip.  The kernel reads the table, the host never does:
 * one launch, no workspace, no upload, no synchronisation (capturable; a replay follows the table's contents at that time).
 * A row that does not lie inside the frame (top < 0, left < 0, height < 1, width < 1, top + height > H or left + width > W) is
 * not followed: the frames of that clip come out as zeros, no address is formed from the row.
 * Arithmetic: torch.nn.functional.interpolate(crop, n_px, mode, align_corners=False), no antialias, in fp32 on the bytes.
 * The source coordinate of output index o of an axis is the exact rational ((2 o + 1) crop - n_px) / (2 n_px) (= (o + 0.5) *
 * crop / n_px - 0.5): integer floor, fraction t from the remainder.  interp 0, bilinear: the coordinate is clamped below at
 * 0, weights (1 - t, t), the upper neighbour clamped to the crop's last sample.  interp 1, bicubic: cubic convolution with
 * A = -0.75 on the four samples floor - 1 .. floor + 2, each index clamped into the crop, the coordinate itself not clamped.
 * flip != 0: output column ox is what column n_px - 1 - ox would be.  Rows are combined after columns; the result is
 * clamp(rint(sum), 0, 255), rint half to even.  A box of n_px x n_px is a copy, byte for byte (weights exactly 0 and 1).
 * CC_ERR_INVALID for a NULL src / dst / table, F <= 0, frames_per_clip <= 0, a format other than the two uint8 codes or an
 * interp other than 0 / 1; CC_ERR_UNSUPPORTED outside 1 <= n_px <= 1024, 4 <= H, W <= 8192; all before any launch.
 * DESIGN.md, "Train-time augmentation". */
int cc_resized_crop_flip_u8(const void* src, int32_t fmt, int32_t F, int32_t H, int32_t W, int32_t frames_per_clip,
                            const int32_t* boxes_dev, int32_t n_px, int32_t interp, void* dst, int32_t dst_fmt, void* stream);

/* Ragged clip batches: what a decoder produces - clips of mixed H x W and mixed lengths, packed back to back in ONE byte
 * buffer with no alignment padding - collated into the uniform [n_out, n_px, n_px, 3] / [n_out, 3, n_px, n_px] frames the
 * encoders take.  cc_collate_resize_crop_u8 is cc_resize_crop_u8 per frame and cc_collate_crop_flip_u8 is
 * cc_resized_crop_flip_u8 per frame: the kernels call the same device functions, so each output frame is byte for byte what the
 * per-size entry point gives for its source frame.  DESIGN.md, "Ragged clip batches".
 *
 * LAUNCH BOUND: one call of cc_collate_resize_crop_u8 is at most TWO launches (the horizontal pass of the frames that run both
 * passes, then one launch that writes every output frame) and one call of cc_collate_crop_flip_u8 is ONE launch - at most
 * three for either, whatever the number of clips, of output frames and of distinct sizes.  The third grid dimension runs over
 * output frames, at most CC_COLLATE_MAX_PLANES of them at a time (fewer where the grid would pass 2^31 threads); more frames
 * than planes are folded onto the planes, none is refused.  The grid covers the largest frame of the call.
 *
 * src: the packed bytes, src_bytes of them; every frame is [H, W, 3] (fmt = CC_FRAMES_U8_HWC) or [3, H, W]
 * (CC_FRAMES_U8_CHW), at ANY byte address.  clips_host: HOST int64 [n_clips, 4] rows (byte offset, frames t, H, W) - what
 * the entry point checks before any launch: CC_ERR_INVALID unless 0 <= offset, t >= 1 and offset + t * H * W * 3 <= src_bytes for
 * every clip, and the status cc_resize_crop_status (resp. cc_resized_crop_flip_u8) gives for a size it refuses.
 * rows_dev: DEVICE int64 table, one row per OUTPUT frame; the host never reads it, the kernels read a frame's row before
 * anything else and follow it only when it holds up against src_bytes (and plans_ints, ws_bytes): a row that does not comes out
 * as a zero frame, no address is formed from it.  Zero frames are written by the last launch, so dst is fully defined.
 *   cc_collate_resize_crop_u8, CC_COLLATE_ROW = 6 values: [0] kind (0 = a zero frame, 1 = transform)  [1] byte offset of the
 *     source frame in src  [2] H  [3] W  [4] int32 offset of the frame's plan (cc_resize_plan_build of (H, W, n_px, resize)) in
 *     plans_dev  [5] byte offset in ws of the frame's horizontal result (3 x (row1 - row0) x n_px bytes; read only where both
 *     passes run; frames must not share it)
 *   cc_collate_crop_flip_u8, CC_COLLATE_BOX_ROW = 10 values: [0] kind  [1] byte offset  [2] H  [3] W  [4] top  [5] left
 *     [6] height  [7] width  [8] flip  [9] interp (0 bilinear, 1 bicubic)
 * plans_dev: the plans of the call's sizes one behind the other, plans_ints int32 values in all.
 * cc_collate_resize_crop_workspace_bytes: n_out x the largest horizontal result among the clips' sizes (0 where no size runs
 * both passes) - frame i may then use offset i * (bytes / n_out).
 * CC_ERR_INVALID for a NULL src / dst / table / plans / clips_host, n_out <= 0, n_clips <= 0 or a format other than the two uint8
 * codes; CC_ERR_WORKSPACE for a workspace that cannot hold one horizontal result of the call's largest size; all before any
 * launch.  No upload, no synchronisation (capturable once the tables are on the device). */
#define CC_RESIZE_MAX_TAPS 65
#define CC_COLLATE_ROW 6
#define CC_COLLATE_BOX_ROW 10
#define CC_COLLATE_MAX_PLANES 4096
/* the status cc_resize_crop_u8 gives for frames of this size (CC_OK, CC_ERR_UNSUPPORTED, CC_ERR_INVALID); no GPU needed */
int cc_resize_crop_status(int32_t H, int32_t W, int32_t n_px, int32_t resize);
size_t cc_collate_resize_crop_workspace_bytes(const int64_t* clips_host, int32_t n_clips, int32_t n_out, int32_t n_px,
                                              int32_t resize);
int cc_collate_resize_crop_u8(const void* src, size_t src_bytes, int32_t fmt, const int64_t* clips_host, int32_t n_clips,
                              const int64_t* rows_dev, int32_t n_out, const int32_t* plans_dev, size_t plans_ints, int32_t n_px,
                              int32_t resize, void* dst, int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream);
int cc_collate_crop_flip_u8(const void* src, size_t src_bytes, int32_t fmt, const int64_t* clips_host, int32_t n_clips,
                            const int64_t* rows_dev, int32_t n_out, int32_t n_px, void* dst, int32_t dst_fmt, void* stream);

/* YUV 4:2:0 sources: what decoders produce (a software decoder's yuv420p, a hardware decoder's pitched NV12 surfaces) taken
 * by the frame preprocessing directly - the conversion to RGB happens in the fetch of the first pass that touches the source,
 * no RGB image of the source size is ever in memory.  DESIGN.md, "YUV 4:2:0 sources".
 *
 * THE CONVERSION, a fixed integer definition.  8-bit Y, Cb, Cr.  matrix: CC_YUV_BT601 (Kr = 0.299, Kb = 0.114) or CC_YUV_BT709
 * (Kr = 0.2126, Kb = 0.0722), Kg = 1 - Kr - Kb.  range: CC_YUV_LIMITED (oy = 16, sy = 255/219, sc = 255/224) or CC_YUV_FULL
 * (oy = 0, sy = sc = 1).  Five real coefficients cY = sy, cRV = 2 (1 - Kr) sc, cGU = 2 Kb (1 - Kb) / Kg sc,
 * cGV = 2 Kr (1 - Kr) / Kg sc, cBU = 2 (1 - Kb) sc, each C = round(c 2^16) computed on the host in double
 * (cc_yuv_coefficients).  Per pixel in int32, >> an arithmetic shift:
 *   y = Y - oy, u = Cb - 128, v = Cr - 128
 *   R = clamp((CY y + CRV v         + 32768) >> 16, 0, 255)
 *   G = clamp((CY y - CGU u - CGV v + 32768) >> 16, 0, 255)
 *   B = clamp((CY y + CBU u         + 32768) >> 16, 0, 255)
 *                  CY     CRV    CGU    CGV    CBU
 *   601 limited  76309 104597  25675  53279 132201        (the constants of swscale's ITU601 table; swscale's BYTES are not
 *   601 full     65536  91881  22553  46802 116130         claimed - its converters differ among themselves)
 *   709 limited  76309 117489  13975  34925 138438
 *   709 full     65536 103206  12276  30679 121609
 * Every channel is within 1 LSB of clamp(floor(real + 0.5)) of the real formula; the accumulator stays below 2^31.
 * Chroma is REPLICATED: luma (y, x) uses chroma sample (y >> 1, x >> 1), chroma planes are ceil(H / 2) x ceil(W / 2); no
 * chroma interpolation, no siting.
 *
 * cc_yuv420_layout describes every 8-bit 4:2:0 arrangement, in bytes from the source's first byte: frame f starts at
 * f * frame_stride; in a frame Y(y, x) is at y * y_pitch + x, Cb(cy, cx) at u_offset + cy * c_pitch + cx * c_step and Cr the same
 * from v_offset.  Tight I420: c_step 1, V behind U; YV12: the offsets swapped; NV12: c_step 2, v_offset = u_offset + 1; NV21:
 * the reverse; a pitched decoder surface: its pitches.  cc_yuv420_layout_tight fills it for tight CC_YUV420_I420 /
 * CC_YUV420_NV12 frames one behind the other and returns the bytes of one frame, H W + 2 ceil(H / 2) ceil(W / 2) (0, and
 * nothing written, for another kind, a matrix / range outside {0, 1} or H, W outside 1 .. 8192).
 *
 * Every entry point takes src_bytes and checks, before any launch, that every address the descriptor can form for (F, H, W)
 * lies inside [0, src_bytes): a descriptor that fails, a negative field, a pitch shorter than its row, a c_step outside
 * {1, 2}, a matrix or range outside {0, 1}: CC_ERR_INVALID.  Sources may start at ANY byte address, H and W may be odd;
 * 4 <= H, W <= 8192, else CC_ERR_UNSUPPORTED (as the RGB entries).  Not taken by THESE entries: 4:2:2, 4:4:4 and samples
 * of more than 8 bits (P010) - the cc_*_yuv_u8 entries below take them; by neither: interlaced chroma siting, chroma
 * interpolation, BT.2020, alpha.
 *
 *   cc_yuv420_to_rgb_u8             the conversion alone -> [F, H, W, 3] / [F, 3, H, W] (dst_fmt); one launch.
 *   cc_resize_crop_yuv420_u8        cc_resize_crop_u8 with this source: the same plan, the same workspace
 *                                   (cc_resize_crop_workspace_bytes), the same status rules, at most two launches, capturable.
 *   cc_resized_crop_flip_yuv420_u8  cc_resized_crop_flip_u8 with this source: one launch, the same box rules.
 *   cc_collate_resize_crop_yuv420_u8 / cc_collate_crop_flip_yuv420_u8   the ragged forms: the packed buffer holds TIGHT frames
 *                                   of one kind (CC_YUV420_I420 or CC_YUV420_NV12; another kind: CC_ERR_INVALID), a frame of H x W
 *                                   is H W + 2 ceil(H / 2) ceil(W / 2) bytes and the clip table's and the rows' byte offsets count
 *                                   in those; the same row tables, launch bound and zero-frame rule as the RGB entries.
 * CONTRACT of the four fused entries: dst is bit for bit what the RGB entry gives on cc_yuv420_to_rgb_u8's output. */
#define CC_YUV_BT601 0
#define CC_YUV_BT709 1
#define CC_YUV_LIMITED 0
#define CC_YUV_FULL 1
#define CC_YUV420_I420 0
#define CC_YUV420_NV12 1
typedef struct cc_yuv420_layout {
    int64_t frame_stride, y_pitch, u_offset, v_offset, c_pitch;
    int32_t c_step, matrix, range;
} cc_yuv420_layout;
/* out5: (CY, CRV, CGU, CGV, CBU); CC_ERR_INVALID for a matrix / range outside {0, 1}; no GPU needed */
int cc_yuv_coefficients(int32_t matrix, int32_t range, int32_t* out5);
size_t cc_yuv420_layout_tight(int32_t kind, int32_t H, int32_t W, int32_t matrix, int32_t range, cc_yuv420_layout* out);
int cc_yuv420_to_rgb_u8(const void* src, size_t src_bytes, const cc_yuv420_layout* layout, int32_t F, int32_t H, int32_t W,
                        void* dst, int32_t dst_fmt, void* stream);
int cc_resize_crop_yuv420_u8(const void* src, size_t src_bytes, const cc_yuv420_layout* layout, int32_t F, int32_t H, int32_t W,
                             const void* plan_dev, int32_t n_px, int32_t resize, void* dst, int32_t dst_fmt, void* ws,
                             size_t ws_bytes, void* stream);
int cc_resized_crop_flip_yuv420_u8(const void* src, size_t src_bytes, const cc_yuv420_layout* layout, int32_t F, int32_t H,
                                   int32_t W, int32_t frames_per_clip, const int32_t* boxes_dev, int32_t n_px, int32_t interp,
                                   void* dst, int32_t dst_fmt, void* stream);
int cc_collate_resize_crop_yuv420_u8(const void* src, size_t src_bytes, int32_t kind, int32_t matrix, int32_t range,
                                     const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out,
                                     const int32_t* plans_dev, size_t plans_ints, int32_t n_px, int32_t resize, void* dst,
                                     int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream);
int cc_collate_crop_flip_yuv420_u8(const void* src, size_t src_bytes, int32_t kind, int32_t matrix, int32_t range,
                                   const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out,
                                   int32_t n_px, void* dst, int32_t dst_fmt, void* stream);

/* YUV sources in general: the other pixel formats decoders emit - 4:2:2 and 4:4:4 sampling, and samples of 10, 12 or 16 bits in
 * 16-bit words (a hardware decoder's pitched P010 / P016 surfaces, a software decoder's yuv420p10le, yuv422p, yuv444p, ...) -
 * through the same fetch, so everything behind it is the code of the RGB and the 4:2:0 entries.  The cc_*_yuv420_u8 entries
 * above are these with sub_x = sub_y = 1, depth 8, shift 0: one code path, the same bytes.  DESIGN.md, "YUV sources".
 *
 * THE CONVERSION for depth d in {8, 10, 12, 16}.  A sample is n = word >> shift.  d = 8: word is a byte and shift is 0.
 * Otherwise word is a little-endian 16-bit word and 0 <= shift <= 16 - d: P010 is d = 10 with shift 6, yuv420p10le d = 10 with
 * shift 0, P016 d = 16 with shift 0.  Bits below shift are discarded, whatever they hold.  Real formula, Kr, Kb, Kg as above:
 *   limited range: oy = 16 2^(d-8), sy = 255 / (219 2^(d-8)), sc = 255 / (224 2^(d-8))
 *   full range:    oy = 0, sy = sc = 255 / (2^d - 1)
 *   chroma centre 2^(d-1);  R = sy (Y - oy) + 2 (1 - Kr) sc (V - centre)
 *                           G = sy (Y - oy) - 2 Kb (1 - Kb) / Kg sc (U - centre) - 2 Kr (1 - Kr) / Kg sc (V - centre)
 *                           B = sy (Y - oy) + 2 (1 - Kb) sc (U - centre)
 * Integer definition: C = floor(c 2^Q + 0.5) computed in double, Q = 16 for d = 8 (the tables and bytes above) and Q = 20 for
 * d > 8 (cc_yuv_coefficients_depth); each channel is clamp((sum + 2^(Q-1)) >> Q, 0, 255) in int32, >> an arithmetic shift.
 *                       CY    CRV    CGU    CGV    CBU
 *   d 10 601 limited  305236 418389 102698 213115 528805        d 16 601 limited  4769 6537 1605 3330 8263
 *   d 10 601 full     261375 366448  89949 186658 463157        d 16 709 limited  4769 7343  873 2183 8652
 *   d 10 709 limited  305236 469956  55902 139699 553753
 *   d 10 709 full     261375 411614  48962 122356 485008
 * For samples 0 .. 2^d - 1 the accumulator stays at or below 5.8e8 < 2^31 and every channel is within 1 LSB of
 * clamp(floor(real + 0.5)); a larger n (possible only where shift < 16 - d) is outside the definition - no address depends on a
 * sample.  Chroma is REPLICATED: luma (y, x) uses chroma (y >> sub_y, x >> sub_x); chroma planes have
 * ceil(H / 2^sub_y) x ceil(W / 2^sub_x) samples, odd H and W are legal.
 * OUT OF SCOPE: BT.2020 and any PQ / HLG tone mapping (10-bit frames are converted as the SDR signal their matrix describes);
 * packed formats (YUYV, UYVY), big-endian words, 4:1:1, alpha planes; interpolated chroma siting and dithering.
 *
 * cc_yuv_layout, all positions in bytes from the source's first byte: frame f at f * frame_stride; in a frame Y(y, x) at
 * y * y_pitch + x * B (B = bytes of a sample, 1 at depth 8, else 2), Cb(cy, cx) at u_offset + cy * c_pitch + cx * c_step and Cr
 * the same from v_offset; c_step = B where the chroma planes are separate, 2 B where interleaved; sub_x, sub_y: log2 of the
 * chroma subsampling, 0 or 1.  cc_yuv_layout_tight fills it for tight frames of a named format one behind the other (Y plane,
 * then U and V planes, or one interleaved UV plane) and returns the bytes of one frame (0, and nothing written, for another
 * format, a matrix / range outside {0, 1} or H, W outside 1 .. 8192):
 *                 8-bit            10-bit (shift)                     12-bit (shift)           16-bit
 *   planar        I420 I422 I444   I420P10 I422P10 I444P10 (0)        I420P12 (0)              I444P16
 *   semi-planar   NV12             P010 (6)                           P012 (4)                 P016
 *
 * DESCRIPTOR CHECK before any launch.  CC_ERR_INVALID: a depth outside {8, 10, 12, 16}; a shift outside 0 .. 16 - depth, or
 * nonzero at depth 8; sub_x / sub_y outside {0, 1}; a c_step other than one or two samples; a matrix / range outside {0, 1}.
 * Then sizes outside 4 .. 8192: CC_ERR_UNSUPPORTED.  Then CC_ERR_INVALID again: a negative field; a pitch shorter than its row
 * in bytes; for 16-bit samples an odd src address, offset, pitch or frame stride; any luma or chroma byte of (F, H, W) at or
 * beyond src_bytes.  8-bit sources may start at ANY byte address.
 *
 *   cc_yuv_to_rgb_u8              the conversion alone -> [F, H, W, 3] / [F, 3, H, W] (dst_fmt); one launch.
 *   cc_resize_crop_yuv_u8         cc_resize_crop_u8 with this source: the same plan and workspace, at most two launches.
 *   cc_resized_crop_flip_yuv_u8   cc_resized_crop_flip_u8 with this source: one launch, the same box rules.
 *   cc_collate_resize_crop_yuv_u8 / cc_collate_crop_flip_yuv_u8   the ragged forms: the packed buffer holds TIGHT frames of one
 *                                 named format (another: CC_ERR_INVALID); the clip table's and the rows' byte offsets count in
 *                                 those frames and, for 16-bit samples, are even (an odd clip offset: CC_ERR_INVALID; an odd
 *                                 row offset: a zero frame); the same row tables, launch bound and zero-frame rule.
 * CONTRACT of the four fused entries: dst is bit for bit what the RGB entry gives on cc_yuv_to_rgb_u8's output, and no
 * source-sized RGB image is stored. */
#define CC_YUV_I420 0          /* = CC_YUV420_I420 */
#define CC_YUV_NV12 1          /* = CC_YUV420_NV12 */
#define CC_YUV_I422 2
#define CC_YUV_I444 3
#define CC_YUV_I420P10 4
#define CC_YUV_I422P10 5
#define CC_YUV_I444P10 6
#define CC_YUV_P010 7
#define CC_YUV_I420P12 8
#define CC_YUV_P012 9
#define CC_YUV_P016 10
#define CC_YUV_I444P16 11
#define CC_YUV_FORMATS 12
typedef struct cc_yuv_layout {
    int64_t frame_stride, y_pitch, u_offset, v_offset, c_pitch;
    int32_t c_step, sub_x, sub_y, depth, shift, matrix, range;
} cc_yuv_layout;
/* out5: (CY, CRV, CGU, CGV, CBU) of the depth; CC_ERR_INVALID for a matrix / range outside {0, 1} or a depth outside
 * {8, 10, 12, 16}; no GPU needed */
int cc_yuv_coefficients_depth(int32_t matrix, int32_t range, int32_t depth, int32_t* out5);
size_t cc_yuv_layout_tight(int32_t format, int32_t H, int32_t W, int32_t matrix, int32_t range, cc_yuv_layout* out);
int cc_yuv_to_rgb_u8(const void* src, size_t src_bytes, const cc_yuv_layout* layout, int32_t F, int32_t H, int32_t W, void* dst,
                     int32_t dst_fmt, void* stream);
int cc_resize_crop_yuv_u8(const void* src, size_t src_bytes, const cc_yuv_layout* layout, int32_t F, int32_t H, int32_t W,
                          const void* plan_dev, int32_t n_px, int32_t resize, void* dst, int32_t dst_fmt, void* ws,
                          size_t ws_bytes, void* stream);
int cc_resized_crop_flip_yuv_u8(const void* src, size_t src_bytes, const cc_yuv_layout* layout, int32_t F, int32_t H, int32_t W,
                                int32_t frames_per_clip, const int32_t* boxes_dev, int32_t n_px, int32_t interp, void* dst,
                                int32_t dst_fmt, void* stream);
int cc_collate_resize_crop_yuv_u8(const void* src, size_t src_bytes, int32_t format, int32_t matrix, int32_t range,
                                  const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out,
                                  const int32_t* plans_dev, size_t plans_ints, int32_t n_px, int32_t resize, void* dst,
                                  int32_t dst_fmt, void* ws, size_t ws_bytes, void* stream);
int cc_collate_crop_flip_yuv_u8(const void* src, size_t src_bytes, int32_t format, int32_t matrix, int32_t range,
                                const int64_t* clips_host, int32_t n_clips, const int64_t* rows_dev, int32_t n_out, int32_t n_px,
                                void* dst, int32_t dst_fmt, void* stream);

/* S2 - the meanP similarity tail, CLIP4Clip._loose_similarity (modules/clip4clip.py:357-366) with
 * _mean_pooling_for_similarity_visual (:305-316):
 *   v_hat = v/|v| per frame; v_bar = sum_t mask*v_hat / max(sum_t mask, 1 if 0); v_bar /= |v_bar|
 *   t_hat = t/|t|;  logits[Bt,Bv] = exp(logit_scale) * t_hat v_bar^T           (all fp32)
 * visual [Bv, Tn, E] fp32, video_mask [Bv, Tn] int64 (as the reference passes it), text [Bt, E].
 * pooled_out (optional) [Bv, E] receives v_bar.  ws: (Bv + Bt) * E floats. */
size_t cc_similarity_workspace_bytes(int32_t Bt, int32_t Bv, int32_t E);

/* The operands of the similarity GEMM as a by-product of their producers (the evaluation loop, main.py:381-534: features
 * are cached batch by batch and multiplied once at the end).  A plane row = 3E fp16 values, cc_similarity_plane_row_bytes(E):
 *   cc_normalize_rows_planes_f32        rows / |row| (clip4clip.py:361-362) -> planes [R, 3E] (video_side 0: the text operand,
 *                                       1: rows that are pooled video features already) and, optionally, fp32 `out`
 *   cc_video_pool_normalize_planes_f32  clip4clip.py:305-316,357-360 -> video-side planes [Bv, 3E] (+ fp32 `pooled`, optional)
 *   cc_scaled_dot_planes_f32            logits [Bt, Bv] = mult * text . video^T from the planes: ONE GEMM launch, nothing else.
 *                                       The video plane buffer must hold video_rows >= cc_similarity_padded_rows(Bv) rows with
 *                                       the rows behind Bv ZERO (the tiles read whole multiples of their width).
 *   cc_scaled_dot_planes_products_f32   the same with `products` (3, 2 or 1) of the three fp16 products per multiply-add issued:
 *                                       3 = hi.hi + hi.lo + lo.hi (both operands to 22 bits: 2e-6 on a cosine of unit rows - the
 *                                       default everywhere, rank-exact against the reference's fp32 product on its fixtures);
 *                                       2 = fp16(text) x video-to-22-bits; 1 = fp16 x fp16 (measured on 10k x 1k unit rows:
 *                                       bench.py `similarity_10k_x_1k.products`).  All are inside the 1e-3 BASELINE.json's
 *                                       north_star asks of similarities; the GEMM's matrix-core work is products / 3.
 * E % 64 == 0.  Same values as cc_scaled_dot_nt_f32 on the normalised rows. */
size_t cc_similarity_plane_row_bytes(int32_t E);
int32_t cc_similarity_padded_rows(int32_t Bv);
int cc_normalize_rows_planes_f32(const float* in, float* out, void* planes, int32_t video_side, int32_t R, int32_t E,
                                 void* stream);
int cc_video_pool_normalize_planes_f32(const float* visual, const int64_t* video_mask, int32_t Bv, int32_t Tn, int32_t E,
                                       float* pooled, void* planes, void* stream);
/* The windows of long videos: visual [Bv, S, E] fp32 holds the per-segment features of whole videos, windows [nW, 3] int32 ON
 * THE DEVICE = (video, start segment, stop segment); plane row w (video side) = cc_video_pool_normalize_planes_f32 on the
 * segments [start, stop) of that video with a mask of ones, bit for bit (one wave per window, the same device code).
 * E % 64 == 0, E <= 1024 (CC_ERR_UNSUPPORTED beyond).  The table cannot be checked on the host: an entry with video outside
 * [0, Bv), start < 0, stop > S or start >= stop reads nothing and gives a zero row. */
int cc_video_window_pool_planes_f32(const float* visual, const int32_t* windows, int32_t Bv, int32_t S, int32_t nW, int32_t E,
                                    void* planes, void* stream);
int cc_scaled_dot_planes_f32(const void* text_planes, const void* video_planes, int32_t Bt, int32_t Bv,
                             int32_t video_rows, int32_t E, float mult, float* logits, int32_t ldl, void* stream);
int cc_scaled_dot_planes_products_f32(const void* text_planes, const void* video_planes, int32_t Bt, int32_t Bv,
                                      int32_t video_rows, int32_t E, float mult, int32_t products, float* logits,
                                      int32_t ldl, void* stream);

/* Exact top-k search over plane rows (search.hip): for every query row the k best of Bg gallery rows, without the
 * [Bq, Bg] matrix.  query_planes [Bq, 3E] and gallery_planes [>= Bg, 3E] are plane rows as the two producers above write
 * them; the first products * E halfs of a query row are multiplied with the first products * E halfs of a gallery row, so
 * text queries against a video gallery give rows of the matrix S of cc_scaled_dot_planes_products_f32 and video queries
 * against a text gallery rows of S^T.  Gallery rows at index Bg or above are never read (no tile padding).
 *   score(q, g) = (mult * 2^-20) * acc, acc ONE fp32 accumulator fed by v_mfma_f32_16x16x32_f16 over the 32-wide k-slices in
 *   ascending order: the bits cc_scaled_dot_planes_products_f32 stores for the same pair.
 *   Row q of scores / ids [Bq, k] = the first k entries of the stable descending sort of score(q, 0 .. Bg - 1): larger score
 *   first, equal scores by smaller id, -0 and +0 equal; entries beyond Bg are (-inf, -1).  Non-finite plane values are
 *   outside the contract.
 * Limits: 1 <= k <= 128, products 1..3, E % 64 == 0, E <= 1024, Bq <= 16 * 65535; the one combination the streaming kernel's
 * LDS cannot hold is products * E == 3072 (E = 1024, products = 3) together with k == 128 - all CC_ERR_UNSUPPORTED.  NULL
 * operands or Bq, Bg, E <= 0: CC_ERR_INVALID; a NULL or short workspace: CC_ERR_WORKSPACE - every check before anything is
 * read or launched.  Two launches, no host synchronisation (capturable).  The workspace holds partial lists only -
 * Bq * cc_similarity_topk_slices * k pairs of 8 bytes; nothing of size Bq * Bg exists.
 * cc_similarity_topk_slices: the contiguous gallery slices the streaming launch cuts Bg rows into (= partial lists per
 * query row the merge launch reads); a plan query, no GPU needed, >= 1. */
int32_t cc_similarity_topk_slices(int32_t Bq, int32_t Bg, int32_t k);
size_t cc_similarity_topk_workspace_bytes(int32_t Bq, int32_t Bg, int32_t k);
int cc_similarity_topk_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                  float mult, int32_t products, int32_t k, float* scores, int32_t* ids, void* ws,
                                  size_t ws_bytes, void* stream);
/* Top-k search under the CAMoE dual softmax (camoe_dsl), still without a matrix.  D[i, j] = n * S[i, j] * exp(S[i, j] - m_j) / s_j
 * needs two floats per VIDEO row j: m_j = max_i S[i, j] and s_j = sum_i exp(S[i, j] - m_j) over the text rows i.
 *
 * cc_dsl_col_stats_planes_f32: m[Bv], s[Bv] = what cc_dsl_col_stats_f32 gives on the matrix cc_scaled_dot_planes_products_f32
 * stores for the same planes (texts as rows), computed from the plane rows.  Only the first Bt text rows and the first Bv
 * video rows are read (no padding, rows behind them may hold anything); Bt == 0 gives (-inf, 0) (text_planes and ws may then
 * be NULL).  Non-finite plane values are outside the contract.
 *   Every S(i, j) has the matrix op's bits (one fp32 accumulator, 32-wide k-slices ascending, the operand order of
 *   gemm_f16_kernel, then sc * acc as described above), so m is BIT-EQUAL to the column maximum of that matrix.
 *   s: fixed summation tree, no atomics, the same bits on every run.  The text rows are cut into
 *   cc_dsl_col_stats_planes_slices(Bt) contiguous slices of 16-row tiles - a function of Bt alone - so the pair of a video
 *   row does not depend on Bv or on the rows that share the call: adding clips in batches equals adding them at once.
 *   Tree: a lane folds 4 text rows a step into a running pair (online rescale: s <- s * expf(m - m') + sum of 4 expf(x - m'),
 *   7 roundings a step for an old term, ceil(ceil(tiles / slices) / 4) steps at most, tiles = ceil(Bt / 16)); the 16 pairs
 *   of a workgroup are merged in a fixed order (19 roundings), the slices' pairs in slice order by a second launch
 *   (slices + 3).  Longest chain of roundings: 7 * ceil(ceil(tiles / slices) / 4) + 19 + slices + 3 (search.hip).
 *   Two launches, no host synchronisation (capturable); no workgroup reads what another one of the same launch wrote.
 *   ws: cc_dsl_col_stats_planes_workspace_bytes(Bt, Bv) = slices * Bv pairs; nothing of size Bt * Bv exists.
 * Limits: products 1..3, E % 64 == 0, E <= 1024, Bv <= 16 * 65535: CC_ERR_UNSUPPORTED.  NULL operands, Bt < 0, Bv <= 0 or
 * E <= 0: CC_ERR_INVALID; a NULL or short workspace (Bt > 0): CC_ERR_WORKSPACE - in this order, before anything is launched.
 *
 * cc_similarity_topk_dsl_planes_f32: cc_similarity_topk_planes_f32 ranking D instead of S,
 *   D(q, g) = (n_total * S) * (expf(S - m[x]) / s[x]),  x = g (stats_on_gallery = 1: a gallery of clips, text queries) or
 *   x = q (stats_on_gallery = 0: a gallery of captions, clip queries; m, s [Bq]),
 * evaluated with the fp32 operations of cc_dsl_apply_f32: a score has the bits that entry point writes over the matrix op's
 * entry for the same m, s, n_total.  The order contract is the plain op's (stable descending, equal scores by smaller id,
 * -0 == +0 with the sign restored, (-inf, -1) beyond Bg; +-inf order as floats; NaN scores are outside the contract).
 * Rows at or above Bg are never read, their statistics included.  Limits, workspace (cc_similarity_topk_workspace_bytes)
 * and the two launches are the plain op's; NULL m or s, n_total < 0 or stats_on_gallery other than 0 / 1: CC_ERR_INVALID. */
int32_t cc_dsl_col_stats_planes_slices(int32_t Bt);
size_t cc_dsl_col_stats_planes_workspace_bytes(int32_t Bt, int32_t Bv);
int cc_dsl_col_stats_planes_f32(const void* text_planes, const void* video_planes, int32_t Bt, int32_t Bv, int32_t E, float mult,
                                int32_t products, float* m, float* s, void* ws, size_t ws_bytes, void* stream);
int cc_similarity_topk_dsl_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                      float mult, int32_t products, int32_t k, const float* m, const float* s,
                                      int32_t stats_on_gallery, int32_t n_total, float* scores, int32_t* ids, void* ws,
                                      size_t ws_bytes, void* stream);
/* Grouped top-k search: the k best GROUPS of gallery rows, each by its best row (the sentences of a video, the windows of
 * a long video), still in one pass without the matrix.  The rows of a group are adjacent; group_head [Bg] int32 names the
 * first row of every row's group: group_head[r] <= r, group_head[group_head[r]] == group_head[r], non-decreasing.
 *   Result: of the plain entry's stable descending row order (larger score first, equal scores by smaller id, -0 == +0) the
 *   first k rows that are the first of their group to appear.  Entry i is the best row of the i-th best group and its
 *   score; ties between groups go to the group whose best row has the smaller id, ties inside a group to the smallest id;
 *   fewer than k groups: (-inf, -1).  Scores are the bits of cc_scaled_dot_planes_products_f32 (the _dsl entry: the bits
 *   cc_dsl_apply_f32 writes over them, as cc_similarity_topk_dsl_planes_f32).  group_head[r] == r for every r gives the plain
 *   entry's result bit for bit.  Rows and heads at or above Bg are never read.  A malformed group_head gives an unspecified
 *   ranking and no access outside the Bg rows, the lists or the workspace (every index taken from it is clamped).
 * Limits, workspace (cc_similarity_topk_workspace_bytes), launches and the order of the early returns are the plain
 * entries'; a NULL group_head: CC_ERR_INVALID.  A group longer than a wave's share of the rows is streamed by one wave:
 * exact, unbalanced. */
int cc_similarity_topk_grouped_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                          float mult, int32_t products, int32_t k, const int32_t* group_head, float* scores,
                                          int32_t* ids, void* ws, size_t ws_bytes, void* stream);
int cc_similarity_topk_grouped_dsl_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg,
                                              int32_t E, float mult, int32_t products, int32_t k, const float* m, const float* s,
                                              int32_t stats_on_gallery, int32_t n_total, const int32_t* group_head, float* scores,
                                              int32_t* ids, void* ws, size_t ws_bytes, void* stream);
/* Masked search: a bit per gallery row says whether the row may be ranked (rows taken out of a gallery, a tenant's subset,
 * "everything but the query's own clip").  One mask format for all three entries: int32 words, bit b of word w stands for
 * row 32 w + b, 1 = selectable; a mask row is mask_words >= ceil(Bg / 32) words, bits at or above Bg are ignored whatever
 * they hold.
 *
 * cc_similarity_topk_masked_planes_f32: the four entries above in one, over the selectable rows only.  row_mask holds ONE
 * mask row for all queries (mask_rows = 1) or one per query row (mask_rows = Bq, mask_words apart).  m == s == NULL ranks
 * S, both non-NULL the dual softmax D as cc_similarity_topk_dsl_planes_f32 (stats_on_gallery, n_total as there; ignored
 * without m, s); group_head == NULL ranks rows, otherwise groups as cc_similarity_topk_grouped_planes_f32.
 *   Result: the unmasked entry's, of the matrix with the unselectable columns dropped - the same score bits, the same order
 *   (stable descending, equal scores by smaller id), ids are still row indices of the whole gallery; (-inf, -1) beyond the
 *   number of selectable rows.  Grouped: a group is ranked by its best SELECTABLE row; a group without one gives no entry.
 *   Statistics and heads are indexed as in the unmasked entries; an all-ones mask gives their results bit for bit.
 *   mask_rows = 1: a 16-row tile without a selectable row (an aligned halfword of the mask that is 0) is neither read nor
 *   multiplied - a search over a clustered subset reads that subset's bytes.  Per-query masks skip nothing.
 * Limits, workspace (cc_similarity_topk_workspace_bytes / _slices), the two launches and the order of the early returns are
 * the plain entry's; CC_ERR_INVALID also for a NULL row_mask, mask_rows other than 1 or Bq, mask_words < ceil(Bg / 32), or
 * exactly one of m / s (and, with both, n_total < 0 or stats_on_gallery other than 0 / 1) - before anything is read.
 *
 * cc_dsl_col_stats_planes_masked_f32: cc_dsl_col_stats_planes_f32 over the text rows whose bit is set in text_mask (one mask
 * row, >= ceil(Bt / 32) words).  The tree is the unmasked one (slices from Bt alone, wave and lane order) with the
 * unselectable rows' terms left out - neither their maximum nor their expf enters, tiles without a selectable row are not
 * read: m is bit-equal to the column maximum over the selectable rows, an all-ones mask gives the unmasked entry's bits, no
 * selectable row gives (-inf, 0).  Workspace, limits and returns are the unmasked entry's; a NULL text_mask with Bt > 0:
 * CC_ERR_INVALID.
 *
 * cc_pack_row_mask_u8: flags [rows][n] bytes (non-zero = selectable) -> out_words [rows][words_per_row] mask words,
 * words_per_row >= ceil(n / 32); bits at or above n are written as 0.  One launch.  NULL pointers, rows <= 0, n <= 0 or too
 * few words: CC_ERR_INVALID. */
int cc_similarity_topk_masked_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                         float mult, int32_t products, int32_t k, const int32_t* row_mask, int32_t mask_rows,
                                         int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery,
                                         int32_t n_total, const int32_t* group_head, float* scores, int32_t* ids, void* ws,
                                         size_t ws_bytes, void* stream);
int cc_dsl_col_stats_planes_masked_f32(const void* text_planes, const void* video_planes, int32_t Bt, int32_t Bv, int32_t E,
                                       float mult, int32_t products, const int32_t* text_mask, float* m, float* s, void* ws,
                                       size_t ws_bytes, void* stream);
int cc_pack_row_mask_u8(const uint8_t* flags, int32_t rows, int32_t n, int32_t* out_words, int32_t words_per_row, void* stream);
/* Deep lists and cursors: more than 128 entries, or the entries that follow a known one, still exact and without the matrix.
 * One entry for the four rankings with cc_similarity_topk_masked_planes_f32's conventions, each part optional: row_mask ==
 * NULL: every row is selectable (mask_rows, mask_words are then not looked at); m == s == NULL ranks S, both non-NULL the dual
 * softmax D; group_head == NULL ranks rows, otherwise groups.  1 <= k <= CC_TOPK_DEEP_MAXK.
 *   Result: scores / ids [Bq][k]: the first k entries of the ordering the other entries cut at 128 (stable descending, equal
 *   scores by smaller id, the same score bits), (-inf, -1) behind the selectable rows or groups.
 *   after_scores (fp32 [Bq]) and after_ids (int32 [Bq]), both or neither, on the device: the list of query row q then starts
 *   BEHIND the entry (after_scores[q], after_ids[q]) of that ordering - typically the last column of an earlier result, so
 *   two calls with k = a and k = b give the columns [0, a) and [a, a + b) of one call with k = a + b.  The pair need not be
 *   selectable any more (a row removed since: the list continues behind the place it had); after_ids[q] < 0 (the fill:
 *   nothing lies behind it) gives the fill.  Grouped: the pair is a group's best row, as the grouped entries return it.
 *   How: a (score, id) pair is one 64-bit key whose unsigned order is the result's order, so "below key X" is an exact,
 *   stateless continuation point.  The list is built in pages of P = the longest list the streaming launch's LDS holds for
 *   (E, products), at most 128 (127 for E = 1024, products = 3): ceil(k / P) pairs of launches, the streaming one keeping only
 *   the keys below the last key of the page before (below the key of the after_* pair: one small launch in front builds
 *   it), the merge writing its page at column offset and its last key to a device buffer - no host read between pages, no
 *   atomics: capturable.  Without after_* the first page is the plain entry's launch.  Groups: the bound is applied to a
 *   finished group's candidate, not to its rows, so no group returns through its second-best row.  Every page is one pass
 *   over the gallery.
 * ws: cc_similarity_topk_deep_workspace_bytes(Bq, Bg, E, products, k) bytes: the plain entry's workspace at min(k, P) plus
 * 8 Bq bytes for the bounds - it does not grow with the number of pages (0 for arguments the entry refuses).
 * Returns in this order, before anything is read: CC_ERR_INVALID (a NULL pointer other than the optional ones, Bq / Bg / E
 * <= 0, k < 1, exactly one of m / s, with both n_total < 0 or stats_on_gallery other than 0 / 1, with a mask mask_rows
 * other than 1 or Bq or mask_words < ceil(Bg / 32), exactly one of after_scores / after_ids), CC_ERR_UNSUPPORTED (k >
 * CC_TOPK_DEEP_MAXK, products outside 1..3, E % 64 != 0, E > 1024, Bq > 16 * 65535), CC_ERR_WORKSPACE.  (The cap is a
 * decision: 32 pages of 128, at most 64 launches a call.) */
#define CC_TOPK_DEEP_MAXK 4096
size_t cc_similarity_topk_deep_workspace_bytes(int32_t Bq, int32_t Bg, int32_t E, int32_t products, int32_t k);
int cc_similarity_topk_deep_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                       float mult, int32_t products, int32_t k, const int32_t* row_mask, int32_t mask_rows,
                                       int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery, int32_t n_total,
                                       const int32_t* group_head, const float* after_scores, const int32_t* after_ids, float* scores,
                                       int32_t* ids, void* ws, size_t ws_bytes, void* stream);
/* Rank of a known row or group: where target[q] stands for query row q, without the matrix and without a list.  The arguments
 * are cc_similarity_topk_masked_planes_f32's where they coincide; row_mask == NULL: every row is selectable (mask_rows,
 * mask_words are then not looked at); m == s == NULL ranks S, both non-NULL the dual softmax D; group_head == NULL ranks rows.
 * target: int32 [Bq] on the device.  x(q, r) below is the score the top-k entries give the pair, bit for bit.
 *   Rows: t_q = x(q, target[q]) - always computed from the target row, whose own mask bit is not consulted.  Over the
 *   selectable rows r < Bg: counts[q] = (#{x > t_q}, #{x == t_q}, #{r < target[q], x == t_q}) and score[q] = t_q: the three
 *   numbers cc_rank_counts_cols_f32 writes for the matrix row with gt_cols[q] = target[q] (plain float compares: -0 == +0, a
 *   NaN is neither greater nor equal).  The 0-based rank in the search's full ordering is counts[0] + counts[2].
 *   Groups: a group's score is the largest x of its selectable rows; target[q] is any row of the target group, t_q that
 *   group's score (-inf without a selectable row); the counts run over the groups that have a selectable row: greater, equal
 *   (the target's own included), and equal with the group lying in front of the target's.  Non-finite planes stay outside the
 *   contract here, as for the grouped searches.
 *   A target outside [0, Bg): counts (0, 0, 0), score -inf.
 * counts: int32 [Bq][3]; score: fp32 [Bq].  Three launches on the stream - the targets' scores (one wave per query row, the
 * MFMA sequence of every other score), the counting pass on the top-k grid, the sum over its slices - no atomics, no host
 * synchronisation: capturable.  ws: cc_similarity_rank_workspace_bytes(Bq, Bg) bytes (0 for Bq <= 0 or Bg <= 0).
 * Limits: E % 64 == 0, E <= 1024, products 1..3 (no k, so none of the top-k entries' LDS exclusions).  Returns in this order:
 * CC_ERR_INVALID (a NULL pointer other than the optional ones, Bq / Bg / E <= 0, exactly one of m / s, with both n_total < 0 or
 * stats_on_gallery other than 0 / 1, with a mask mask_rows other than 1 or Bq or mask_words < ceil(Bg / 32)),
 * CC_ERR_UNSUPPORTED, CC_ERR_WORKSPACE - before anything is read. */
size_t cc_similarity_rank_workspace_bytes(int32_t Bq, int32_t Bg);
int cc_similarity_rank_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E, float mult,
                                  int32_t products, const int32_t* target, const int32_t* row_mask, int32_t mask_rows,
                                  int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery, int32_t n_total,
                                  const int32_t* group_head, int32_t* counts, float* score, void* ws, size_t ws_bytes, void* stream);
/* A gallery split in shards (centerclip_amd/search_sharded.py; DESIGN.md, "Sharded gallery"): the three pieces that turn the
 * per-shard results of the entries above into the result of the concatenated gallery.  None reads anything on the host, none
 * uses atomics: capturable.
 *
 * cc_topk_merge_lists_f32: S descending lists per query row -> one.  scores fp32 / ids int32 [S][Bq][k], ids local to their
 * shard, id < 0 = a fill (its score is not looked at); 1 <= S <= CC_TOPK_MERGE_MAX_LISTS, 1 <= k <= CC_TOPK_DEEP_MAXK.
 *   out_scores fp32 [Bq][k], out_ids int64 [Bq][k] = ((int64)shard << 32) | id (-1: fill, score -inf), out_src int32 [Bq][k] =
 *   shard * k + index of the entry taken (-1: fill) - the caller gathers labels or any other payload with it.
 *   Order: larger score first, compared as the top-k entries' key does (the ordered bits of score + 0.0f: -0 and +0 are
 *   equal; the score leaves with the bits it came with), equal scores by smaller shard, then smaller id; fills last.
 *   Precondition, not checked: every input list is in that order (what the top-k entries return).  A violated precondition
 *   gives an unspecified selection, never an access outside the buffers.
 *   How: the keys are unique, so an entry's output slot is its own index plus, for each other list, the number of that list's
 *   entries in front of it - a binary search per list; one lane per entry, ceil(S k / 256) workgroups per query row.
 *   Returns CC_ERR_INVALID (a NULL pointer, S < 1, Bq <= 0, k < 1), then CC_ERR_UNSUPPORTED (S or k above its cap); there is
 *   no workspace.
 *
 * cc_similarity_target_score_planes_f32: the first launch of cc_similarity_rank_planes_f32 alone - score[q] = t_q of target[q]
 * (rows; with group_head the best selectable row of the target's group, -inf without one; with m, s the dual softmax, on
 * either side); a target outside [0, Bg): -inf.  Arguments, limits and the order of the refusals are that entry's, without
 * counts and workspace (CC_ERR_INVALID, then CC_ERR_UNSUPPORTED).
 *
 * cc_similarity_count_planes_f32: its counting pass against a bound the caller holds.  Over the candidates of query row q -
 * the selectable rows, or with group_head the groups that have one, each by its best row - with score x:
 *   counts[q] = (#{x > bound_scores[q]}, #{x == bound_scores[q]}, #{x == bound_scores[q], position < bound_front[q]}),
 * position = the row, or the group's best row.  bound_front[q] < 0: (0, 0, 0); bound_front[q] >= Bg: every equal candidate is
 * in front.  Plain float compares (-0 == +0; a NaN bound counts nothing).  Integers over a stream that any split of the
 * gallery partitions: the counts of the parts add up to the counts of the whole - with the bound a target's score from
 * cc_similarity_target_score_planes_f32 and bound_front its row (its group's head), the sum is cc_similarity_rank_planes_f32's
 * counts.  Two launches (the rank entry's second and third).  ws: cc_similarity_count_workspace_bytes(Bq, Bg) bytes (0 for
 * Bq <= 0 or Bg <= 0).  Returns in the rank entry's order: CC_ERR_INVALID, CC_ERR_UNSUPPORTED, CC_ERR_WORKSPACE. */
#define CC_TOPK_MERGE_MAX_LISTS 64
int cc_topk_merge_lists_f32(const float* scores, const int32_t* ids, int32_t S, int32_t Bq, int32_t k, float* out_scores,
                            int64_t* out_ids, int32_t* out_src, void* stream);
int cc_similarity_target_score_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E,
                                          float mult, int32_t products, const int32_t* target, const int32_t* row_mask,
                                          int32_t mask_rows, int32_t mask_words, const float* m, const float* s,
                                          int32_t stats_on_gallery, int32_t n_total, const int32_t* group_head, float* score,
                                          void* stream);
size_t cc_similarity_count_workspace_bytes(int32_t Bq, int32_t Bg);
int cc_similarity_count_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E, float mult,
                                   int32_t products, const float* bound_scores, const int32_t* bound_front, const int32_t* row_mask,
                                   int32_t mask_rows, int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery,
                                   int32_t n_total, const int32_t* group_head, int32_t* counts, void* ws, size_t ws_bytes,
                                   void* stream);
int cc_video_pool_normalize_f32(const float* visual, const int64_t* video_mask, int32_t Bv, int32_t Tn,
                                int32_t E, float* pooled, void* stream);
int cc_loose_similarity_f32(const float* text, const float* visual, const int64_t* video_mask,
                            int32_t Bt, int32_t Bv, int32_t Tn, int32_t E, float logit_scale,
                            float* logits, int32_t ldl, float* pooled_out,
                            void* ws, size_t ws_bytes, void* stream);
/* The same with the mask addressed through element strides (mask[v, t] = video_mask[v*row_stride + t*col_stride]):
 * the segment mask after clustering is every fd-th column of the frame mask (clip4clip.py:436-447), taken as a strided
 * view instead of a gathered copy. */
int cc_loose_similarity_strided_f32(const float* text, const float* visual, const int64_t* video_mask,
                                    int64_t mask_row_stride, int64_t mask_col_stride, int32_t Bt, int32_t Bv,
                                    int32_t Tn, int32_t E, float logit_scale, float* logits, int32_t ldl,
                                    float* pooled_out, void* ws, size_t ws_bytes, void* stream);
/* The same on the packed all-gather buffer of the multi-GPU step (modules/utils.py:47-64 + clip4clip.py:351-355 as
 * ONE collective): videos come in groups of `group` (one record per rank); video v = (g, l) has its frames at
 * visual + g*vis_group_stride + l*Tn*E (floats) and its mask row at video_mask + g*mask_group_stride +
 * l*mask_row_stride (int64 elements).  group >= Bv is the plain layout. */
int cc_loose_similarity_grouped_f32(const float* text, const float* visual, const int64_t* video_mask, int32_t group,
                                    int64_t vis_group_stride, int64_t mask_group_stride, int64_t mask_row_stride,
                                    int64_t mask_col_stride, int32_t Bt, int32_t Bv, int32_t Tn, int32_t E,
                                    float logit_scale, float* logits, int32_t ldl, float* pooled_out,
                                    void* ws, size_t ws_bytes, void* stream);
/* rows [R, E] -> rows / |row|: the text half of _loose_similarity (clip4clip.py:361-362) for the pre-pooled
 * (2-D visual_output) branch */
int cc_normalize_rows_f32(const float* in, float* out, int32_t R, int32_t E, void* stream);
/* logits[Bt,Bv] = mult * a[Bt,E] b[Bv,E]^T for already-normalised rows (|element| <= 1; the kernel splits each fp32
 * operand into two fp16 parts scaled by 2^10 and accumulates hi.hi + hi.lo + lo.hi in fp32 on the fp16 matrix cores -
 * 22-bit operands, fp32-level results; elements beyond +-63 overflow to inf).  E % 64 == 0.
 * ws: cc_similarity_workspace_bytes(Bt, Bv, E) (the split planes). (the sharded eval
 * similarity matrix, main.py:502-534, computed in one launch per row block). */
int cc_scaled_dot_nt_f32(const float* a, const float* b, int32_t Bt, int32_t Bv, int32_t E, float mult,
                         float* logits, int32_t ldl, void* ws, size_t ws_bytes, void* stream);

/* N4, forward values only - CrossEn (modules/losses.py:8-18) in both directions and their mean as CLIP4Clip.forward's
 * training branch forms it (modules/clip4clip.py:245-253): loss3[0] = mean_i -log_softmax(sim[i,:])[i],
 * loss3[1] = the same on sim^T, loss3[2] = (loss3[0] + loss3[1]) / 2.  sim [n,n] fp32 addressed through element strides.
 * ws: 2*n floats.  (No backward: training is out of scope; this is the loss a validation pass reports.) */
int cc_contrastive_loss_f32(const float* sim, int32_t n, int64_t row_stride, int64_t col_stride, float* loss3,
                            void* ws, size_t ws_bytes, void* stream);

/* N4 - the training branch's loss WITH its gradient (modules/clip4clip.py:245-262, 357-366; modules/losses.py:8-18): from the
 * features as the towers return them - text [n, E], visual [n, Tn, E] (per-segment), video_mask [n, Tn] int64 (element
 * strides) - forms S = exp(logit_scale) * normalise(text) . normalise(masked mean of per-frame-normalised visual)^T,
 * loss3 = (CrossEn(S), CrossEn(S^T), their mean) and, for an incoming gradient grad_scale of loss3[2], what torch.autograd
 * yields for it: d_text [n, E], d_visual [n, Tn, E], d_logit_scale [1].  fp32, fixed summation orders (deterministic).
 * The towers have no backward in this library (encoder backward and DDP all-reduce are out of scope):
 * this is the gradient a caller feeds into its own backward of the encoders.  E <= 1024. */
size_t cc_contrastive_grad_workspace_bytes(int32_t n, int32_t Tn, int32_t E);
int cc_contrastive_loss_grad_f32(const float* text, const float* visual, const int64_t* video_mask,
                                 int64_t mask_row_stride, int64_t mask_col_stride, int32_t n, int32_t Tn, int32_t E,
                                 float logit_scale, float grad_scale, float* loss3, float* d_text, float* d_visual,
                                 float* d_logit_scale, void* ws, size_t ws_bytes, void* stream);
/* the same with logit_scale read from device memory when logit_scale_dev != null (the nn.Parameter itself: a training step then
 * neither waits on the host for its value nor bakes it into a captured hipGraph) */
int cc_contrastive_loss_grad_dev_f32(const float* text, const float* visual, const int64_t* video_mask,
                                     int64_t mask_row_stride, int64_t mask_col_stride, int32_t n, int32_t Tn, int32_t E,
                                     float logit_scale, const float* logit_scale_dev, float grad_scale, float* loss3,
                                     float* d_text, float* d_visual, float* d_logit_scale, void* ws, size_t ws_bytes,
                                     void* stream);

/* camoe_dsl in training (CAMoE's dual-softmax loss; the reference keeps its line commented out at modules/clip4clip.py:430-432):
 * the chain above with D = n * S (.) softmax(S, dim=0) between the logits and the two CrossEn terms,
 * loss3 = (CrossEn(D), CrossEn(D^T), their mean), and the gradient carried through D back to the features and logit_scale:
 *   dS_ij = n P_ij (G_ij (1 + S_ij) - t_j),  P = softmax over the rows of each column of S,  G = dL/dD,  t_j = sum_k G_kj S_kj P_kj.
 * Same arguments, limits and determinism as cc_contrastive_loss_grad_f32 / _dev_f32; a workspace query of its own. */
size_t cc_contrastive_grad_dsl_workspace_bytes(int32_t n, int32_t Tn, int32_t E);
int cc_contrastive_loss_grad_dsl_f32(const float* text, const float* visual, const int64_t* video_mask,
                                     int64_t mask_row_stride, int64_t mask_col_stride, int32_t n, int32_t Tn, int32_t E,
                                     float logit_scale, float grad_scale, float* loss3, float* d_text, float* d_visual,
                                     float* d_logit_scale, void* ws, size_t ws_bytes, void* stream);
int cc_contrastive_loss_grad_dsl_dev_f32(const float* text, const float* visual, const int64_t* video_mask,
                                         int64_t mask_row_stride, int64_t mask_col_stride, int32_t n, int32_t Tn, int32_t E,
                                         float logit_scale, const float* logit_scale_dev, float grad_scale, float* loss3,
                                         float* d_text, float* d_visual, float* d_logit_scale, void* ws, size_t ws_bytes,
                                         void* stream);

/* camoe_dsl at evaluation: D = sim * softmax(sim, dim=0) * n_total on a [rows, cols] fp32 matrix (texts as rows, row stride in
 * elements, unit column stride), as three steps so that a row-sharded matrix can combine its blocks' statistics in between:
 *   cc_dsl_col_stats_f32      m[j] = max_i sim[i,j], s[j] = sum_i exp(sim[i,j] - m[j]) over the rows given.  rows == 0 is legal
 *                             (sim and ws may be null) and yields the neutral element (-inf, 0).  A column that holds a NaN gets
 *                             m = s = NaN, as torch.softmax would.  Fixed summation order (row slabs merged in slab order, no
 *                             atomics): the same bits on every run.  ws: cc_dsl_col_stats_workspace_bytes(rows, cols).
 *   cc_dsl_rescale_stats_f32  s[j] <- s[j] * exp(m_local[j] - m_global[j]), and 0 where s[j] == 0: a block's sums brought to the
 *                             maximum over all blocks (between an all-reduce MAX of m and an all-reduce SUM of s).
 *   cc_dsl_apply_f32          sim[i,j] <- n_total * sim[i,j] * exp(sim[i,j] - m[j]) / s[j], in place. */
size_t cc_dsl_col_stats_workspace_bytes(int32_t rows, int32_t cols);
int cc_dsl_col_stats_f32(const float* sim, int32_t rows, int32_t cols, int64_t row_stride, float* m, float* s, void* ws,
                         size_t ws_bytes, void* stream);
int cc_dsl_rescale_stats_f32(const float* m_local, const float* m_global, float* s, int32_t cols, void* stream);
int cc_dsl_apply_f32(float* sim, int32_t rows, int32_t cols, int64_t row_stride, const float* m, const float* s,
                     int32_t n_total, void* stream);

/* N1 - the rank extraction of compute_metrics (utils/metrics.py:11-26) on the device: for row i with
 * ground-truth column g = diag_offset + i, counts[2i] = #{j: sim[i,j] > sim[i,g]} and counts[2i+1] =
 * #{j: sim[i,j] == sim[i,g]} (>= 1).  The reference's rank list `ind` is the concatenation over rows of
 * range(counts[2i], counts[2i] + counts[2i+1]) - R@k / MdR / MnR follow from 2 ints per row instead of a
 * device->host copy and NumPy sort of the whole matrix.  Element (i,j) = sim[i*row_stride + j*col_stride]
 * (swap the strides to rank sim^T, i.e. video->text). */
int cc_rank_counts_f32(const float* sim, int32_t rows, int32_t cols, int64_t row_stride, int64_t col_stride,
                       int32_t diag_offset, int32_t* counts, void* stream);

/* The same with an explicit ground-truth column per row (gt_cols [rows] int32, device) - the multi-sentence
 * protocol of tensor_text_to_video_metrics (utils/metrics.py:38-65), where the sentences of one video share its
 * column.  counts3 [rows,3]: #greater, #equal (>= 1), #equal with a smaller column index (the position of the
 * ground truth among its ties under a stable descending sort; the reference's argsort leaves that order open). */
int cc_rank_counts_cols_f32(const float* sim, int32_t rows, int32_t cols, int64_t row_stride, int64_t col_stride,
                            const int32_t* gt_cols, int32_t* counts3, void* stream);

/* The same against a reference value handed in per row (ref_vals [rows] fp32, device): counts [rows,2] = #entries of the
 * row greater than / equal to ref_vals[i].  For the clip-sharded evaluation: a rank holds a ROW block
 * [Nt/G, Nv] of the matrix of main.py:502-534; the video->text rank of video v counts, over all text rows, the entries of
 * column v above the ground-truth entry, which lives in one rank's block - every rank counts its rows against the
 * broadcast ground-truth values (swap the strides to walk columns) and the per-rank counts are summed. */
int cc_rank_counts_ref_f32(const float* sim, int32_t rows, int32_t cols, int64_t row_stride, int64_t col_stride,
                           const float* ref_vals, int32_t* counts, void* stream);

/* tensor_video_to_text_sim (utils/metrics.py:68-76) on the device: out [n_groups, cols] = for every group g and column
 * (video) v the maximum of sim[r, v] over the rows (sentences) r with group[r] == g, NaN entries ignored, -inf where a
 * group has no row here (a rank's row block of the clip-sharded evaluation: the per-rank results are combined with a MAX
 * all-reduce).  group [rows] int32 in [0, n_groups); rows = 0 only fills out with -inf. */
int cc_group_max_rows_f32(const float* sim, int32_t rows, int32_t cols, int64_t row_stride, const int32_t* group,
                          int32_t n_groups, float* out, void* stream);

/* ==========================================================================================
 * N4, first slice of training: the backward of one ResidualAttentionBlock (modules/clip.py:228-253; the reference gets
 * it from torch.autograd in main.py:321).  The dgrad / wgrad contractions run on cc_linear_f16 with swapped operand roles
 * (centerclip_amd/train.py); these entry points are the pieces that are not a GEMM.  fp32 arithmetic, fixed summation
 * orders (identical bits on every run).
 *   cc_layernorm_backward_f32   x [rows, W] (row stride x_stride), dy [rows, W] -> dx [rows, W] = dres (optional, the
 *                               residual branch's gradient) + LayerNorm backward; dgamma, dbeta [W] (both NULL: a frozen
 *                               LayerNorm - the second launch, which reduces the per-workgroup partial sums to dgamma /
 *                               dbeta, is skipped; the first still leaves those partials in ws).  W % 4 == 0, W <= 1024,
 *                               x_stride >= W, x_stride % 4 == 0.
 *   cc_quick_gelu_backward_f16  du_pre = du * d/dx [x sigmoid(1.702 x)] at x = u_pre (fp16, the c_fc output before the
 *                               activation, clip.py:192-194); n % 4 == 0
 *   cc_gelu_f16 / cc_gelu_backward_f16   the same pair for the exact GELU x Phi(x) (CC_ACT_GELU): Phi(x) = erfc(-x / sqrt 2) / 2,
 *                               d/dx = Phi(x) + x exp(-x^2 / 2) / sqrt(2 pi)
 *   cc_attention_backward_f16   qkv [nseq*L, 3W] fp16 (as cc_attention_f16), d_out [nseq*L, W] fp32 -> d_qkv [nseq*L, 3W] fp32
 *                               (softmax(q k^T / 8 + mask) v per 64-wide head); fp16 MFMA operands (dO and dS scaled by
 *                               powers of two chosen on the device), fp32 accumulators.  L <= 64: one launch, a workgroup
 *                               per (sequence, head).  64 < L <= 256 (ViT-B/16): a query-side launch (dQ; log-sum-exp and
 *                               D = sum_j P dP per query into ws) and a key-side launch (dV, dK);
 *                               256 < L <= 320 (ViT-L/14 at 224 px: 257) the same pair with a fifth 64-key tile on the query
 *                               side; L > 320: CC_ERR_UNSUPPORTED
 *   cc_column_sums_f32          out [cols] = column sums of in [rows, cols] (bias gradients)
 *   cc_cast_scaled_f16          fp32 -> fp16 with a power-of-two scale chosen on the device from the tensor's largest
 *                               magnitude (scale * max in [8192, 16384], scale <= 2^126: maxima below 2^-112 get 2^126);
 *                               *scale_out (device) receives it; amax_scratch: one device float.  cc_unscale_f32 divides an
 *                               fp32 product by one or two such scales.
 * ========================================================================================== */
size_t cc_layernorm_backward_workspace_bytes(int32_t rows, int32_t W);
/* (dx_amax / out_amax below, may be null: one device float that holds 0 - or an earlier maximum - on entry and max(it, the
 *  largest magnitude written) on exit, so that cc_cast_transpose_f16(scaled = 2) can scale that tensor without reading it
 *  first; one atomic per workgroup of the producing kernel) */
int cc_layernorm_backward_f32(const float* x, int64_t x_stride, const float* gamma, const float* dy, const float* dres,
                              float* dx, float* dgamma, float* dbeta, int32_t rows, int32_t W, float eps, float* dx_amax,
                              void* ws, size_t ws_bytes, void* stream);
int cc_quick_gelu_f16(const void* in_f16, void* out_f16, int64_t n, void* stream);     /* QuickGELU on fp16 (training forward) */
int cc_quick_gelu_backward_f16(const void* u_pre_f16, const float* du, float* du_pre, int64_t n, float* out_amax, void* stream);
int cc_gelu_f16(const void* in_f16, void* out_f16, int64_t n, void* stream);           /* exact GELU on fp16 (training forward) */
int cc_gelu_backward_f16(const void* u_pre_f16, const float* du, float* du_pre, int64_t n, float* out_amax, void* stream);
size_t cc_attention_backward_workspace_bytes(int32_t nseq, int32_t L, int32_t heads);    /* 0 for L <= 64 (ws may be null) */
int cc_attention_backward_f16(const void* qkv_f16, const float* d_out, float* d_qkv, int32_t nseq, int32_t L,
                              int32_t heads, int32_t W, int32_t causal, float* out_amax, void* ws, size_t ws_bytes,
                              void* stream);
size_t cc_column_sums_workspace_bytes(int32_t rows, int32_t cols);
int cc_column_sums_f32(const float* in, int32_t rows, int32_t cols, float* out, void* ws, size_t ws_bytes, void* stream);
int cc_cast_scaled_f16(const float* in, void* out_f16, int64_t n, float* amax_scratch, float* scale_out, void* stream);
int cc_unscale_f32(float* x, int64_t n, const float* scale_a, const float* scale_b, void* stream);
/* c [M, N] fp32 = (a [M, K] w [N, K]^T) / *scale_dev: cc_linear_f16's "f32" form with the unscale above folded into the
 * epilogue (the dgrad / wgrad products of an operand cast by cc_cast_scaled_f16 / cc_cast_transpose_f16; the division by a
 * power of two is exact, so the result equals cc_linear_f16 followed by cc_unscale_f32 bit for bit). */
int cc_linear_unscaled_f16(const void* a_f16, const void* w_f16, float* c, int32_t M, int32_t N, int32_t K,
                           const float* scale_dev, void* stream);
/* The fp16 operand copies a Linear's backward multiplies, from ONE read of the matrix: `in` fp32 [rows, cols] (or in_f16, a
 * saved fp16 activation) -> out_f16 [rows, cols] (may be null) and out_t_f16 [cols, rows_pad] (may be null) = the transpose with zero columns
 * behind `rows` (rows_pad >= rows, a multiple of 64: the contraction of dW = dY^T X; cols % 4 == 0).  scaled != 0: the fp32
 * input is scaled by cc_cast_scaled_f16's device-chosen power of two (amax_scratch: one device float, *scale_out the scale);
 * scaled == 2: *amax_scratch already holds the tensor's largest magnitude (written by the kernel that produced the tensor,
 * see dx_amax / out_amax above) and the pass that finds it is skipped.
 * col_sums (may be null; fp32 input only): the column sums of the unscaled matrix [cols] from the same read - the Linear's bias
 * gradient - via per-tile partials in ws (cc_cast_transpose_colsum_workspace_bytes), added in tile order.  col_sums null with a
 * ws of that size: the partials [rows_pad / 64][cols] are left in ws and nothing is added (cc_wgrad_tn_f16 adds them). */
size_t cc_cast_transpose_colsum_workspace_bytes(int32_t rows_pad, int32_t cols);
int cc_cast_transpose_f16(const float* in, const void* in_f16, void* out_f16, void* out_t_f16, int32_t rows, int32_t cols,
                          int32_t rows_pad, int32_t scaled, float* amax_scratch, float* scale_out, float* col_sums, void* ws,
                          size_t ws_bytes, void* stream);

/* Weight gradient of a Linear layer from the row-major matrices the backward holds - no transposed copies (round 5):
 *   dw [N1, N2] fp32 = (dy^T x) / *scale_dev,   dy [M, N1], x [M, N2] fp16 row-major, the contraction over their rows
 * (main.py:321: torch.autograd's dW = dY^T X of y = x W^T).  N1 % 128 == 0, N2 % 128 == 0.  The row range is cut into slices so
 * that the grid fills the chip; the slices' partial products are added in slice order (bit-stable from run to run).
 * scale_dev (may be null: 1): the power of two dy was multiplied by (cc_cast_transpose_f16 / cc_cast_scaled_f16).
 * col_partial / col_chunks / bias_grad (all or none): the per-tile partial column sums [col_chunks][N1] cc_cast_transpose_f16
 * leaves in its ws when called without col_sums (col_chunks = rows_pad / 64) -> bias_grad [N1], added in the association of
 * cc_cast_transpose_f16's own reduction (same bits), in the launch that adds the slices.
 * ws: cc_wgrad_tn_workspace_bytes(M, N1, N2). */
size_t cc_wgrad_tn_workspace_bytes(int32_t M, int32_t N1, int32_t N2);
int cc_wgrad_tn_f16(const void* dy_f16, const void* x_f16, float* dw, int32_t M, int32_t N1, int32_t N2,
                    const float* scale_dev, const float* col_partial, int32_t col_chunks, float* bias_grad, void* ws,
                    size_t ws_bytes, void* stream);
/* BertAdam (utils/optimization.py:100-170: the optimizer main.py:161-167 builds), multi-tensor.  csrc/bertadam.hip.
 * Per tensor: grad is clipped in place to max_grad_norm (clip_grad_norm_ on the single tensor; <= 0: no clipping),
 * next_m = b1 m + (1-b1) g, next_v = b2 v + (1-b2) g^2, param -= lr * (next_m / (sqrt(next_v) + e) + weight_decay * param); no
 * bias correction.  lr = lr_scheduled = lr * schedule(step / t_total, warmup) is host arithmetic (centerclip_amd.train.BertAdam):
 * the record's `lr`, or - lr_dev != null - read from that device float (a training step captured into a hipGraph is replayed
 * with the schedule's new value written there first).  All tensors fp32.
 *
 * One table of `count` records in device memory drives TWO launches for all tensors: every tensor's norm workgroups (fp64
 * partial sums of squares into ws), then every tensor's step workgroups, each finding its tensor by bisection.  Records are
 * ordered, norm_blk0 / step_blk0 = the running sums of norm_blocks / step_blocks = cc_bertadam_norm_blocks(n) /
 * cc_bertadam_step_blocks(n) (host-side queries), total_* their sums, ws >= total_norm_blocks doubles.  A tensor of
 * n <= CC_BERTADAM_MULTI_MAX_N elements (biases, LayerNorm weights) has norm_blocks == 0 and step_blocks == 1: its one workgroup
 * forms the sum of squares itself.  The norm launch is skipped when max_grad_norm <= 0 or total_norm_blocks == 0 (ws may then
 * be null).  A tensor's bits do not depend on what else the table holds.  The records hold device pointers: the caller keeps
 * them valid until the launches have run (centerclip_amd.train.BertAdam stages them through pinned memory). */
#define CC_BERTADAM_MULTI_MAX_N 8192
typedef struct cc_bertadam_item {
    float* param; float* grad; float* next_m; float* next_v;
    const float* lr_dev;
    int64_t n;
    float lr, weight_decay;
    int32_t norm_blk0, norm_blocks, step_blk0, step_blocks;
} cc_bertadam_item;                                            /* 72 bytes */
int32_t cc_bertadam_norm_blocks(int64_t n);
int32_t cc_bertadam_step_blocks(int64_t n);
int cc_bertadam_multi_f32(const void* items_dev, int32_t count, int32_t total_norm_blocks, int32_t total_step_blocks, float b1,
                          float b2, float e, float max_grad_norm, void* ws, size_t ws_bytes, void* stream);
/* The same under a device-side loss scale (see "Loss scaling on the device" below): the gradients still carry the scale; every
 * gradient is multiplied by *mult_dev as it is loaded (and that value is what is written back), so the result is bit for bit
 * the plain entry point on gradients multiplied by *mult_dev first - for a power-of-two scale, on the gradients divided by it.
 * *found_inf_dev != 0: the launches write nothing - parameters, moments and gradients keep their bits (GradScaler.step skipping
 * optimizer.step()).  Both words are device floats that cc_grad_scaler_stats_f32 wrote. */
int cc_bertadam_multi_scaled_f32(const void* items_dev, int32_t count, int32_t total_norm_blocks, int32_t total_step_blocks,
                                 float b1, float b2, float e, float max_grad_norm, void* ws, size_t ws_bytes,
                                 const float* mult_dev, const float* found_inf_dev, void* stream);

/* ==========================================================================================
 * AdamW (torch.optim.AdamW, the optimizer main.py:168-175 builds for --optim AdamW) and global gradient clipping
 * (torch.nn.utils.clip_grad_norm_, main.py:316-333), multi-tensor.  csrc/adamw.hip.
 *
 * One table of `count` cc_adamw_item records in device memory drives every entry point below.  Records are ordered, blk0 is
 * the running sum of blocks = cc_adamw_blocks(n), total_blocks = the sum of all blocks; each workgroup finds its tensor by
 * bisection over blk0.  The records hold device pointers: the caller keeps them valid until the launches have run
 * (centerclip_amd.train stages the table through pinned memory).  All tensors fp32; float4 access where all of a record's
 * pointers are 16-byte aligned, a scalar tail for n % 4 != 0 (and for unaligned views).
 *
 * Arithmetic (per element, compiled WITHOUT fp contraction: every operation rounds on its own, in this order):
 *     g *= coef (only with coef_dev; the clipped g is written back)
 *     p = p * decay
 *     m = m + omb1 * (g - m)   (omb1 >= 0.5: g - (g - m) * (1 - omb1)) - torch's lerp_(g, 1 - b1), i.e. b1 m + (1 - b1) g
 *     v = b2 * v + (omb2 * g) * g
 *     p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps))
 * with the per-class scalars (cc_adamw_scalars, index scalar_index) computed on the host in double and rounded to float:
 * decay = 1 - lr wd, omb1 = 1 - b1, omb2 = 1 - b2, step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t), t = the step
 * count after this step.  The elements are independent, so a launch over many tensors gives the bits of one launch per tensor.
 * ========================================================================================== */
typedef struct cc_adamw_item {
    float* param; float* grad; float* exp_avg; float* exp_avg_sq;
    int64_t n;
    int32_t blk0, blocks;
    int32_t scalar_index;                                      /* into the scalars_dev array */
    int32_t reserved;
} cc_adamw_item;                                               /* 56 bytes */
typedef struct cc_adamw_scalars {
    float decay, beta1, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps;
} cc_adamw_scalars;                                            /* 32 bytes */
int32_t cc_adamw_blocks(int64_t n);
/* One AdamW step of every record.  coef_dev (may be null): a device float the gradients are multiplied by first (the clip
 * coefficient of cc_grad_clip_coef_f32) - bit for bit cc_grad_scale_f32 followed by the step without it. */
int cc_adamw_multi_f32(const void* items_dev, int32_t count, int32_t total_blocks, const void* scalars_dev, const float* coef_dev,
                       void* stream);
/* Global L2 norm of the records' gradients: cc_grad_norm_partials_f32 writes one fp64 sum of squares per workgroup into ws
 * (>= cc_grad_norm_workspace_bytes(total_blocks)); cc_grad_clip_coef_f32 adds them in a fixed order (no atomics: the same bits
 * on every run) and writes norm_coef[0] = ||g|| and norm_coef[1] = min(1, max_norm / (||g|| + 1e-6)) in fp32.  No host
 * synchronisation: both can be captured into a hipGraph. */
size_t cc_grad_norm_workspace_bytes(int32_t total_blocks);
int cc_grad_norm_partials_f32(const void* items_dev, int32_t count, int32_t total_blocks, void* ws, size_t ws_bytes, void* stream);
int cc_grad_clip_coef_f32(const void* ws, int32_t total_blocks, float max_norm, float* norm_coef, void* stream);
/* g *= *coef_dev for every record's gradient (the in-place scaling of clip_grad_norm_). */
int cc_grad_scale_f32(const void* items_dev, int32_t count, int32_t total_blocks, const float* coef_dev, void* stream);

/* Loss scaling on the device (torch.amp.GradScaler's recipe, main.py:320-328, without a host decision: capturable).
 * The gradients carry the loss scale S; nothing ever unscales them in a pass of its own.
 *   cc_grad_scaler_stats_f32   the successor of cc_grad_clip_coef_f32 (one workgroup, the same fixed order over the partial
 *       sums of cc_grad_norm_partials_f32): out3[0] = ||g / S||, out3[1] = the multiplier inv_scale * min(1, max_norm /
 *       (||g / S|| + 1e-6)) (max_norm < 0: no clipping, the multiplier is inv_scale), out3[2] = found_inf (1.f when a gradient
 *       element is inf or NaN - the fp64 sum of squares of fp32 values is non-finite exactly then - else 0.f).  For a
 *       power-of-two S, out3[0] and the clip coefficient are bit for bit what cc_grad_clip_coef_f32 gives on g / S.
 *   cc_adamw_multi_scaled_f32  cc_adamw_multi_f32 with the multiplier as its coef_dev and the flag: *found_inf_dev != 0 ->
 *       the launch writes nothing; otherwise bit for bit cc_adamw_multi_f32(coef_dev = mult_dev).
 *   cc_grad_scaler_update_f32  GradScaler.update on one lane.  scale2 = {scale, 1 / scale}; counters3 = {growth tracker,
 *       steps taken, steps skipped}.  found_inf: scale *= backoff, tracker = 0, skipped += 1; else taken += 1, tracker += 1
 *       and at tracker == growth_interval: scale *= growth (kept if that is not finite), tracker = 0.  scale2[1] is renewed. */
int cc_grad_scaler_stats_f32(const void* ws, int32_t total_blocks, const float* inv_scale_dev, float max_norm, float* out3,
                             void* stream);
int cc_adamw_multi_scaled_f32(const void* items_dev, int32_t count, int32_t total_blocks, const void* scalars_dev,
                              const float* mult_dev, const float* found_inf_dev, void* stream);
int cc_grad_scaler_update_f32(float* scale2, const float* found_inf_dev, int32_t* counters3, float growth_factor,
                              float backoff_factor, int32_t growth_interval, void* stream);

/* ==========================================================================================
 * sim_header 'seqTransf' (modules/clip4clip.py:335-349, the loose_type head the reference runs besides meanP).
 *   visual_output [B, T, D] fp32 (per-segment features before pooling), video_mask [B, T] int64 read at
 *   mask + b * mask_row_stride + t * mask_col_stride (elements; the strided segment mask needs no copy)
 *   -> x = visual_output + frame_position_embeddings[0:T]; x = transformerClip(x, key mask); out = x + visual_output.
 * The blocks are module_cross.ResidualAttentionBlock (module_cross.py:88-112): CLIP's block with the additive attention
 * mask (1 - video_mask[b, j]) * -1e6 on KEY j, the same for every query and head.
 *   cc_key_masked_attention_f16   qkv [nseq*L, 3W] fp16 (as cc_attention_f16), out [nseq*L, W] fp16; mask [nseq, L]
 *                                 (strided).  Keys with mask 0 get weight exactly 0 and their k / v rows are never read; a
 *                                 sequence whose keys are ALL masked gets the unmasked softmax (the exact value of the formula,
 *                                 where every score moves by the same -1e6).  fp32 arithmetic, W = 64 * heads, L <= 80.
 *   cc_key_masked_attention_backward_f16   cc_attention_backward_f16's conventions: d_out [nseq*L, W] fp32 -> d_qkv
 *                                 [nseq*L, 3W] fp32, out_amax (may be null) as there.  The dk / dv rows of masked keys are
 *                                 exactly 0.
 *   cc_seqtransf_forward_f32      the whole head in one enqueue (position rows, `layers` blocks on the LayerNorm / GEMM kernels
 *                                 of the encoders with the new attention, the outer residual): feat, out [B, T, D] fp32
 *                                 contiguous (out may alias feat), pos [>= T, D] fp32, blocks[l] (the fields up to c_proj_bias;
 *                                 LayerNorm eps 1e-5), D = 64 * heads <= 1024, D % 64 == 0, T <= 80.  ws >=
 *                                 cc_seqtransf_workspace_bytes(B, T, D).  No host synchronisation (graph-capturable).
 * ========================================================================================== */
int cc_key_masked_attention_f16(const void* qkv_f16, void* out_f16, int32_t nseq, int32_t L, int32_t heads, int32_t W,
                                const int64_t* mask, int64_t mask_row_stride, int64_t mask_col_stride, void* stream);
int cc_key_masked_attention_backward_f16(const void* qkv_f16, const int64_t* mask, int64_t mask_row_stride,
                                         int64_t mask_col_stride, const float* d_out, float* d_qkv, int32_t nseq, int32_t L,
                                         int32_t heads, int32_t W, float* out_amax, void* stream);
size_t cc_seqtransf_workspace_bytes(int32_t B, int32_t T, int32_t D);
int cc_seqtransf_forward_f32(const float* feat, const int64_t* mask, int64_t mask_row_stride, int64_t mask_col_stride,
                             const float* pos, const cc_block_weights* blocks, int32_t layers, int32_t B, int32_t T, int32_t D,
                             int32_t heads, float* out, void* ws, size_t ws_bytes, void* stream);

/* ==========================================================================================
 * Diagnostics (not on the product path; process-wide state, not thread-safe).
 * While armed, every launch of the tiled GEMM kernel is issued with a start / stop event pair that receives the dispatch's
 * own begin / end timestamps (what rocprofv3 --kernel-trace reads), so a kernel symbol can be timed IN SITU, inside an
 * eagerly enqueued step between its real neighbours.  bench.py's `roofline` uses it.  Never arm during graph capture.
 *   cc_debug_gemm_timing_begin(cap)  arm for up to `cap` launches (earlier records are dropped); cap <= 0 disarms + frees
 *   cc_debug_gemm_timing_end()       disarm; -> number of launches recorded
 *   cc_debug_gemm_timing_read(i, us_out, info12_out)   (after synchronising the stream) duration of launch i in
 *        microseconds + its record: BM, BN, WM, WN, epilogue id, BK | split << 16, then M, N, K of the carrier and of the
 *        rider problem (zeros without a rider).
 * The per-workgroup stamp hooks (cc_debug_set_*_profile) exist only in development builds (-DCC_DEV_KNOBS).
 * ========================================================================================== */
int cc_debug_gemm_timing_begin(int cap);
int cc_debug_gemm_timing_end(void);
int cc_debug_gemm_timing_read(int i, float* us_out, int* info12_out);

#ifdef __cplusplus
}
#endif
#endif /* CENTERCLIP_HIP_H */
