/*
 * kvpress_hip.h -- C ABI of libkvpress_hip.so: the MI355X (gfx950) implementation of the
 * kvpress per-layer KV score -> top-k -> gather hot path.
 *
 * The reference (NVIDIA/kvpress v0.5.4) is pure Python and has no FFI; its boundary for this
 * path is the Python protocol BasePress.forward_hook -> ScorerPress.compress -> score()
 * (kvpress/presses/base_press.py:101-162, scorer_press.py:76-102).  This header is what a
 * binding of that path binds: every entry point names the reference lines it replaces.
 * kvpress_amd/_native.py is the ctypes binding; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only (no torch / framework types);
 *   - all pointers are DEVICE pointers on the current HIP device unless stated otherwise;
 *   - 4-D tensors are [B, H, S, D] views with the last dim contiguous; strides are in ELEMENTS
 *     (sb, sh, ss) so sliced cache views (keys[:, :, n_sink:], chunk slices) need no copy;
 *   - outputs and workspaces are caller-allocated; *_workspace_bytes() gives the size;
 *   - every call is asynchronous on `stream` (a hipStream_t), allocates no device memory, never
 *     synchronises (kvp_leverage_status and kvp_threshold_count excepted) and is thread-safe;
 *   - process-wide state, created on first use and kept until exit: one host-pinned status word
 *     (kvp_async_error_check below) and, per device, a stream guard that orders the one-launch
 *     select of long rows ("one cluster select per device" at kvp_topk_select);
 *   - return 0 (KVP_OK) or a negative KVP_E* code; kvp_last_error() returns the calling
 *     thread's last message.
 *   - scores are always float32 (the reference returns the model dtype; float32 is a superset
 *     and makes the top-k well defined -- DESIGN.md "Parity contract").
 */
#ifndef KVPRESS_HIP_H
#define KVPRESS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KVP_VERSION 100 /* 0.1.0 */

typedef void* kvp_stream_t; /* hipStream_t */

enum kvp_dtype { KVP_F32 = 0, KVP_F16 = 1, KVP_BF16 = 2 };
enum kvp_status { KVP_OK = 0, KVP_EINVAL = -1, KVP_EUNSUPPORTED = -2, KVP_EWORKSPACE = -3, KVP_EHIP = -4, KVP_EASYNC = -5,
                  KVP_ENUMERIC = -6 /* kvp_leverage_status: the Cholesky factorisation failed */ };
/* Order of the retained indices.  POSITION: ascending token position (default; makes the gather a
 * monotone stream).  SCORE: descending score, ties by ascending position -- the element order
 * torch.topk(sorted=True) produces at scorer_press.py:95, for tensor-exact comparisons. */
enum kvp_order { KVP_ORDER_POSITION = 0, KVP_ORDER_SCORE = 1 };
/* OR-ed into `order`: the workspace was zero-filled once (its first kvp_topk_workspace_bytes() bytes) and has
 * only been used by kvp_topk_select on ONE stream since.  The call then skips its memset: the histograms in
 * the workspace are self-cleaning (left zero on completion). */
#define KVP_TOPK_WS_CLEAN 0x100
/* OR-ed into `order`: select the k SMALLEST scores instead of the k largest (ties still go to the lowest position);
 * AdaKVPress's bottom-k across heads (kvpress/presses/adakv_press.py:66-67) without negating the scores. */
#define KVP_TOPK_SMALLEST 0x200

int kvp_version(void);
const char* kvp_last_error(void);
/* Failures a kernel can only detect while it RUNS.  The one-launch select of long rows (kvp_topk_select and the fused
 * kvp_*_compress entry points on rows of 16385 .. 262144 scores) synchronises the 32 workgroups of a row with in-kernel barriers;
 * if they never become co-resident (CU masking, a partitioned device) its bounded spin gives up.  torch.topk
 * (kvpress/presses/scorer_press.py:95) cannot return wrong indices silently, so neither does this library: the affected rows'
 * indices are written as -1 (kvp_gather_kv* turn a negative index into a row of all-ones bit patterns = NaN instead of reading
 * anywhere), a process-wide host-pinned status word is set, and the NEXT call of kvp_topk_select*, kvp_*_compress*, kvp_gather_kv*
 * or kvp_async_error_check on any thread returns KVP_EASYNC (once per report; kvp_last_error() has the text).  After KVP_EASYNC
 * every workspace that was being used with KVP_TOPK_WS_CLEAN must be zero-filled again.  kvp_async_error_check() only polls the
 * word (no synchronisation): call it after a stream sync to learn about everything enqueued before. */
int kvp_async_error_check(void);

/* ---- KnormPress.score: -keys.norm(dim=-1)  (kvpress/presses/knorm_press.py:38) -------------
 * out[b,h,s] = scale * ||x[b,h,s,:]||_2   (scale = -1 for Knorm; +1 for ||V|| in ExpectedAttention,
 * expected_attention_press.py:160).  out is contiguous [B,H,S] float32. */
int kvp_rownorm_score(const void* x, int dtype, int64_t B, int64_t H, int64_t S, int64_t D,
                      int64_t sb, int64_t sh, int64_t ss, float scale, float* out, kvp_stream_t stream);

/* ---- QFilterPress.score: -(q_filter * keys).sum(dim=-1)  (kvpress/presses/qfilter_press.py:79-82) ----------------
 * out[b,h,s] = scale * sum_d x[b,h,s,d] * filt[h,d]   (scale = -1; filt = the layer's [H,D] slice of the learned
 * Q-filters, same dtype as x, f_sh = element stride between heads, rows contiguous).  out contiguous [B,H,S] float32. */
int kvp_rowdot_score(const void* x, int dtype, int64_t B, int64_t H, int64_t S, int64_t D,
                     int64_t sb, int64_t sh, int64_t ss, const void* filt, int64_t f_sh, float scale, float* out,
                     kvp_stream_t stream);

/* ---- SnapKVPress.score (kvpress/presses/snapkv_press.py:60-105) ----------------------------
 * q: RoPE'd queries of the last W tokens [B,Hq,W,D] (the host keeps q_proj + RoPE,
 *    snapkv_press.py:53-58 / utils.py:43-46: q_proj is a model-owned nn.Linear);
 * k: keys [B,Hkv,S,D].  Computes softmax(q k^T / sqrt(D)) over all S keys with the causal mask
 * on the last W columns (:62-66), mean over the W rows (:95), avg_pool1d(kernel_size,
 * pad=kernel_size/2, stride 1, zero padded, divisor kernel_size) (:96), mean over the
 * Hq/Hkv group (:99-100), and fills the last W positions with max(scores)+1, max global over
 * B and Hkv (:103) -- on the device, no host sync.  scores: [B,Hkv,S] float32, contiguous.
 * kernel_size must be odd.  Requires S > W. */
size_t kvp_snapkv_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D);
int kvp_snapkv_score(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sw,
                     const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype,
                     int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D, int kernel_size,
                     float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* Same, with the RoPE of the window queries (snapkv_press.py:56-58) done inside the library:
 * q is the PRE-RoPE q_proj output viewed [B,Hq,W,D]; cos/sin are the last W rows of the layer's
 * position embeddings, [Bc,W,D] with Bc = B or 1 (cs_sb = 0 broadcasts), same dtype as q.
 * q_rot = q*cos + rotate_half(q)*sin is evaluated exactly as the reference's torch ops do in the
 * model dtype (every product and the sum rounded to that dtype), so q_rot is bit-identical. */
int kvp_snapkv_score_rope(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sw,
                          const void* cos, const void* sin, int64_t cs_sb, int64_t cs_sw,
                          const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype,
                          int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D, int kernel_size,
                          float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* FINCH scores (kvpress/presses/finch_press.py:56-83): the window attention of kvp_snapkv_score_rope for a window of ANY
 * length W (the question that follows the context), no pooling; with normalize_scores != 0 window row w is weighted by its
 * number of visible keys S - W + w before the mean over the window (:71-74).  Window columns = max + 1 (:82).
 * Arguments and workspace (kvp_snapkv_workspace_bytes) as kvp_snapkv_score_rope. */
int kvp_finch_score(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sw,
                    const void* cos, const void* sin, int64_t cs_sb, int64_t cs_sw,
                    const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype,
                    int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D, int normalize_scores,
                    float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* Same, when the attention layer returned its weights (snapkv_press.py:88-89):
 * attn is the [B,Hq,W,S-W] view attentions[..., -W:, :-W] (last dim contiguous). */
int kvp_snapkv_score_from_attn(const void* attn, int64_t a_sb, int64_t a_sh, int64_t a_sw, int dtype,
                               int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int kernel_size,
                               float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- ExpectedAttentionPress.get_query_statistics (kvpress/presses/expected_attention_press.py:62-86) ----
 * kvp_ea_qstats: mean and covariance of the pre-RoPE queries q [B,Hq,Sq,D] (sinks already
 * stripped by the host, :70-71): mu[b,h,:] = mean_s q; cov = (q-mu)^T (q-mu) / Sq (:74-80).
 * mu [B,Hq,D], cov [B,Hq,D,D] float32 contiguous; cov may be NULL (use_covariance=False).
 * The averaged-RoPE step (:110-123) is 128x128 host-side math on mu/cov and stays in the host. */
size_t kvp_ea_qstats_workspace_bytes(int64_t B, int64_t Hq, int64_t Sq, int64_t D);
int kvp_ea_qstats(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, int dtype,
                  int64_t B, int64_t Hq, int64_t Sq, int64_t D,
                  float* mu, float* cov, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- ExpectedAttentionPress.score (kvpress/presses/expected_attention_press.py:126-165) ----
 * kvp_ea_score (:137-163): with the post-RoPE mu [B,Hq,D] / cov [B,Hq,D,D] (float32, cov may be
 * NULL): for keys/values [B,Hkv,S,D] drop the first n_sink positions; logits = k.mu/sqrt(D) +
 * k^T cov k / (2D) per q-head; softmax over the S-n_sink keys; mean over the group;
 * (s + epsilon) * ||v||_2 if use_vnorm; positions < n_sink get max(scores)+1 (global max).
 * scores [B,Hkv,S] float32. */
size_t kvp_ea_score_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D);
int kvp_ea_score(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                 const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, int dtype,
                 const float* mu, const float* cov,
                 int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D,
                 int64_t n_sink, int use_vnorm, float epsilon,
                 float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- ScorerPress.compress: top-k + gather (kvpress/presses/scorer_press.py:94-100) ----------
 * kvp_topk_select: for each of the R rows of scores[R, S] (row stride in elements) write the
 * indices of the k largest scores to idx[R, k] (int32).  torch.topk leaves ties unspecified;
 * here the LOWEST POSITION wins among equal scores, and -0.0 == +0.0.  0 <= k <= S.
 * One cluster select per device: rows of 16385 .. 262144 scores are selected by ONE launch whose workgroups wait for each other
 * (kvp_async_error_check above), so only one such launch may be in flight on a device.  Within a process the library sees to that
 * itself (the per-device stream guard makes a call on another stream wait for the previous one).  Processes that SHARE a GPU must
 * set KVP_TK_CLUSTER=0 in their environment, which takes the multi-launch select instead; otherwise two of them can hold the CUs
 * each other's rows wait for, and the bounded spin ends in KVP_EASYNC. */
size_t kvp_topk_workspace_bytes(int64_t R, int64_t S, int64_t k);
/* workspace for order == KVP_ORDER_SCORE (the select's + the sort's); KVP_ORDER_POSITION needs only the one above */
size_t kvp_topk_order_workspace_bytes(int64_t R, int64_t S, int64_t k);
int kvp_topk_select(const float* scores, int64_t R, int64_t S, int64_t row_stride, int64_t k, int order,
                    int32_t* idx, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* kvp_gather_kv: k_out[b,h,j,:] = k[b,h,idx[b*H+h, j],:], same for v (scorer_press.py:96-100).
 * Outputs are contiguous [B,H,n,D] in the input dtype; inputs are not modified.  When K + V exceed the memory-side cache
 * (cutoff 192 MiB; the cache itself is 256 MiB) the rows are moved with non-temporal loads / stores: the copy then neither displaces what the next kernels
 * re-read nor leaves its output behind as dirty cache lines. */
int kvp_gather_kv(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                  const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, int dtype,
                  int64_t B, int64_t H, int64_t S, int64_t D,
                  const int32_t* idx, int64_t n, void* k_out, void* v_out, kvp_stream_t stream);

/* scores[r, idx[r, j]] = value for every j < n (AdaKVPress's safeguard `scores.scatter_(-1, top_indices, finfo.max)`,
 * kvpress/presses/adakv_press.py:62-63); idx int32 [R, n] contiguous, scores rows row_stride elements apart. */
int kvp_scores_fill_at(float* scores, int64_t R, int64_t S, int64_t row_stride, const int32_t* idx, int64_t n, float value,
                       kvp_stream_t stream);

/* ---- ChunkPress: per-chunk top-k (kvpress/presses/chunk_press.py:67-85) ---------------------------------------------
 * scores[R, nseg * seg_len] contiguous; the k largest of EACH chunk of seg_len columns are selected (same tie rule as
 * kvp_topk_select); idx[R, nseg * k] holds them chunk after chunk as row positions + pos_base, i.e. ascending overall. */
size_t kvp_topk_segmented_workspace_bytes(int64_t R, int64_t nseg, int64_t seg_len, int64_t k);
int kvp_topk_select_segmented(const float* scores, int64_t R, int64_t nseg, int64_t seg_len, int64_t k, int64_t pos_base,
                              int order, int32_t* idx, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- KeyRerotationPress.rerotate_keys after the gather (kvpress/presses/key_rerotation_press.py:50-128) ------------
 * k: contiguous [B,H,n,D] keys gathered with idx[B*H, n] (ascending positions); in place
 * k[b,h,j] <- k * cos(f) + rotate_half(k) * sin(f),  f = (j - idx[b,h,j]) * inv_freq[d mod D/2]  (inv_freq: D/2 floats,
 * module.rotary_emb.inv_freq), cos/sin cast to the key dtype and every op rounded in it, as torch does. */
int kvp_rerotate_keys(void* k, int dtype, int64_t B, int64_t H, int64_t n, int64_t D, const int32_t* idx,
                      const float* inv_freq, kvp_stream_t stream);
/* The gather and the re-rotation above in one pass (key_rerotation_press.py:157-160 + :107-128; finch_press.py:111-119): same
 * arguments as kvp_gather_kv + inv_freq, same bits as kvp_gather_kv followed by kvp_rerotate_keys on k_out; the gathered keys are
 * written once instead of written, read and written again.  2-byte dtypes with D % 16 == 0 and 16-byte aligned rows take the
 * one-pass kernel, everything else runs the two kernels it replaces. */
int kvp_gather_kv_rerotate(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb, int64_t v_sh,
                           int64_t v_ss, int dtype, int64_t B, int64_t H, int64_t S, int64_t D, const int32_t* idx, int64_t n,
                           const float* inv_freq, void* k_out, void* v_out, kvp_stream_t stream);

/* ---- fused ScorerPress.compress (scorer_press.py:76-102 with the scorer inlined) ---------------------------------
 * One call = score -> select n_kept -> gather into caller-allocated contiguous k_out / v_out [B,H,n_kept,D].  Same
 * kernels and results as the modular sequence kvp_*_score + kvp_topk_select + kvp_gather_kv; the score-writing kernel
 * also accumulates the select's first histogram, and SnapKV's window columns are appended to the selection instead of
 * being scored with max + 1 (snapkv_press.py:103), which removes the global max and the pad fill.
 * flags: KVP_TOPK_WS_CLEAN if the first kvp_topk_workspace_bytes(R, S, n_kept) bytes of ws were zero-filled once and
 * the workspace has only been used by these calls on ONE stream since (they leave it clean), else 0;
 * | KVP_ORDER_SCORE: the rows of k_out / v_out in descending score order, ties by ascending position (SnapKV: the window tokens
 * first) -- the order in which the reference stores them (scorer_press.py:95-100); default: ascending position.
 * kvp_knorm_compress and the two kvp_snapkv_compress_* entries run the one-launch select on long rows: "one cluster select per
 * device" at kvp_topk_select holds for them too (KVP_TK_CLUSTER=0 when processes share a GPU). */
size_t kvp_knorm_compress_workspace_bytes(int64_t B, int64_t H, int64_t S, int64_t n_kept);
int kvp_knorm_compress(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                       const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, int dtype,
                       int64_t B, int64_t H, int64_t S, int64_t D, int64_t n_kept,
                       void* k_out, void* v_out, void* ws, size_t ws_bytes, int flags, kvp_stream_t stream);
size_t kvp_snapkv_compress_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D, int64_t n_kept);
/* arguments as kvp_snapkv_score_rope (pre-RoPE window queries + the window's cos/sin) plus V and the outputs */
int kvp_snapkv_compress_rope(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sw,
                             const void* cos, const void* sin, int64_t cs_sb, int64_t cs_sw,
                             const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                             const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, int dtype,
                             int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D, int kernel_size,
                             int64_t n_kept, void* k_out, void* v_out, void* ws, size_t ws_bytes, int flags,
                             kvp_stream_t stream);

/* ---- KeyDiffPress.score (kvpress/presses/keydiff_press.py:45-46) ----------------------------------
 * anchor[b,h,:] = mean_s k[b,h,s,:] / max(||k[b,h,s,:]||, 1e-12)   (F.normalize(keys).mean(dim=2))
 * scores[b,h,s] = -cosine_similarity(k[b,h,s,:], anchor[b,h,:])     (eps 1e-8), contiguous [B,H,S] float32. */
size_t kvp_keydiff_workspace_bytes(int64_t B, int64_t H, int64_t S, int64_t D);
int kvp_keydiff_score(const void* k, int dtype, int64_t B, int64_t H, int64_t S, int64_t D,
                      int64_t sb, int64_t sh, int64_t ss, float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- CURPress.score (kvpress/presses/cur_press.py:32-66) without the random projection ------------------------------
 * k2 = sum_d k^2, v2 = sum_d v^2; with local_window_size w > 0 each is divided by its sum over the windows of w consecutive
 * tokens (zero-padded tail); combined by leverage type; divided by the row sum; the first num_sinks positions are set to 1.
 * scores: contiguous [B,H,S] float32. */
enum kvp_cur_leverage { KVP_CUR_KEY = 0, KVP_CUR_VALUE = 1, KVP_CUR_KV_AVG = 2, KVP_CUR_KV_PRODUCT = 3 };
size_t kvp_cur_workspace_bytes(int64_t B, int64_t H, int64_t S);
int kvp_cur_score(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                  int dtype, int64_t B, int64_t H, int64_t S, int64_t D, int leverage_type, int64_t local_window_size,
                  int64_t num_sinks, float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- TOVAPress.score tail (kvpress/presses/tova_press.py:52-53) -----------------------------------
 * scores[b,h,s] <- mean over h' of scores[b,h',s] for every h, in place (`attn_weights.mean(1)` followed by
 * `.repeat(1, num_kv_heads, 1)`, applied to the per-kv-group means kvp_snapkv_score* produce with W = 1, kernel 1).
 * Strides in elements. */
int kvp_scores_head_mean(float* scores, int64_t B, int64_t H, int64_t S, int64_t stride_b, int64_t stride_h,
                         kvp_stream_t stream);

/* ---- window q_proj + RoPE in the library (kvpress/utils.py:43-46 + snapkv_press.py:53-58) ---------------------------
 * hidden_win: hidden_states[:, -W:] [B, W, hidden] (element strides x_sb, x_sw; last dim contiguous); wq: q_proj.weight
 * [Hq * D, hidden] contiguous, no bias; cos/sin: the window's rotary tables [1 or B, W, D].  bf16 / f16, W = 64, D = 128,
 * hidden % 256 == 0, else KVP_EUNSUPPORTED (the caller then runs its own q_proj and kvp_snapkv_*_rope).
 * kvp_snapkv_qproj_rope writes the RoPE'd window queries q_rot [B, Hq, W, D] (contiguous, input dtype): fp32 accumulation
 * in a fixed order, rounded to the dtype like a GEMM output, then rotated with torch's per-op rounding.
 * kvp_snapkv_score_hidden / kvp_snapkv_compress_hidden = kvp_snapkv_score_rope / kvp_snapkv_compress_rope from there
 * (kvp_snapkv_compress_hidden: one cluster select per device, as kvp_snapkv_compress_rope). */
int kvp_snapkv_qproj_rope(const void* hidden_win, int64_t x_sb, int64_t x_sw, const void* wq, const void* cos, const void* sin,
                          int64_t cs_sb, int64_t cs_sw, int dtype, int64_t B, int64_t Hq, int64_t W, int64_t D, int64_t hidden,
                          void* q_rot, kvp_stream_t stream);
int kvp_snapkv_score_hidden(const void* hidden_win, int64_t x_sb, int64_t x_sw, const void* wq, int64_t hidden,
                            const void* cos, const void* sin, int64_t cs_sb, int64_t cs_sw,
                            const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype,
                            int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D, int kernel_size,
                            float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);
int kvp_snapkv_compress_hidden(const void* hidden_win, int64_t x_sb, int64_t x_sw, const void* wq, int64_t hidden,
                               const void* cos, const void* sin, int64_t cs_sb, int64_t cs_sw,
                               const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                               const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, int dtype,
                               int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t W, int64_t D, int kernel_size,
                               int64_t n_kept, void* k_out, void* v_out, void* ws, size_t ws_bytes, int flags,
                               kvp_stream_t stream);

/* ---- NonCausalAttnPress.score (kvpress/presses/non_causal_attention_press.py:47-122) --------------------------------------------
 * q: PRE-RoPE queries [B,Hq,S,D]; cos/sin: the rotary tables of the same S positions [Bc,S,D] (cs_sb = 0 broadcasts), RoPE'd in the
 * library with torch's per-op rounding (:114); k: post-RoPE keys, v: values [B,Hkv,S,D], all in `dtype`, strides in elements.
 * Per chunk of `chunk` tokens (the last one zero-padded; padded keys get logit -1e-9 from every row, padded queries 0: :70-88):
 * logits = q k^T (NOT scaled, rounded to the dtype like the matmul output), float32 row softmax, sum over the chunk's queries (:89-93),
 * mean over the Hq/Hkv group (:118), times ||v|| (:120), avg_pool1d(3, pad 1) (:121), then the z-score over the WHOLE [B,Hkv,S] tensor
 * (mean, unbiased std clamped at 1e-6: :122).  raw (may be NULL): the scores before the z-score; scores: the z-scores; both
 * contiguous [B,Hkv,S] float32.  bf16 / f16 with D in {64,96,128,256}, chunk % 32 == 0, chunk <= 512, Hq/Hkv <= 16 and 16-byte aligned
 * key rows run on the matrix cores; everything else (float32, other shapes) on a generic kernel.  S >= 1;
 * B*Hkv*S = 1 gives a NaN z-score, as torch's std of one element does. */
size_t kvp_ncattn_workspace_bytes(int64_t B, int64_t Hkv, int64_t S);
int kvp_ncattn_score(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* cos, const void* sin, int64_t cs_sb,
                     int64_t cs_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb,
                     int64_t v_sh, int64_t v_ss, int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D,
                     int64_t chunk, float* raw, float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- LeverageScorePress.compute_leverage_scores + score (kvpress/presses/leverage_press.py:47-110) ---------------------------------
 * k: PRE-RoPE keys [B,H,S,D] (D <= 256); phi: the Gaussian sketch [B,H,D,sketch] the caller drew (:68-75; last dim contiguous, strides
 * p_sb, p_sh, p_sd in elements), same dtype as k.  x_s = phi^T (k_s - mean_s k) rounded to the dtype (:78-79), G = sum_s x_s x_s^T
 * symmetrised, L = cholesky(G + jitter I) with jitter 1e-2, x10, at most 5 tries (:47-56, :90; float64), raw_s = max(0, ||L^-1 x_s||^2)
 * (:95-109), then the global z-score of :110 (NaN for B*H*S = 1, as torch's std).  raw may be NULL.  1 <= sketch <= 256. */
size_t kvp_leverage_workspace_bytes(int64_t B, int64_t H, int64_t S, int64_t D, int64_t sketch);
int kvp_leverage_score(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* phi, int64_t p_sb, int64_t p_sh,
                       int64_t p_sd, int dtype, int64_t B, int64_t H, int64_t S, int64_t D, int64_t sketch, float* raw,
                       float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);
/* The failure of leverage_press.py:56 (`raise RuntimeError("Cholesky failed after 5 tries")`): reads the per-head status the last
 * kvp_leverage_score on workspace `ws` (same shape arguments) left, SYNCHRONISING `stream` -- as the reference's check of `info` does
 * at :53 -- and returns KVP_ENUMERIC with that message if a head failed (its scores are NaN), else KVP_OK. */
int kvp_leverage_status(const void* ws, int64_t B, int64_t H, int64_t S, int64_t D, int64_t sketch, kvp_stream_t stream);

/* ---- CompactorPress.score tail (kvpress/presses/compactor_press.py:114-122) -------------------------------------------------------
 * scores[b,h,sink_start + s] = blending * z_lev[b,h,s] + z_attn[b,h,s] for s < S_inner (z_* contiguous [B,H,S_inner] float32); the
 * first sink_start and last sink_end positions of each row of scores (contiguous [B,H,S_inner+sink_start+sink_end]) get the global
 * max of the blended scores (F.pad(..., value=scores.max()), :121; NaN if any blended score is NaN, as torch's max). */
size_t kvp_compactor_combine_workspace_bytes(void);
int kvp_compactor_combine(const float* z_lev, const float* z_attn, int64_t B, int64_t H, int64_t S_inner, int64_t sink_start,
                          int64_t sink_end, float blending, float* scores, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- MergingPress.merge (kvpress/presses/merging_press.py:99-177) -------------------------------------------------------------------
 * After kvp_topk_select + kvp_gather_kv: every evicted token's value is folded into the value of its most cosine-similar kept token,
 * IN PLACE in the gathered V' (v_out).  k / v: the cache's keys and values [B,H,S,D] (element strides); kept_idx: int32 [B,H,n_kept] in
 * the order the select wrote them (either kvp_order); k_out (read only) / v_out: the contiguous gathered K' / V' [B,H,n_kept,D].  The
 * evicted tokens are the complement of the kept set in ascending position (:124-127).  target = argmax_j cos(k_e, k'_j) over the kept
 * list (ties: the LOWEST index in it, torch's first occurrence), max_sim its cosine (:137-139); the gates (:141-150): max_sim >=
 * similarity_threshold (compared in float32) and, for merge_fraction < 1, max_sim >= the per-row torch.quantile(1 - merge_fraction) of
 * max_sim with failed entries at -inf, with ATen's float32 rank and lerp (a NaN quantile, which torch returns when the lower order
 * statistic is -inf and the lerp weight is below 0.5, lets nothing in that row merge); w = clamp(max_sim, 0) * gate * |v_e| / (|v_e| +
 * |v'_t| + 1e-6) with |v'_t| from V' before the merge (:152-156); rows with sum(w) > 0 become ((v' + sum w v_e) / (1 + sum w)) rounded
 * to the dtype, the sums in float32 in ascending evicted position, the others are left untouched (:158-173).  target (int32) and
 * max_sim (float32), [B,H,S - n_kept] contiguous, may be NULL.  Nothing happens when n_kept == 0 or n_kept == S (:120-121).  D <= 256;
 * bf16 / f16 with D in {64,96,128,256} and 16-byte aligned key rows run the similarity GEMM on the matrix cores, everything else on a
 * generic kernel.  Workspace: 32 bytes per (b, h, token) + O(B*H*S / 1024); never anything of size n_evict x n_kept.  Bit-identical
 * results from run to run (no float atomics). */
size_t kvp_merge_workspace_bytes(int64_t B, int64_t H, int64_t S, int64_t n_kept, int64_t D);
int kvp_merge_values(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                     const int32_t* kept_idx, const void* k_out, void* v_out, int dtype, int64_t B, int64_t H, int64_t S, int64_t n_kept,
                     int64_t D, double similarity_threshold, double merge_fraction, void* ws, size_t ws_bytes, int32_t* target,
                     float* max_sim, kvp_stream_t stream);

/* ---- CAMPress: per-step attention accumulation (kvpress/presses/cam_press.py:258-283, 326-361) ----------------------------------------
 * Every decoding step of a layer: a[b,hkv,s] = mean over the G = Hq / Hkv query heads of the group of softmax_s(q_g . k_s / sqrt(D)) over
 * ALL S keys (the newest token's own key included, :346-348), in float32, and in place
 *     running[b,hkv,s] = (s < S_prev ? running[b,hkv,s] : 0) + a[b,hkv,s]     for s < S
 * which is the reference's zero pad of the running sum (:273-281) and its `+=` (:283) without a torch.cat per step; S_prev = 0 is its
 * first step (:270-271).  q: the PRE-RoPE query of the newest token [B,Hq,1,D]; cos / sin: its row of the position embeddings [Bc,1,D],
 * Bc = B or 1 (cs_sb = 0 broadcasts); the RoPE is evaluated as in kvp_snapkv_score_rope (:341-344).  k: keys [B,Hkv,S,D] (element
 * strides).  running: float32 rows of capacity cap >= S (element strides r_sb, r_sh).  D even and <= 256, G <= 16.  S is split over
 * workgroups (two-pass softmax statistics, combined in a fixed order: bit-identical from run to run, no float atomics).  Workspace:
 * 4 bytes per (b, query head, key) + O(B * Hq * 256). */
size_t kvp_cam_attn_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t S);
int kvp_cam_attn_accumulate(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sw, const void* cos, const void* sin, int64_t cs_sb,
                            int64_t cs_sw, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype, int64_t B, int64_t Hq,
                            int64_t Hkv, int64_t S, int64_t D, float* running, int64_t r_sb, int64_t r_sh, int64_t cap, int64_t S_prev,
                            void* ws, size_t ws_bytes, kvp_stream_t stream);
/* The same when the attention layer returned its weights (cam_press.py:259-265): attn is the last query row, [B,Hq,S] (element strides
 * a_sb, a_sh, last dim contiguous) in `dtype`; only the group mean (:356-361) and the accumulation run. */
int kvp_cam_attn_accumulate_row(const void* attn, int64_t a_sb, int64_t a_sh, int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S,
                                float* running, int64_t r_sb, int64_t r_sh, int64_t cap, int64_t S_prev, kvp_stream_t stream);

/* ---- CAMPress: merge plan (kvpress/presses/cam_press.py:144-183) ---------------------------------------------------------------------
 * kept: the T kept positions, ascending, int32 [B,T]; attn: the running sum, float32 [B,H,>=S] (element strides a_sb, a_sh).  sel, int32
 * [B,n_sel] ascending, is either the M merge candidates themselves (n_sel == M) or the superset kept + candidates (n_sel == T + M: the
 * position-order selects of the top T and the top T + M scores; the candidates are then found here, the i-th entry of sel that is not
 * kept -- no sort or set difference on the host for :144-157).  For candidate i at position p: start[b,i] = #{kept <= p} (searchsorted
 * right, :159), budget = min(merge_budget, T - start) (:164-169), mean = sum of attn over kept[start .. start + budget) / max(budget, 1)
 * (:172-176), prob[b,h,i] = attn[b,h,p] / mean with NaN -> 0, +-inf -> 1, clamped to [0, 1] (:179-183).  cand (may be NULL) and start:
 * int32 [B,M]; prob: float32 [B,H,M], contiguous.  1 <= T <= S, 0 <= M <= S - T, merge_budget > 0. */
int kvp_cam_merge_plan(const int32_t* kept, const int32_t* sel, int64_t n_sel, const float* attn, int64_t a_sb, int64_t a_sh, int64_t B,
                       int64_t H, int64_t S, int64_t T, int64_t M, int64_t merge_budget, int32_t* cand, int32_t* start, float* prob,
                       kvp_stream_t stream);

/* ---- CAMPress: merge and prune (kvpress/presses/cam_press.py:188-213) ----------------------------------------------------------------
 * New contiguous tensors k_out, v_out [B,H,T,D] and attn_out float32 [B,H,T]: k_out and attn_out are the gathers of k and attn at the
 * kept positions (:205-213); v_out[b,h,t] = v[kept[t]] + sum over the candidates i with start[b,i] <= t < start[b,i] + budget_i of
 * mask[b,h,i] / budget_i * v[cand[i]] (:189-202), where start is kvp_cam_merge_plan's and mask float32 [B,H,M] (the Bernoulli draw of
 * prob, :186).  The sum runs in float32 in ascending candidate order and is rounded to the dtype once; a row without contributors
 * keeps its bits.  k, v and attn are NOT written (the reference scatter-adds into the cache's values in place, :202).  D <= 256. */
int kvp_cam_merge_prune(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                        const float* attn, int64_t a_sb, int64_t a_sh, const int32_t* kept, const int32_t* cand, const int32_t* start,
                        const float* mask, int dtype, int64_t B, int64_t H, int64_t S, int64_t T, int64_t M, int64_t D,
                        int64_t merge_budget, void* k_out, void* v_out, float* attn_out, kvp_stream_t stream);

/* ---- CriticalKVPress.vwl1norm + the rescale (kvpress/presses/criticalkv_press.py:57-76, :87; CriticalAdaKVPress :174-175) -------------
 * values: [B,Hkv,S,D] (element strides); wo: o_proj.weight [hidden, Hq*D] in the same dtype, rows wo_ld elements apart (a bias is ignored,
 * as the reference ignores it).  With G = Hq / Hkv
 *     norm[b,k,s] = (1/G) sum_{g<G} sum_{c<hidden} | sum_{d<D} v[b,k,s,d] * wo[c, (k*G + g)*D + d] |
 * -- the reference's per-head `V_h @ Wo_h` of [S, hidden] (:69), its L1 norm (:70) and the mean over the group (:75) without the
 * intermediate.  scores_in NULL: out = norm; else out = (scores_in + eps) * norm, float32, the sum rounded before the product (:87);
 * scores_in: float32 [B*Hkv, S], rows scores_stride elements apart; out: float32 [B*Hkv, S] contiguous, may alias scores_in.
 * bf16 / f16 with D in {64,96,128,256} and 16-byte aligned rows of values and wo run on the matrix cores (products exact, float32
 * accumulation and sums; the value rows of a token tile stay in registers for all G heads and every row of wo; nothing of size
 * [S, hidden] or [Hq, S] is stored); everything else (float32, other D, unaligned rows) on a generic kernel.  hidden and S need not be
 * multiples of any tile.  The workspace is empty today (the query returns 0; ws may be NULL).  Bit-identical from run to run. */
size_t kvp_vwl1norm_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, int64_t hidden);
int kvp_vwl1norm_rescale(const void* values, int64_t v_sb, int64_t v_sh, int64_t v_ss, int dtype, const void* wo, int64_t wo_ld, int64_t B,
                         int64_t Hq, int64_t Hkv, int64_t S, int64_t D, int64_t hidden, const float* scores_in, int64_t scores_stride,
                         float eps, float* out, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* scores[r, idx[r, j]] = value for every j < counts[r]: the per-head prefix `scatter_` of the two-stage selection
 * (kvpress/presses/criticalkv_press.py:169-171, :177-179) on the rows of a KVP_ORDER_SCORE select.  idx int32 [R, n] contiguous; counts
 * int32 [R] on the device, 0 <= counts[r] <= n (clamped); scores rows row_stride elements apart. */
int kvp_scores_fill_prefix(float* scores, int64_t R, int64_t S, int64_t row_stride, const int32_t* idx, int64_t n, const int32_t* counts,
                           float value, kvp_stream_t stream);

/* ---- KVzipPress.score_kvzip (kvpress/presses/kvzip_press.py:312-332, :350-354; with the scales also :336-337, :348) -------------------
 * The maximum cross-attention of one context chunk during the "repeat the context" forward.  q: PRE-RoPE queries of the Lq repeated
 * tokens [B,Hq,Lq,D]; cos / sin: their rotary tables [Bc,Lq,D], Bc = B or 1 (cs_sb = 0 broadcasts), RoPE'd in the library as in
 * kvp_snapkv_score_rope (:312-313).  k: the layer's keys as they sit in the cache after that forward, [B,Hkv,S,D] with S = context
 * length + Lq (element strides; no subsampled copy as at :319-327).  0 <= sink <= start < end <= S - Lq.  Row t of query head hG+g sees
 *     V(t) = [0, sink) u [start, end) u { S - Lq + u : u <= t }
 * p = softmax over V(t) of q.k / sqrt(D) in float32 (:330-332), and
 *     out[b,h,j - start] = max over g < G, t < Lq of p[g,t,j] * row_scale[b,t] * col_scale[b,hG+g,j - start]       start <= j < end
 * (:350-351).  row_scale float32 [B,Lq] and col_scale float32 [B,Hq,end-start], contiguous, non-negative (KVzip+'s 1/||h_t|| and
 * ||V_j Wo_{h,g}||, :336-337, :348), either may be NULL (= 1).  out: float32, row (b,h) at out + (b*Hkv + h) * out_stride, so a press
 * writes straight into its score table (:354).  Nothing of extent Lq x keys is stored: pass 1 keeps (max, log-sum) per row over all of
 * V(t), skipping key tiles above the causal diagonal; pass 2 recomputes the chunk's logits and keeps the column maximum of
 * 2^(s - lse).  bf16 / f16 with D in {64,96,128,256} and 16-byte aligned key rows run on the matrix cores, everything else (float32,
 * other even D, unaligned rows) on a generic kernel.  Workspace: the rotated queries + 12 bytes per (b, query head, row) per key split
 * + the partial maxima.  Bit-identical from run to run (no atomics). */
size_t kvp_kvzip_score_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Lq, int64_t D, int64_t sink, int64_t ctx);
int kvp_kvzip_score(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* cos, const void* sin, int64_t cs_sb, int64_t cs_sw,
                    const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S,
                    int64_t Lq, int64_t D, int64_t sink, int64_t start, int64_t end, const float* row_scale, const float* col_scale,
                    float* out, int64_t out_stride, void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- KVzapPress.score (kvpress/presses/kvzap_press.py:79-81; the surrogate's bodies :33-35 linear, :38-45 mlp) --------------------------
 * x: the hidden states the attention layer received, [B,S,K] (element strides x_sb, x_ss; rows contiguous).  w1 [N,K], b1 [N], w2 [Hout,N],
 * b2 [Hout]: one layer of KVzapModel.layers, contiguous, in x's dtype.  N == 0 is the linear model: w1 is [Hout,K], b1 its bias, w2 / b2
 * are ignored.
 *     mlp:    out[b,o,s] = b2[o] + sum_j w2[o,j] * gelu(b1[j] + sum_k x[b,s,k] * w1[j,k])          linear: out[b,o,s] = b1[o] + sum_k x w1[o,k]
 * out: float32 [B,Hout,S] through element strides (the transpose of :81 is part of the store).  Layer one accumulates in float32, the bias
 * is added in float32, the GELU is the erf form in float32 (nn.GELU()), layer two is float32 fmas over the unrounded activations in a
 * fixed order.  bf16 / f16 with 16-byte aligned rows, K % 32 == 0 and Hout <= 16: more than 16 tokens run on the matrix cores (N % 32 == 0,
 * 32 <= N <= 1024: a workgroup owns a tile of tokens and all N hidden columns, nothing of extent S x N is stored; the linear model on an
 * mma16 kernel bound by reading x once); up to 16 tokens (a decoding step) spread the rows of w1 over the chip, write float32 partials per
 * slice into the workspace and add them in slice order in a second launch.  Everything else (float32, unaligned rows, other K / N,
 * Hout <= 256) runs on a generic kernel.  S == 0 succeeds and writes nothing.  Bit-identical from run to run (no atomics). */
size_t kvp_kvzap_score_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t K, int64_t N, int64_t Hout);
int kvp_kvzap_score(const void* x, int64_t x_sb, int64_t x_ss, int dtype, const void* w1, const void* b1, const void* w2, const void* b2,
                    int64_t B, int64_t S, int64_t K, int64_t N, int64_t Hout, float* out, int64_t o_sb, int64_t o_sh, int64_t o_ss,
                    void* ws, size_t ws_bytes, kvp_stream_t stream);

/* ---- DMSPress's eviction (kvpress/presses/dms_press.py:106-112): torch.where(scores < threshold) and the shift ---------------------------
 * scores: float32 [B,H,n] through element strides (a [..., :n] view of the press's buffer passes as it is).  Phase 1, kvp_threshold_count:
 * the number of entries with score < threshold (a NaN compares false: kept) into *total, a HOST address -- the call waits for the
 * stream, as the reference's torch.where does -- and the per-block offsets into the workspace.  Phase 2, kvp_threshold_select, with the
 * same arguments, that workspace and that total: out_b / out_h / out_p int64 [total] receive (b, h, position + shift) of those entries
 * in row-major order (torch.where's), ready for module.masked_key_indices.  No atomics; n = 1 and n = 131072 take the same kernels. */
size_t kvp_threshold_select_workspace_bytes(int64_t B, int64_t H, int64_t n);
int kvp_threshold_count(const float* scores, int64_t s_sb, int64_t s_sh, int64_t s_sn, int64_t B, int64_t H, int64_t n, float threshold,
                        void* ws, size_t ws_bytes, int64_t* total, kvp_stream_t stream);
int kvp_threshold_select(const float* scores, int64_t s_sb, int64_t s_sh, int64_t s_sn, int64_t B, int64_t H, int64_t n, float threshold,
                         int64_t shift, const void* ws, size_t ws_bytes, int64_t total, int64_t* out_b, int64_t* out_h, int64_t* out_p,
                         kvp_stream_t stream);

/* ---- FastKVzipPress's gate (kvpress/presses/fastkvzip_press.py:54-71) and the protected positions of :240-247 -----------------------------
 * x: the hidden states the attention layer received, [B,S,K] (element strides x_sb, x_ss; rows contiguous).  One layer's FastKVzipGate in
 * its natural layouts: wq [Hkv*G*D, K] and bq [Hkv*G*D] (q_proj), wk [Hkv*D, K] (k_proj, no bias), b [Hkv,G], contiguous, in x's dtype;
 * gq [D], gk [D] (the RMSNorm weights) and k_base [Hkv,J,D], contiguous float32.  With RMSNorm_g(v) = g * v / sqrt(mean(v^2) + eps):
 *     q[s,h,g,:] = RMSNorm_gq(x[s] wq[(hG+g)D .. +D]^T + bq[..])              k[s,h,:] = RMSNorm_gk(x[s] wk[hD .. +D]^T)
 *     logit = <k[s,h], q[s,h,g]> / sqrt(D) + b[h,g]                           base_j = <k_base[h,j], q[s,h,g]> / sqrt(D)
 *     out[b,h,s] = (1/G) sum_g 1 / (1 + sum_{j<J} exp(base_j - logit))        (J == 0: exactly 1)
 * and out[b,h,s] = 1.0f exactly for s < protect_head or s >= S - protect_tail (either count may exceed S), written by the same launch.
 * out: float32 [B,Hkv,S] through element strides, so a press writes each layer into its slice of one [L,B,Hkv,S] table.  The products
 * accumulate in float32 and everything after them is float32 (the reference rounds the projections and the normalised vectors to the
 * gate's dtype); every sum has one fixed order (d, then j, then g), no atomics: bit-identical from run to run.  bf16 / f16 with 16-byte
 * aligned rows, K % 32 == 0, D == 16, J <= 16 and G <= 8 run on the matrix cores: a workgroup owns a tile of 128 tokens and all
 * (G+1)*16 projected columns of a group of kv heads, so neither q [S, Hkv*G*D] nor the logits [Hkv,S,J,G] are ever stored.  Everything
 * else (float32, unaligned rows, other K, D <= 64, any J and G with (G+1)*D <= 8192) runs on a generic kernel.  S == 0 succeeds and
 * writes nothing.  ws / ws_bytes are RESERVED: no path stores anything outside its workgroups' LDS today, the size query returns 0 and the
 * arguments are not read (ws may be NULL); they are in the signature so that a path that needs scratch can be added without a new entry. */
size_t kvp_fastkvzip_score_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t K, int64_t Hkv, int64_t G, int64_t D, int64_t J);
int kvp_fastkvzip_score(const void* x, int64_t x_sb, int64_t x_ss, int dtype, const void* wq, const void* bq, const void* wk, const void* b,
                        const float* gq, const float* gk, const float* k_base, int64_t B, int64_t S, int64_t K, int64_t Hkv, int64_t G,
                        int64_t D, int64_t J, float eps, int64_t protect_head, int64_t protect_tail, float* out, int64_t o_sb, int64_t o_sh,
                        int64_t o_ss, void* ws, size_t ws_bytes, kvp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KVPRESS_HIP_H */
