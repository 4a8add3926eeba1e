/*
 * libmust3r_hip -- C ABI of the MI355X-native MUSt3R multi-view forward path.
 *
 * Drop-in boundary: everything behind the reference's two nn.Module forwards
 *     Dust3rEncoder.forward(img, true_shape) -> (x, pos)              must3r/model/encoder.py:46-52
 *     MUSt3R.forward / forward_list(x, pos, true_shape, mem, render)  must3r/model/decoder.py:158-350
 * plus the fp32 output activation of engine/inference.py:16-27.
 *
 * Conventions
 *   - plain C types only: raw DEVICE pointers (tensor.data_ptr()), sizes, an opaque context handle and a
 *     hipStream_t passed as void*.  No torch types, no exceptions across the boundary.
 *   - every entry point returns 0 on success, non-zero on error; must3r_hip_last_error() returns a
 *     thread-local, NUL-terminated description of the last failure.
 *   - the caller owns all input/output buffers.  The context owns its weights (fp32 master + packed 16-bit
 *     copies) and a grow-only workspace arena; no allocation happens on the hot path once shapes have been
 *     seen.  A context is bound to one device and is not re-entrant (one forward in flight per context),
 *     like the reference (slam/slam.py:533 runs forwards from a single worker thread).
 *   - "16-bit" buffers hold bf16 or fp16 elements according to the `dtype` argument.
 *   - stream order: every entry point that takes a `stream` enqueues ALL of its work on it -- kernels, memsets, and the copies of the tables it builds on
 *     the host -- and returns without waiting for it; nothing goes to the null stream or to a stream of the library's own, so the caller's stream order is the
 *     only ordering between calls (tests/test_stream_order_gpu.py holds every such entry point to this on a delayed side stream).  The entry points of
 *     must3r_hip_cross_sublayer_args take their stream as the descriptor's `stream` field instead of a trailing argument and are held to the same guarantee
 *     (tests/test_cross_grad_gpu.py).  The one entry point that
 *     synchronises the host with `stream` is must3r_hip_export_count (it returns totals).  Beyond that a call may wait on the host only for staging of its own:
 *     host-built tables travel through rings of pinned slots (per calling thread: 4 for must3r_hip_resample, 4 for must3r_hip_attn_forward_f32 /
 *     must3r_hip_attn_grad and the attention and cross-attention sublayer entry points built on them; per context: 32 for the view tables of must3r_hip_encode / must3r_hip_decode),
 *     and a call that finds its next slot still in flight waits for THAT copy, not for the stream; the growth of a context's workspace to a larger shape
 *     synchronises once.
 *     A context, and a calling thread's staging, serve one stream at a time: the device slots of the forwards' view tables are ordered by stream order only, so
 *     two streams must not share a context (or interleave calls of one thread) without ordering the streams themselves.
 */
#ifndef MUST3R_HIP_H
#define MUST3R_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUST3R_HIP_ABI_VERSION 21

typedef struct must3r_hip_ctx must3r_hip_ctx;

/* MFMA operand type (accumulation, softmax, LayerNorm and the residual stream are always fp32) */
/* MUST3R_F16_W2: fp16 operands with every weight matrix split as W_hi + W_lo (two MFMA passes per GEMM, fp32
 * accumulation): removes the weight-rounding term that dominates the fp16 error (precision). Only valid
 * for must3r_hip_encode / must3r_hip_decode; buffers are fp16. */
/* MUST3R_F16_WA: as MUST3R_F16_W2 for the attention-side Linears (qkv, proj, projq, projk, projv, cross proj), the patch / enc->dec
 * embeddings and the head, but the Mlp weights (fc1, fc2, feedback Mlp) are plain fp16: 2/3 of the GEMM FLOPs run ONE MFMA pass.
 * Measured / emulated error: between the two; inside the 1e-3 target. */
enum { MUST3R_BF16 = 0, MUST3R_F16 = 1, MUST3R_F16_W2 = 2, MUST3R_F16_WA = 3 };
/* OR-able flag on `dtype` (BASELINE.json configs[4], "fp8 MFMA attention path"; replaces the attention back ends of
 * must3r/model/blocks/attention.py:57-79): Q and K enter the score product as OCP e4m3 bytes through the MX-scaled
 * v_mfma_scale_f32_32x32x64_f8f6f4 (twice the 16-bit MFMA rate); the softmax, its numerators P, V, the accumulators and the outputs
 * stay fp32 / 16-bit (3 mantissa bits on V alone cost 9e-3 of pointmap error, on Q and K 2e-3: DESIGN.md section 4).
 *   must3r_hip_op_attention: Q and K ARE e4m3 arrays (ldq, ldk in bytes); V and O 16-bit (ldv, ldo in elements).
 *   must3r_hip_encode / must3r_hip_decode: q and k are quantised on the fly; with MUST3R_MEM_KV the memory buffers hold rows of
 *   [K e4m3: dec_dim bytes | V 16-bit: 2*dec_dim bytes] = 3*dec_dim bytes (3/4 of the 16-bit footprint).
 * r06: PARKED.  Measured on BASELINE.json configs[4]: +0.4 % (680.4 vs 677.9 views/s) at 1.2e-3 ... 1.4e-3 from the 16-bit path -- outside the 1e-3 target for
 * nothing.  The flag is honoured only by libraries built with `make EXTRA=-DM3R_ATTN_FP8` (must3r_hip_has_fp8_attention() == 1); the default
 * library refuses it with status 1 and an error string that says so, and contains neither attn4_kernel<.., F8> nor the quantisation kernel. */
#define MUST3R_ATTN_FP8 0x100
int must3r_hip_has_fp8_attention(void);

/* layout of the caller-visible memory tensors; CachedDecoderBlock MEMORY_MODES, must3r/model/blocks/layers.py:9 */
enum { MUST3R_MEM_KV = 0, MUST3R_MEM_NORM_Y = 1, MUST3R_MEM_RAW = 2 };

/* constructor arguments of Dust3rEncoder (encoder.py:14-23) and MUSt3R (decoder.py:19-37) */
typedef struct must3r_hip_config {
    int32_t img_size, patch_size;
    int32_t enc_dim, enc_depth, enc_heads;
    int32_t dec_dim, dec_depth, dec_heads;
    int32_t mlp_ratio;
    float rope_freq; /* 'RoPE100' -> 100 (blocks/pos_embed.py:20) */
    float rope_f0;   /* F0 = old/new size (blocks/pos_embed.py:12-19) */
} must3r_hip_config;

int must3r_hip_abi_version(void);
const char* must3r_hip_last_error(void);
/* ABI 8.  Process-wide A/B switches of the library (measuring instruments, not model semantics: DESIGN.md section 10 lists them -- "PERSIST", "GEMM256",
 * "G256K", "G256P", "G256P_SPLIT", "SPARSE_256", "SPARSE_LO", "BK128", "LN_ROWS", "LNFOLD", "ENC_CHUNK_ROWS", "ATTN_LZ", "LNFOLD256", "G256_GM",
 * "NN_LEAF_LOG2", "NN_QUERY_LANES_LOG2").  Each has a default and an allowed
 * range; an unknown name or a value outside the range is refused (status 1, must3r_hip_last_error() says why).  Without a call a switch takes its value from the
 * environment variable M3R_<NAME> (validated alike; a bad value is reported on stderr and ignored).  No counterpart in the reference: its only back-end
 * switch is toggle_memory_efficient_attention (must3r/model/blocks/attention.py:18-27). */
int must3r_hip_set_option(const char* name, long long value);

/* lifetime.  replaces: eval(encoder_args)/eval(decoder_args) + .to(device) in load_model, model/__init__.py:38-46 */
int must3r_hip_create(const must3r_hip_config* cfg, int device, must3r_hip_ctx** out);
void must3r_hip_destroy(must3r_hip_ctx* ctx);

/* Weight ingestion.  replaces: load_state_dict(strict=True), model/__init__.py:43-44.
 * `name` is the reference state-dict key prefixed by "encoder." or "decoder." (SURVEY.md section 8b), e.g.
 * "encoder.blocks_enc.0.attn.qkv.weight".  `data` is fp32, contiguous, on host (is_device=0) or device.
 * The tensor is copied.  Unknown names and shape mismatches are errors. */
int must3r_hip_load_weight(must3r_hip_ctx* ctx, const char* name, const float* data, int is_device,
                           int ndim, const int64_t* shape);
/* strict check that every parameter of the selected module(s) has been loaded; builds the fused / permuted
 * device copies (K|V projection, pixel-shuffled head, RoPE table).  The reference returns encoder and decoder
 * as two independent nn.Modules (model/__init__.py:50), so each half can be finalized on its own context. */
enum { MUST3R_PART_ENCODER = 1, MUST3R_PART_DECODER = 2 };
int must3r_hip_finalize_weights(must3r_hip_ctx* ctx, int parts);

/* Dust3rEncoder.forward (encoder.py:46-52): img fp32 [n_views,3,H,W] (one aspect ratio per call)
 *   -> tokens fp32 [n_views, N, enc_dim] (after norm_enc), pos int64 [n_views, N, 2] = (y, x); N = H/16 * W/16. */
int must3r_hip_encode(must3r_hip_ctx* ctx, int dtype, const float* img, int n_views, int H, int W,
                      float* out_tokens, int64_t* out_pos, void* stream);

/* one aspect-ratio group of a decoder call (one list entry of MUSt3R.forward_list, decoder.py:158).
 * With n_scenes = B > 1 every array carries the batch dimension in front, like the reference's tensors (decoder.py:170-186):
 * tokens [B, n_views, n_tokens, enc_dim], pos [B, n_views, n_tokens, 2], pointmaps [B, n_views, H, W, 7], all contiguous. */
typedef struct must3r_hip_group {
    const float* tokens;  /* fp32 [n_views, n_tokens, enc_dim] encoder output */
    const int64_t* pos;   /* int64 [n_views, n_tokens, 2] */
    int32_t n_views, n_tokens, H, W;
    float* pointmaps;     /* out fp32 [n_views, H, W, 7] raw head output (decoder.py:149-156) */
    /* ABI 7: elements between the pointmaps of consecutive SCENES of this group; 0 = n_views*H*W*7 (the contiguous [B, n_views, H, W, 7] of the
     * reference).  A caller that walks a scene's views over several calls (the sequential memory update) can hand every call the slice
     * [:, i:i+n] of ONE [B, V, H, W, 7] buffer instead of concatenating the calls' outputs afterwards (must3r_amd.engine.run_scenes). */
    int64_t pointmaps_scene_stride;   /* must be a multiple of 4 (the head epilogue stores 16-byte vectors); the call is refused otherwise */
} must3r_hip_group;

/* ---- ABI 8: context-parallel cross attention (SURVEY.md section 8f "later"; the keys of must3r/model/decoder.py:301-321's cross attention spread over processes) ----
 * The memory of ONE scene is SHARDED over `world` ranks (one process per GPU): every rank holds some of the memory rows of every layer, runs the same one-view
 * memory update on the same tokens (the projections / self attention / Mlp of a 768-row call are replicated, they do not shard), but attends only ITS rows and
 * contributes one PARTIAL per layer: un-normalised O fp32 [rows][dec_dim] (or, with partial16, O / l in the 16-bit operand type) followed by fp32 (m, l)
 * [rows][heads][2] -- the flash-attention partial.  The library then
 * calls `exchange`, which must leave rank r's partial in slot r on every rank (an all-gather over xGMI: RCCL's ncclAllGather, or
 * torch.distributed.all_gather_into_tensor on the caller's stream), and merges the `world` slots.  A rank may hold no rows at all (n_mem = 0).
 * Only for memory-update calls of ONE view on ONE scene in MUST3R_MEM_KV mode against a non-empty (global) memory: the per-frame call of the streaming schedule
 * (engine/inference.py:232-366).  The new K|V rows are appended to THIS rank's buffers as usual; the caller decides which rank keeps them
 * (must3r_amd.parallel.run_video_sharded(context_parallel=True): the frame's owner keeps, the others rewind).
 * `exchange` runs on the calling thread between launches on `stream`: it must enqueue the collective in stream order and must not synchronise the device with the
 * library's launches still queued behind it unless it has to (a host-staged exchange may).  Non-zero return aborts the call (status 1). */
typedef int (*must3r_hip_cp_exchange_fn)(void* user, int layer, void* slots, size_t slot_bytes, int n_slots, int my_slot, void* stream);
typedef struct must3r_hip_cp {
    int32_t world, rank;     /* ranks the memory is sharded over (>= 1; 1 = a group of one rank, the exchange still runs), this rank */
    int32_t n_mem_total;     /* memory rows over ALL ranks before this call (> 0); must3r_hip_decode_args.n_mem = THIS rank's rows (>= 0) */
    int32_t partial16;       /* 0: fp32 partials (un-normalised O); 1: the 16-bit partial format of the library's own split-KV path (O / l in the operand type + fp32
                              * (m, l)): half the bytes on the links, one more 16-bit rounding of an intermediate (inside the precision mode's tolerance; tests) */
    void* slots;             /* device buffer of world x slot_bytes bytes, 16-byte aligned; slot r = rank r's partial of the layer being exchanged */
    size_t slot_bytes;       /* >= must3r_hip_cp_slot_bytes(ctx, rows of the call) (partial16: must3r_hip_cp_slot_bytes16), a multiple of 16 */
    must3r_hip_cp_exchange_fn exchange;
    void* user;
} must3r_hip_cp;

typedef struct must3r_hip_decode_args {
    int32_t dtype;        /* MUST3R_BF16 / MUST3R_F16 / MUST3R_F16_W2 / MUST3R_F16_WA (the default of the Python modules: fp16 operands, split weights
                           * in the attention-side Linears, plain in the Mlp Linears): operand type AND element type of the memory buffers (fp16 for the
                           * three F16 modes);
                           * | MUST3R_ATTN_FP8: e4m3 Q / K, MUST3R_MEM_KV memory rows are [K e4m3 | V 16-bit] = 3*dec_dim bytes */
    int32_t mem_mode;     /* MUST3R_MEM_* */
    int32_t render;       /* decoder.py:267 `render`: memory is read-only, no exclusion mask */
    int32_t first_call;   /* current_mem is None: view 0 of group 0 gets no image2_embed (decoder.py:280-282) */
    int32_t n_groups;
    const must3r_hip_group* groups;
    int32_t n_mem;        /* Nm: valid memory tokens (per scene) before this call */
    /* per decoder layer: 16-bit ([K e4m3 | V 16-bit] byte rows with MUST3R_ATTN_FP8 + MUST3R_MEM_KV) [mem_capacity, mem_dim] row-major, mem_dim = 2*dec_dim (KV)
     * or dec_dim.  Rows [0,n_mem) are read; unless render, rows [n_mem, n_mem + sum(n_views*n_tokens)) are WRITTEN -- the in-place
     * form of torch.concatenate at decoder.py:239/330.  The call is refused when they would not fit mem_capacity. */
    void* const* mem;
    /* optional (`return_feats=True`, decoder.py:344-347 / :258-262): fp32 [dec_depth][R][dec_dim], R = n_scenes * sum(n_views*n_tokens),
     * rows scene-major, then group order; entry l = the residual stream after decoder block l, the last one after norm_dec
     * (decoder.py:150).  NULL = not wanted.  (feats[0] of the reference, the encoder tokens, is the caller's own input.) */
    float* feats;
    /* ---- ABI 5 ---- */
    int32_t mem_capacity; /* rows every scene's buffer can hold (> 0): bounds-checked against n_mem + the rows this call appends */
    /* B of the reference's tensors (decoder.py:170: x[i] is [B, nimg, Ni, Denc]): n_scenes independent scenes of identical shapes
     * (same groups, same n_mem) decoded by ONE launch sequence -- M = B x rows in every GEMM, B x views in the attention tables.
     * Scene b's memory of layer l is mem[l] + b * mem_scene_stride rows (mem_scene_stride >= mem_capacity); the scenes never
     * interact, results are bit-identical to B calls with n_scenes = 1 wherever the kernels' tile shapes coincide and within the
     * mode's tolerance otherwise.  0 / 1 = one scene. */
    int32_t n_scenes;
    int64_t mem_scene_stride;
    /* ---- ABI 8 ---- */
    const must3r_hip_cp* cp;   /* NULL: off.  Context-parallel cross attention (above): `mem` / `n_mem` describe this rank's SHARD of the memory */
    /* CausalMUSt3R.forward (decoder.py:435-553; the class the checkpoints are trained as), memory dropout off: in a memory update of several views, view i
     * cross-attends the old memory and the new (pre-feedback) tokens of the views BEFORE it in the call -- make_attn_mask decoder.py:389-433 -- instead of the new
     * tokens of every other view; when the memory is empty view 0 attends view 1's tokens (decoder.py:399-402).  One group (the class has no list dispatch); render
     * and one-view calls are MUSt3R's.  The tuple's tail (protected images / tokens, decoder.py:461-464) is the caller's bookkeeping. */
    int32_t causal;
} must3r_hip_decode_args;

/* bytes of one rank's partial for a context-parallel call of `rows` token rows: rows x (dec_dim + 2 x dec_heads) floats, rounded up to 256;
 * ...16: with partial16 = 1: rows x (2 dec_dim bytes + 2 x dec_heads floats) */
size_t must3r_hip_cp_slot_bytes(const must3r_hip_ctx* ctx, int rows);
size_t must3r_hip_cp_slot_bytes16(const must3r_hip_ctx* ctx, int rows);

/* MUSt3R.forward / forward_list (decoder.py:158-350).  Render calls whose view tables exceed the library's staging slot
 * (1365 views) are cut into ranges of scenes / views inside the library: rendered views are independent. */
int must3r_hip_decode(must3r_hip_ctx* ctx, const must3r_hip_decode_args* args, void* stream);

/* postprocess activation (engine/inference.py:19-27; tools/geometry.py:14-18): pointmaps fp32 [npix,7]
 *   -> pts3d [npix,3], pts3d_local [npix,3], conf [npix] */
int must3r_hip_postprocess(const float* pointmaps, float* pts3d, float* pts3d_local, float* conf, size_t npix,
                           void* stream);
/* the same with the activation named (ABI 6): ActivationType of must3r/model/blocks/head.py:8-21 -- NORM_EXP as above, LINEAR leaves
 * channels 0:3 / 3:6 as they are; conf = 1 + exp(ch 6) in both (engine/inference.py:26-27). */
enum { MUST3R_ACT_NORM_EXP = 0, MUST3R_ACT_LINEAR = 1 };
int must3r_hip_postprocess_act(const float* pointmaps, int activation, float* pts3d, float* pts3d_local, float* conf, size_t npix,
                               void* stream);
/* backward of the activation (ABI 16): grad_raw fp32 [npix,7] from raw [npix,7] and the gradients at pts3d [npix,3], pts3d_local
 * [npix,3] and conf [npix] (any of the three may be NULL = zero).  Nothing is saved by the forward: d = |x| and x^ = x / d are recomputed.
 * NORM_EXP, y = x / max(d, 1e-8) * expm1(d):  grad_x = (expm1(d) / d) (g - <x^, g> x^) + e^d <x^, g> x^ for d >= 1e-8, the derivative of
 * the clipped expression below that, 0 at d = 0.  LINEAR: the gradients pass through.  Channel 6: g * exp(raw[6]) in both. */
int must3r_hip_postprocess_act_grad(const float* pointmaps, int activation, const float* grad_pts3d, const float* grad_pts3d_local,
                                    const float* grad_conf, float* grad_pointmaps, size_t npix, void* stream);

/* postprocess(..., compute_cam=True) (engine/inference.py:16-48), SURVEY.md section 8f rank 1: the activation above
 * plus, per view, focal = dust3r estimate_focal_knowing_depth(pts3d_local, pp=(W/2,H/2), 'weiszfeld')
 * (engine/inference.py:33-35) and (R, T) = roma.rigid_points_registration(pts3d_local -> pts3d, weights conf-1)
 * (engine/inference.py:37-40) written as c2w [n_views,4,4] row-major (engine/inference.py:42-46).
 * pointmaps fp32 [n_views,H,W,7]; outputs fp32; scratch: >= must3r_hip_postprocess_cam_scratch_bytes device bytes.
 * Uses a cooperative launch (all blocks co-resident). */
size_t must3r_hip_postprocess_cam_scratch_bytes(int n_views, int H, int W);
int must3r_hip_postprocess_cam(const float* pointmaps, int n_views, int H, int W, float* pts3d, float* pts3d_local,
                               float* conf, float* focal, float* c2w, void* scratch, size_t scratch_bytes, void* stream);
int must3r_hip_postprocess_cam_act(const float* pointmaps, int activation, int n_views, int H, int W, float* pts3d, float* pts3d_local,
                                   float* conf, float* focal, float* c2w, void* scratch, size_t scratch_bytes, void* stream);

/* Retrieval front-end on the encoder tokens, SURVEY.md section 8f rank 4 (retrieval/model.py).
 * must3r_hip_affine: out[M,N] fp32 = (A[M,K] - sub[K]) . B + bias[N] + resid[M,N]; with is_double the subtraction, the
 *   products and the sums are float64 like Whitener.forward (retrieval/model.py:67-79: x.double() - m, matmul with p), with
 *   b_transposed B is an nn.Linear weight [N,K] (the projector, :139-151,169).  sub / bias / resid may be NULL; sub, B and
 *   bias are float64 arrays when is_double, fp32 otherwise.
 * must3r_hip_row_norm: attention = x.norm(dim=-1) (:130-131).
 * must3r_hip_l2_normalize: F.normalize(x, dim) of a contiguous fp32 tensor seen as [outer, L, inner] (eps 1e-12):
 *   Whitener(l2norm=dim) (:77-78).  out may alias x.
 * must3r_hip_layernorm_act_f32: nn.LayerNorm(C, eps) (+ nn.GELU, exact form z Phi(z), when gelu) on fp32 rows: the hidden layers of a
 *   multi-layer projector (build_projector :139-151, Linear - LayerNorm - GELU stacks); gamma / beta may be NULL.
 * must3r_hip_topk_gather: how_select_local (:91-101): per image the k tokens of largest attention in the order of a
 *   stable descending sort (NaN first, as torch.topk ranks it; ties and NaNs among themselves: lower index first), their
 *   features, attentions and int64 indices.  k <= N <= 4096, C % 4 == 0.
 * must3r_hip_weighted_spoc: weighted_spoc (:82-88): normalize(sum_n attn[n] * feat[n,:]). */
int must3r_hip_affine(int is_double, const float* A, const void* sub, const void* B, int b_transposed, const void* bias,
                      const float* resid, float* out, int M, int N, int K, void* stream);
int must3r_hip_row_norm(const float* x, int M, int C, float* out, void* stream);
int must3r_hip_l2_normalize(const float* x, int64_t outer, int L, int64_t inner, float* out, void* stream);
int must3r_hip_layernorm_act_f32(const float* x, const float* gamma, const float* beta, float eps, int M, int C, int gelu,
                                 float* out, void* stream);
int must3r_hip_topk_gather(const float* feat, const float* attn, int n_images, int N, int C, int k, float* out_feat,
                           float* out_attn, int64_t* out_idx, void* stream);
int must3r_hip_weighted_spoc(const float* feat, const float* attn, int n_images, int N, int C, float* out, void* stream);

/* ---- ABI 11: ASMK back-end of the retrieval mode (demo/inference.py:31-60 MUSt3R_Retriever.__call__; retrieval/processor.py:83-96:
 * binary kernel, use_idf False, multiple_assignment 1 for build_ivf and 5 for query_ivf, similarity_threshold 0, alpha 3, topk None).
 * The same images are database and query; the local features are forward_local's rows, image i owning rows [off_i, off_{i+1}).
 * Deterministic: no atomics, every output has one writer and a fixed order of operations.
 * must3r_hip_asmk_centroid_sqnorm: out[K] = |c|^2 of a codebook [K,D] fp32, once per codebook.
 * must3r_hip_asmk_quantize: ids int32 [M,k] = the k nearest centroids of each feature row (squared L2, ranked by |c|^2 - 2 x.c on the
 *   fp32 MFMA), ascending; an exact tie goes to the lower centroid id; a NaN distance (non-finite input) ranks as +inf, so every id is in [0, K).  One k = 5 search serves both sides: its first column is the
 *   database assignment.  Needs D % 64 == 0, 1 <= k <= 8, k <= K, 16-byte aligned feat / centroids, and `scratch` of
 *   must3r_hip_asmk_quantize_scratch_bytes(M, K, k) device bytes.
 * must3r_hip_asmk_aggregate: per image and side (k_use = 1: database, 5: query, of the k_ids columns of `ids`): W = the ascending distinct
 *   words of its assignments; for w in W, r_w = sum of (x_j - c_w) over the rows j assigned to w, in ascending j, in fp32, each difference
 *   rounded and then added ((des[mask] - centroid).sum(0) on float32 arrays); bit d of w = r_w[d] > 0.  offsets_dev: DEVICE int32
 *   [n_images + 1]; image i writes |W| words (int32) at slot off_i * k_use of `words` [M * k_use] and its bits (uint32 [D / 32] per
 *   word, bit d % 32 of word d / 32) at the same slot of `bits`, and counts[i] = |W|.  max_rows: the largest off_{i+1} - off_i; an image
 *   with more than 4096 (word, row) pairs (rows * k_use) is refused (counts[i] = -1 if the promise is broken), and so is an image with
 *   an id outside [0, K) of the codebook [K, D] (counts[i] = -1; no centroid row is read for it).
 * must3r_hip_asmk_scores: out float64 [n_q, n_d] (row = query, column = database: the reference's `scores` after its un-ranking,
 *   demo/inference.py:57-58): for w in W_q and W_d, ascending: h = popcount(bits_q xor bits_d), s = 1 - 2h/D, sigma = s^alpha if
 *   s >= threshold else 0 (fp32); score = sum sigma in float64, then with `normalize` / sqrt(|W_d|) / sqrt(|W_q|) (0 for an empty side).
 *   PARITY UNPINNED upstream: the 1/sqrt(|W|) normalisation and the tie order. */
int must3r_hip_asmk_centroid_sqnorm(const float* centroids, int K, int D, float* out, void* stream);
size_t must3r_hip_asmk_quantize_scratch_bytes(int M, int K, int k);
int must3r_hip_asmk_quantize(const float* feat, int M, const float* centroids, const float* c_sqnorm, int K, int D, int k, int32_t* ids,
                             void* scratch, size_t scratch_bytes, void* stream);
int must3r_hip_asmk_aggregate(const float* feat, const float* centroids, int K, int D, const int32_t* ids, int k_ids, int k_use,
                              const int32_t* offsets_dev, int n_images, int max_rows, int32_t* words, uint32_t* bits, int32_t* counts,
                              void* stream);
int must3r_hip_asmk_scores(const int32_t* words_q, const uint32_t* bits_q, const int32_t* counts_q, const int32_t* offsets_q, int k_q, int n_q,
                           const int32_t* words_d, const uint32_t* bits_d, const int32_t* counts_d, const int32_t* offsets_d, int k_d, int n_d,
                           int D, float alpha, float threshold, int normalize, double* out, void* stream);

/* ---- ABI 21, additive: learning the retrieval mode's two artefacts on the device (csrc/asmk_train.hip) -- the k-means update behind the ASMK codebook
 * (the assignment step is must3r_hip_asmk_quantize with k = 1) and the covariance behind the PCA whitening (retrieval/model.py:18-35
 * pcawhitenlearn_shrinkage).  The stream is a parameter of both; the scratch and its size come last, as in the other ABI 21 entry points.
 * Deterministic: no floating-point atomics, every floating-point output has one writer and a fixed order of operations.
 * must3r_hip_kmeans_update: feat fp32 [M,D], centroids fp32 [K,D] (the ones the ids were assigned against), ids int32, row j at ids[j * ids_stride]
 *   (ids_stride = 1: a vector; = k: column 0 of a [M,k] tensor), order int64 [M]: the STABLE ascending argsort of the ids (rows grouped by cluster, ascending
 *   row index inside a cluster).  Outputs: counts int32 [K], exact; new_centroids fp32 [K,D]: for counts[c] > 0, fp32(sum / counts[c]) with the sum of the
 *   cluster's rows in fp64, SEQUENTIAL in ascending row index -- bit-for-bit repeatable, and independent of every other row and cluster of the call; for
 *   counts[c] == 0 the old centroids[c], bit for bit (a reseeding rule belongs to the caller).  dist fp64 [M]: sum_d (double(x_jd) - double(c_{ids[j]},d))^2
 *   against the OLD centroids; objective fp64 [1] (device) = sum_j dist[j], in an order that depends on M alone.
 *   Refused (non-zero return, must3r_hip_last_error): a NULL pointer, feat / centroids / new_centroids not 16-byte aligned, order / dist / objective / scratch
 *   not 8-byte aligned, D % 16 != 0, K < 1, M < 1, and an id outside [0, K) or an order entry outside [0, M): the ids are checked on the device before
 *   anything is read through one, and when one is bad NO output is written.  To report that, the call reads one 16-byte record back: the call synchronises
 *   `stream` (after everything is queued).  host_record (HOST double [2], may be NULL) receives that record: the objective and the number of empty clusters.
 *   An order that is not the stable argsort of the ids is not detected: every read stays in bounds and the outputs are unspecified.
 *   `scratch`: must3r_hip_kmeans_update_scratch_bytes(M, K) device bytes.
 * must3r_hip_cov_accumulate: x fp32 [M,D] (D % 16 == 0, 16-byte aligned), shift fp64 [D]; with u_r = double(x_r) - shift it accumulates into the caller's
 *   fp64 state S [D,D] += sum_r u_r u_r^T, s [D] += sum_r u_r, n [1] += M.  The products run on v_mfma_f64_16x16x4_f64 with the rows as the contraction; only
 *   the 64 x 64 tiles on and below the diagonal are computed, and S[b][a] is written as the copy of S[a][b]: S is exactly symmetric.  The rows are split by a
 *   rule of (M, D) alone; every split writes fp64 partials that a second launch adds in split order: repeatable bit for bit, no atomics.  Two calls over
 *   the halves of a chunk and one call over the chunk associate differently and agree to rounding only.  Asynchronous on `stream`.
 *   `scratch`: must3r_hip_cov_accumulate_scratch_bytes(M, D) device bytes (0 for a refused shape). */
size_t must3r_hip_kmeans_update_scratch_bytes(int M, int K);
int must3r_hip_kmeans_update(const float* feat, int M, int D, const float* centroids, int K, const int32_t* ids, int64_t ids_stride, const int64_t* order,
                             float* new_centroids, int32_t* counts, double* dist, double* objective, double* host_record, void* stream, void* scratch,
                             size_t scratch_bytes);
size_t must3r_hip_cov_accumulate_scratch_bytes(int M, int D);
int must3r_hip_cov_accumulate(const float* x, int M, int D, const double* shift, double* S, double* s, double* n, void* stream, void* scratch,
                              size_t scratch_bytes);

/* SLAM keyframe test, SURVEY.md section 8f rank 3 (slam/model.py:62-91 get_overlap_score; slam/nns.py:40-92).
 * must3r_hip_nn_query replaces KDTree_scipy.query (nns.py:52-57: scipy KDTree.query(k=1), Euclidean): out_dist[i] =
 * min_j |q_i - db_j| for fp32 xyz points [n,3] on the device, +inf when n_db == 0 (nns.py:53-54).  Exact (brute force).
 * must3r_hip_quadrant_ids replaces get_quadrant_id (slam/tools.py:9-31) on rays p - cam_center (nns.py:81,88):
 * out[i] in [0, 2*divider^2). */
int must3r_hip_nn_query(const float* db_xyz, int64_t n_db, const float* q_xyz, int64_t n_q, float* out_dist, void* stream);
int must3r_hip_quadrant_ids(const float* pts_xyz, int64_t n, const float* cam_center_host3, int divider, int32_t* out, void* stream);

/* ---- ABI 12: exact 1-NN index over the keyframe map (replaces the full scan of must3r_hip_nn_query for a map queried many times) ----
 * Build once per change of the point set, query any number of times; everything runs on `stream` into caller-owned device buffers.
 * divider = 0: one segment over all points (KDTree_scipy, nns.py:40-57); divider d in [1, 8]: 2 d^2 quadrant segments
 * (QuandrantSearcher, nns.py:60-92), a point's quadrant being quadrant_ids[i] (must3r_hip_quadrant_ids of its add batch's cam centre).
 * must3r_hip_nn_index_build: xyz fp32 [n][3] and quadrant_ids int32 [n] (read only when divider > 0) on the device, n <= 2^30;
 *   index: must3r_hip_nn_index_bytes(n, divider) bytes, scratch: must3r_hip_nn_index_scratch_bytes(n) bytes (free after the build).
 *   Non-finite points are dropped.  Two builds of the same input give byte-identical index buffers (no order decided by atomics).
 *   Leaves hold 2^NN_LEAF_LOG2 points (must3r_hip_set_option, default 5).
 * must3r_hip_nn_index_query: out_dist[i] = the distance must3r_hip_nn_query gives for q_i over the points of q_i's quadrant (the ray
 *   q_i - cam_center_host3, as must3r_hip_quadrant_ids; cam_center_host3 is not read when divider = 0), bit for bit; +inf for an
 *   empty quadrant and for a non-finite query.  divider must be the build's: the index records it, and a query with another divider
 *   writes NaN to every out_dist[i].  No scratch: out_dist holds the query quadrant ids first.  A query is walked by 2^NN_QUERY_LANES_LOG2
 *   lanes together (must3r_hip_set_option, default 3; the distances do not depend on it). */
size_t must3r_hip_nn_index_bytes(int64_t n, int divider);
size_t must3r_hip_nn_index_scratch_bytes(int64_t n);
int must3r_hip_nn_index_build(const float* xyz, const int32_t* quadrant_ids, int64_t n, int divider, void* index, void* scratch, void* stream);
int must3r_hip_nn_index_query(const void* index, const float* q_xyz, int64_t n_q, const float* cam_center_host3, int divider, float* out_dist,
                              void* stream);

/* ---- ABI 13: scene export -- the compaction and the affine map behind get_3D_model_from_scene (demo/gradio.py:75-156) ----
 * One read of the scene's confidences serves up to MUST3R_EXPORT_MAX_THR thresholds: must3r_hip_export_count counts, per block of
 * MUST3R_EXPORT_BLOCK pixels and per threshold, the pixels with conf >= thr (NaN never passes; mesh = 1: the quads whose triangles
 * (a, b, c') resp. (b, c', d) have three passing corners), scans the counts over (view, block) in view-major order on the device and
 * returns the totals per threshold (points, or faces) in totals_host after one small copy (the call synchronises `stream`).
 * The scatter calls then write, for threshold index k of that count, directly in file layout and in the reference's order (view by view,
 * row-major inside a view; compaction inside a block is ordered, nothing is appended through atomics):
 *   position  float32(((m0 x + m1 y) + m2 z) + m3) per row of the view's 3x4 fp64 matrix M, every operation rounded in fp64, one rounding
 *             to fp32;  colour  rint(clip(c, 0, 1) * 255) in fp32 as uint8, alpha 255.
 *   MUST3R_EXPORT_GLB: out_pos float32 [n][3] and out_col uint8 [n][4];  MUST3R_EXPORT_PLY: out_pos holds 16-byte records x y z float32,
 *   r g b a uint8 (out_col is not read).  minmax (device, 6 floats: min xyz, max xyz of the written positions) is reduced in the same
 *   pass through per-block partials; +inf / -inf when nothing was written.
 * must3r_hip_export_vertices: mesh mode, every pixel of every view (not compacted) as GLB planes, vertex index = pixels of the views
 *   before + r W + c.  must3r_hip_export_scatter_faces: uint32 [n_faces][3]; per view the surviving triangles (a,b,c'), then (c',b,a),
 *   then (b,c',d), then (d,c',b), each group in quad row-major order (dust3r.viz.pts3d_to_trimesh + cat_meshes).
 * views_host: host array; conf [H][W], pts [H][W][3], rgb [H][W][3] fp32 on the device, views may differ in size.  The same table,
 * n_thr and mesh flag are passed to every call of one export; scratch: must3r_hip_export_scratch_bytes (0 with a message on a bad
 * table), filled by export_count and read by the scatters.  A scene of 2^32 or more pixels is refused. */
#define MUST3R_EXPORT_MAX_THR 8
#define MUST3R_EXPORT_BLOCK 1024
#define MUST3R_EXPORT_GLB 0
#define MUST3R_EXPORT_PLY 1
typedef struct must3r_hip_export_view {
    const float* conf;
    const float* pts;
    const float* rgb;
    int32_t H, W;
    double M[12];   /* row-major 3x4 */
} must3r_hip_export_view;
size_t must3r_hip_export_scratch_bytes(const must3r_hip_export_view* views_host, int n_views, int n_thr, int mesh);
int must3r_hip_export_count(const must3r_hip_export_view* views_host, int n_views, const float* thr_host, int n_thr, int mesh,
                            void* scratch, size_t scratch_bytes, int64_t* totals_host, void* stream);
int must3r_hip_export_scatter_points(const must3r_hip_export_view* views_host, int n_views, const float* thr_host, int n_thr, int k,
                                     int layout, const void* scratch, void* out_pos, void* out_col, float* minmax, void* stream);
int must3r_hip_export_vertices(const must3r_hip_export_view* views_host, int n_views, int n_thr, void* scratch, float* out_pos,
                               void* out_col, float* minmax, void* stream);
int must3r_hip_export_scatter_faces(const must3r_hip_export_view* views_host, int n_views, const float* thr_host, int n_thr, int k,
                                    const void* scratch, uint32_t* out_faces, void* stream);

/* ---- ABI 14: checkpoint evaluation -- the forward values of eval.py's metric and of must3r/engine/losses.py (Regr3D, ConfLoss), and
 * normalize_pointcloud's norm_factor (must3r/tools/geometry.py:21-84); metrics.hip ----
 * must3r_hip_metrics_loss: one pass over a batch of B scenes x V views of H x W pixels.  Per pixel, in fp32:
 *   g  = in_camera0[b] applied to gt_pts (world);  valid_g = valid && (|g| <= dist_clip when has_dist_clip);  sky_g = sky && !valid_g
 *   gl = w2c[b][v] applied to gt_pts (only with pr_local);  valid_l, sky_l likewise
 *   g, gl are divided by gt_scale[b], pr_pts and pr_local by pr_scale[b] (NULL = 1); with gt_warp resp. pr_warp[b] the global points are
 *   first multiplied by log1p(d) / max(d, 1e-8), d their norm (normalize_pointcloud's 'warp-log1p')
 *   loss_in_log 1: x -> x / max(|x|, 1e-8) * log1p(|x|) on both terms, 2 ('before'): on the global term only
 *   l = |pr - g| where valid_g, sky_loss_value where sky_g (sky pixels count only when sky is given and sky_loss_value > 0)
 *   with conf: cl = l * conf - alpha * log(conf)
 * Outputs per (scene, view): counts int64 [B][V][2] (global, local) and sums fp64 [B][V][4] (l global, l local, cl global, cl local; the
 * local / conf entries are 0 without pr_local / conf).  Pixels outside the selection are never read into a sum (their points may be NaN
 * or inf).  Accumulation is fp64 per thread, wave and block; per-block partials go to a slab in scratch and are summed in index order;
 * blocks never span two views, so the figures of a scene are bit-identical from run to run and whatever else is in the batch.
 * Optional per-pixel outputs (all four or none): pix_g / pix_l fp32 [B][V][H][W] (l, NaN outside the selection), msk_g / msk_l uint8.
 * must3r_hip_metrics_factor: norm_factor fp32 [B] of pts [B][V][H][W][3] (transformed by trf [B][4][4] first when given) over the valid
 * pixels: MUST3R_NORM_AVG_DIS sum d / (nnz + 1e-8), AVG_LOG1P (also 'warp-log1p') sum log1p(d) / (nnz + 1e-8), SQRT_DIS
 * (mean sqrt d)^2, MEDIAN_DIS the lower median, all clipped at 1e-8; SQRT / MEDIAN of an empty scene are NaN.  The median is an exact
 * radix select over the bit patterns of the distances (3 histogram passes of 2048 / 2048 / 1024 bins); it needs dist fp32 [B][V*H*W],
 * which receives every distance (NaN where not selected).  Blocks never span two scenes.
 * Scratch sizes: the two *_scratch_bytes calls (0 with a message on bad sizes).  All pointers are device pointers. */
#define MUST3R_NORM_AVG_DIS 0
#define MUST3R_NORM_AVG_LOG1P 1
#define MUST3R_NORM_SQRT_DIS 2
#define MUST3R_NORM_MEDIAN_DIS 3
typedef struct must3r_hip_metrics_loss_args {
    int32_t n_scenes, n_views, H, W;
    const float* gt_pts;          /* [B][V][H][W][3] world coordinates */
    const float* in_camera0;      /* [B][4][4] row-major */
    const float* w2c;             /* [B][V][4][4], required with pr_local */
    const float* pr_pts;          /* [B][V][H][W][3] */
    const float* pr_local;        /* or NULL */
    const float* conf;            /* [B][V][H][W] or NULL */
    const uint8_t* valid;         /* [B][V][H][W] */
    const uint8_t* sky;           /* or NULL */
    const float* gt_scale;        /* [B] or NULL */
    const float* pr_scale;        /* [B] or NULL */
    const uint8_t* pr_warp;       /* [B] or NULL */
    int32_t gt_warp, has_dist_clip, loss_in_log;
    float dist_clip, sky_loss_value, alpha;
    int64_t* counts;              /* [B][V][2] */
    double* sums;                 /* [B][V][4] */
    float* pix_g; float* pix_l; uint8_t* msk_g; uint8_t* msk_l;   /* optional */
} must3r_hip_metrics_loss_args;
size_t must3r_hip_metrics_loss_scratch_bytes(int n_scenes, int n_views, int H, int W);
int must3r_hip_metrics_loss(const must3r_hip_metrics_loss_args* args, void* scratch, size_t scratch_bytes, void* stream);
size_t must3r_hip_metrics_factor_scratch_bytes(int n_scenes, int n_views, int H, int W, int mode);
int must3r_hip_metrics_factor(const float* pts, const float* trf, const uint8_t* valid, int n_scenes, int n_views, int H, int W, int mode,
                              float* factor, float* dist, void* scratch, size_t scratch_bytes, void* stream);

/* ---- ABI 16: the backward pass of must3r_hip_metrics_loss -- the gradient of the Regr3D / ConfLoss figures at pr_pts, pr_local and conf;
 * metrics.hip ----
 * must3r_hip_metrics_loss_grad takes the argument block of the forward call (its outputs counts / sums / pix_* / msk_* are not used) and
 * the block below.  The selections valid_g / valid_l / sky_g / sky_l and the chain x -> warp -> / pr_scale -> log map -> |. - target| are
 * recomputed per pixel exactly as the forward computes them; ground truth is read only under valid.  With u = r / |r| (0 where r = 0) and
 * J(x) = (log1p(d) / d)(I - x^ x^T) + x^ x^T / (1 + d) the (symmetric) Jacobian of the log map and of the warp (0 at d = 0):
 *   direct term  grad_pts(p) = J_warp(x) J_log(y) (omega_g(p) u_g) / pr_scale[b] on valid_g pixels, grad_local likewise on valid_l pixels
 *                (no warp; log map as the forward applies it); sky pixels and unselected pixels get exactly 0
 *   weighting    MUST3R_LOSS_W_SCALAR  omega = w (reduction 'sum')            MUST3R_LOSS_W_MEAN  omega = w / N (reduction 'mean')
 *                MUST3R_LOSS_W_CONF    omega = w conf / N, and grad_conf = w_g [sel_g](l_g - alpha / conf) / N_g + w_l [sel_l](...) / N_l
 *                MUST3R_LOSS_W_PIXEL   omega = w[p], w_g / w_l fp32 [B][V][H][W] (reduction 'none')
 *                In the first three w_g / w_l point to one device scalar each; N_g / N_l are the batch totals of counts (the forward's
 *                output, read on the device); a term with N = 0 contributes nothing.  The scalar weights are applied last, so the
 *                gradients are linear in them to the rounding of that one product (equal w_g and w_l are factored out).
 *   scale path   for the scenes with own_factor[b] != 0 (pr_scale[b] was computed from pr_pts with factor_mode): with
 *                S_b = -(1 / pr_scale[b]) sum <g_y(p), y(p)> over the valid_g pixels of the global and the valid_l pixels of the local
 *                term (g_y the gradient at y = warp(x) / pr_scale), every valid pixel gets grad_pts(p) += S_b dps/dx(p):
 *                AVG_DIS x^ / (n_b + 1e-8), AVG_LOG1P x^ / ((1 + d)(n_b + 1e-8)), SQRT_DIS sqrt(pr_scale) x^ / (sqrt(d) n_b), 0 at d = 0,
 *                n_b = n_valid[b] the valid pixels of the scene.  A factor at the 1e-8 clip and MEDIAN_DIS (detached in the reference)
 *                have no scale path: pass n_own = 0 or own_factor = 0 for them.  n_own (host): the number of scenes with own_factor set;
 *                0 skips the reduction launches.
 * Every element of grad_pts, grad_local (iff pr_local) and grad_conf (optional; required by W_CONF) is written exactly once, zeros
 * included; nothing is accumulated across launches and no floating-point atomics are used: the sums of S_b are fp64 in lane / wave /
 * block / slab order, so the gradients are bit-identical from run to run. */
enum { MUST3R_LOSS_W_SCALAR = 0, MUST3R_LOSS_W_MEAN = 1, MUST3R_LOSS_W_CONF = 2, MUST3R_LOSS_W_PIXEL = 3 };
typedef struct must3r_hip_metrics_loss_grad_args {
    const float* w_g;             /* one device scalar, or [B][V][H][W] with W_PIXEL */
    const float* w_l;             /* likewise; required with pr_local */
    int32_t weighting;            /* MUST3R_LOSS_W_* */
    int32_t factor_mode;          /* MUST3R_NORM_* of the scale path; read only when n_own > 0 */
    int32_t n_own;                /* scenes with own_factor set (host copy of the count) */
    int32_t reserved;
    const int64_t* counts;        /* [B][V][2], the forward's output; required by W_MEAN / W_CONF */
    const uint8_t* own_factor;    /* [B]; required when n_own > 0 */
    const int64_t* n_valid;       /* [B]; required when n_own > 0 */
    float* grad_pts;              /* [B][V][H][W][3] */
    float* grad_local;            /* [B][V][H][W][3], required iff pr_local */
    float* grad_conf;             /* [B][V][H][W] or NULL */
} must3r_hip_metrics_loss_grad_args;
size_t must3r_hip_metrics_loss_grad_scratch_bytes(int n_scenes, int n_views, int H, int W);
int must3r_hip_metrics_loss_grad(const must3r_hip_metrics_loss_args* args, const must3r_hip_metrics_loss_grad_args* grad, void* scratch,
                                 size_t scratch_bytes, void* stream);

/* ---- ABI 9: image ingestion -- the reference's three image loaders in front of the forwards ----
 * must3r/demo/inference.py:63-76 load_images: ImgNorm (ToTensor, Normalize(0.5, 0.5)), then get_resize_function
 *   (must3r/tools/image.py:55-97): torchvision CenterCrop + Resize on the fp32 tensor (torchvision >= 0.17: antialiased bilinear)
 *   -> MUST3R_RESAMPLE_AA_BILINEAR = F.interpolate(x[None], size, mode="bilinear", align_corners=False, antialias=True): a triangle
 *   filter of support max(in/out, 1), weights normalised per output pixel, width pass first, fp32 intermediate.
 * must3r/slam/model.py:99-120 preproc_frame (and dust3r's load_images behind must3r/retrieval/model.py:12,49): dust3r _resize_pil_image
 *   (PIL LANCZOS when shrinking, BICUBIC otherwise) on the uint8 frame, an integer crop, then ImgNorm
 *   -> MUST3R_RESAMPLE_PIL_LANCZOS / _BICUBIC: bit-exact with Pillow's Image.resize on RGB uint8: coefficients in double, fixed point
 *   with 22 fractional bits, int32 sums from 1 << 21, clip8 after each pass, horizontal pass over the rows the vertical pass reads.
 * get_resize_function(..., is_mask=True) -> MUST3R_RESAMPLE_NEAREST_EXACT = F.interpolate(mode="nearest-exact").
 * An axis whose size does not change is copied exactly (the replaced libraries skip that pass). */
enum { MUST3R_RESAMPLE_AA_BILINEAR = 0, MUST3R_RESAMPLE_PIL_LANCZOS = 1, MUST3R_RESAMPLE_PIL_BICUBIC = 2, MUST3R_RESAMPLE_NEAREST_EXACT = 3 };
/* source layouts: interleaved uint8 rows (RGB from PIL / a decoder; each byte u enters as the fp32 value (u / 255 - 0.5) / 0.5 of a
 * 256-entry table built on the host), or fp32 planes used as they are (AA_BILINEAR / NEAREST_EXACT only) */
enum { MUST3R_IMG_U8_HWC = 0, MUST3R_IMG_F32_CHW = 1 };

/* Host only (no GPU needed), the coefficients one axis of a call uses: in_size source pixels -> out_size.  *ksize = taps per output
 * (the stride of `weights`); with bounds and weights NULL only *ksize is written.  bounds int32 [out_size][2] = (first source pixel,
 * taps); weights [out_size][ksize]: int32 fixed point (<< 22) for the PIL modes, fp32 otherwise; unused taps are 0. */
int must3r_hip_resample_coeffs(int mode, int in_size, int out_size, int* ksize, int32_t* bounds, void* weights);

/* One image of a resample call.  The source region [crop_y, +crop_h) x [crop_x, +crop_w) is resampled to resize_h x resize_w, and
 * the window [out_y, +out_h) x [out_x, +out_w) of that is written as fp32 planes [channels][out_h][out_w] at out + out_offset.
 * load_images: crop = torchvision's centre crop, resize = the bucket, window = all of it.  preproc_frame: crop = the whole frame,
 * resize = _resize_pil_image's size, window = preproc_frame's crop box. */
typedef struct must3r_hip_image_desc {
    const void* src;          /* DEVICE pointer to pixel (0, 0) of the source (not of the crop) */
    int32_t src_format;       /* MUST3R_IMG_* */
    int32_t channels;         /* 1 ... 4 (3 for RGB) */
    int32_t H, W;             /* source size */
    int64_t row_stride;       /* between source rows: bytes (U8_HWC, >= W * channels) or elements (F32_CHW, >= W) */
    int64_t plane_stride;     /* F32_CHW: elements between channel planes */
    int32_t crop_y, crop_x, crop_h, crop_w;
    int32_t resize_h, resize_w;
    int32_t out_y, out_x, out_h, out_w;
    int64_t out_offset;       /* elements */
} must3r_hip_image_desc;

/* device bytes of scratch a must3r_hip_resample call with these descriptors needs (0 on invalid descriptors): the host-built tables
 * (normalisation table, per-image descriptors, coefficients) and the intermediate of the two passes */
size_t must3r_hip_image_scratch_bytes(int mode, const must3r_hip_image_desc* descs, int n_images);
/* Resamples n_images images (any mix of sizes) with one upload of the tables and ONE launch per pass.  `out` fp32 on the device;
 * `scratch` >= must3r_hip_image_scratch_bytes device bytes, 256-byte aligned; `stream` belongs to the current device.  The descriptor array
 * is read on the host during the call; the tables travel through pinned host slots of the calling thread (a ring of 4, grown on demand,
 * reused once their copy has completed), so the call does not wait for earlier work on the stream; coefficients of recently seen
 * (in, out) sizes are cached per thread.  The sources, `out` and `scratch` must stay valid until the work queued on `stream` has run. */
int must3r_hip_resample(int mode, const must3r_hip_image_desc* descs, int n_images, float* out, void* scratch, size_t scratch_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Operator-level entry points (the same kernels the two forwards are built from), exported so that parity
 * tests and roofline measurements can drive each kernel alone.
 * ------------------------------------------------------------------------------------------------------ */
enum { MUST3R_EPI_STORE16 = 0, MUST3R_EPI_STORE16_GELU = 1, MUST3R_EPI_QKV_ROPE = 2, MUST3R_EPI_RESID_F32 = 3,
       MUST3R_EPI_F32 = 4, MUST3R_EPI_HEAD = 5 };

/* out[M,N] = epi(A[M,K] . W[N,K]^T + bias): nn.Linear (+ fused epilogue).  A, W 16-bit.  N, K multiples of 64; lda % 8 == 0; ldc % 4 == 0
 * (16-bit outputs: ldc % 8 == 0 and a 16-byte aligned `out` -- the epilogue stores 16 bytes per lane). */
int must3r_hip_op_gemm(int dtype, int epi, const void* A, const void* W, const float* bias, void* out,
                       int M, int N, int K, int lda, int ldc,
                       const int64_t* pos, const float* rope_tab, int rope_cols, int rope_npos, /* QKV_ROPE */
                       const float* bias2, int row_start2, int accumulate,                      /* F32 / HEAD */
                       int ntok, int gw, int H, int W_img,                                      /* HEAD */
                       int wsplit, /* 2: W is [N, 2K] = [W_hi | W_lo], out = A W_hi^T + A W_lo^T; else 0 */
                       void* stream);
/* ABI 7 (r05).  Split weights whose LOW part is 2:4-sparse: in every group of 4 consecutive k of a weight row the 2 entries of largest magnitude of
 * W_lo = fp16(W - fp16(W)) are kept, so that the chip-filling kernel multiplies the low part of a 64-deep K-tile with ONE sparse MFMA per output fragment
 * (v_smfmac_f32_16x16x64_f16, twice the dense rate).  The library packs and uses this copy by itself for the split weights of a
 * context (M3R_SPARSE_LO=0: never); these two entry points drive the pair alone (tests, probes).
 *   pack : w fp32 [rows, K] (rows % 32 == 0, K % 64 == 0) -> vals fp16 [K/64][rows][32], idx uint32 [K/64][rows/32][64]
 *   gemm : out = epi(A . (W_hi + sparse W_lo)^T + bias); W2 = the dense [N, 2K] = [W_hi | W_lo] rows (hi half read), fp16 operands; N % 128 == 0, K % 64 == 0;
 *          launches too small to fill the chip with 256 x 128 tiles run the dense two-pass kernels on W2 instead. */
int must3r_hip_op_sparse24_pack(const float* w, int rows, int K, void* vals, void* idx, void* stream);
int must3r_hip_op_gemm_sp(int epi, const void* A, const void* W2, const void* Wlo_sp, const void* Widx_sp, const float* bias, void* out,
                          int M, int N, int K, int lda, int ldc, const int64_t* pos, const float* rope_tab, int rope_cols, int rope_npos, void* stream);
/* "LN fold" (one-view memory update): the LayerNorm between two Linears is applied AFTER the second product instead of before it.
 * Producer role (epi = RESID_F32 / F32): as must3r_hip_op_gemm, and additionally the new fp32 rows rounded to fp16 (x16_out, row stride
 * ldc), an optional fp32 copy (copy32_out) and per row and 16-column fragment (sum x, sum x^2) into stats_out [M][N/16][2].
 * Consumer role (epi = STORE16 / STORE16_GELU / QKV_ROPE; ln_stats != NULL): A = those raw fp16 rows, W2 = split fp16 copy of gamma (.) W,
 * bias = W beta + b, ln_s[n] = sum_k (gamma (.) W)[n][k]; out = epi(rstd_m (A W2^T - mu_m ln_s) + bias) = epi(LN(x) W^T + b).
 * ln_shift [M] (optional): the producer rounds and sums x - ln_shift[m] (an estimate of the row mean: the mean the previous consumer
 * measured), the consumer adds the mean it measures to it (ln_shift_init: the buffer holds nothing yet).
 * must3r/model/blocks/layers.py:91-99 (norm1 -> attn.qkv, norm2 -> cross_attn.projq, norm3 -> mlp.fc1). */
int must3r_hip_op_gemm_lnfold(int dtype, int epi, const void* A, const void* W2, const float* bias, void* out, int M, int N, int K,
                              int lda, int ldc, void* x16_out, float* copy32_out, float* stats_out, const float* ln_stats,
                              const float* ln_s, float ln_eps, float* ln_shift, int ln_shift_init, const int64_t* pos,
                              const float* rope_tab, int rope_cols, int rope_npos, float out_scale, int scale_cols, void* stream);
/* ABI 18.  Every launch form of the LN fold of a one-view update, reachable one by one (tests): the arguments of must3r_hip_op_gemm_lnfold plus what it does not
 * carry -- plain fp16 weights (wsplit = 0: the fc1 consumer, the fc2 and embed producers of MUST3R_F16_WA mode) and bias2 / row_start2 (the embed producer).  Forwards
 * to the launcher must3r_hip_decode uses and adds no arithmetic; `picked` (optional) reports the kernel as must3r_hip_gemm_op does.  must3r_hip_op_gemm_lnfold is unchanged.
 * Refused with an error: another dtype than MUST3R_F16; a wsplit other than 0 / 2; null A, W or out; M < 0; ln_stats (consumer) together with x16_out / copy32_out /
 * stats_out (producer); a consumer without ln_s, bias or ln_shift, on another epilogue than STORE16 / STORE16_GELU / QKV_ROPE, or with K != 768; producer outputs on
 * another epilogue than RESID_F32 / F32; stats_out without x16_out or with N != 768; producer outputs with ldc != N (x16_out, copy32_out and the fragment sums are
 * addressed with out's stride); bias2 on another epilogue than F32, negative row_start2; out_scale on another epilogue than STORE16 / QKV_ROPE or with scale_cols no
 * multiple of 64; and whatever must3r_hip_op_gemm refuses. */
typedef struct must3r_hip_lnfold_op {
    int32_t dtype;                     /* MUST3R_F16 */
    int32_t epi;                       /* MUST3R_EPI_* */
    const void* A; const void* W; const float* bias; void* out;
    int32_t M, N, K, lda, ldc;
    int32_t wsplit;                    /* 2: W is [N, 2K] = [W_hi | W_lo]; 0: plain [N, K] */
    void* x16_out; float* copy32_out; float* stats_out;          /* producer */
    const float* ln_stats; const float* ln_s; float ln_eps;      /* consumer */
    float* ln_shift;
    int32_t ln_shift_init;
    const int64_t* pos; const float* rope_tab;
    int32_t rope_cols, rope_npos;
    float out_scale;
    int32_t scale_cols;
    const float* bias2;
    int32_t row_start2;
    const char** picked;
} must3r_hip_lnfold_op;
int must3r_hip_op_gemm_lnfold_ex(const must3r_hip_lnfold_op* d, void* stream);
/* ABI 8 (r06).  The same fold on the chip-filling 256 x 256 tiles (batched decoder calls, encoder chunks; fp16; the library uses it by itself in MUST3R_F16_WA mode,
 * M3R_LNFOLD256=0: never).  wsplit = 2: W = [N, 2K] split rows + the packed sparse low part (must3r_hip_op_sparse24_pack), epi STORE16 / QKV_ROPE (consumer) or
 * RESID_F32 (producer); wsplit = 0: plain fp16 W [N, K], epi STORE16_GELU (consumer) or RESID_F32 (producer).  N % 256 == 0.
 * Producer: M % 256 == 0; x16_out rows (stride ldc) of x - ln_shift[m], (sum, sum of squares) per row and 64-COLUMN wave tile into stats_out [M][N/64][2], optional
 * copy32_out.  Consumer: ln_stats in that layout ([M][K/64][2]; K = 768 or 1024); ln_shift [M] (required; optional on producers) must hold valid values: += the measured mean. */
int must3r_hip_op_gemm_fold256(int epi, int wsplit, const void* A, const void* W, const void* Wlo_sp, const void* Widx_sp, const float* bias, void* out,
                               int M, int N, int K, int lda, int ldc, void* x16_out, float* copy32_out, float* stats_out, const float* ln_stats,
                               const float* ln_s, float ln_eps, float* ln_shift, const int64_t* pos, const float* rope_tab, int rope_cols, int rope_npos,
                               float out_scale, int scale_cols, void* stream);
/* ABI 17.  Every argument form in which the model launches its GEMMs, reachable one by one (tests): the grouped and per-scene fields of the launch descriptor that
 * must3r_hip_op_gemm / _op_gemm_sp do not carry.  Forwards to the launcher must3r_hip_decode uses; the kernel is the one the default dispatch picks for the shape and
 * is reported through `picked` (optional): "<family>/e<epilogue>/w<1 plain | 2 split | 3 sparse low part>/n<tile width>".  Nothing here changes what
 * must3r_hip_op_gemm does; the LN-fold fields keep their own entry points.
 *   weights: wsplit = 2: W is [N, 2K] = [W_hi | W_lo] (fp16); Wlo_sp / Widx_sp (optional, both or neither, wsplit = 2 only): the packed 2:4-sparse low part of a
 *     parameter of wsp_rows rows (must3r_hip_op_sparse24_pack)
 *   out_scale != 0: columns < scale_cols (a multiple of 64) of a 16-bit store are multiplied by it before rounding (after RoPE)
 *   batch > 1: problem g reads A + g strideA, W + w strideW, bias + w strideB with w = g / wdiv (wdiv > 1) or g, and writes to out_table[g] (DEVICE array of `batch`
 *     pointers; `out` is not used); strides in elements.  The sparse low part of weight group w starts at row w * (strideW / 2K) of the packed parameter.
 *   EPI_F32: bias2 is added on rows m >= row_start2, with row_period2 > 0 on rows (m % row_period2) >= row_start2; accumulate: out += product, no bias
 *   EPI_HEAD: rows are views of ntok tokens on a grid gw wide, written pixel-shuffled into [view][H][Wimg][7]; head_views > 0: the views belong to scenes of
 *     head_views views whose blocks lie head_scene_skip floats further apart than contiguous
 * Refused with an error: out_scale on another epilogue than STORE16 / QKV_ROPE or with scale_cols no multiple of 64; batch > 1 without out_table; wdiv > 1 that does not divide batch (or without batch > 1); row_period2 > 0 without bias2, negative row_start2 /
 * row_period2; head_views / head_scene_skip on another epilogue than EPI_HEAD, negative, or head_scene_skip % 4 != 0; one of Wlo_sp / Widx_sp alone, or without wsplit = 2;
 * wsp_rows smaller than the rows the weight groups index or not a multiple of 32; negative batch, wdiv or strides; and whatever must3r_hip_op_gemm refuses. */
typedef struct must3r_hip_gemm_op {
    int32_t dtype;                     /* MUST3R_BF16 / MUST3R_F16 */
    int32_t epi;                       /* MUST3R_EPI_* */
    const void* A; const void* W; const float* bias; void* out;
    int32_t M, N, K, lda, ldc;
    int32_t wsplit;                    /* 2: split weights, else 0 */
    const void* Wlo_sp; const void* Widx_sp;
    int32_t wsp_rows;
    float out_scale;
    int32_t scale_cols;
    int32_t batch;                     /* 0 / 1: one problem */
    int64_t strideA, strideW, strideB;
    void* const* out_table;
    int32_t wdiv;
    const int64_t* pos; const float* rope_tab;
    int32_t rope_cols, rope_npos;
    const float* bias2;
    int32_t row_start2, row_period2, accumulate;
    int32_t ntok, gw, H, Wimg;
    int32_t head_views;
    int64_t head_scene_skip;
    const char** picked;
} must3r_hip_gemm_op;
int must3r_hip_op_gemm_ex(const must3r_hip_gemm_op* d, void* stream);
/* cos/sin table fp32 [npos][16][2] for RoPE2D(freq, F0) with head dim 64 (host pointer) */
int must3r_hip_rope_table(float freq, float f0, int npos, float* out_host);

/* softmax(Q K^T / 8) V per head of 64; views: int32 [n_views][6] = q_row0, nq, kv_row0, nk, skip_lo, skip_hi
 * (DEVICE pointer).  Q/K/V/O 16-bit with row strides in elements (dtype | MUST3R_ATTN_FP8: Q/K e4m3 bytes with ldq/ldk in bytes, V/O 16-bit).
 * A view's K / V rows must span less than 2 GiB (nk * ld * element size): the staging uses 32-bit byte offsets.
 * nsplit > 1 selects split-KV (flash-decoding) with `scratch` of must3r_hip_attention_scratch_bytes() bytes and
 * total_q_rows = max(q_row0 + nq); nsplit <= 1 needs neither. */
size_t must3r_hip_attention_scratch_bytes(int nsplit, int total_q_rows, int heads);
int must3r_hip_op_attention(int dtype, const void* Q, const void* K, const void* V, void* O,
                            int ldq, int ldk, int ldv, int ldo, int heads,
                            const int32_t* views_dev, int n_views, int max_nq,
                            int nsplit, void* scratch, int total_q_rows, void* stream);
/* ABI 10.  The attention routes the decoder launches, reachable one by one (tests): every field of the launch the decoder sets, and the context-parallel
 * stages.  Forwards to the same launchers as must3r_hip_decode; nothing here changes what must3r_hip_op_attention does.
 *   stage 0: the plain launch -- (m, l) pre-fill (split-KV without dense_rows only), main kernel, combine (split-KV only) -> O
 *   stage 1: one rank's partial -- pre-fill (as stage 0), main kernel, merge of the nsplit (>= 2) local splits into slot_o / slot_ml (p16: O / l in the 16-bit type)
 *   stage 2: the partial of a rank without keys: O = 0, (m, l) = (-inf, 0) for total_q_rows rows -> slot_o / slot_ml
 *   stage 3: the final merge of nslots partials at slot_o + s * stride_o (elements of the partial's O type) / slot_ml + s * stride_ml (floats) -> O
 * Layouts of a partial: O [total_q_rows][heads * 64] (fp32, or the 16-bit type with p16), (m, l) [total_q_rows][heads][2] fp32.
 * A query row whose view has no valid key (nk = 0, or every key excluded) gets O = 0 on every route.  With split-KV, dense_rows = 1 promises that every row
 * below total_q_rows belongs to a view of the launch (no pre-fill); without it, rows outside every view are left untouched.  `picked` (optional) receives
 * the main kernel stages 0 and 1 ran ("attn3/q16", "attn3/q32"); stages 2 and 3 leave it alone. */
typedef struct must3r_hip_attn_op {
    int32_t dtype;                     /* MUST3R_BF16 / MUST3R_F16 */
    const void* Q; const void* K; const void* V; void* O;
    int32_t ldq, ldk, ldv, ldo;        /* row strides in elements */
    int32_t heads;
    const int32_t* views_dev;          /* DEVICE int32 [n_views][6] as must3r_hip_op_attention */
    int32_t n_views;
    int32_t view0_inline;              /* 1: n_views must be 1 and the view is `view0` (views_dev is not read) */
    int32_t view0[6];
    int32_t max_nq, max_nk;            /* max over views of nq / nk (max_nk 0: unknown) */
    int32_t q_prescaled;               /* 1: Q carries 1/8 * log2(e) already (the decoder's projections fold it in); 0: the kernel scales */
    int32_t nsplit;                    /* <= 1: single pass */
    void* scratch;                     /* must3r_hip_attention_scratch_bytes(nsplit, total_q_rows, heads) bytes when nsplit > 1 */
    int32_t total_q_rows, dense_rows;
    int32_t stage;                     /* 0 .. 3 above */
    void* slot_o; float* slot_ml;      /* stage 1 / 2: the output partial; stage 3: slot 0 */
    int32_t p16, nslots;
    int64_t stride_o, stride_ml;       /* stage 3 */
    const char** picked;
} must3r_hip_attn_op;
int must3r_hip_op_attention_ex(const must3r_hip_attn_op* d, void* stream);

/* y = LN(x (+ add)) * w + b over rows of C; optional outputs may be NULL */
int must3r_hip_op_layernorm(int dtype, const float* x, const float* add, const float* w, const float* b,
                            void* out16, void* out16_lo, float* out32, float* copy32, int M, int C, float eps,
                            void* stream);
/* ABI 15.  Every LayerNorm launch form the model uses, reachable one by one (tests): the fields of the launch descriptor one for one.  Forwards to the
 * launcher must3r_hip_decode uses; the kernel is chosen as there (one row per wave below 65536 rows or with LN_ROWS = 0, row-walking waves otherwise)
 * and reported through `picked` (optional): "ln", "ln_rows/3" (C <= 768), "ln_rows/4".  Nothing here changes what must3r_hip_op_layernorm does.
 *   input: exactly one of x (fp32) / x16 (16-bit) [M][C]; add (optional, fp32) is added before the statistics
 *   outputs, all optional: out16 / out16_lo (= T(y - float(T(y)))) / out16_dup (= out16) with row stride ld16 (0 = C); out32; copy32 = x + add (fp32);
 *     raw16 = T(x + add), fp16 saturated at +-65504.  The three out16* need out16.
 *     mean_out [M] (ABI 18): the row means of x + add the statistics used (the LN fold's first shift); such a launch always runs the one-row-per-wave kernel.
 *   rows_per_group > 0: row r is of group g = r / rows_per_group and uses w + g C, b + g C; add is [rows_per_group][C] and applied to groups < add_groups.
 * Refused with an error: both or neither of x / x16, null w / b, ld16 non-zero and < C or not a multiple of 4, negative add_groups / rows_per_group,
 * C > 1024 or not a multiple of 4. */
typedef struct must3r_hip_ln_op {
    int32_t dtype;                     /* MUST3R_BF16 / MUST3R_F16 */
    const float* x; const void* x16; const float* add; const float* w; const float* b;
    void* out16; void* out16_lo; void* out16_dup;
    int32_t ld16;
    float* out32; float* copy32; void* raw16;
    int32_t M, C;
    float eps;
    int32_t rows_per_group, add_groups;
    const char** picked;
    float* mean_out;                   /* ABI 18 */
} must3r_hip_ln_op;
int must3r_hip_op_layernorm_ex(const must3r_hip_ln_op* d, void* stream);
int must3r_hip_op_im2col(int dtype, const float* img, void* out16, int n_views, int H, int W, void* stream);
int must3r_hip_op_cast(int dtype, const float* in, void* out16, void* out16_lo, size_t n, void* stream);

/* ABI 19.  Training forward and backward of the prediction head (decoder.py:149-156, blocks/head.py:63-72, tools/image.py:9-14), stateless:
 *   x fp32 [R][D], R = n_views N, N = (H/16)(Wimg/16);  gamma, beta [D];  W [O][D], b [O], O = 7 * 256 (the reference's row order c 256 + i 16 + j)
 *   y = (x - mu) rstd gamma + beta;  z = y W^T + b;  pointmaps[v][16 gy + i][16 gx + j][c] = z[v N + gy gw + gx][c 256 + i 16 + j]     fp32 [n_views][H][Wimg][7]
 * must3r_hip_head_forward runs the two launches must3r_hip_decode runs for its head (split-precision 16-bit operands, fp32-equivalent), on operands packed from
 * the fp32 parameters on every call (weights change between training steps; nothing is cached).  dtype: MUST3R_BF16 / MUST3R_F16.
 * must3r_hip_op_head_linear is its Linear stage alone, from the fp32 y (the post-LayerNorm tensor return_feats hands out).
 *
 * must3r_hip_head_grad: from G = dL/dpointmaps fp32 [n_views][H][Wimg][7], with dZ[r][c 256 + i 16 + j] = G[v][16 gy + i][16 gx + j][c] (never materialised):
 *   db[o] = sum_r dZ[r][o]                  dW[o][k] = gamma[k] sum_r dZ[r][o] x^[r][k] + beta[k] db[o]            x^ = (x - mu) rstd
 *   dY = dZ W                               dgamma[k] = sum_r dY[r][k] x^[r][k]       dbeta[k] = sum_r dY[r][k]
 *   g^ = dY gamma                           dx = rstd (g^ - mean_k(g^) - x^ mean_k(g^ x^))
 * fp32 operands on v_mfma_f32_16x16x4_f32 (exact products, k-ordered fmaf chain); (mu, rstd) are recomputed from x, the forward saves nothing.  The weight
 * gradient splits its sum over the rows across must3r_hip_head_grad_splits(R) blocks -- a function of R alone -- and adds the partials in split order; no atomics
 * anywhere: repeated calls agree bit for bit, and a row of dx does not depend on which other rows the call holds.
 * Every output may be NULL and then costs nothing: without dW and db no weight-gradient launch, without dx no data-gradient launch and no LayerNorm backward.
 * dY lives in the dx buffer, so dgamma / dbeta need dx (refused otherwise).  An output that is not asked for is not written.
 * Refused with an error: null required pointers, H or Wimg not multiples of 16, D not a multiple of 64 or above 1024, pointers not 16-byte aligned, scratch smaller
 * than must3r_hip_head_grad_scratch_bytes (row statistics, the permuted W, the split partials, the LayerNorm column partials; returns 0 on a bad shape). */
typedef struct must3r_hip_head_grad_args {
    const float* x; const float* gamma; const float* beta; const float* W; const float* G;
    int32_t n_views, H, Wimg, D;
    float eps;
    int32_t reserved;
    float* dx; float* dgamma; float* dbeta; float* dW; float* db;
} must3r_hip_head_grad_args;
int must3r_hip_head_grad_splits(int rows);
size_t must3r_hip_head_forward_scratch_bytes(int n_views, int H, int Wimg, int D);
int must3r_hip_head_forward(int dtype, const float* x, const float* gamma, const float* beta, const float* W, const float* b, int n_views, int H, int Wimg, int D,
                            float eps, float* pointmaps, void* scratch, size_t scratch_bytes, void* stream);
int must3r_hip_op_head_linear(int dtype, const float* y, const float* W, const float* b, int n_views, int H, int Wimg, int D, float* pointmaps, void* scratch,
                              size_t scratch_bytes, void* stream);
size_t must3r_hip_head_grad_scratch_bytes(int n_views, int H, int Wimg, int D);
int must3r_hip_head_grad(const must3r_hip_head_grad_args* a, void* scratch, size_t scratch_bytes, void* stream);
/* ABI 21, additive.  The head over a batch stored landscape (H <= Wimg) whose views may be portrait: the reference's transpose_to_landscape(head,
 * activate=True) (blocks/head.py:24-60), with the orientation per view from a DEVICE array in the dtype and meaning of must3r_hip_patch_rows_args.transposed
 * (int32 [n_views], non-zero = portrait), so that one tensor serves both calls and the host never learns the flags.  With gh = H/16, gw = Wimg/16:
 *   landscape view   token t = gy gw + gx   pointmaps[v][16 gy + i][16 gx + j][c] = z[v N + t][c 256 + i 16 + j]           as must3r_hip_head_forward
 *   portrait view    token t = py gh + px   pointmaps[v][16 px + j][16 py + i][c] = z[v N + t][c 256 + i 16 + j]           head(x, (Wimg, H)).swapaxes(1, 2)
 * The backward is the adjoint: G is read through the same per-view map, dx follows the view's rows, dW / db / dgamma / dbeta sum over all views.
 * Forward: the two launches of must3r_hip_head_forward write every view in place with the landscape geometry; then the 16 x 16 x 7 tiles of the flagged views
 * are turned through LDS into the scratch and copied back (two launches whose blocks return at once in an unflagged view: those views pay no second pass, a
 * flagged view's pixels are read and written twice more).  Backward: one launch turns the flagged views' tiles of G into the scratch in the slot order of their
 * tokens, and the gather kernels of must3r_hip_head_grad take each row from G or from there by its view's flag -- the same 448-byte runs, the same k-ordered
 * chain, the same split rule (the row count alone) and reduces; a 128-row tile may hold views of both kinds.  No atomics, one writer per element; repeated
 * calls agree bit for bit.  transposed == NULL: exactly must3r_hip_head_forward / must3r_hip_head_grad, launch for launch.
 * The descriptors embed the existing arguments plus the flag pointer and the stream (a hipStream_t: all work goes to it, nothing waits on the host).
 * scratch: at least must3r_hip_head_*_many_ar_scratch_bytes -- the plain entry point's plus one copy of the pointmaps (0 on a bad shape), 16-byte aligned.
 * Refused with an error before anything is launched: what the plain entry points refuse, H > Wimg with flags, transposed not 4-byte aligned. */
typedef struct must3r_hip_head_forward_ar_args {
    const float* x; const float* gamma; const float* beta; const float* W; const float* b;
    int32_t dtype, n_views, H, Wimg, D;
    float eps;
    float* pointmaps;             /* [n_views, H, Wimg, 7] */
    const int32_t* transposed;    /* [n_views] on the device, optional */
    void* stream;                 /* hipStream_t */
} must3r_hip_head_forward_ar_args;
typedef struct must3r_hip_head_grad_ar_args {
    must3r_hip_head_grad_args g;
    const int32_t* transposed;    /* [n_views] on the device, optional */
    void* stream;                 /* hipStream_t */
} must3r_hip_head_grad_ar_args;
size_t must3r_hip_head_forward_many_ar_scratch_bytes(int n_views, int H, int Wimg, int D);
int must3r_hip_head_forward_many_ar(const must3r_hip_head_forward_ar_args* a, void* scratch, size_t scratch_bytes);
size_t must3r_hip_head_grad_many_ar_scratch_bytes(int n_views, int H, int Wimg, int D);
int must3r_hip_head_grad_many_ar(const must3r_hip_head_grad_ar_args* a, void* scratch, size_t scratch_bytes);
/* the backward kernels one by one, in the plain forms a later Linear / LayerNorm backward calls (fp32, row-major):
 *   linear_dgrad_f32:  out[M][K] = dZ[M][O] (row stride ldz) W[O][K];  O % 16 == 0, K % 4 == 0, ldz % 4 == 0
 *   linear_wgrad_f32:  dW[O][K] = sum_r dZ[r][o] A[r][k] (row strides ldz, lda), db[O] = sum_r dZ[r][o]; either may be NULL; O, K, ldz, lda multiples of 4
 *   layernorm_grad:    dx [M][D] (may alias dy), dgamma [D], dbeta [D] of y = LN(x) gamma + beta from dy; each may be NULL; D % 64 == 0, D <= 1024 */
int must3r_hip_op_linear_dgrad_f32(const float* dZ, int ldz, const float* W, float* out, int M, int O, int K, void* stream);
size_t must3r_hip_op_linear_wgrad_scratch_bytes(int M, int O, int K);
int must3r_hip_op_linear_wgrad_f32(const float* dZ, int ldz, const float* A, int lda, float* dW, float* db, int M, int O, int K, void* scratch,
                                   size_t scratch_bytes, void* stream);
size_t must3r_hip_op_layernorm_grad_scratch_bytes(int M, int D);
int must3r_hip_op_layernorm_grad(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, int M, int D, float eps,
                                 void* scratch, size_t scratch_bytes, void* stream);

/* ABI 20.  Training forward and backward of the attention core, softmax(Q K^T / 8) V per head of 64 (blocks/attention.py CoreAttention.attention), stateless, fp32
 * operands on v_mfma_f32_16x16x4_f32.  The views are the table of must3r_hip_op_attention, int32 [n_views][6] = q_row0, nq, kv_row0, nk, skip_lo, skip_hi, but given
 * as a HOST pointer: the entry points group the views on the host and upload what the kernels read into the scratch buffer.  Per head, s = 1/8, key j of a view
 * valid when j < nk and j is not in [skip_lo, skip_hi):
 *   S_ij = s q_i.k_j      lse_i = log sum_valid exp(S_ij)      P_ij = exp(S_ij - lse_i)  (0 where invalid)
 *   O_i  = sum_j P_ij v_j                 delta_i = dO_i . O_i
 *   dV_j = sum_i P_ij dO_i                dP_ij = dO_i . v_j            dS_ij = P_ij (dP_ij - delta_i)
 *   dQ_i = s sum_j dS_ij k_j              dK_j  = s sum_i dS_ij q_i
 * A query row without a valid key has O = 0 (lse = -inf), gives nothing to dK / dV and has dQ = 0.  q, k, v, dO, O, dQ, dK, dV are fp32 with a row stride in
 * elements each (at least heads * 64, a multiple of 4), so that q, k and v may be the column blocks of one packed [R][3 D] tensor; lse is [rows][heads].
 * must3r_hip_attn_forward_f32 writes O (required) and lse (optional).  must3r_hip_attn_grad needs dO and writes whichever of dQ, dK, dV are non-NULL: it runs
 * the forward kernel once more (row statistics and delta into scratch; O is never stored), then one launch for dK and dV (skipped when neither is asked for) and one
 * for dQ (skipped without dQ).  An output that is not asked for is not written.
 * Key groups: dK and dV sum over every view that reads a key row.  The views are partitioned by kv_row0; a group spans rows [kv_row0, kv_row0 + max nk) and one
 * block per (group, head, 64-row tile) adds the views' contributions in the order of the table -- no atomics, repeated calls agree bit for bit, and a group's
 * result does not depend on the other groups of the call.  Views that share key rows must therefore share kv_row0 (the decoder's cross attention does, causal
 * prefixes included: one group per scene); two groups whose spans overlap are refused.  Rows of dK / dV outside every group's span and rows of dQ outside every view
 * are not written; a key row inside a span that no view attends gets zeros.  must3r_hip_attn_train_groups returns the number of groups of a table, or -1 with an
 * error where must3r_hip_attn_grad would refuse it (no device needed).
 * Scratch (must3r_hip_attn_train_scratch_bytes; total_q_rows = max(q_row0 + nq), total_kv_rows = max(kv_row0 + nk); 0 on a bad shape; no device needed):
 * [views | groups | per-group view lists | lse (log2 domain) rows x heads | delta rows x heads].
 * Refused with an error: null required pointers, heads <= 0, a leading dimension below heads * 64 or not a multiple of 4, pointers not 16-byte aligned, negative
 * table entries, skip_lo > skip_hi or skip_hi > nk, more than 65535 views, overlapping groups (attn_grad), scratch too small. */
typedef struct must3r_hip_attn_train_args {
    const float* q; const float* k; const float* v; const float* dO;   /* dO: must3r_hip_attn_grad only */
    int32_t ldq, ldk, ldv, lddo;
    int32_t heads, n_views;
    const int32_t* views;              /* HOST int32 [n_views][6] */
    float* O; float* lse;              /* must3r_hip_attn_forward_f32 */
    float* dQ; float* dK; float* dV;   /* must3r_hip_attn_grad, each optional */
    int32_t ldo, lddq, lddk, lddv;
} must3r_hip_attn_train_args;
size_t must3r_hip_attn_train_scratch_bytes(int n_views, int total_q_rows, int total_kv_rows, int heads);
int must3r_hip_attn_train_groups(const int32_t* views_host, int n_views);
int must3r_hip_attn_forward_f32(const must3r_hip_attn_train_args* a, void* scratch, size_t scratch_bytes, void* stream);
int must3r_hip_attn_grad(const must3r_hip_attn_train_args* a, void* scratch, size_t scratch_bytes, void* stream);

/* ABI 21, additive.  Key masks in the attention core of ABI 20 (memory dropout: the random subset of memory rows the reference's training class hides from a view,
 * decoder.py:388-433, blocks/dropout.py).  The descriptor embeds the ABI 20 one as its first member; besides the prefix nk and the interval [skip_lo, skip_hi) a
 * view may name one row of a packed bit matrix:
 *   key j of a view is valid when j < nk, j is not in [skip_lo, skip_hi) and, if view_mask[view] = r >= 0, bit j % 32 of word mask_bits[r][j / 32] is 1.
 * Everything else is ABI 20: the formulas, the key groups, the order of additions, and the rule for a query row without a valid key (O = 0, lse = -inf, nothing
 * into dK / dV, dQ = 0).  mask_bits is a DEVICE array uint32 [mask_rows][mask_ld], 8-byte aligned, mask_ld even (the 64 bits of a key tile are one aligned 8-byte
 * load) with 32 mask_ld >= nk for every view that names a row; bits at or past a view's nk are ignored.  view_mask is a HOST array int32 [core.n_views], -1: no
 * mask; it is uploaded with the view table, in the same copy through the same pinned ring.  Rows are shared freely among views, scenes and heads (the reference
 * draws one mask per view position of a call and uses it for every scene, layer and head), so mask_rows is about the number of views of a call.
 * A (view, key tile) pair whose 64 bits are all zero is skipped like a tile wholly inside the skip range: no K / V tile is fetched for it in the forward and the dQ
 * walk, no Q / dO tile in the dK / dV walk.  The masked kernels are separate instantiations; mask_bits == NULL with view_mask == NULL launches the unmasked ones,
 * the bits of must3r_hip_attn_forward_f32 / must3r_hip_attn_grad.  The stream travels in the descriptor (`stream`, a hipStream_t): all work goes to it, the
 * uploaded tables included, and no call waits for it on the host.  No atomics; repeated calls agree bit for bit.
 * Scratch (must3r_hip_attn_masked_scratch_bytes; no device needed; 0 on a bad shape): that of ABI 20 plus n_views int32 rounded up to 256 bytes, placed behind
 * the view lists: [views | groups | per-group view lists | mask rows | lse | delta].  It is enough for a call without masks too.
 * Refused with an error before anything is read or launched: everything the ABI 20 calls refuse; mask_bits without view_mask or the reverse; mask_ld odd or <= 0;
 * mask_rows < 0; a view_mask entry outside [-1, mask_rows); 32 mask_ld below the nk of a view that names a row; mask_bits not 8-byte aligned. */
typedef struct must3r_hip_attn_masked_args {
    must3r_hip_attn_train_args core;
    const uint32_t* mask_bits;         /* DEVICE uint32 [mask_rows][mask_ld] */
    const int32_t* view_mask;          /* HOST int32 [core.n_views], -1: none */
    int32_t mask_rows, mask_ld;
    void* stream;                      /* hipStream_t */
} must3r_hip_attn_masked_args;
size_t must3r_hip_attn_masked_scratch_bytes(int n_views, int total_q_rows, int total_kv_rows, int heads);
int must3r_hip_attn_masked_forward(const must3r_hip_attn_masked_args* a, void* scratch, size_t scratch_bytes);
int must3r_hip_attn_masked_grad(const must3r_hip_attn_masked_args* a, void* scratch, size_t scratch_bytes);

/* ABI 21.  Training forward and backward of the two residual sublayers of the reference's Block (blocks/layers.py:36-54; also two of the three sublayers of
 * CachedDecoderBlock), fp32, stateless, no atomics: repeated calls agree bit for bit and a row of a row-wise output does not depend on the other rows of the call.
 *   MLP sublayer        y^ = LN(x) gamma + beta;  z = y^ W1^T + b1;  h = gelu(z);  out = x + h W2^T + b2                        W1 [hidden][D], W2 [D][hidden]
 *   attention sublayer  y^ = LN(x) gamma + beta;  qkv = y^ Wqkv^T + bqkv  [M][3 D] = q | k | v;  q, k rotated by RoPE2D;
 *                       o = softmax(q k^T / 8) v per head of 64 and view (ABI 20);  out = x + o Wproj^T + bproj                 Wqkv [3 D][D], Wproj [D][D]
 *   gelu(z) = z Phi(z),  gelu'(z) = Phi(z) + z phi(z),  Phi(z) = erfc(-z / sqrt 2) / 2 (the negative tail is a product, not a cancellation),
 *   phi(z) = exp(-z^2 / 2) / sqrt(2 pi); both finite for every finite z, gelu' exactly 1 / 0 for z >= 40 / z <= -40.
 *   RoPE2D (croco), per head of 64: columns [0, 32) rotate with pos[r][0], [32, 64) with pos[r][1]; the pairs are (i, i + 16), i < 16, with the angle
 *   pos * f0 * freq^(-i / 16): a' = a cos - b sin, b' = b cos + a sin.  direction -1 is the transposed rotation (sin -> -sin), which is the backward.
 * The operator forms (row-major fp32, leading dimensions in elements):
 *   op_linear_f32      out[M][N] (ldc) = A[M][K] (lda) W[N][K]^T + bias[N] (bias may be NULL) on v_mfma_f32_16x16x4_f32, 128 x 128 x 16 tiles; epi:
 *                        MUST3R_LIN_BIAS; MUST3R_LIN_BIAS_RES: out = res (ldres; may alias out) + that; MUST3R_LIN_BIAS_GELU: out = gelu(z), and zout (ldz) = z
 *                        where zout is given.  Refused: K % 16, N % 4, a leading dimension % 4 or shorter than its row, pointers not 16-byte aligned.
 *   op_layernorm_f32   y[M][D] = (x - mu) rstd gamma + beta, D % 64 == 0, D <= 1024, 16-byte aligned pointers; two-pass statistics of its own (the backward's
 *                        recomputed statistics use the same formulas in another summation order)
 *   op_gelu_f32        g[n] = gelu(z[n]), dg[n] = gelu'(z[n]); either output may be NULL
 *   op_gelu_grad_f32   dz[M][N] (lddz) = dh (ldh) gelu'(z (ldz)); N and the leading dimensions % 4, 16-byte aligned; dz may alias dh
 *   op_rope_f32        rotates the first rope_cols (a multiple of 64) columns of t[R][ld] in place; pos int64 [R][2] and rope_tab, the table of
 *                        must3r_hip_rope_table ([rope_npos][16][2]), are DEVICE pointers.  The caller guarantees 0 <= pos < rope_npos (the kernel clamps, it
 *                        never reads outside the table).  direction +1 / -1.
 *   op_layernorm_grad_add   must3r_hip_op_layernorm_grad with dx = add + (the LayerNorm backward); add [M][D] may be NULL (then it is that entry point) and
 *                        may alias dx.  A template flag of the same kernel: the entry points without add keep their bits.
 * The sublayer entry points.  The forward saves nothing; *_grad recomputes the sublayer's forward into scratch and differentiates it.  Every gradient output may be
 * NULL, costs nothing then and is not written: no dW and db of a Linear, no weight-gradient launch (db of the last Linear alone: its column sums of dy and no forward); no dx, dgamma and dbeta, no data gradient of the first Linear
 * and no LayerNorm backward; no dgamma and dbeta, no column sums.  dx = dy + (the gradient through the branch).
 *   mlp_sublayer_grad   y^, (z -> S1, h -> S2), [dW2, db2 = wgrad(dy, h)], dh = dgrad(dy, W2) -> S2, dz = dh gelu'(z) in place, [dW1, db1 = wgrad(dz, y^)],
 *                       dy^ = dgrad(dz, W1) over y^, layernorm_grad_add(x, dy^, add = dy).
 *   attn_sublayer_grad  y^, qkv (rotated), o = attn_forward_f32, [dWproj, dbproj = wgrad(dy, o)], do = dgrad(dy, Wproj), dqkv = attn_grad (q, k, v and dQ, dK, dV
 *                       the column blocks of the packed tensors), the transposed rotation of dq | dk, [dWqkv, dbqkv = wgrad(dqkv, y^)], dy^ = dgrad(dqkv, Wqkv)
 *                       over y^, layernorm_grad_add(x, dy^, add = dy).
 * Shapes: D % 64 == 0, D <= 1024 (the LayerNorm backward's limit), heads = D / 64, hidden % 16 == 0.  views: the HOST table of ABI 20, int32 [n_views][6], inside
 * the M rows (queries and keys are rows of the same tensor); ragged tables are fine, a row of no view attends nothing (o = 0, so out = x + bproj), overlapping key
 * groups are refused by attn_sublayer_grad as by must3r_hip_attn_grad.
 * Scratch, each part rounded up to 256 bytes, in this order (no device needed; 0 on a bad shape; rows are not chunked):
 *   mlp_sublayer_scratch_bytes(M, D, hidden)  = 4 M D + 2 * 4 M hidden + max(op_linear_wgrad_scratch_bytes(M, D, hidden), (M, hidden, D))
 *                                               + op_layernorm_grad_scratch_bytes(M, D)                       [y^ | S1 | S2 | partials | LayerNorm]
 *   attn_sublayer_scratch_bytes(M, D, n_views) = 4 M D + 12 M D + 4 M D + 4 M D + 12 M D + max(op_linear_wgrad_scratch_bytes(M, 3 D, D), (M, D, D))
 *                                               + op_layernorm_grad_scratch_bytes(M, D) + attn_train_scratch_bytes(n_views, M, M, D / 64)
 *                                                                                  [y^ | qkv | o | do | dqkv | partials | LayerNorm | attention core]
 * The forward entry points take the same scratch (they use its first parts).
 * Refused with an error: null required pointers, M <= 0, D not a multiple of 64 or above 1024, hidden not a multiple of 16, pointers not 16-byte aligned, a table
 * with negative entries or reaching past M, overlapping key groups (grad), rope_npos <= 0, scratch NULL, misaligned or too small. */
#define MUST3R_LIN_BIAS 0
#define MUST3R_LIN_BIAS_RES 1
#define MUST3R_LIN_BIAS_GELU 2
typedef struct must3r_hip_mlp_sublayer_args {
    const float* x; const float* gamma; const float* beta; const float* W1; const float* b1; const float* W2; const float* b2;
    const float* dy;                   /* *_grad only */
    int32_t M, D, hidden;
    float eps;
    float* out;                        /* *_forward only */
    float* dx; float* dgamma; float* dbeta; float* dW1; float* db1; float* dW2; float* db2;   /* *_grad, each optional */
} must3r_hip_mlp_sublayer_args;
typedef struct must3r_hip_attn_sublayer_args {
    const float* x; const float* gamma; const float* beta; const float* Wqkv; const float* bqkv; const float* Wproj; const float* bproj;
    const float* dy;                   /* *_grad only */
    const int64_t* pos;                /* DEVICE int64 [M][2] */
    const float* rope_tab;             /* DEVICE fp32 [rope_npos][16][2] */
    const int32_t* views;              /* HOST int32 [n_views][6] */
    int32_t M, D, n_views, rope_npos;
    float eps;
    int32_t reserved;
    float* out;                        /* *_forward only */
    float* dx; float* dgamma; float* dbeta; float* dWqkv; float* dbqkv; float* dWproj; float* dbproj;   /* *_grad, each optional */
} must3r_hip_attn_sublayer_args;
int must3r_hip_op_linear_f32(int epi, const float* A, int lda, const float* W, const float* bias, const float* res, int ldres, float* out, int ldc, float* zout,
                             int ldz, int M, int N, int K, void* stream);
int must3r_hip_op_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int M, int D, float eps, void* stream);
int must3r_hip_op_gelu_f32(const float* z, float* g, float* dg, long long n, void* stream);
int must3r_hip_op_gelu_grad_f32(const float* dh, int ldh, const float* z, int ldz, float* dz, int lddz, int M, int N, void* stream);
int must3r_hip_op_rope_f32(float* t, int ld, const int64_t* pos, const float* rope_tab, int rope_npos, int R, int rope_cols, int direction, void* stream);
int must3r_hip_op_layernorm_grad_add(const float* x, const float* gamma, const float* dy, const float* add, float* dx, float* dgamma, float* dbeta, int M, int D,
                                     float eps, void* scratch, size_t scratch_bytes, void* stream);
size_t must3r_hip_mlp_sublayer_scratch_bytes(int M, int D, int hidden);
int must3r_hip_mlp_sublayer_forward(const must3r_hip_mlp_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream);
int must3r_hip_mlp_sublayer_grad(const must3r_hip_mlp_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream);
size_t must3r_hip_attn_sublayer_scratch_bytes(int M, int D, int n_views);
int must3r_hip_attn_sublayer_forward(const must3r_hip_attn_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream);
int must3r_hip_attn_sublayer_grad(const must3r_hip_attn_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream);

/* ABI 21, additive.  Training forward and backward of the third residual sublayer of the reference's CachedDecoderBlock (blocks/layers.py:90-99,
 * CachedCrossAttention blocks/attention.py:129-149): the cross attention of the tokens x over the token memory.  fp32, stateless, composed like
 * must3r_hip_attn_sublayer_* from the operator forms above; no atomics.
 *   y^ = LN(x) gamma + beta                               x [M][D]
 *   q  = y^ Wq^T + bq                                     no RoPE: the reference builds cross_attn with pos_embed=None
 *   k | v = mem Wk^T + bk | mem Wv^T + bv                 mem [Rm][ldmem], projected ONCE per memory row into one packed [Rm][2 D] tensor
 *   o  = softmax(q k^T / 8) v per head of 64 and view     ABI 20; views = HOST int32 [n_views][6]: the q rows index x, the kv rows index mem
 *   out = x + o Wproj^T + bproj
 * Wk == NULL (then bk, Wv, bv and their gradients are NULL too) is the reference's `kv` memory mode: mem is [Rm][ldmem >= 2 D] and already holds k | v, nothing
 * is projected.  Otherwise ldmem >= D.  Leading dimensions are multiples of 4; D % 64 == 0, D <= 1024, heads = D / 64; pointers 16-byte aligned; biases may be NULL.
 * The stream travels in the descriptor (`stream`, a hipStream_t): all work goes to it, the uploaded view tables included, and no call waits for it on the host.
 * The forward saves nothing; cross_sublayer_grad recomputes the forward into scratch and differentiates it:
 *   y^, q, k | v, [o = attn_forward_f32, dWproj, dbproj = wgrad(dy, o)], do = dgrad(dy, Wproj), (dq, dk | dv) = attn_grad, [dWk, dbk = wgrad(dk, mem)],
 *   [dWv, dbv = wgrad(dv, mem)], [dmem = dk Wk + dv Wv: ONE launch of the data-gradient kernel whose weight operand is the two row blocks Wk, Wv -- one k-ordered
 *   accumulator chain per element, the bits of must3r_hip_op_linear_dgrad_f32 on a packed [2 D][D] copy of Wk over Wv, no such copy and no read-modify-write of
 *   dmem], [dWq, dbq = wgrad(dq, y^)], dy^ = dgrad(dq, Wq) over y^, layernorm_grad_add(x, dy^, add = dy).
 * In the `kv` mode dmem = dK | dV is written by the attention backward straight into the caller's buffer (lddk = lddv = lddmem).
 * Every gradient output may be NULL, costs nothing then and is not written: none of dmem, dWk, dbk, dWv, dbv, no dK / dV launch; none of dx, dgamma, dbeta, dWq, dbq,
 * no dQ launch, no data gradient through Wq and no LayerNorm backward; no dW and db of a Linear, no weight-gradient launch for it; dbproj alone, the column sums of
 * dy and no recomputed forward.  dx = dy + (the gradient through the branch).
 * Coverage: a row of x that belongs to no view has o = 0 (out = x + bproj, dx = dy).  Memory rows outside every key group's span take exact zeros in the packed
 * dK | dV (zeroed on the caller's stream when the spans do not cover [0, Rm)), so that dmem is written completely and dWk, dWv never see unwritten scratch.
 * Determinism: repeated calls agree bit for bit; a view's rows of out / dx and a scene's rows of dmem are the same bits alone and in a batch.  Overlapping key groups
 * are refused by cross_sublayer_grad as by must3r_hip_attn_grad.
 * Scratch (no device needed; 0 on a bad shape; rows are not chunked), each part rounded up to 256 bytes, in this order:
 *   cross_sublayer_scratch_bytes(M, Rm, D, n_views, kv_ready) = 4 M D + 4 M D + [8 Rm D] + 4 M D + 4 M D + 4 M D + [8 Rm D]
 *         + max(op_linear_wgrad_scratch_bytes(M, D, D), [op_linear_wgrad_scratch_bytes(Rm, D, D)]) + op_layernorm_grad_scratch_bytes(M, D)
 *         + attn_train_scratch_bytes(n_views, M, Rm, D / 64)
 *                                                [y^ | q | k|v | o | do | dq | dk|dv | weight-gradient partials | LayerNorm | attention core]
 *   the parts in brackets are absent with kv_ready != 0 (the `kv` mode).  The forward takes the same scratch.
 * Refused with an error before anything is read or launched: null required pointers (x, mem, gamma, beta, Wq, Wproj, views; out / dy), M or Rm <= 0, D not a
 * multiple of 64 or above 1024, ldmem / lddmem short or not a multiple of 4, pointers not 16-byte aligned, a table with negative entries or reaching past the M query
 * rows or the Rm key rows, skip_lo > skip_hi or skip_hi > nk, Wk without Wv or the reverse (and bk, bv or their gradients without Wk), overlapping key groups (grad),
 * scratch NULL, misaligned or too small. */
typedef struct must3r_hip_cross_sublayer_args {
    const float* x; const float* mem; const float* gamma; const float* beta;
    const float* Wq; const float* bq; const float* Wk; const float* bk; const float* Wv; const float* bv; const float* Wproj; const float* bproj;
    const float* dy;                   /* *_grad only */
    const int32_t* views;              /* HOST int32 [n_views][6] */
    float* out;                        /* *_forward only */
    float* dx; float* dmem; float* dgamma; float* dbeta; float* dWq; float* dbq; float* dWk; float* dbk; float* dWv; float* dbv; float* dWproj;
    float* dbproj;                     /* *_grad, each optional; dmem [Rm][lddmem] */
    int32_t M, Rm, D, n_views, ldmem, lddmem;
    float eps;
    int32_t reserved;
    void* stream;                      /* hipStream_t */
} must3r_hip_cross_sublayer_args;
size_t must3r_hip_cross_sublayer_scratch_bytes(int M, int Rm, int D, int n_views, int kv_ready);
int must3r_hip_cross_sublayer_forward(const must3r_hip_cross_sublayer_args* a, void* scratch, size_t scratch_bytes);
int must3r_hip_cross_sublayer_grad(const must3r_hip_cross_sublayer_args* a, void* scratch, size_t scratch_bytes);

/* ABI 21, additive.  The cross-attention sublayer above with key masks handed to its attention core (must3r_hip_attn_masked_*): mask_bits, view_mask, mask_rows
 * and mask_ld as there, the key rows of the masks index mem like the kv rows of the table.  Everything else is must3r_hip_cross_sublayer_*: the operand forms, the
 * `kv` mode, the segmented dmem, the optional outputs, coverage, determinism and the stream in core.stream.  A memory row that every view of its group has
 * dropped gets exact zeros in dK | dV, hence dmem = 0 in the `kv` mode and no contribution to dWk, dWv and dmem otherwise.  mask_bits == NULL with view_mask ==
 * NULL is must3r_hip_cross_sublayer_forward / _grad, bit for bit.  Scratch: cross_sublayer_scratch_bytes with attn_masked_scratch_bytes in the place of
 * attn_train_scratch_bytes.  Refused before anything is read or launched: what the unmasked calls refuse and what must3r_hip_attn_masked_* refuses of the masks. */
typedef struct must3r_hip_cross_sublayer_masked_args {
    must3r_hip_cross_sublayer_args core;
    const uint32_t* mask_bits;         /* DEVICE uint32 [mask_rows][mask_ld] */
    const int32_t* view_mask;          /* HOST int32 [core.n_views], -1: none */
    int32_t mask_rows, mask_ld;
} must3r_hip_cross_sublayer_masked_args;
size_t must3r_hip_cross_sublayer_masked_scratch_bytes(int M, int Rm, int D, int n_views, int kv_ready);
int must3r_hip_cross_sublayer_masked_forward(const must3r_hip_cross_sublayer_masked_args* a, void* scratch, size_t scratch_bytes);
int must3r_hip_cross_sublayer_masked_grad(const must3r_hip_cross_sublayer_masked_args* a, void* scratch, size_t scratch_bytes);

/* ABI 21, additive.  Training forward and backward of what the reference's decoder does to the new tokens of all layers after a memory update
 * (feedback_mechanism.py:39-53, decoder.py:325-330): the feedback offset is added to the tokens of every layer but the last and each layer's norm_y is
 * applied, for all layers in one launch each way (the training counterpart of the grouped LayerNorm with add_groups of the inference path):
 *   Y_l = LN_l(X_l + (l < add_layers ? offset : 0)) gamma_l + beta_l        l = 0 .. L - 1 <= 31; X_l, Y_l [R][D] fp32 contiguous; offset [R][D], NULL with add_layers 0
 * gamma_l and beta_l are given for every layer, or for none: the reference's `raw` memory mode, the add alone.  D % 64 == 0, D <= 1024; pointers 16-byte aligned.
 * The backward gives, from dY_l: dX_l; doffset = the sum over l < add_layers of dX_l, added in ascending l (zeros with add_layers 0); dgamma_l and dbeta_l.
 * The per-layer pointers travel BY VALUE in the descriptor, and so does the stream (`stream`, a hipStream_t): all work goes to it, nothing waits on the host.
 * Every output may be NULL, costs nothing then and is not written: a NULL y[l] skips the layer's forward; no dgamma and no dbeta at all, no column sums and no
 * reduce launch; no doffset, nothing accumulated; nothing asked for, no launch.
 * Determinism: no atomics, one writer per element; a row's Y, dX and doffset do not depend on the other rows (the same bits alone and in a batch); the column
 * sums go through one partial per (layer, block of 16 rows) and a fixed-order reduce, the block count a function of R alone; repeated calls agree bit for bit.
 * A layer without the add has the bits of must3r_hip_op_layernorm_f32 (one row routine, csrc/train_ln.hpp).  The backward's statistics are the forward's.
 * Scratch (no device needed; 0 on a bad shape): feedback_prepare_scratch_bytes = 8 L ceil(R / 16) D rounded up to 256, the column-sum partials; the backward
 * takes it where a dgamma or dbeta is asked for, and reads neither argument otherwise; the forward never does.
 * Refused with an error before anything is read or launched: a NULL descriptor, L outside [1, 32], R <= 0, D not a multiple of 64 or above 1024, add_layers
 * outside [0, L], add_layers > 0 without offset, a NULL x[l] (dy[l], in the backward), gamma without beta or for some layers only, dgamma / dbeta without gamma,
 * pointers not 16-byte aligned, scratch NULL, misaligned or too small (a backward with column sums). */
#define MUST3R_FEEDBACK_MAX_LAYERS 32
typedef struct must3r_hip_feedback_prepare_args {
    const float* x[MUST3R_FEEDBACK_MAX_LAYERS];
    const float* gamma[MUST3R_FEEDBACK_MAX_LAYERS];
    const float* beta[MUST3R_FEEDBACK_MAX_LAYERS];
    const float* dy[MUST3R_FEEDBACK_MAX_LAYERS];     /* *_grad only */
    float* y[MUST3R_FEEDBACK_MAX_LAYERS];            /* *_forward only, each optional */
    float* dx[MUST3R_FEEDBACK_MAX_LAYERS];           /* *_grad, each optional */
    float* dgamma[MUST3R_FEEDBACK_MAX_LAYERS];
    float* dbeta[MUST3R_FEEDBACK_MAX_LAYERS];
    const float* offset;
    float* doffset;                                  /* *_grad, optional */
    int32_t L, R, D, add_layers;
    float eps;
    int32_t reserved;
    void* stream;                                    /* hipStream_t */
} must3r_hip_feedback_prepare_args;
size_t must3r_hip_feedback_prepare_scratch_bytes(int L, int R, int D);
int must3r_hip_feedback_prepare_forward(const must3r_hip_feedback_prepare_args* a, void* scratch, size_t scratch_bytes);
int must3r_hip_feedback_prepare_grad(const must3r_hip_feedback_prepare_args* a, void* scratch, size_t scratch_bytes);

/* ABI 21, additive.  The optimizer step of the reference's training recipe (must3r/engine/train.py: torch.optim.AdamW under croco's
 * NativeScalerWithGradNormCount): the global gradient norm with the non-finite test, the clip coefficient and GradScaler.update() in one pass over the
 * gradients (optim_norm), and decoupled-decay Adam in one pass over parameters and moments (optim_adamw).  fp32 storage, no atomics, no host synchronisation.
 * The table: HOST arrays of tensors {p, g, m, v, step, n, group} (DEVICE fp32 pointers, 16-byte aligned; step one fp32 scalar per tensor, as torch.optim.AdamW
 * keeps it; n >= 1 elements, int64) and of groups {lr, weight_decay, beta1, beta2, eps} (fp64, as the host holds them; lr is the group's effective rate).  The
 * library cuts every tensor into chunks of MUST3R_OPTIM_CHUNK elements and uploads tensors and chunk list in one copy into the caller's scratch through a ring of
 * pinned buffers, so that a second call does not wait for the first.  Offsets are 64-bit: no limit of 2^31 on the total.  A tensor whose n is not a multiple of 4
 * ends in a scalar tail.  The stream travels in the descriptor (`stream`, a hipStream_t): all work goes to it, the upload included.
 * optim_norm reads g and n of the table alone (p, m, v, step, group and the group table are not looked at) and writes the control record, without the host:
 *   total     = sum of g^2 over the table, in fp64: one partial per chunk, the partials added in a fixed order (bitwise repeatable)
 *   inv_scale = 1 / *scale in fp32, read BEFORE the update below; 1 without a scaler state
 *   norm      = sqrt(total) inv_scale, rounded to fp32 once
 *   found_inf = total is not finite (some gradient element is not finite: squares of finite fp32 values cannot overflow fp64)
 *   coef      = inv_scale (max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1)           torch.nn.utils.clip_grad_norm_'s rule, in fp32
 * and, where a scaler state is given (DEVICE scale fp32 [1], growth_tracker int32 [1]), GradScaler.update(): on found_inf scale *= backoff_factor and
 * tracker = 0; otherwise tracker += 1 and, at growth_interval, scale *= growth_factor and tracker = 0.
 * optim_adamw: nothing at all where control is given and found_inf is set.  Otherwise step += 1 for every tensor of the table (t below), and per element
 *   g' = g coef                 p = p (1 - lr wd)               coef = 1 with control == NULL (a plain optimizer step, never skipped)
 *   m  = b1 m + (1 - b1) g'     v = b2 v + (1 - b2) g' g'
 *   p  = p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)         bc1 = 1 - b1^t, bc2 = 1 - b2^t
 * in fp32; lr / bc1 and sqrt(bc2) are computed in fp64 and rounded once, and 1 - lr wd, b1, 1 - b1, b2, 1 - b2, eps are fp64 values rounded once.  g is never
 * written: the unscale and the clip live in coef.  An element's new p, m, v depend on its own old values, g, coef and its tensor's numbers alone, not on the
 * other tensors of the table or their order.  A tensor must not be named twice.
 * Scratch (no device needed; 0 on a bad shape, the reason in the last error), each part rounded up to 256 bytes, with C = total_elems / MUST3R_OPTIM_CHUNK +
 * n_tensors (the most chunks such a table can have):
 *   optim_scratch_bytes(n_tensors, total_elems) = 96 n_tensors + 16 C + 8 C + 8 n_tensors       [tensors | chunks | fp64 partials | lr / bc1, sqrt(bc2)]
 *   both calls take the same scratch (the same buffer may serve both: they are ordered by the stream).
 * Refused with an error before anything on the device is read or launched: a NULL descriptor, tensors (adamw: groups) NULL, n_tensors < 1 (adamw: n_groups < 1),
 * a NULL g (adamw: p, m, v, step), pointers not 16-byte aligned, n <= 0, a total above 2^46; adamw: a group index outside the table, a beta outside [0, 1),
 * eps < 0, lr < 0, weight_decay < 0; norm: control NULL, a scaler state with only one of its two pointers, factors <= 0 or growth_interval < 1 with a scaler
 * state, max_norm NaN; scratch NULL, misaligned or too small. */
#define MUST3R_OPTIM_CHUNK 32768
typedef struct must3r_hip_optim_tensor {
    float* p; const float* g; float* m; float* v; float* step;   /* DEVICE */
    int64_t n;
    int32_t group, reserved;
} must3r_hip_optim_tensor;
typedef struct must3r_hip_optim_group { double lr, weight_decay, beta1, beta2, eps; } must3r_hip_optim_group;
typedef struct must3r_hip_optim_control { float norm, coef; int32_t found_inf, reserved; } must3r_hip_optim_control;
typedef struct must3r_hip_optim_args {
    const must3r_hip_optim_tensor* tensors;      /* HOST [n_tensors] */
    const must3r_hip_optim_group* groups;        /* HOST [n_groups]; optim_adamw only */
    int32_t n_tensors, n_groups;
    must3r_hip_optim_control* control;           /* DEVICE, 16-byte aligned; optim_norm writes it, optim_adamw reads it (optional there) */
    float* scale; int32_t* growth_tracker;       /* DEVICE, optim_norm only, both or neither */
    float max_norm;                              /* optim_norm only; <= 0: no clip */
    float growth_factor, backoff_factor;
    int32_t growth_interval;
    void* stream;                                /* hipStream_t */
} must3r_hip_optim_args;
size_t must3r_hip_optim_scratch_bytes(int64_t n_tensors, int64_t total_elems);
int must3r_hip_optim_norm(const must3r_hip_optim_args* a, void* scratch, size_t scratch_bytes);
int must3r_hip_optim_adamw(const must3r_hip_optim_args* a, void* scratch, size_t scratch_bytes);

/* ABI 21, additive.  The matrix products of the training Linears on the 16-bit MFMA (v_mfma_f32_16x16x32_bf16, fp32 accumulation), switched the way
 * torch.autocast switches: by a mode of the calling host thread, not by an argument (the reference's recipe trains under --amp bf16).
 *   In MUST3R_TRAIN_LINEAR_BF16 mode must3r_hip_op_linear_f32, must3r_hip_op_linear_dgrad_f32, must3r_hip_op_linear_wgrad_f32 and the two-parameter data
 *   gradient of the cross sublayer (dmem = dK Wk + dV Wv) round both operands of their product to bf16 (nearest even, NaN and inf kept: Tensor.to(bfloat16))
 *   as they stage them, multiply on the 16-bit MFMA and accumulate in fp32.  Every training entry point built on them follows: the MLP, attention and cross
 *   sublayers (masked forms included) and the decoder's embedding and feedback Linears.  The `_f32` in these names is the STORAGE type: every tensor in memory
 *   -- activations, master weights, outputs, gradients, scratch -- is fp32 in either mode; there is no cast pass and no 16-bit copy of a weight.  Shapes,
 *   alignment rules, descriptors, scratch queries and stream order are the same in both modes.
 *   What stays fp32 arithmetic in either mode: the bias, residual and GELU epilogues (on the fp32 accumulator), the bias gradient (column sums of the unrounded
 *   dZ), the reduction of the weight-gradient partials, LayerNorm forward and backward, the attention core (scores, softmax, P V and their gradients), RoPE, the
 *   residual stream, the head (must3r_hip_head_forward / _head_grad / _op_head_linear: its own split-precision forms and the fp32 gather forms), the loss family
 *   and the optimizer.  The attention core has a mode of its own (must3r_hip_train_attention_mode below); bf16 storage of activations is not built.
 *   In MUST3R_TRAIN_LINEAR_F32 mode (the default of every thread) the four functions launch exactly the kernels of ABI 21 before this entry point existed.
 *   The bf16 kernels use no atomics either: one writer per element, a fixed order of additions, a row of out / dX independent of the other rows.
 * A backward pass that recomputes a sublayer's forward must run in the mode its forward ran in (must3r_amd records it per autograd node). */
#define MUST3R_TRAIN_LINEAR_F32  0
#define MUST3R_TRAIN_LINEAR_BF16 1
/* Per host thread; default F32.  Sets the mode in which must3r_hip_op_linear_f32, _dgrad_f32, _wgrad_f32 and every training entry point
   built on them multiply; returns the previous mode.  mode = -1 only queries.  Any other value: returns -1, last error set, nothing changed. */
int must3r_hip_train_linear_mode(int mode);

/* ABI 21, additive.  The matrix products of the training attention core on the 16-bit MFMA, switched like the Linears above: by a mode of the calling host
 * thread (the reference trains under torch.autocast(bfloat16), where the attention products run in bf16).
 *   In MUST3R_TRAIN_ATTENTION_BF16 mode must3r_hip_attn_forward_f32, must3r_hip_attn_grad, must3r_hip_attn_masked_forward and must3r_hip_attn_masked_grad, and
 *   through them the attention sublayer and the cross sublayer (masked forms included), launch the bf16 siblings of their three kernels: the same view table,
 *   key groups, skip ranges, mask bits, scratch layout (lse2 and delta fp32), grids and launch order; no descriptor, scratch query or stream rule changes.
 *   Everything in memory stays fp32 (the `_f32` in the names is the storage type).  With s = 1/8 and ^ = rounded to bf16 (nearest even, NaN and inf kept) in
 *   registers, fp32 accumulation throughout:
 *     S = s (Q^ K^T^), scale and log2 e applied in fp32 after the product; online softmax in fp32, the row sum l adds the unrounded p;
 *     O = (sum P^ V^) / l;  lse as in fp32 mode;  delta = dO . O with the unrounded dO;
 *     P = exp2(S c - lse2) (0 for an invalid key);  dV = P^T^ dO^;  dP = dO^ V^T^;  dS = P (dP - delta) in fp32;  dQ = s dS^ K^;  dK = s dS^T^ Q^.
 *   Rows without a valid key keep their rules (O = 0, lse = -inf, no contribution, dQ = 0).  No atomics, one writer per element, a fixed order of additions;
 *   a view's O and dQ and a scene's dK and dV are the same bits alone and in a batch.
 *   In MUST3R_TRAIN_ATTENTION_F32 mode (the default of every thread) the four functions launch exactly the kernels they launched before this entry point
 *   existed.  The two modes are independent: must3r_hip_train_linear_mode does not touch the attention core and this mode does not touch a Linear.
 *   bf16 storage of activations is not built; the 16-bit inference forward (must3r_hip_attention) is a different kernel and takes no masks.
 * A backward pass must run in the mode its forward ran in (must3r_amd records it per autograd node). */
#define MUST3R_TRAIN_ATTENTION_F32  0
#define MUST3R_TRAIN_ATTENTION_BF16 1
/* Per host thread; default F32.  Returns the previous mode.  mode = -1 only queries.  Any other value: returns -1, last error set, nothing changed. */
int must3r_hip_train_attention_mode(int mode);

/* ABI 21, additive.  The gather in front of the trainable encoder's patch embedding (dust3r's PatchEmbedDust3R and ManyAR_PatchEmbed as a Linear over
 * rows; csrc/train_encoder.hip): the fp32 image batch img [V][3][H][W] becomes fp32 rows [V N][768], N = (H / 16)(W / 16), in the column order of the flattened
 * conv weight, k = c 256 + dy 16 + dx (the order of must3r_hip_op_im2col, whose rows are 16-bit and know one orientation), and the int64 positions pos [V N][2].
 * The orientation is per view and comes from a DEVICE array: transposed[v] != 0 marks a portrait view of a batch stored landscape; NULL means no view is.
 *   landscape   grid H/16 x W/16   token t = (py, px) = (t / (W/16), t % (W/16))   rows[v N + t][k] = img[v][c][16 py + dy][16 px + dx]   pos = (py, px)
 *   portrait    grid W/16 x H/16   token t = (py, px) = (t / (H/16), t % (H/16))   rows[v N + t][k] = img[v][c][16 px + dx][16 py + dy]   pos = (py, px)
 * The portrait form is the reference's proj(img.swapaxes(-1, -2)) with the positions of the swapped grid; the host never learns which views are portrait.
 * The Linear that follows is must3r_hip_op_linear_f32 on the rows: nothing is fused.  Either output may be NULL, costs nothing then and is not written
 * (rows == NULL: positions alone).  The stream travels in the descriptor (`stream`, a hipStream_t): all work goes to it, nothing waits on the host.
 * Determinism: a permutation -- one writer per element, no atomics, no arithmetic on the values; 64-bit offsets.
 * Refused with an error before anything is read or launched: a NULL descriptor, a NULL img, both outputs NULL, V <= 0, H or W not a positive multiple of 16,
 * img, rows or pos not 16-byte aligned, transposed not 4-byte aligned, more than 2^29 - 1 rows. */
typedef struct must3r_hip_patch_rows_args {
    const float*   img;          /* [V, 3, H, W] */
    const int32_t* transposed;   /* [V] on the device, optional */
    float*         rows;         /* [V * N, 768], optional */
    int64_t*       pos;          /* [V * N, 2], optional */
    int32_t V, H, W, reserved;
    void* stream;                /* hipStream_t */
} must3r_hip_patch_rows_args;
int must3r_hip_patch_rows(const must3r_hip_patch_rows_args* a);

/* ABI 21, additive.  The ground truth of a training batch from its depth maps, on the device (csrc/train_data.hip): what the reference's datasets compute per
 * view in numpy (must3r_base_dataset.py:185-198) and its criterion then stacks and uploads, 14 bytes per pixel where the depth map is 4 or 2.  V views stored
 * landscape [V][Hs][Ws]; all pointers are DEVICE pointers.
 *   depth        fp32, or (depth_u16 = 1) raw uint16 with a per-view pair depth_scale[v] = (div, mul): z = (float(raw) / div) * mul in fp32 -- ScanNet++ is
 *                (1000, 1), a Co3d-style file (65535, maximum_depth).  The uint16 form has no sky (no negative depth).
 *   K            [V][3][3], the intrinsics of the true (untransposed) image: fu = K[0][0], cu = K[0][2], fv = K[1][1], cv = K[1][2]; the rest is not read.
 *   c2w          [V][4][4], camera to world: R its upper 3 x 3, t its last column.  It may be NaN (a view without a pose); the kernel does not test for that.
 *   transposed   int32 [V] in the meaning of must3r_hip_patch_rows_args.transposed, or NULL (no view is): a non-zero entry marks a portrait image that was
 *                stored with its axes swapped (dust3r's transpose_to_landscape).  Its stored pixel (r, c) is true pixel (row = c, col = r): u = r, v = c.
 *                An unflagged view has u = c, v = r.  No data is moved.
 * Per stored pixel, every operation rounded once (nothing is contracted into an FMA), so that a CPU expression reproduces the bits:
 *   x = fp32((double(u) - double(cu)) * double(z) / double(fu))     y = fp32((double(v) - double(cv)) * double(z) / double(fv))
 *   X[i] = ((R[i][0] * x + R[i][1] * y) + R[i][2] * z) + t[i]       in fp32, i = 0..2
 *   pts3d = X (written for every pixel, as the reference does)     valid = z > 0 && isfinite(X[0..2])     sky = z < 0     n_valid[v] = #{z > 0}
 * (n_valid is what the datasets' is_valid_check tests; a NaN pose makes a view all invalid and leaves its n_valid alone.)
 * Every output is optional: a NULL one costs nothing and is not written; at least one is needed.  n_valid is a fixed-order reduce without atomics (lanes, waves,
 * then the view's blocks in order, in a second small launch) through `scratch`: at least 4 * V * MUST3R_GT_VIEW_BLOCKS bytes, read and written only with n_valid.
 * The block count of a view depends on Hs and Ws alone: a view's outputs are the same bits alone and in a batch.  The stream travels in the descriptor: all
 * work goes to it, nothing waits on the host.
 * Refused with an error before anything is read or launched: a NULL descriptor, depth, K or c2w; depth_u16 not 0 / 1, or 1 without depth_scale; no output;
 * V outside 1 .. 65535; Hs or Ws not positive, Ws no multiple of 4, more than 2^31 - 1 pixels a view; depth not 16-byte (uint16: 8-byte) aligned, pts3d not
 * 16-byte aligned, any other pointer not 4-byte aligned; n_valid without enough scratch. */
#define MUST3R_GT_VIEW_BLOCKS 32
typedef struct must3r_hip_gt_args {
    const void*    depth;         /* [V, Hs, Ws] fp32, or uint16 with depth_u16 */
    const float*   depth_scale;   /* [V, 2] (div, mul): the uint16 form only */
    const float*   K;             /* [V, 3, 3] */
    const float*   c2w;           /* [V, 4, 4] */
    const int32_t* transposed;    /* [V], optional */
    float*         pts3d;         /* [V, Hs, Ws, 3], optional */
    uint8_t*       valid;         /* [V, Hs, Ws], optional */
    uint8_t*       sky;           /* [V, Hs, Ws], optional */
    int32_t*       n_valid;       /* [V], optional */
    void*          scratch;       /* with n_valid */
    size_t         scratch_bytes;
    int32_t V, Hs, Ws, depth_u16;
    void* stream;                 /* hipStream_t */
} must3r_hip_gt_args;
int must3r_hip_gt_from_depth(const must3r_hip_gt_args* a);

/* ABI 21, additive.  Training augmentation on the device (csrc/train_augment.hip, must3r_amd/train_augment.py): what the reference's datasets do to a raw frame
 * on the host -- dust3r's _crop_resize_if_necessary (PIL crop and resize, cv2 nearest resize of the depth map), torchvision's ColorJitter + ImgNorm and
 * transpose_to_landscape.  The crop, the Pillow resize and the final window of the IMAGE are must3r_hip_resample in its two PIL modes; the two entry points
 * below are what follows it.  Each is one launch per pass for a batch of V views and reads a per-view table, a HOST array that the call checks, turns into its
 * device form and uploads through pinned slots of the calling thread (a ring of 4, as the resampler's) into `scratch`.  All device work goes to the descriptor's
 * `stream`; nothing is read back and nothing waits on the host.  The batch is stored as [V][Hs][Ws]: a view of true size (h, w) is stored as it is, or, flagged
 * portrait, with its axes swapped (stored (r, c) = true (row c, col r): dust3r's transpose_to_landscape, the convention of must3r_hip_gt_args.transposed).
 * Every view's stored shape must be (Hs, Ws).  A view's output bits do not depend on the batch around it, and two runs give the same bits.
 *
 * Colour.  src holds the resampler's output, fp32 planes [3][h][w] per view at src_offset: ImgNorm values, each one of the 256 entries of its table.  A value v
 * is the byte u = int(127.5f * v + 127.5f + 0.5f), each operation rounded to fp32 (exact for all 256 entries).  The view's flagged operations then run in the
 * view's order on (r, g, b) bytes, each producing bytes again, and the result is written as (u / 255 - 0.5) / 0.5 in fp32, the table's own expression: a view
 * with no flag set is a copy.  The arithmetic is Pillow's, through which torchvision's PIL backend works, operation for operation:
 *   blend(a, b, f)   Image.blend: t = float(a) + f * float(b - a), one fp32 multiply then one fp32 add (no FMA); 0 if t <= 0, 255 if t >= 255, else trunc(t)
 *   BRIGHTNESS       blend(0, x, f) per channel                                      ImageEnhance.Brightness
 *   SATURATION       blend(L, x, f), L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16     ImageEnhance.Color
 *   CONTRAST         blend(m, x, f), m = int(sum(L) / count + 0.5) in double, over the whole view as it stands when contrast is applied (after the operations
 *                    in front of it in the view's order): a first pass sums L in integers (lanes, waves, tiles; no atomics), the second applies
 *   HUE              RGB -> HSV, H = (H + shift) mod 256, HSV -> RGB; shift = trunc(double(f) * 255) mod 256 (non-negative), f in [-0.5, 0.5].
 *                    RGB -> HSV: V = max; max == min: H = S = 0; else cr = float(max - min), S = int(double(cr / float(max)) * 255), rc, gc, bc =
 *                    float(max - c) / cr in fp32, h = bc - gc (fp32) if r == max, else float(2.0 + double(rc) - double(bc)) if g == max, else
 *                    float(4.0 + double(gc) - double(rc)); h = float(fmod(double(h) / 6.0 + 1.0, 1.0)); H = int(double(h) * 255); H, S clipped to [0, 255].
 *                    HSV -> RGB in double: S == 0: r = g = b = V; else hh = H * 6.0 / 255.0, i = floor(hh), f = hh - i, fs = S / 255.0,
 *                    p = round(V (1 - fs)), q = round(V (1 - fs f)), t = round(V (1 - fs (1 - f))), round half away from zero, clipped to [0, 255];
 *                    (r, g, b) by i mod 6: (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q).
 * Depth.  A view's raw depth map (its own DEVICE pointer, size and row stride; fp32, or uint16 with depth_u16) goes through the image's geometry by nearest
 * neighbour: with the first crop (crop_x, crop_y, crop_w, crop_h), the size it was rescaled to (resize_w, resize_h) and the window's corner (win_x, win_y) inside
 * that, pixel (x, y) of the out_w x out_h window reads depth[crop_y + sy][crop_x + sx],
 *   sx = min(floor((x + win_x) * (double(crop_w) / resize_w)), crop_w - 1)     sy = min(floor((y + win_y) * (double(crop_h) / resize_h)), crop_h - 1)     in double.
 * Values are moved, never computed with: a negative (sky) value, 0 and NaN pass through untouched, and the element type is kept.
 * Refused with an error before anything is uploaded or launched: a NULL descriptor, src, views, out, scratch or (depth) a view's src; V outside 1 .. 65535; Hs or
 * Ws not positive, more than 2^31 - 1 pixels a view; pointers not aligned to their element, scratch not 256-byte aligned or smaller than the query's answer; a
 * flag (apply, portrait, depth_u16) that is not 0 or 1; an order that is no permutation of 0 .. 3; a factor that is not finite, an applied hue factor outside
 * [-0.5, 0.5]; a view whose stored shape is not (Hs, Ws); planes outside src_elems; a crop outside its source or a window outside its resize. */
enum { MUST3R_AUG_BRIGHTNESS = 0, MUST3R_AUG_CONTRAST = 1, MUST3R_AUG_SATURATION = 2, MUST3R_AUG_HUE = 3 };
#define MUST3R_AUG_TILE 64
typedef struct must3r_hip_augment_color_view {
    int64_t src_offset;      /* elements into src: this view's planes [3][h][w] */
    int32_t h, w;            /* the view's true size */
    int32_t portrait;        /* 1: written with its axes swapped */
    int32_t order[4];        /* the four MUST3R_AUG_* operations in the order they are applied */
    int32_t apply[4];        /* by operation: 0 / 1 */
    float   factor[4];       /* by operation */
    int32_t reserved;
} must3r_hip_augment_color_view;
typedef struct must3r_hip_augment_color_args {
    const float* src;        /* DEVICE: the resampler's output */
    int64_t      src_elems;  /* its length */
    const must3r_hip_augment_color_view* views;   /* HOST [V] */
    float*       out;        /* DEVICE [V, 3, Hs, Ws] */
    void*        scratch;
    size_t       scratch_bytes;
    int32_t V, Hs, Ws, reserved;
    void* stream;            /* hipStream_t */
} must3r_hip_augment_color_args;
size_t must3r_hip_augment_color_scratch_bytes(int V, int Hs, int Ws);
int must3r_hip_augment_color(const must3r_hip_augment_color_args* a);

typedef struct must3r_hip_augment_depth_view {
    const void* src;         /* DEVICE: pixel (0, 0) of the raw depth map */
    int64_t row_stride;      /* elements between its rows */
    int32_t H, W;            /* its size */
    int32_t crop_x, crop_y, crop_w, crop_h;
    int32_t resize_w, resize_h;
    int32_t win_x, win_y, out_w, out_h;
    int32_t portrait, reserved;
} must3r_hip_augment_depth_view;
typedef struct must3r_hip_augment_depth_args {
    const must3r_hip_augment_depth_view* views;   /* HOST [V] */
    void*  out;              /* DEVICE [V, Hs, Ws], fp32 or uint16 */
    void*  scratch;
    size_t scratch_bytes;
    int32_t V, Hs, Ws, depth_u16;
    void* stream;            /* hipStream_t */
} must3r_hip_augment_depth_args;
size_t must3r_hip_augment_depth_scratch_bytes(int V);
int must3r_hip_augment_depth(const must3r_hip_augment_depth_args* a);

/* ---- baseline JPEG decoding (ABI 21, additive; csrc/jpeg_parse.hpp, csrc/jpeg_entropy.hpp, csrc/jpeg.hip) -------------------------
 * From the bytes of a file to the MUST3R_IMG_U8_HWC pixels the resampler takes, bit-equal to libjpeg-turbo's default decode (accurate integer IDCT, fancy
 * upsampling, 16-bit YCbCr -> RGB) as Pillow's open().convert("RGB") runs it.  Accepted: SOF0 / SOF1 with 8-bit samples, Huffman coding, one interleaved
 * scan, 8-bit quantisation tables, one component or three YCbCr components with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, with or without restart
 * intervals.  Everything else the parser reports as unsupported with a reason, before anything is launched.
 *
 * The parser runs on the host and needs no GPU.  It never trusts a length field: every read is checked against the buffer.  The info record is plain data
 * (no pointers): geometry, the quantisation table of each component (zig-zag order, as in the file), the four Huffman tables in the form the kernels read
 * (a 9-bit lookahead and the canonical arrays), the restart interval and the byte range of the entropy-coded data.  `seg_offsets` receives the byte offset
 * (from the start of the file) of every restart segment's first byte, n_segments entries; segment s ends two bytes (its RSTn marker) before segment s + 1
 * starts, the last at scan_offset + scan_bytes. */
#define MUST3R_JPEG_SUBSEQ_BYTES 128   /* bytes of one subsequence of the parallel entropy decode */
#define MUST3R_JPEG_PATH_FAST 0        /* must3r_hip_jpeg_decode, flags: the subsequence scheme verified */
#define MUST3R_JPEG_PATH_SEQUENTIAL 1  /* the verification failed: one thread per restart segment decoded the image again */
typedef struct must3r_hip_jpeg_huff {
    uint16_t look[512];     /* by the next 9 bits: (code length << 8) | symbol; 0: the code is longer than 9 bits */
    int32_t  maxcode[18];   /* [l], l = 1 ... 16: the largest code of length l, -1 without one; [17]: a sentinel above every code */
    int32_t  valoff[18];    /* [l]: index into vals of the first code of length l, minus that code */
    uint8_t  vals[256];
} must3r_hip_jpeg_huff;
typedef struct must3r_hip_jpeg_info {
    int32_t width, height, components;        /* components: 1 (grey) or 3 (YCbCr) */
    int32_t hs, vs;                           /* luma sampling factors (1x1 for grey); chroma is 1x1 */
    int32_t mcus_x, mcus_y, blocks_per_mcu;   /* the scan: mcus_x * mcus_y MCUs of hs * vs luma blocks, then Cb, then Cr */
    int32_t n_blocks;                         /* mcus_x * mcus_y * blocks_per_mcu */
    int32_t restart_interval;                 /* MCUs per restart segment; 0: one segment */
    int32_t n_segments;
    int32_t reserved;
    int64_t scan_offset, scan_bytes;          /* the entropy-coded data, from the first byte after SOS up to the marker that ends the scan */
    int32_t comp_dc[3], comp_ac[3];           /* per component: which of dc[2] / ac[2] */
    uint16_t quant[3][64];                    /* per component, zig-zag order */
    uint8_t  natural[64];                     /* zig-zag index -> row-major index */
    must3r_hip_jpeg_huff dc[2], ac[2];
} must3r_hip_jpeg_info;
/* 0: accepted, *info is filled (and seg_offsets, when seg_capacity >= n_segments; with a smaller capacity only info is filled: query n_segments first).
 * 1: not accepted; `reason` (when not NULL, reason_capacity bytes) holds why as a C string.  No other outcome, no GPU call, no allocation. */
int must3r_hip_jpeg_parse(const void* data, size_t data_bytes, must3r_hip_jpeg_info* info, uint32_t* seg_offsets, size_t seg_capacity,
                          char* reason, size_t reason_capacity);
typedef struct must3r_hip_jpeg_image {
    const must3r_hip_jpeg_info* info;   /* HOST: as must3r_hip_jpeg_parse filled it */
    const uint32_t* seg_offsets;        /* HOST [info->n_segments] */
    const void* data;                   /* DEVICE: the whole file, data_bytes bytes, 16-byte aligned */
    size_t data_bytes;
    void*  out;                         /* DEVICE: uint8 [height][width][3], rows of out_row_stride bytes (>= 3 * width), 16-byte aligned */
    int64_t out_row_stride;
} must3r_hip_jpeg_image;
typedef struct must3r_hip_jpeg_batch {
    const must3r_hip_jpeg_image* images;   /* HOST [n_images] */
    int32_t n_images, reserved;
    int32_t* flags;          /* DEVICE [n_images], written: MUST3R_JPEG_PATH_FAST or MUST3R_JPEG_PATH_SEQUENTIAL per image */
    void*  scratch;          /* DEVICE, 256-byte aligned */
    size_t scratch_bytes;    /* >= must3r_hip_jpeg_scratch_bytes of the same images */
    void*  stream;           /* hipStream_t: every copy, memset and launch of the call goes there; nothing is read back */
} must3r_hip_jpeg_batch;
/* device bytes of scratch for one decode call of these images (0 on invalid descriptors): the descriptor tables, the subsequence states, the int16
 * coefficients [n_blocks][64] and the component planes padded to whole MCUs.  Only info and seg_offsets of each image are read. */
size_t must3r_hip_jpeg_scratch_bytes(const must3r_hip_jpeg_image* images, int n_images);
/* Decodes the batch.  Entropy decoding does not depend on restart markers: every thread decodes one subsequence of MUST3R_JPEG_SUBSEQ_BYTES bytes of a
 * restart segment from an assumed state, then again from its predecessor's exit state while the states change (a bounded number of rounds); an exclusive
 * scan of the completed-block counts places every subsequence's coefficients.  The write pass checks that every subsequence's recorded exit came from its
 * predecessor's: by induction from the segment's first bit the result then IS the sequential decode.  An image that fails the check (a periodic stream
 * can defeat the synchronisation for ever) is decoded again by one thread per segment, in a launch predicated on the image's device flag.  Then DC
 * prediction (a segmented scan), dequantisation + IDCT, and upsampling + colour conversion.  The stream is assumed intact: on a damaged one every access stays
 * in bounds and the pixels are unspecified. */
int must3r_hip_jpeg_decode(const must3r_hip_jpeg_batch* batch);

/* ---- PNG decoding (ABI 21, additive; csrc/png_parse.hpp, csrc/png_inflate.hpp, csrc/png.hip) --------------------------------------
 * From the bytes of a file to pixels on the device, bit-equal to Pillow: inflate (RFC 1951) of the zlib stream the IDAT chunks hold, the Adler-32 check,
 * the five scanline filters, and the caller's layout.  Accepted: non-interlaced files of colour type 0 at 8 or 16 bits, colour type 2 at 8 bits and colour
 * type 6 at 8 bits, with one or more consecutive IDAT chunks and no tRNS or acTL chunk.  Everything else the parser reports with a reason, before anything
 * is launched.
 *
 * The parser runs on the host and needs no GPU.  It never trusts a length field: every read is checked against the buffer.  Chunk CRCs are not verified
 * (the pixel payload is covered by the Adler-32 check of the decode call).  The info record is plain data; `idat_ranges` receives the byte range of every
 * IDAT chunk's payload, n_idat entries.  The caller copies these payloads back to back: the device sees one contiguous zlib stream per image. */
#define MUST3R_PNG_OUT_RGB8   0   /* uint8 [H][W][3] (MUST3R_IMG_U8_HWC): grey replicated, alpha dropped; 8-bit files only */
#define MUST3R_PNG_OUT_GRAY8  1   /* uint8 [H][W]; colour type 0 at 8 bits only */
#define MUST3R_PNG_OUT_GRAY16 2   /* uint16 [H][W], little-endian; colour type 0 at 16 bits only */
/* the status word of one image after a decode call; decoding of the image stops at the first of these */
#define MUST3R_PNG_STATUS_OK          0
#define MUST3R_PNG_STATUS_BLOCK_TYPE  1   /* deflate block type 3 */
#define MUST3R_PNG_STATUS_CODE_SET    2   /* an over-subscribed or otherwise invalid set of code lengths */
#define MUST3R_PNG_STATUS_CODE        3   /* bits that are no code of the table in use */
#define MUST3R_PNG_STATUS_SYMBOL      4   /* literal/length symbol 286 or 287, distance symbol 30 or 31 */
#define MUST3R_PNG_STATUS_DISTANCE    5   /* a distance beyond what has been written */
#define MUST3R_PNG_STATUS_OVERFLOW    6   /* output beyond the expected size */
#define MUST3R_PNG_STATUS_ENDS_EARLY  7   /* the stream ends inside a block */
#define MUST3R_PNG_STATUS_SIZE        8   /* the final size is not the expected one */
#define MUST3R_PNG_STATUS_STORED_LEN  9   /* a stored block whose LEN and ~LEN do not match */
#define MUST3R_PNG_STATUS_ADLER      10   /* the Adler-32 of the inflated bytes is not the trailer's */
#define MUST3R_PNG_STATUS_FILTER     11   /* a scanline with a filter type above 4 */
typedef struct must3r_hip_png_info {
    int32_t width, height;
    int32_t color_type, bit_depth;   /* 0 / 8, 0 / 16, 2 / 8 or 6 / 8 */
    int32_t channels, bpp;           /* samples per pixel; bytes per pixel, the step of the Sub / Average / Paeth filters */
    int32_t n_idat, reserved;
    int64_t rowbytes;                /* width * bpp */
    int64_t inflated_bytes;          /* height * (1 + rowbytes), at most 2^28 */
    int64_t idat_bytes;              /* the payloads of all IDAT chunks together: the zlib stream */
} must3r_hip_png_info;
typedef struct must3r_hip_png_range { uint64_t offset, length; } must3r_hip_png_range;   /* bytes from the start of the file */
/* 0: accepted, *info is filled (and idat_ranges, when max_ranges >= n_idat; with a smaller capacity only info is filled: query n_idat first).
 * 1: not accepted; `reason` (when not NULL, reason_bytes bytes) holds why as a C string.  No other outcome, no GPU call, no allocation. */
int must3r_hip_png_parse(const void* data, size_t nbytes, must3r_hip_png_info* info, must3r_hip_png_range* idat_ranges, size_t max_ranges,
                         char* reason, size_t reason_bytes);
typedef struct must3r_hip_png_image {
    const must3r_hip_png_info* info;   /* HOST: as must3r_hip_png_parse filled it */
    const void* zdata;                 /* DEVICE: the IDAT payloads back to back, info->idat_bytes bytes, 16-byte aligned and readable up to the next multiple of 16 */
    void*  out;                        /* DEVICE: [height][width] pixels of out_format, rows of out_row_stride bytes, 16-byte aligned */
    int64_t out_row_stride;
    int32_t out_format, reserved;      /* MUST3R_PNG_OUT_* */
    void*  inflated;                   /* DEVICE or NULL.  Not NULL: the scanlines are kept here and not in the scratch, info->inflated_bytes rounded up to a
                                          multiple of 256 plus 256 bytes, 256-byte aligned.  The first inflated_bytes bytes are the inflated stream with every
                                          scanline's bytes unfiltered in place (the filter-type bytes stay); what follows them is unspecified */
} must3r_hip_png_image;
typedef struct must3r_hip_png_batch {
    const must3r_hip_png_image* images;   /* HOST [n_images] */
    int32_t n_images, reserved;
    int32_t* status;         /* DEVICE [n_images], written: MUST3R_PNG_STATUS_* per image.  An image whose status is not OK has unspecified pixels */
    void*  scratch;          /* DEVICE, 256-byte aligned */
    size_t scratch_bytes;    /* >= must3r_hip_png_scratch_bytes of the same images */
    void*  stream;           /* hipStream_t: every copy, memset and launch of the call goes there; nothing is read back */
} must3r_hip_png_batch;
/* device bytes of scratch for one decode call of these images (0 on invalid descriptors): the descriptor table and, for every image without an `inflated`
 * buffer of its own, its inflated scanlines.  Only info and inflated of each image are read. */
size_t must3r_hip_png_scratch_bytes(const must3r_hip_png_image* images, int n_images);
/* Decodes the batch: png_inflate_kernel (one workgroup per image: the 32 KiB history, a staged stretch of the stream and the two decode tables in LDS),
 * png_adler_kernel (a parallel reduction over the inflated bytes against the stream's trailer), png_unfilter_kernel (a wave takes 64 consecutive rows,
 * skewed by one byte a row) and png_pack_kernel (the caller's layout).  A stream that is damaged sets the image's status word and stops that image's
 * inflate; every access stays in bounds and the other images are not affected. */
int must3r_hip_png_decode(const must3r_hip_png_batch* batch);

/* debug: lane -> element mapping of the gfx950 transposing LDS read the attention kernel relies on; writes 256 int16 */
int must3r_hip_debug_tr_probe(void* out256_i16_dev, void* stream);

/* ABI 21, additive.  The per-frame step of the SLAM agent (must3r/slam/model.py: get_camera_pose :147-172, get_overlap_score :62-91, mean_focal :131-137 and
 * the keyframe test of postproc_pred :231-235) as device work (csrc/slam.hip, must3r_amd/slam.py): everything between the decoder call and the keyframe
 * decision is enqueued on the descriptor's `stream` without a host read, then ONE record of MUST3R_SLAM_RECORD_DOUBLES doubles is copied back per frame.
 * All pointers are DEVICE pointers.
 *
 * must3r_hip_slam_pose: B >= 1 views of raw head output pm [B][H][W][7] -> activated pts3d / pts3d_local / conf (the launches and bits of
 * must3r_hip_postprocess_cam_act: the raw form costs one pass where the activated form would cost two), focal [B] (the Weiszfeld routine of csrc/cam.hip on
 * the UNrectified local points), c2w [B][4][4] and the rectified z of pts3d_local, written in place as fp32(z * ratio) with
 * ratio = fp32(fp32(seq_focal) / focal), what the reference's in-place multiply through a view leaves behind.
 *   focal_state  double [MUST3R_SLAM_FOCAL_STATE_DOUBLES] = (sum f_i c_i, sum c_i, n, sum f c / sum c), the agent's running sums in fp64, zeroed by the
 *                caller at reset.  seq_focal = sum f c / sum c is read from it on the device when use_seq_focal != 0; n == 0 there, use_seq_focal == 0 or a
 *                NULL focal_state mean "none" (ratio 1).  With update_focal != 0 (B must be 1) the view's f_i = focal and c_i = mean(conf - 1) (the fp64 sum of
 *                the registration weights over H W) are added AFTER seq_focal was read, (f_i, c_i) is written to focal_log[n] (when n < focal_log_cap;
 *                the caller grows the array by doubling) and n is advanced: mean_focal of the reference after its append.
 *   is_first     R = I, T = 0, no rectification (the focal and the sums are still computed).
 * Otherwise the registration of diag(1, 1, ratio) p_local -> p_world with weights conf - 1 is solved from the sums of the unrectified points (the
 * 3-vector and the 3 x 3 moment are rectified before the solve), so z is rewritten by one small pass and the pixels are not read a second time.
 * The cooperative exchange of csrc/cam.hip is reused unchanged: a launch that cannot be made co-resident fails with an error.
 * scratch: must3r_hip_slam_pose_scratch_bytes(B, H, W) bytes (the camera pass's exchange slots and partial sums + one ratio per view), 256-byte aligned.
 * Refused before anything is read or launched: a NULL descriptor, pm, pts3d, pts3d_local, conf, focal, c2w or scratch; B < 1, H or W not positive; an
 * unknown activation; update_focal with B != 1 or without focal_state; a negative focal_log_cap, or a positive one without focal_log; scratch too small.
 *
 * must3r_hip_slam_keyframe: the keyframe test of ONE frame from pts3d, the rectified pts3d_local and conf [H][W], and c2w [4][4] in device memory (the
 * camera centre is never a host argument).  Launches: slam_select_kernel (block 0: the mask conf > min_conf on the ::subsamp grid, its count n_sel, and the
 * selected world points and depths compacted in row-major grid order -- ballots and a running offset, no atomics; block 1: mean of conf, fixed-order fp64
 * sum, and the lower median of the full conf map, torch.median's value, by a 4 x 8-bit radix select), slam_walk_kernel (quadrant id of every selected point
 * against the device's camera centre and the exact walk of must3r_hip_nn_index_query, one text with it: csrc/nn_walk.hpp; d = double(dist), with
 * MUST3R_SLAM_MODE_NORM divided by double(fp32(z + 1e-9f)); +inf becomes DBL_MAX), slam_rank_kernel (the two order statistics numpy's linear percentile
 * interpolates between, virtual index (n_sel - 1) * quantile, by an 8 x 8-bit radix select on the fp64 values: exact) and slam_record_kernel (the score by
 * numpy's _lerp rule, a + (b - a) g, and b - (b - a)(1 - g) for g >= 0.5, every operation rounded; the record).  Counts in LDS are the only atomics and
 * decide no order: two runs give the same bits, and a frame's bits do not depend on the frame before it.
 *   index        a must3r_hip_nn_index_build buffer with the same `divider`, or NULL: an empty map, every distance DBL_MAX.
 *   subsamp      0 = every pixel (as 1).   quantile = percentile / 100 in fp64, in [0, 1].
 *   mode         MUST3R_SLAM_MODE_NN (walk, percentile score; n_sel == 0: score 0) with or without _NORM; else _MEANCONF or _MEDIANCONF: score = that statistic.
 *   sel          out, fp32 [candidates][3]: rows [0, n_sel) are pts3d[::s, ::s][msk].     dist  out, optional, fp32 [candidates]: rows [0, n_sel) the distances.
 *   focal, focal_state   optional, copied into the record (focal[0], focal_state[3]).
 *   record       out, double [MUST3R_SLAM_RECORD_DOUBLES]: n_sel, order statistic below, above, score, conf median, conf mean, focal, mean focal,
 *                camera centre (3), c2w (16), virtual index; the rest 0.
 * scratch: must3r_hip_slam_keyframe_scratch_bytes(H, W, subsamp) bytes (12 per candidate + 256), 256-byte aligned.
 * Refused before anything is read or launched: a NULL descriptor, pts3d, pts3d_local, conf, c2w, sel, record or scratch; H or W not positive or more than
 * 2^24 pixels; subsamp < 0; divider outside [0, 8]; quantile outside [0, 1] or NaN; no mode or an unknown mode bit, MUST3R_SLAM_MODE_NORM without _NN,
 * _NN together with a conf mode, both conf modes; scratch too small; sel, record or scratch not 8-byte aligned. */
#define MUST3R_SLAM_RECORD_DOUBLES 32
#define MUST3R_SLAM_FOCAL_STATE_DOUBLES 4
#define MUST3R_SLAM_MODE_NN 1
#define MUST3R_SLAM_MODE_NORM 2
#define MUST3R_SLAM_MODE_MEANCONF 4
#define MUST3R_SLAM_MODE_MEDIANCONF 8
typedef struct must3r_hip_slam_pose_args {
    const float* pm;            /* [B, H, W, 7] raw head output */
    float*  pts3d;              /* [B, H, W, 3] out */
    float*  pts3d_local;        /* [B, H, W, 3] out, z rectified */
    float*  conf;               /* [B, H, W] out */
    float*  focal;              /* [B] out */
    float*  c2w;                /* [B, 4, 4] out */
    double* focal_state;        /* [MUST3R_SLAM_FOCAL_STATE_DOUBLES], optional */
    double* focal_log;          /* [focal_log_cap, 2], optional */
    void*   scratch;
    size_t  scratch_bytes;
    int32_t B, H, W, activation;   /* MUST3R_ACT_* */
    int32_t is_first, use_seq_focal, update_focal, focal_log_cap;
    void* stream;               /* hipStream_t */
} must3r_hip_slam_pose_args;
size_t must3r_hip_slam_pose_scratch_bytes(int B, int H, int W);
int must3r_hip_slam_pose(const must3r_hip_slam_pose_args* a);
typedef struct must3r_hip_slam_keyframe_args {
    const float*  pts3d;        /* [H, W, 3] */
    const float*  pts3d_local;  /* [H, W, 3], z rectified */
    const float*  conf;         /* [H, W] */
    const float*  c2w;          /* [4, 4] */
    const float*  focal;        /* [1], optional */
    const double* focal_state;  /* [MUST3R_SLAM_FOCAL_STATE_DOUBLES], optional */
    const void*   index;        /* must3r_hip_nn_index_build's, optional */
    float*  sel;                /* [candidates, 3] out */
    float*  dist;               /* [candidates] out, optional */
    double* record;             /* [MUST3R_SLAM_RECORD_DOUBLES] out */
    void*   scratch;
    size_t  scratch_bytes;
    double  quantile;
    float   min_conf;
    int32_t H, W, subsamp, divider, mode;
    void* stream;               /* hipStream_t */
} must3r_hip_slam_keyframe_args;
size_t must3r_hip_slam_keyframe_scratch_bytes(int H, int W, int subsamp);
int must3r_hip_slam_keyframe(const must3r_hip_slam_keyframe_args* a);

/* ABI 21, additive: scene rendering.  A point rasteriser for headless previews (csrc/render.hip, must3r_amd/render.py): what the
 * reference shows through demo/viser.py and the open3d PipelineView of slam/slam.py -- the confidence-filtered point cloud seen from a pinhole camera -- as
 * colour, depth and source-index images on the device.  The views are the export's table (ABI 13): conf, pts, rgb, H, W and a 3 x 4 fp64 matrix M per view.
 *
 * must3r_hip_render: everything is enqueued on the descriptor's `stream`, nothing is read back, and the host waits only for the staging of the call's own
 * tables (a ring of 4 pinned slots per calling thread).  Two launches after one memset of the keys:
 *   splat    The host composes A[c][v] = w2c[c] . M[v] in fp64 with plain scalar loops: per element the three products summed in ascending k, then (in the
 *            last column) the translation added.  A source pixel with fp32 point (x, y, z) gives per camera, in fp64 with every operation rounded,
 *                X_a = ((A[a][0] x + A[a][1] y) + A[a][2] z) + A[a][3],   Z = X_2,   u = fx (X_0 (1.0 / Z)) + cx,   v = fy (X_1 (1.0 / Z)) + cy.
 *            It is dropped, before any conversion to an integer, when conf >= fp32(thr) fails (NaN never passes), when any of x, y, z, u, v is not finite,
 *            or when Z >= fp64(z_near) and Z <= fp64(z_far) fails.  Otherwise it covers the square of point_size pixels whose first column is
 *            floor(u - (point_size - 1) / 2) (a true floor: u = -0.3 lands in column -1) and whose first row is floor(v - (point_size - 1) / 2), clipped
 *            to the image, and every covered target pixel takes a 64-bit unsigned atomicMin of (bits(fp32(Z)) << 32) | global source index (views in
 *            table order, pixels row-major).  Z is positive there, so the bit pattern orders as the value does; an integer minimum does not depend on
 *            arrival order, so the images are repeatable bit for bit, and a tie in fp32 depth goes to the lower source index.
 *   resolve  one thread per target pixel: an empty key gives the background bytes, +inf depth and index 0xFFFFFFFF; otherwise the index, the depth fp32 of
 *            the key and the colour bytes rint(clip(c, 0, 1) * 255) of the source pixel (the export's rule).
 * All cameras of one call share (W, H).  Outputs: rgb uint8 [n_cams][H][W][3], depth float32 [n_cams][H][W], index uint32 [n_cams][H][W]; any may be NULL (a
 * view's rgb plane may be NULL when the rgb output is).
 * scratch: must3r_hip_render_scratch_bytes(desc) bytes, 256-byte aligned = four sections, each rounded up to 256 bytes: 40 n_views (view table),
 * 40 n_cams (camera table), 96 n_cams n_views (A) and 8 n_cams H W (keys); 0 with a message on a bad descriptor (its scratch and outputs are not looked at).
 * Refused before anything is read, uploaded or launched: a NULL descriptor or table; n_views or n_cams < 1; point_size outside
 * [1, MUST3R_RENDER_MAX_POINT_SIZE]; a view or a camera with a non-positive size; cameras of different sizes; a camera without 0 < z_near <= z_far < inf; a
 * view of 2^31 or a scene of 2^32 or more pixels; 2^31 or more target pixels; a NULL, small or misaligned scratch; a view with a NULL plane. */
#define MUST3R_RENDER_MAX_POINT_SIZE 8
typedef struct must3r_hip_render_camera {
    double w2c[12];             /* row-major 3x4, world to camera, OpenCV axes: x right, y down, z forward */
    double fx, fy, cx, cy;
    float z_near, z_far;
    int32_t W, H;
} must3r_hip_render_camera;
typedef struct must3r_hip_render_desc {
    const must3r_hip_export_view* views;    /* HOST [n_views] */
    const must3r_hip_render_camera* cams;   /* HOST [n_cams] */
    int32_t n_views, n_cams;
    float thr;
    int32_t point_size;
    uint8_t background[3];
    uint8_t reserved[5];
    void* scratch;
    size_t scratch_bytes;
    uint8_t* rgb;               /* [n_cams, H, W, 3] out, optional */
    float* depth;               /* [n_cams, H, W] out, optional */
    uint32_t* index;            /* [n_cams, H, W] out, optional */
    void* stream;               /* hipStream_t */
} must3r_hip_render_desc;
size_t must3r_hip_render_scratch_bytes(const must3r_hip_render_desc* d);
int must3r_hip_render(const must3r_hip_render_desc* d);

/* ABI 21, additive: scene rendering, triangles.  A second primitive for the same three images (csrc/render_mesh.hip, csrc/render_tri.hpp; DESIGN.md
 * section 14.1): the triangles of the exported mesh (must3r_hip_export_scatter_faces), rasterised under the point path's guarantees -- fp64 with every
 * operation rounded, the same 64-bit key z-buffer, everything on the descriptor's `stream`, nothing read back, one staging slot.  must3r_hip_render, its
 * descriptor and its bits are unchanged.
 *   triangles   Per view, each quad anchored at pixel i = r W + c with r < H - 1, c < W - 1 has the corners a = i, b = i + 1, c' = i + W, d = i + W + 1; kind 0
 *               is (a, b, c'), kind 1 is (b, c', d).  The export writes each in both windings, so the renderer is double-sided and draws each once.
 *               Triangle id = 2 (global source index of the anchor) + kind; a scene of 2^31 or more pixels is refused.  A view with H < 2 or W < 2 has no
 *               triangle; that is no error.
 *   vertices    Each corner is projected exactly as the point path projects a source pixel (A = w2c . M, X_a, Z, u, v above).  A triangle is dropped, before
 *               any conversion to an integer, when any corner fails the point path's tests: conf >= fp32(thr), finite x, y, z, u, v, and
 *               z_near <= Z <= z_far.  There is no near-plane clipping: a triangle with a corner outside the depth range is dropped whole.
 *   candidates  Target pixel (q, r) is sampled at its centre px = q + 0.5, py = r + 0.5 (a point at u lands in column floor(u)).  Columns run from
 *               ceil(min(u_k) - 0.5) to floor(max(u_k) - 0.5) inclusive, rows likewise, both clipped to the image with fp64 comparisons before any integer
 *               is formed (u may be 1e300).
 *   coverage    Number the corners 0, 1, 2 in the order given above, which is ascending source index.  For an edge from corner j to corner k,
 *                   E_jk(p) = (u_k - u_j) * (py - v_j) - (v_k - v_j) * (px - u_j).
 *               s0 = E_01, s1 = E_12, s2 = -E_02, den = (s0 + s1) + s2.  The pixel is covered when den is finite and non-zero and s0, s1, s2 are all >= 0
 *               or all <= 0 (comparisons are false on NaN).  Every edge shared by two triangles is evaluated from its lower-index endpoint in both -- (b, c')
 *               inside a quad, (b, d) / (a, c') across columns, (c', d) / (a, b) across rows -- so both see the same bits and the inclusive test leaves no
 *               crack between them; double coverage is harmless under a minimum.
 *   depth       Perspective-correct: lam0 = s1 / den, lam1 = s2 / den, lam2 = s0 / den; t_k = lam_k * (1.0 / Z_k); iz = (t0 + t1) + t2; Zp = 1.0 / iz.  The
 *               key is (bits(fp32(Zp)) << 32) | triangle id, taken by the same 64-bit unsigned atomicMin behind the same plain-load early-out.  There is no
 *               depth-range test after interpolation.  A tie in fp32 depth goes to the lower triangle id.
 *   resolve     An empty key gives the background, +inf and 0xFFFFFFFF; otherwise the depth is the key's fp32 and `index` is the triangle id.  For colour the
 *               resolve thread recomputes the triangle's three projections, s, lam, t and Zp at its own pixel from the id; per channel
 *               c = ((t0 * c0 + t1 * c1) + t2 * c2) * Zp on the corners' fp32 colours widened to fp64, and the byte is the export's
 *               rint(clip(fp32(c), 0, 1) * 255).  Nothing per pixel is stored beyond the 8-byte key.
 * A triangle whose candidate box holds at most MUST3R_RENDER_MESH_WAVE_AREA target pixels is rasterised by the lane that owns its anchor; a larger one is
 * taken by its whole wavefront, whose 64 lanes stride the box.  The result is a minimum over the same (pixel, key) pairs either way.
 * Outputs, scratch (the same four sections and sizes: must3r_hip_render_mesh_scratch_bytes) and refusals are must3r_hip_render's, without point_size and with
 * the scene of 2^31 or more pixels. */
/* Swept on the benchmark scene (200 coherent views of 384 x 512 into 512 x 384; profiles/render_mesh_scratch_builds.jsonl, medians of 7): 8 close cameras take
 * 24.1 / 16.6 / 15.0 / 15.0 / 15.0 ms at 4 / 16 / 64 / 256 / 1024 and 14.9 ms with the wave path compiled out; 120 orbit cameras 82.5 / 82.9 / 82.2 / 82.5 /
 * 82.6 ms and 79.0 ms.  A small value hands mid-sized triangles to 64 lanes that mostly idle; from 64 on, one wavefront's worth of samples, the value no longer
 * shows, because that scene holds almost no larger triangle (241 of 31.7 M at the close cameras).  64 is the smallest value without a measured cost. */
#define MUST3R_RENDER_MESH_WAVE_AREA 64
typedef struct must3r_hip_render_mesh_desc {
    const must3r_hip_export_view* views;    /* HOST [n_views] */
    const must3r_hip_render_camera* cams;   /* HOST [n_cams] */
    int32_t n_views, n_cams;
    float thr;
    uint8_t background[3];
    uint8_t reserved[1];
    void* scratch;
    size_t scratch_bytes;
    uint8_t* rgb;               /* [n_cams, H, W, 3] out, optional */
    float* depth;               /* [n_cams, H, W] out, optional */
    uint32_t* index;            /* [n_cams, H, W] out, optional: triangle ids */
    void* stream;               /* hipStream_t */
} must3r_hip_render_mesh_desc;
size_t must3r_hip_render_mesh_scratch_bytes(const must3r_hip_render_mesh_desc* d);
int must3r_hip_render_mesh(const must3r_hip_render_mesh_desc* d);

/* timing hooks used by bench.py: per-stage HIP-event timers recorded on the call's stream */
int must3r_hip_set_profiling(must3r_hip_ctx* ctx, int enabled);
/* returns the number of records written (<= max); each record: name (<=31 chars), milliseconds, flops.
 * First the kernel CLASSES (gemm128, gemm64, attn_self, attn_cross, attn_combine, layernorm, misc), then (ABI 6) one row per kernel
 * symbol, names prefixed "k:" -- GEMMs "k:<family>/e<epilogue>/w<1 plain|2 split>/n<tile width>", attention "k:attn3/q32/cross" ... --
 * so that every row can be matched with one symbol of a rocprofv3 --kernel-trace of the same command. */
typedef struct must3r_hip_prof_record { char name[32]; double ms; double flops; int64_t calls; } must3r_hip_prof_record;
int must3r_hip_get_profile(must3r_hip_ctx* ctx, must3r_hip_prof_record* out, int max, int reset);

#ifdef __cplusplus
}
#endif
#endif /* MUST3R_HIP_H */
