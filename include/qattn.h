/*
 * qattn.h — C ABI of libqattn.so, the MI355X (gfx950) hot path of selau642/QuantizedAttention.
 *
 * The reference (three Python modules over Helion/Triton kernels) has no native boundary of its
 * own: each entry point below replaces one @helion.kernel call (or the torch glue around it) and is
 * cited as reference `file:line`.  The Python mirror of the reference's public functions
 * (quantizedattention_amd/attention_{int8,bf16,jvp}.py) binds exactly these symbols through ctypes
 * (quantizedattention_amd/_lib.py); INTEGRATION.md shows the binding for other hosts.
 *
 * Conventions (all entries):
 *   - Plain device pointers (HBM, allocated by the caller, contiguous row-major), sizes as long/int,
 *     `stream` is a hipStream_t (NULL = the default stream).  Work is enqueued asynchronously on
 *     `stream`; nothing is synchronised and no memory is allocated by the library.
 *   - Return value: 0 = enqueued, 1 = unsupported shape / argument (nothing launched),
 *     2 = launch failure (hipGetLastError() != hipSuccess).
 *   - "rows" N = BH * S with BH = batch * heads; tensors [B,H,S,D] are addressed as [BH*S, D].
 *     Block-scale arrays hold one fp16 per 32 consecutive rows: index (b*H+h)*S/32 + s/32
 *     (attention_int8.py:161-168).
 *   - qks = fp32(1/sqrt(D) * 1.44269504) (attention_int8.py:151-153, attention_bf16.py:188-190);
 *     sms = fp32(1/sqrt(D)).  lse values are base-2 (log2 of the softmax denominator plus max).
 *   - head_dim D in {64, 128}.  Dtypes: i8 = int8_t, f16 = _Float16 (IEEE half), bf16 = bfloat16,
 *     f32 = float.
 */
#ifndef QATTN_H
#define QATTN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- versioning
 * QATTN_ABI_VERSION counts incompatible changes of the entries below (a changed argument list under
 * an old name; INTEGRATION.md §"ABI versions" lists them).  A host compiled against this header
 * checks qattn_abi_version() == QATTN_ABI_VERSION after loading the library and refuses to call it
 * otherwise: a library of another version would read its arguments with another meaning.
 * qattn_source_hash() is the sha256 (hex) of the kernel sources and compile flags the library was
 * built from (quantizedattention_amd/_srchash.py); the Python binding refuses a library whose hash
 * differs from the sources beside it (a stale prebuilt library). */
#define QATTN_ABI_VERSION 8
int qattn_abi_version(void);
const char* qattn_source_hash(void);

/* ---------------------------------------------------------------- what every attention entry keeps
 * Status: 0 done (or nothing to do), 1 an argument the entry does not support (nothing was launched),
 * 2 a launch failed.
 * Empty problems.  No query rows (bh == 0 or sq == 0, whatever sk is) is nothing to do: status 0,
 * no launch, no pointer read -- for arguments that are valid otherwise: the shape checks come first,
 * so group >= 1 and bh % group == 0 still hold (a host with no query heads passes group = 1, not
 * Hq / Hkv = 0, or skips the call as the Python wrappers do).  Query rows without keys (sk == 0 with bh > 0 and sq > 0) are refused
 * with status 1 by every forward and backward entry of every path -- int8, bf16, JVP and MX-FP4
 * alike: every query keeps a key (a softmax over no keys has no value, and a gradient through it
 * none either).
 * Addresses.  Every tensor pointer is 16-byte aligned: the kernels read 16-byte vectors and LDS-DMA
 * dwordx4 from the base addresses.  The entries do not check it (qattn_bf16_fwd_ws_ex's ws apart);
 * the Python binding and the TORCH_LIBRARY operators copy a misaligned input and refuse a misaligned
 * buffer before they call. */

/* ---------------------------------------------------------------- int8 path (attention_int8.py) */

/* Per-32-row block quantiser (attention_int8.py:178-186 q, 188-195 k, 241-247 v).
 *   x      f16 [rows, D]              in
 *   idx    i8  [rows, D]              out: trunc(RNE_f16(f32(x') / f32(s)))
 *   scale  f16 [rows/32]              out: s = RNE_f16(amax|x'| / 127)   (all-zero block: s = 0, idx 0)
 *   deq    f16 [rows, D] or NULL      out: f16(idx * s)  (the fp16 operand of the forward P.V product)
 *   kmean  f16 [rows/rows_per_head, D] or NULL: when given, x' = f16(x - kmean[head]) (k-smoothing,
 *          build contract for attention_int8.py:24-25), else x' = x.
 * Bit-exact with the reference's eager-torch rounding.  rows % 32 == 0. */
int qattn_int8_quant(const void* x, void* idx, void* scale, void* deq, const void* kmean, long rows,
                     int rows_per_head, int head_dim, void* stream);
/* Same, with an optional exact bf16 image of idx (img bf16 [rows, D], or NULL): the backward's
 * transposed-read operand for q and k, written in the same pass.  deq and img are exclusive. */
int qattn_int8_quant_img(const void* x, void* idx, void* scale, void* deq, void* img,
                         const void* kmean, long rows, int rows_per_head, int head_dim,
                         void* stream);

/* deq = f16(idx * s) with s the block scale of each 32-row block (rows % 32 == 0): the quantiser's
 * deq output rebuilt from stored indices and scales (the int8 key/value cache of kv_cache.py). */
int qattn_int8_dequant(const void* idx, const void* scale, void* deq, long rows, int head_dim,
                       void* stream);

/* V quantiser for the int8 P.V product (attention_int8.py:241-247, same indices and scales as
 * qattn_int8_quant) that also writes the V^T operand image of those indices:
 *   v f16 [rows, D] -> v_i8 i8 [rows, D], sv f16 [rows/32] (bit-exact, as qattn_int8_quant) and
 *   vt i8 [rows/32][D/32][64][16]: for each 32-row block and 32-wide d block b, lane L = 32h + c holds
 *   v_i8[row pi(h, j)][32b + c], j = 0..15, pi(h, j) = (j & 3) + 8(j >> 2) + 4h (the A operand of
 *   v_mfma_i32_32x32x32_i8 in the forward's key order).  rows % 32 == 0. */
int qattn_int8_quant_vt(const void* v, void* v_i8, void* sv, void* vt, long rows, int head_dim,
                        void* stream);
/* vt of qattn_int8_quant_vt from stored indices v_i8 (a restored int8 key/value cache). */
int qattn_int8_v_image(const void* v_i8, void* vt, long rows, int head_dim, void* stream);

/* k_mean = f16(mean over the S tokens of each head) — k f16 [bh*seq, D] -> kmean f16 [bh, D]
 * (SageAttention smoothing; replaces the crashing `k.mean(0)` of attention_int8.py:24-25). */
int qattn_kmean(const void* k, void* kmean, long bh, long seq, int head_dim, void* stream);

/* qattn_kmean followed by qattn_int8_quant_img of the smoothed k, in one launch (attention_int8.py:
 * 24-25 smoothing, 188-195 k quantiser): kmean f16 [bh, D], k_i8 i8 [bh*seq, D], sk f16
 * [bh*seq/32] and (k_bf != NULL) the bf16 image bf16(k_i8) out, bit-identical with the two calls.
 * seq % 32 == 0. */
int qattn_int8_quant_k_smooth(const void* k, void* kmean, void* k_i8, void* sk, void* k_bf, long bh,
                              long seq, int head_dim, void* stream);

/* int8 SageAttention-3 forward, per (batch, head) (attention_int8.py:197-257; per-head contract F2).
 *   q_i8, k_i8  i8 [bh*seq, D]; sq, sk, sv f16 [bh*seq/32]; vt = the V^T operand image of
 *   qattn_int8_quant_vt; out O f16 [bh*seq, D]; lse f16 [bh*seq] (base 2).
 *   S = f16(f32(q_i8.k_i8) * sq*sk*qks), P = exp2(S - m), P_i8 = trunc(P / sp) with sp =
 *   exp2(rowmax - m)/127, and the P.V contraction on the int8 MFMA as the reference's
 *   hl.dot(P_int8, v_int8) (int8:249): each 32-key tile's exact int32 product is dequantised by
 *   sp * sv (int8:249-250).  seq % 32 == 0. */
int qattn_int8_attn_fwd(const void* q_i8, const void* sq, const void* k_i8, const void* sk,
                        const void* vt, const void* sv, void* out, void* lse, long bh, long seq,
                        int head_dim, float qks, void* stream);

/* Generalised shapes (the reference's int8 path has none of these): bh = batch *
 * query heads with sq_tok query rows each; the key/value tensors have bh / group heads of sk_tok
 * rows (query head h reads key/value head h / group: grouped-query attention); causal = 1 keeps
 * key <= query (top-left aligned positions), causal = 2 keeps key <= query + sk_tok - sq_tok
 * (bottom-right aligned: new queries against a key/value cache, sk_tok >= sq_tok); masked scores
 * are excluded.  Block scales index the
 * query rows and the key/value rows separately.  sq_tok % 32 == sk_tok % 32 == 0, bh % group == 0.
 * qattn_int8_attn_fwd is this with sq_tok = sk_tok = seq, group = 1, causal = 0.
 * The forward marks the (rare) waves whose literal-P-chain vote still holds at the end and redoes
 * them: qattn_int8_attn_fwd_qf in the same kernel, the entries on pre-quantised q
 * (and the split entry) with a second kernel on `stream`. */
int qattn_int8_attn_fwd_ex(const void* q_i8, const void* sq, const void* k_i8, const void* sk,
                           const void* vt, const void* sv, void* out, void* lse, long bh,
                           long sq_tok, long sk_tok, int group, int causal, int head_dim,
                           float qks, void* stream);

/* qattn_int8_attn_fwd_ex quantising q inside the attention kernel (the reference quantises inside its
 * forward, attention_int8.py:178-186): q f16 [bh*sq_tok, D] in; q_i8 i8 [bh*sq_tok, D] and sq f16
 * [bh*sq_tok/32] out, bit-exact with qattn_int8_quant; q_bf bf16 [bh*sq_tok, D] = bf16(q_i8) out
 * (the backward's image) when not NULL.  O and lse as qattn_int8_attn_fwd_ex on those q_i8, sq. */
int qattn_int8_attn_fwd_qf(const void* q, void* q_i8, void* sq, void* q_bf, const void* k_i8,
                           const void* sk, const void* vt, const void* sv, void* out, void* lse,
                           long bh, long sq_tok, long sk_tok, int group, int causal, int head_dim,
                           float qks, void* stream);

/* Key-split (flash-decoding) form of qattn_int8_attn_fwd_ex, non-causal, for short query blocks
 * against long key ranges (the int8 key/value cache): each workgroup covers
 * keys_per_split keys (multiple of 32) of its query rows and writes the partial softmax state
 *   opart f16 [nsplit][bh*sq_tok][D] = O_s / l_s (the key range's normalised output) and
 *   ml f32x2 [nsplit][bh*sq_tok] = {running max m_s, row sum l_s}, nsplit = ceil(sk_tok/keys_per_split);
 * qattn_int8_split_combine merges the splits into out f16 [rows, D] and lse f16 [rows] (rows =
 * bh*sq_tok): w_s = 2^(m_s - M) l_s, O = sum_s w_s opart_s / sum_s w_s, lse = f16(M + f16(log2 L)).
 * head_dim 128 only for the split forward (returns 1 otherwise). */
int qattn_int8_attn_fwd_split(const void* q_i8, const void* sq, const void* k_i8, const void* sk,
                              const void* vt, const void* sv, void* opart, void* ml, long bh,
                              long sq_tok, long sk_tok, int group, int keys_per_split, int head_dim,
                              float qks, void* stream);
int qattn_int8_split_combine(const void* opart, const void* ml, void* out, void* lse, long rows,
                             int nsplit, int head_dim, void* stream);

/* Backward prologue, one pass (attention_int8.py:372-374, 398): dO f16 -> dO_i8 [rows, D] + sdO f16
 * [rows/32] (same quantiser), dO_bf = bf16(dO_i8) [rows, D] (optional, NULL to skip), and LD f32x2
 * [rows] = {f32(lse), f32(f16(rowsum(dO*O)))}. */
int qattn_int8_bwd_prep(const void* dO, const void* O, const void* lse, void* dO_i8, void* sdO,
                        void* LD, void* dO_bf, long bh, long seq, int head_dim, void* stream);

/* Exact widening copy i8 -> bf16 of n elements (n % 16 == 0): the transposed-read operand images
 * of q_i8, k_i8, dO_i8 used by the dK / dQ / dV products (no reference counterpart). */
int qattn_i8_to_bf16(const void* x, void* y, long n, void* stream);

/* Corrected int8 backward (attention_int8.py:268-432 with SURVEY F4 fixed: dS = P*(dP - D),
 * sm_scale, deterministic per-head accumulation, k_mean term dropped since rowsum(dS) = 0).
 * Quantisation granularity as the reference: P and dS per 32x32 tile (amax/127, trunc), dO per
 * 32-row block, q/k/v int8 + scales from the forward.  Launches the dV, dK and dQ kernels.
 *   dq, dk, dv f16 [bh*seq, D] out; q_bf/k_bf/dO_bf = qattn_i8_to_bf16 images. */
int qattn_int8_attn_bwd(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                        const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                        const void* LD, const void* q_bf, const void* k_bf, const void* dO_bf,
                        void* dq, void* dk, void* dv, long bh, long seq, int head_dim, float qks,
                        float sms, void* stream);

/* qattn_int8_attn_bwd for the generalised shapes of qattn_int8_attn_fwd_ex: dq, dO and the
 * query-side tensors have bh heads of sq_tok rows, dk, dv and the key/value side bh / group heads of
 * sk_tok rows (dk, dv of a key/value head sum over its group of query heads). */
int qattn_int8_attn_bwd_ex(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                           const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                           const void* LD, const void* q_bf, const void* k_bf, const void* dO_bf,
                           void* dq, void* dk, void* dv, long bh, long sq_tok, long sk_tok, int group,
                           int causal, int head_dim, float qks, float sms, void* stream);

/* qattn_int8_attn_bwd_ex with a caller-provided dS workspace (no recomputation in the dQ pass):
 * the fused dK+dV kernel also stores each quantised 32x32 dS tile (dS_i8, 1 KiB, and its scale
 * s_dS) in ws, and the dQ kernel reads them back instead of recomputing S, dP, P and dS
 * (attention_int8.py:399-420).  dq, dk, dv are bit-identical to qattn_int8_attn_bwd_ex's.
 * ws must hold qattn_int8_bwd_ws_bytes(bh, sq_tok, sk_tok) bytes, 16-byte aligned; it is scratch
 * (overwritten, not read before written).  Returns 1 for ws == NULL, and for a shape whose records the
 * kernels cannot address: group * (sq_tok/32) * (sk_tok/32) KiB per key/value head of 2^31 bytes or
 * more, group * sq_tok/32 > QATTN_WS_MAX_QUERY_TILES or sk_tok/32 > QATTN_WS_MAX_KEY_TILES (the
 * per-tile tables the dK+dV and the dQ kernel keep in LDS; qattn_int8_bwd_plan answers 0, recompute,
 * for the same shapes). */
#define QATTN_WS_MAX_QUERY_TILES 1790
#define QATTN_WS_MAX_KEY_TILES 2800
long qattn_int8_bwd_ws_bytes(long bh, long sq_tok, long sk_tok);
/* The largest dS-record workspace the backwards (int8 and bf16 alike) allocate before they fall back
 * to recomputation: QATTN_BWD_WS_MAX bytes if that is set, else 16 GiB (a workspace allocation
 * that fails also falls back to recomputation). */
long qattn_bwd_ws_cap(void);
int qattn_int8_attn_bwd_ws(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                           const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                           const void* LD, const void* q_bf, const void* k_bf, const void* dO_bf,
                           void* dq, void* dk, void* dv, void* ws, long bh, long sq_tok, long sk_tok,
                           int group, int causal, int head_dim, float qks, float sms, void* stream);

/* qattn_int8_attn_bwd_ws in chunks of kv_chunk key/value heads (each with its group query heads):
 * dK+dV then dQ per chunk, every chunk re-using the same ws, which must hold
 * qattn_int8_bwd_ws_bytes(kv_chunk * group, sq_tok, sk_tok) bytes.  Bit-identical to
 * qattn_int8_attn_bwd_ws; a chunk's records can stay in the Infinity Cache between the two passes.
 * Returns 1 for ws == NULL or kv_chunk < 1. */
int qattn_int8_attn_bwd_wsc(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                            const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                            const void* LD, const void* q_bf, const void* k_bf, const void* dO_bf,
                            void* dq, void* dk, void* dv, void* ws, long kv_chunk, long bh,
                            long sq_tok, long sk_tok, int group, int causal, int head_dim, float qks,
                            float sms, void* stream);

/* The two parts of qattn_int8_attn_bwd_ws (square, ungrouped, non-causal), launchable alone:
 * dK + dV writing the dS workspace, then dQ reading it. */
int qattn_int8_bwd_dkdv_ws(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                           const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                           const void* LD, const void* q_bf, const void* dO_bf, void* dk, void* dv,
                           void* ws, long bh, long seq, int head_dim, float qks, float sms,
                           void* stream);
int qattn_int8_bwd_dq_ws(const void* k_bf, const void* sk, void* dq, void* ws, long bh, long seq,
                         int head_dim, float sms, void* stream);

/* The parts of qattn_int8_attn_bwd, launchable alone (per-kernel timing / overlap):
 * dK and dV (attention_int8.py:375-378, 423-428), dV only, dK only, dQ only (414-420). */
int qattn_int8_bwd_dkdv(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                        const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                        const void* LD, const void* q_bf, const void* dO_bf, void* dk, void* dv,
                        long bh, long seq, int head_dim, float qks, float sms, void* stream);
int qattn_int8_bwd_dv(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                      const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                      const void* LD, const void* q_bf, const void* dO_bf, void* dk, void* dv,
                      long bh, long seq, int head_dim, float qks, float sms, void* stream);
int qattn_int8_bwd_dk(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                      const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                      const void* LD, const void* q_bf, const void* dO_bf, void* dk, void* dv,
                      long bh, long seq, int head_dim, float qks, float sms, void* stream);
int qattn_int8_bwd_dq(const void* dO_i8, const void* sdO, const void* q_i8, const void* sq,
                      const void* k_i8, const void* sk, const void* v_i8, const void* sv,
                      const void* LD, const void* k_bf, void* dq, long bh, long seq, int head_dim,
                      float qks, float sms, void* stream);

/* ---------------------------------------------------------------- bf16 path (attention_bf16.py) */

/* FA2 forward with the reference's "multiple-max" beta rule emulated per 16-key sub-tile
 * (helion_atten_bf16_fwd_training, attention_bf16.py:107-296).
 *   q, k f16 [bh*sq|sk, D]; v bf16 [bh*sk, D]; out O f32 [bh*sq, D]; lse f32 [bh*sq] (base 2).
 *   causal: strict-lower mask with fill -126 in raw logit units (attention_bf16.py:222-233).
 *   sq % 32 == 0, sk % 32 == 0. */
int qattn_bf16_fwd(const void* q, const void* k, const void* v, void* out, void* lse, long bh,
                   long sq, long sk, int head_dim, int causal, float qks, void* stream);

/* qattn_bf16_fwd with grouped-query attention: bh = batch * query heads, k and v
 * have bh / group heads (query head h reads key/value head h / group).  qattn_bf16_fwd is group = 1. */
int qattn_bf16_fwd_ex(const void* q, const void* k, const void* v, void* out, void* lse, long bh,
                      long sq, long sk, int group, int causal, int head_dim, float qks, void* stream);

/* Size in bytes of the V-suffix workspace of qattn_bf16_fwd_ws_ex: bh_kv*(sk/32+1)*head_dim*4. */
long qattn_bf16_fwd_ws_bytes(long bh_kv, long sk, int head_dim);
/* qattn_bf16_fwd_ex with a scratch workspace (16-byte aligned, qattn_bf16_fwd_ws_bytes(bh / group,
 * sk, head_dim) bytes) for the causal case: the per-head suffix sums of V are written there first and
 * replace the fully masked sub-tiles past each 32-query block's diagonal (whose P is one constant,
 * attention_bf16.py:222-285), so the causal forward streams half the key tiles.  Same outputs as
 * qattn_bf16_fwd_ex up to fp32 summation order.  Non-causal calls, and ws == NULL, ignore it. */
int qattn_bf16_fwd_ws_ex(const void* q, const void* k, const void* v, void* out, void* lse, long bh,
                         long sq, long sk, int group, int causal, int head_dim, float qks, void* ws,
                         void* stream);

/* Backward prologue, one pass: dO f32 -> dO_bf bf16 [rows, D] and LD f32x2 [rows] =
 * {lse[row], D = rowsum(dO*O)} (attention_bf16.py:416, computed once per row instead of per tile). */
int qattn_bf16_bwd_prep(const void* dO, const void* O, const void* lse, void* dO_bf, void* LD, long bh,
                        long seq, int head_dim, void* stream);

/* y = bf16(x) (round to nearest even) for n fp16 elements, n % 8 == 0: the transposed-read images of
 * q (dK product) and k (dQ product) of qattn_bf16_bwd (no reference counterpart). */
int qattn_f16_to_bf16(const void* x, void* y, long n, void* stream);

/* Corrected FA2 backward (helion_flash_atten_2_algo_4_bwd, attention_bf16.py:299-448 with SURVEY F3
 * fixed: dS = P*(dP - D), sm_scale, deterministic dq).  q, k f16; v bf16; dO_bf, LD from
 * qattn_bf16_bwd_prep; q_bf, k_bf = qattn_f16_to_bf16 images of q, k.  Out dq [bh*sq, D], dk, dv
 * [bh*sk, D] f32.  Launches one fused dK+dV kernel and one dQ kernel.  sq % 32 == 0,
 * sk % 32 == 0. */
int qattn_bf16_bwd(const void* q, const void* k, const void* v, const void* dO_bf, const void* LD,
                   const void* q_bf, const void* k_bf, void* dq, void* dk, void* dv, long bh, long sq,
                   long sk, int head_dim, int causal, float qks, float sms, void* stream);

/* qattn_bf16_bwd for grouped-query attention: dk, dv [bh/group * sk, D] sum over the group of
 * query heads of their key/value head; q_bf, k_bf as the query / key tensors. */
int qattn_bf16_bwd_ex(const void* q, const void* k, const void* v, const void* dO_bf, const void* LD,
                      const void* q_bf, const void* k_bf, void* dq, void* dk, void* dv, long bh, long sq,
                      long sk, int group, int causal, int head_dim, float qks, float sms, void* stream);

/* Size in bytes of the dS record workspace of qattn_bf16_bwd_ws_ex: bh*(sq/32)*(sk/32)*2048
 * (2 B per score), or -1 for sizes that are not multiples of 32. */
long qattn_bf16_bwd_ws_bytes(long bh, long sq, long sk);

/* qattn_bf16_bwd_ex whose fused dK+dV kernel also stores every bf16 dS tile in ws (device,
 * qattn_bf16_bwd_ws_bytes bytes) and whose dQ pass reads them instead of recomputing S and dP:
 * bit-identical dq, dk, dv. */
int qattn_bf16_bwd_ws_ex(const void* q, const void* k, const void* v, const void* dO_bf,
                         const void* LD, const void* q_bf, const void* k_bf, void* dq, void* dk,
                         void* dv, long bh, long sq, long sk, int group, int causal, int head_dim,
                         float qks, float sms, void* ws, void* stream);

/* qattn_bf16_bwd_ex with separate dV and dK kernels (each recomputes S; two waves per SIMD each):
 * bit-identical dk, dv to the fused kernel; kept for the parity test and as a timing reference. */
int qattn_bf16_bwd_split_ex(const void* q, const void* k, const void* v, const void* dO_bf,
                            const void* LD, const void* q_bf, const void* k_bf, void* dq, void* dk,
                            void* dv, long bh, long sq, long sk, int group, int causal, int head_dim,
                            float qks, float sms, void* stream);

/* ---------------------------------------------------------------- JVP (attention_jvp.py) */

/* Forward-mode tangent attention (helion_attention_jvp_forward_fp32, attention_jvp.py:24-195):
 *   q, k, v, tq, tk, tv bf16 [bh*sq|sk, D]; out O, tO f32 [bh*sq, D]; lse f32 [bh*sq] (base 2).
 *   tO = (P.tV + (P o tS).V - rowsum(P o tS) * O) / l with tS = (tq.k^T + q.tk^T) * sm.
 *   flags must be 0 (reserved).  sq % 32 == 0, sk % 64 == 0. */
int qattn_jvp_fwd(const void* q, const void* k, const void* v, const void* tq, const void* tk,
                  const void* tv, void* out, void* tout, void* lse, long bh, long sq, long sk,
                  int head_dim, int flags, float qks, float sm, void* stream);

/* fp32-accurate JVP (the reference's fp32 contract, SURVEY §8c "fp32 mode"): every operand is given
 * as two bf16 images x = hi + lo (qattn_split_bf16) and every product runs as
 * hi*hi + hi*lo + lo*hi + lo*lo on the bf16 MFMA (exact up to the 2^-17 split residual, fp32
 * accumulation).  Same outputs and
 * conventions as qattn_jvp_fwd; sq % 32 == 0, sk % 32 == 0. */
int qattn_jvp_fwd_x3(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo,
                     const void* v_hi, const void* v_lo, const void* tq_hi, const void* tq_lo,
                     const void* tk_hi, const void* tk_lo, const void* tv_hi, const void* tv_lo,
                     void* out, void* tout, void* lse, long bh, long sq, long sk, int head_dim,
                     float qks, float sm, void* stream);

/* qattn_jvp_fwd / qattn_jvp_fwd_x3 with grouped-query attention (SURVEY §8f N2 for the JVP path):
 * bh = batch * query heads; k, v, tk, tv have bh / group heads (query head h reads key/value head
 * h / group).  The reference's JVP kernel takes equal head counts (jvp:33-41). */
int qattn_jvp_fwd_ex(const void* q, const void* k, const void* v, const void* tq, const void* tk,
                     const void* tv, void* out, void* tout, void* lse, long bh, long sq, long sk,
                     int group, int head_dim, float qks, float sm, void* stream);
int qattn_jvp_fwd_x3_ex(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo,
                        const void* v_hi, const void* v_lo, const void* tq_hi, const void* tq_lo,
                        const void* tk_hi, const void* tk_lo, const void* tv_hi, const void* tv_lo,
                        void* out, void* tout, void* lse, long bh, long sq, long sk, int group,
                        int head_dim, float qks, float sm, void* stream);

/* Primal-only forward of the JVP kernel (O, lse; no tangent operands or chains): the forward of
 * AttentionJVP_autograd_function, whose jvp() then runs qattn_jvp_fwd_ex once.
 * O / lse are bit-identical to those qattn_jvp_fwd_ex / qattn_jvp_fwd_x3_ex return for the same
 * primals.  Arguments as those entries without the tangents. */
int qattn_jvp_primal_ex(const void* q, const void* k, const void* v, void* out, void* lse, long bh,
                        long sq, long sk, int group, int head_dim, float qks, float sm, void* stream);
int qattn_jvp_primal_x3_ex(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo,
                           const void* v_hi, const void* v_lo, void* out, void* lse, long bh, long sq,
                           long sk, int group, int head_dim, float qks, float sm, void* stream);

/* hi = bf16(x), lo = bf16(x - hi) (both round-to-nearest-even) for n fp32 elements, n % 4 == 0. */
int qattn_split_bf16(const void* x, void* hi, void* lo, long n, void* stream);

/* ---------------------------------------------------------------- MX-FP4 inference forward
 * SURVEY §8f N4 (SageAttention3's FP4 path, named in the reference README.md:49-55, not implemented
 * there: no reference interface is replaced).  OCP MX e2m1 with one e8m0 scale per 32 elements,
 * e = floor(log2 amax) - 2, code = RNE(sat(x / 2^e)); layouts in csrc/mxfp4_attn.hip. */

/* Q / K rows: x f16 [rows, head_dim] -> q4 u8 [rows, head_dim/2] (low nibble first), scale u8
 * [rows, head_dim/32].  mean (f16 [rows/seq, head_dim]) or NULL: when given, row r is first
 * smoothed to f16(x - mean[r / seq]) (k_mean from qattn_kmean).  head_dim 64 or 128. */
int qattn_mxfp4_quant_rows(const void* x, const void* mean, void* q4, void* scale, long rows, long seq,
                           int head_dim, void* stream);

/* V: v f16 [bh*seq, head_dim] -> vt u8 [bh][seq/64][head_dim][32] (operand-ordered keys), vscale u8
 * [bh][seq/64][head_dim][2].  seq % 64 == 0. */
int qattn_mxfp4_quant_vt(const void* v, void* vt, void* vscale, long bh, long seq, int head_dim,
                         void* stream);

/* O f16 [bh*sq, 128] = softmax2(S * qks) V with S from the fp4 Q/K, P re-quantised to fp4 per
 * 32 keys, l from the fp32 P; lse f32 [bh*sq] (base 2).  Query head h reads key/value head h/group.
 * sq % 32 == 0, sk % 64 == 0, head_dim 128. */
int qattn_mxfp4_attn_fwd(const void* q4, const void* qscale, const void* k4, const void* kscale,
                         const void* vt, const void* vscale, void* out, void* lse, long bh, long sq,
                         long sk, int group, int head_dim, float qks, void* stream);

/* qattn_mxfp4_attn_fwd with a causal mask, causal as in qattn_int8_attn_fwd_ex: 0 none (the call
 * above), 1 top-left (query row i sees keys j <= i; any sq, sk), 2 bottom-right (j <= i + sk - sq,
 * the last sq rows of a square problem: a query chunk against a cache; sk >= sq).  A masked key's P
 * is exactly 0 before its fp4 quantisation and takes no part in the row max; tiles past a row
 * block's diagonal are not read.  Returns 1 for any other causal and for causal == 2 with sk < sq. */
int qattn_mxfp4_attn_fwd_ex(const void* q4, const void* qscale, const void* k4, const void* kscale,
                            const void* vt, const void* vscale, void* out, void* lse, long bh, long sq,
                            long sk, int group, int causal, int head_dim, float qks, void* stream);

/* The forward in the decoding layout, split over the keys (an MX-FP4 key/value cache,
 * kv_cache_mxfp4.py).  bhv = batch x key/value heads; each key/value head is attended by ONE virtual
 * head of rows = G * sq_head query rows, the G query heads of its group as consecutive [sq_head, 128]
 * blocks of q4 / qscale (q4 u8 [bhv*rows, 64], qscale u8 [bhv*rows, 4]).  rows is any value >= 1.
 * Split y of nsplit = ceil(sk / keys_per_split) runs the keys [y*kps, min(sk, y*kps + kps)) from
 * m = -inf and writes the unnormalised state: opart f32 [nsplit][bhv*rows][128] = O_s, ml f32 x 2
 * [nsplit][bhv*rows] = {m_s, l_s} (m_s an integer or, for a row that sees no key of the split, -inf
 * with l_s = 0 and O_s = 0).  causal: 0 none, 2 bottom-right over the cache (row r is query position
 * r % sq_head and sees key j iff j <= r % sq_head + sk - sq_head).  Returns 1 for head_dim != 128,
 * sk % 64, sk == 0 with rows > 0, keys_per_split < 64 or % 64, sq_head < 1, rows % sq_head, any other
 * causal, causal == 2 with sk < sq_head; 0 without a launch for bhv == 0 or rows == 0. */
int qattn_mxfp4_attn_fwd_split(const void* q4, const void* qscale, const void* k4, const void* kscale,
                               const void* vt, const void* vscale, void* opart, void* ml, long bhv,
                               long rows, long sq_head, long sk, int causal, int keys_per_split,
                               int head_dim, float qks, void* stream);

/* qattn_mxfp4_attn_fwd_split over a preallocated cache with one length per sequence
 * (kv_cache_mxfp4.py PreallocatedKVFP4).  The operands are laid out as above with cap tokens per
 * key/value head (k4 u8 [bhv][cap][64], kscale u8 [bhv][cap][4], vt u8 [bhv][cap/64][128][32], vscale
 * u8 [bhv][cap/64][128][2]); lens is a DEVICE array i32 [bhv / heads_per_seq], and key/value head h
 * holds L = lens[h / heads_per_seq] keys.  nsplit = ceil(sk_max / keys_per_split); split y runs the
 * tiles [y*kps/64, min(ceil(L/64), (y+1)*kps/64)) of its head and writes the empty state (m_s = -inf,
 * l_s = 0, O_s = 0) when that range is empty; no byte of a tile >= ceil(L/64) is read, and what K rows
 * >= L hold never matters.  Row r sees key j iff j <= L - 1 (causal 0) or j <= r % sq_head + L -
 * sq_head (causal 2: the queries are the sequence's last sq_head positions).  opart / ml and the merge
 * (qattn_mxfp4_split_combine) are those of the entry above.
 * Preconditions the caller guarantees (the entry cannot read lens): 1 <= lens[b] <= sk_max <= cap, and
 * with causal == 2 lens[b] >= sq_head.
 * Returns 1 for head_dim != 128, cap or sk_max not multiples of 64, sk_max > cap, sk_max < 64,
 * cap > 2^25, keys_per_split < 64 or % 64, sq_head < 1, rows % sq_head, heads_per_seq < 1,
 * bhv % heads_per_seq, causal not 0 or 2, lens == NULL; 0 without a launch for bhv == 0 or rows == 0. */
int qattn_mxfp4_attn_fwd_split_len(const void* q4, const void* qscale, const void* k4, const void* kscale,
                                   const void* vt, const void* vscale, void* opart, void* ml,
                                   const void* lens, long bhv, long heads_per_seq, long rows, long sq_head,
                                   long cap, long sk_max, int causal, int keys_per_split, int head_dim,
                                   float qks, void* stream);

/* Append to a preallocated MX-FP4 cache, stream-ordered, without reading anything back.  k, v f16
 * [batch*kv_heads][n][128] are n >= 1 new tokens per head; sequence b takes the first counts[b] of
 * them (counts i32 [batch] on the device, 0 <= counts[b] <= n; NULL: n for all) at tokens lens[b] ..
 * of its heads, and lens[b] (i32 [batch], device) grows by that count.  K rows are quantised as
 * qattn_mxfp4_quant_rows does (k_mean f16 [batch*kv_heads][128] or NULL); the V tiles the new tokens
 * touch are quantised again as qattn_mxfp4_quant_vt does, the older keys of a partial tile coming from
 * vtail f16 [batch*kv_heads][64][128], which keeps the fp16 V rows of each sequence's last partial
 * tile at slot token % 64.  Afterwards rows [0, L) of k4 / kscale and tiles [0, ceil(L/64)) of vt /
 * vscale equal, bit for bit, the two quantisers' output for the sequence zero-padded to a multiple of
 * 64.  The caller guarantees lens[b] + counts[b] <= cap (a sequence that would pass cap is left
 * untouched, as one whose count is outside [0, n]).  Returns 1 for head_dim != 128, n < 1, cap % 64,
 * a NULL pointer other than k_mean / counts. */
int qattn_mxfp4_cache_append(const void* k, const void* v, const void* k_mean, void* k4, void* kscale,
                             void* vt, void* vscale, void* vtail, void* lens, const void* counts,
                             long batch, long kv_heads, long n, long cap, int head_dim, void* stream);

/* The paged pool (kv_cache_mxfp4.py PagedKVFP4): the four operands cut into num_pages pages of
 * page_tokens = P tokens (64 * 2^k, 64 <= P <= 1024), a page holding P tokens of all kv_heads heads of
 * ONE sequence: k4 u8 [num_pages][kv_heads][P][64], kscale u8 [num_pages][kv_heads][P][4], vt u8
 * [num_pages][kv_heads][P/64][128][32], vscale u8 [num_pages][kv_heads][P/64][128][2].  block_table is
 * a DEVICE array i32 [sequences][max_pages_per_seq] naming each sequence's pages in order: logical
 * 64-key tile t of head h of sequence b is physical tile (block_table[b][t / (P/64)] * kv_heads + h) *
 * (P/64) + t % (P/64) of all four operands.  Gathered through its table, a sequence holds exactly the
 * bytes the preallocated cache holds.  A table entry is read only below ceil(L / P), L the sequence's
 * length (an append: its length after the append), and an id outside [0, num_pages) is clamped into
 * the pool.  An operand may be larger than 4 GiB; num_pages * kv_heads * P/64, the number of physical
 * tiles, must be below 2^31 and max_pages_per_seq * P at most 2^25 (both return 1).
 *
 * qattn_mxfp4_attn_fwd_split_len over the pool (heads_per_seq = the pool's kv_heads): the same splits,
 * partial results and preconditions (1 <= lens[b] <= sk_max, the tokens of a sequence lie in pages its
 * table row names; causal == 2: lens[b] >= sq_head), and bit for bit the same opart / ml as that entry
 * gives on a preallocated cache with the same tokens.  keys_per_split is independent of P.  Returns 1
 * as that entry does, with sk_max > max_pages_per_seq * P for sk_max > cap, and for a bad page_tokens,
 * num_pages < 1, max_pages_per_seq < 1 or block_table == NULL. */
int qattn_mxfp4_attn_fwd_split_paged(const void* q4, const void* qscale, const void* k4, const void* kscale,
                                     const void* vt, const void* vscale, void* opart, void* ml,
                                     const void* lens, const void* block_table, long bhv,
                                     long heads_per_seq, long rows, long sq_head, long num_pages,
                                     long page_tokens, long max_pages_per_seq, long sk_max, int causal,
                                     int keys_per_split, int head_dim, float qks, void* stream);

/* qattn_mxfp4_cache_append into the pool: the same arguments, quantisers, vtail (f16
 * [batch*kv_heads][64][128]) and lens update, the destination of every row and tile going through
 * block_table i32 [batch][max_pages_per_seq] (device), which the caller has filled for the lengths
 * AFTER the append before this call in stream order.  The caller guarantees lens[b] + counts[b] <=
 * (pages of sequence b) * P.  Returns 1 as that entry does, and for the pool's limits above. */
int qattn_mxfp4_paged_append(const void* k, const void* v, const void* k_mean, void* k4, void* kscale,
                             void* vt, void* vscale, void* vtail, void* lens, const void* counts,
                             const void* block_table, long batch, long kv_heads, long n, long num_pages,
                             long page_tokens, long max_pages_per_seq, int head_dim, void* stream);

/* The packed ("varlen") step over the pool: a ragged batch in one attention launch, one merge and one
 * append (kv_cache_mxfp4.py attention_mxfp4_varlen_paged / PagedKVFP4.append_packed, whose plan_varlen
 * builds the tables).  nseq sequences take part; sequence j lives in slot s_j of lens / block_table
 * (distinct slots in [0, max_seqs)) and brings n_j >= 1 packed tokens, tokens = sum n_j, packed in the
 * order of j.  q4 / qscale are qattn_mxfp4_quant_rows of q f16 [tokens][group * kv_heads][128] (seq =
 * 1, no mean), so packed row (token, query head) is row token * group * kv_heads + head.  Tables, DEVICE
 * i32, written by the caller before the call in stream order:
 *   seq_rec [nseq][8]  {s_j, first packed token (ascending), n_j, ns_j, first partial row, 0, 0, 0},
 *                      ns_j = ceil(ceil64(L_j) / keys_per_split) splits, L_j = lens[s_j];
 *   work    [nwork][4] {j, 128-row block of the virtual head, split < ns_j, 0}: one record per
 *                      workgroup and key/value head, in any order (longest first is fastest).
 * The virtual head of key/value head h of sequence j has group * n_j rows, row r = g * n_j + i being
 * packed token i of query head h * group + g; its partial rows are opart f32 [part_rows][128] / ml f32
 * x 2 [part_rows] at (first partial row of j) + (split * kv_heads + h) * group * n_j + r, so sequence j
 * owns ns_j * kv_heads * group * n_j rows and part_rows is their sum.  Tiles, masks (causal 2: packed
 * token i of j sees keys <= L_j - n_j + i) and arithmetic are qattn_mxfp4_attn_fwd_split_paged's: every
 * sequence gets, bit for bit, that entry's opart / ml for it alone at the same keys_per_split.  Slots
 * that are not listed are never read.  A slot, row or partial row outside the sizes given is clamped or
 * skipped (a wrong table gives a wrong answer, never an address outside the buffers).
 * Preconditions the caller guarantees: 1 <= L_j <= (pages of s_j) * P, causal == 2: n_j <= L_j.
 * Returns 1 for head_dim != 128, a NULL lens / block_table / seq_rec / work, the pool's limits above,
 * keys_per_split < 64 or % 64, causal not 0 or 2, group < 1, max_seqs < 1, nseq > max_seqs or > tokens,
 * tokens * group * kv_heads, part_rows, nwork * kv_heads or max_seqs * kv_heads >= 2^31; 0 without a
 * launch for nseq, nwork or tokens == 0.  Allocates nothing. */
int qattn_mxfp4_attn_fwd_varlen_paged(const void* q4, const void* qscale, const void* k4, const void* kscale,
                                      const void* vt, const void* vscale, void* opart, void* ml,
                                      const void* lens, const void* block_table, const void* seq_rec,
                                      const void* work, long nseq, long nwork, long tokens, long part_rows,
                                      long max_seqs, long kv_heads, long group, long num_pages,
                                      long page_tokens, long max_pages_per_seq, int causal,
                                      int keys_per_split, int head_dim, float qks, void* stream);

/* The packed step with a sliding window and attention sinks: the entry above with causal == 2 and one
 * (window >= 1, sinks >= 0) for the call.  Packed token i of sequence j sits at position p = L_j - n_j + i
 * and sees key k iff k <= p and (k > p - window or k < sinks); every token sees itself.  With nt =
 * ceil(L_j / 64), T = keys_per_split / 64, wt0 = max(0, L_j - n_j - window + 1) / 64 (the first tile any
 * window of j reaches) and nst = ceil(min(sinks, L_j) / 64) sink tiles:
 *   wt0 <= nst (the runs touch): seq_rec[j][5] = seq_rec[j][6] = 0, ns_j = ceil(nt / T) and split s runs
 *     tiles [s T, min(nt, s T + T)), as in the entry above;
 *   wt0 >  nst (a gap): seq_rec[j][5] = wt0, seq_rec[j][6] = nst, ns_j = 1 + ceil((nt - wt0) / T); split 0
 *     runs the sink tiles [0, nst) whatever T is, split s >= 1 tiles [wt0 + (s-1) T, min(nt, wt0 + s T)).
 *     Without sinks (nst = 0) there is no sink split: ns_j = ceil((nt - wt0) / T), split s starts at
 *     wt0 + s T.
 * The pages of the tiles in the gap are never fetched and their block_table entries never used, so they
 * may have been given back to the pool.  Partial rows, work records, clamping and the merge
 * (qattn_mxfp4_varlen_combine) are the entry's above; a row that sees no key of a split writes the empty
 * state (-inf, 0).  With window >= every L_j the bits are those of the entry above at causal == 2.
 * Returns 1 without a launch for window < 1, sinks < 0, causal != 2, and as the entry above. */
int qattn_mxfp4_attn_fwd_varlen_paged_window(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int causal, int keys_per_split, int head_dim,
    float qks, long window, long sinks, void* stream);

/* The packed step with shared prefixes (kv_cache_mxfp4.py attention_mxfp4_varlen_paged(share_prefix=True),
 * whose plan_varlen_shared builds the tables): the first entry above, with the key splits that lie wholly
 * inside pages several sequences hold in common computed once for all of them.  seq_rec, the partial rows,
 * part_rows and the merge (qattn_mxfp4_varlen_combine) are that entry's; so is every bit of opart / ml
 * and of the merged result at the same keys_per_split.  Two more DEVICE i32 tables:
 *   grp_rec [ngroup][4]  {first entry in members, member count >= 2, ns_g, R_g}: group g shares its
 *                        splits [0, ns_g); R_g = group * (sum of n_j over its members) stacked rows;
 *   members [nmember][2] {j, first stacked row of sequence j in its group}, a group's entries consecutive
 *                        and ascending; stacked row r of a group is row r - first of its member's virtual
 *                        head, in that member's own order g * n_j + i.
 * and work records of two kinds: {j, 128-row block, split, 0} as in the first entry, for every split >=
 * ns_g of a member and every split of an ungrouped sequence, and {g, 128-row block of group g's stacked
 * rows, split < ns_g, 1}, whose workgroup fetches the split's tiles once, through the block_table row of
 * the group's first member, and writes every row's state where the first kind would have.
 * Preconditions the caller guarantees beyond the first entry's: the first ceil(ns_g * keys_per_split / P)
 * block_table entries of a group's members are equal, ns_g * keys_per_split <= L_j for every member and,
 * causal == 2, <= L_j - n_j + 1 (no shared key is masked for any row); no sequence in two groups.  Every
 * table index is clamped or checked as in the first entry.
 * Returns 1 as the first entry, and for a NULL grp_rec / members, ngroup < 1, nmember < 2 * ngroup or
 * nmember > nseq; 0 without a launch for nwork or tokens == 0. */
int qattn_mxfp4_attn_fwd_varlen_paged_shared(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int causal, int keys_per_split, int head_dim,
    float qks, const void* grp_rec, const void* members, long ngroup, long nmember, void* stream);

/* The packed step with a tree mask, the verify step of speculative decoding (kv_cache_mxfp4.py
 * attention_mxfp4_varlen_paged(tree=)): the first entry above at causal == 2, with seq_rec[j][7] = nd_j, 0 <=
 * nd_j <= min(n_j, 64), and tree_masks, DEVICE u64 [tokens], one word per packed token (0 outside a tree).
 * The last nd_j packed tokens of sequence j are the nodes of a draft tree (or forest) in topological order,
 * appended already at keys base_j = L_j - nd_j ..; with t = i - (n_j - nd_j), packed token i of j
 *   t <  0: sees keys <= L_j - n_j + i, as in the first entry;
 *   t >= 0: sees key k iff k < base_j, or k = base_j + b with bit b of its word set.
 * The word holds the node's ancestors and the node itself; the kernel uses (word & bits <= t) | bit t, so
 * every mask is a subset of the causal row that holds the token itself (a wrong word gives a wrong answer,
 * never an empty row), and a chain (bits 0 .. t) gives the first entry's bits.  lse is over the visible
 * keys.  Splits, work records, partial rows, clamping and the merge (qattn_mxfp4_varlen_combine) are the
 * first entry's; nd_j is clamped to [0, min(n_j, 64)].  A draft token at tree depth d stands for position
 * L_j - nd_j + d of its path: the rotary entries below are given those positions for draft keys and queries.
 * Returns 1 without a launch for causal != 2 and a NULL tree_masks, and as the first entry. */
int qattn_mxfp4_attn_fwd_varlen_paged_tree(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int causal, int keys_per_split, int head_dim,
    float qks, const void* tree_masks, void* stream);

/* Taking tokens back from the pool (kv_cache_mxfp4.py PagedKVFP4.checkpoint / rollback).  saved f16
 * [nsaved][kv_heads][64][128] is a copy of vtail rows taken when the sequences stood at their lengths L0;
 * recs, DEVICE i32 [nrec][4] = {slot, L0, row of that slot in saved, 0}, distinct slots.  For every record,
 * in one launch: vtail rows [0, L0 % 64) of the slot are restored from saved; when L0 % 64 != 0, V tile
 * L0 / 64 of every head is quantised again FROM THE SAVED ROWS with the keys at or past L0 zero (vt / vscale,
 * through block_table, whose entry L0 / page_tokens is still the sequence's); lens[slot] = L0.  K rows at or
 * past L0 are left as they are (unspecified by the pool's invariant).  Afterwards rows [0, L0) of k4 /
 * kscale, tiles [0, ceil(L0 / 64)) of vt / vscale, the live vtail rows and lens hold, bit for bit, what
 * they held when saved was taken, provided only appends happened in between.  A record whose slot, L0 or
 * row lies outside [0, max_seqs), [0, max_pages_per_seq * page_tokens] or [0, nsaved) writes nothing.
 * Returns 1 for head_dim != 128, a NULL pointer, the pool's limits above, nrec > max_seqs, nsaved < 1; 0
 * without a launch for nrec == 0.  Allocates nothing. */
int qattn_mxfp4_paged_rollback(const void* saved, void* vtail, void* vt, void* vscale, void* lens,
                               const void* block_table, const void* recs, long nrec, long nsaved,
                               long max_seqs, long kv_heads, long num_pages, long page_tokens,
                               long max_pages_per_seq, int head_dim, void* stream);

/* The merge of the packed step: qattn_mxfp4_split_combine's arithmetic in its order, per packed row
 * (token, query head), over the ns_j partial rows of the token's own sequence (found by binary search
 * over seq_rec's first-token column): out f16 [tokens][q_heads][128], lse f32 [tokens][q_heads].
 * Returns 1 for head_dim != 128, seq_rec == NULL, q_heads % kv_heads, nseq > tokens, tokens * q_heads
 * or part_rows >= 2^31; 0 without a launch for nseq or tokens == 0. */
int qattn_mxfp4_varlen_combine(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                               long nseq, long tokens, long q_heads, long kv_heads, long part_rows,
                               int head_dim, void* stream);

/* qattn_mxfp4_paged_append for packed tokens: k, v f16 [tokens][kv_heads][128] token-major; seq_tab
 * i32 [nseq][4] = {slot, count >= 1, first packed token (ascending), 0} and tiles i32 [ntiles][2] = {j,
 * logical 64-key tile}, the tiles [lens/64, (lens + count - 1)/64] of every record j (exactly the V
 * tiles the appends touch), both on the device.  The same quantisers, vtail and lens update; block_table
 * filled for the lengths AFTER the append; the caller guarantees lens[slot] + count <= (pages of the
 * slot) * P and distinct slots.  A record outside those bounds writes nothing.  Returns 1 as that entry
 * does, and for a NULL table, nseq > max_seqs or > tokens, ntiles < nseq, tokens * kv_heads >= 2^31; 0
 * without a launch for nseq or tokens == 0.  Allocates nothing. */
int qattn_mxfp4_paged_append_packed(const void* k, const void* v, const void* k_mean, void* k4, void* kscale,
                                    void* vt, void* vscale, void* vtail, void* lens,
                                    const void* block_table, const void* seq_tab, const void* tiles,
                                    long nseq, long ntiles, long tokens, long max_seqs, long kv_heads,
                                    long num_pages, long page_tokens, long max_pages_per_seq, int head_dim,
                                    void* stream);

/* Rotary position embedding fused into the quantisers of the packed step (kv_cache_mxfp4.py Rope).
 * cos_sin f32 [max_pos][128], contiguous: row p holds cos theta(p, i) at column i and sin theta(p, i) at
 * column 64 + i for pair i in [0, 64) (the cos_sin_cache convention; a table scaled by YaRN, llama3 or NTK
 * is passed as it is).  interleaved 0 (NeoX, rotate half) pairs elements (i, i + 64) of a row, 1 (GPT-J)
 * elements (2i, 2i + 1).  With c, s from the row of the token's position, a pair (a, b) of f16 inputs
 * becomes first = f16(f32(a c) - f32(b s)), second = f16(f32(b c) + f32(a s)): two rounded fp32 products,
 * one rounded fp32 sum, round-to-nearest-even to f16, no fused multiply-add; the rotated f16 row then
 * goes through the quantiser unchanged (keys: f16(x - k_mean) first, as without).  pos i32 [tokens] on
 * the device holds one position per packed token and is clamped to [0, max_pos - 1]: a wrong position
 * gives a wrong answer, never an address outside the table.
 *
 * qattn_mxfp4_quant_rows_rope: qattn_mxfp4_quant_rows without a mean on x f16 [tokens][heads][128], token-
 * major (the packed q of qattn_mxfp4_attn_fwd_varlen_paged), each row rotated first.  Returns 1 for head_dim
 * != 128, a NULL cos_sin or pos, max_pos < 1 or >= 2^31, interleaved outside {0, 1}, tokens * heads >= 2^31;
 * 0 without a launch for tokens or heads == 0. */
int qattn_mxfp4_quant_rows_rope(const void* x, void* q4, void* scale, const void* cos_sin, const void* pos,
                                long tokens, long heads, long max_pos, int interleaved, int head_dim,
                                void* stream);

/* qattn_mxfp4_paged_append_packed with the new keys rotated first (pos[t]: the position of packed token t);
 * V, vtail and the lengths are that entry's.  Returns 1 as that entry does and as the entry above does for
 * cos_sin, pos, max_pos and interleaved. */
int qattn_mxfp4_paged_append_packed_rope(const void* k, const void* v, const void* k_mean, void* k4,
                                         void* kscale, void* vt, void* vscale, void* vtail, void* lens,
                                         const void* block_table, const void* seq_tab, const void* tiles,
                                         long nseq, long ntiles, long tokens, long max_seqs, long kv_heads,
                                         long num_pages, long page_tokens, long max_pages_per_seq,
                                         int head_dim, const void* cos_sin, const void* pos, long max_pos,
                                         int interleaved, void* stream);

/* The device-planned decode step (kv_cache_mxfp4.py DecodeStep): one new token for each of up to n listed
 * sequences of the pool, with no argument below that a host computed from the lengths, so the launches can
 * be captured in a graph once and replayed while the sequences grow.  n, splits, keys_per_split, window and
 * sinks (window 0: none, sinks then 0) are fixed when the step is made; capacity = max_pages_per_seq *
 * page_tokens.  The host still owns the pages: before a step, block_table holds the page that position
 * lens[slot] of every listed slot needs.
 *
 * qattn_mxfp4_decode_step_plan, one launch, reads slots i32 [n] (a slot per entry; any other value marks
 * padding) and lens, the lengths BEFORE the append, and writes four device tables of n rows, with b =
 * slots[i] and L = lens[b]:
 *   seq_tab i32 [n][4] = {b, 1, i, 0} and tiles i32 [n][2] = {i, L / 64}: the arguments of
 *     qattn_mxfp4_paged_append_packed(_rope) at nseq = ntiles = tokens = n;
 *   pos i32 [n] = L: the rotary position of the new key and query;
 *   seq_rec i32 [n][8] = {b, i, 1, ns, i * splits * kv_heads * group, wt0, nst, 0} for the length L + 1, with
 *     ns, wt0, nst what the host plan of the packed step gives one query over L + 1 keys (the first packed
 *     entries above; ns held to splits).
 * An entry with b outside [0, max_seqs) or L outside [0, capacity) is padding: seq_tab {-1, 0, i, 0} and tiles
 * {-1, 0}, which the append skips, pos 0 and ns = 0.  No content of slots or lens makes the kernel read or
 * write outside its tables.  Returns 1 for a NULL pointer, a keys_per_split that is no multiple of 64, max_seqs,
 * kv_heads, group or splits < 1, splits > 65535, a capacity that is no multiple of 64 in [64, 2^25], window or
 * sinks < 0, sinks without a window, n * splits * kv_heads * group >= 2^31; 0 without a launch for n == 0.
 *
 * qattn_mxfp4_attn_fwd_decode_step is the causal packed forward (with the window's mask for window >= 1) of
 * those n one-token sequences over a grid fixed by n, splits and kv_heads: work i32 [n * splits][4] holds
 * {i, 0, s, 0} for every entry i and split s < splits once, in any order, and a workgroup whose s is >= ns of
 * its entry returns at once without a store.  q4 / qscale: the n * kv_heads * group quantised query rows,
 * token-major; opart f32 [n * splits * kv_heads * group][128] and ml f32 x 2 of as many rows.  Every entry gets,
 * bit for bit, what the first packed entry (or the windowed one) gives it at the same keys_per_split.
 * Returns 1 as those entries do for their pool, and for the limits of the plan entry.
 *
 * qattn_mxfp4_decode_step_combine merges entry i's ns splits from its rows [i * splits * q_heads, ..) with
 * qattn_mxfp4_varlen_combine's arithmetic into out f16 [n][q_heads][128] and lse f32 [n][q_heads]; a padding
 * entry (ns < 1) gets out = 0 and lse = -inf.  Nothing allocates. */
int qattn_mxfp4_decode_step_plan(const void* slots, const void* lens, void* seq_tab, void* tiles, void* seq_rec,
                                 void* pos, long n, long max_seqs, long capacity, long kv_heads, long group,
                                 int keys_per_split, long splits, long window, long sinks, void* stream);
int qattn_mxfp4_attn_fwd_decode_step(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work, long n,
    long splits, long max_seqs, long kv_heads, long group, long num_pages, long page_tokens,
    long max_pages_per_seq, int keys_per_split, int head_dim, float qks, long window, long sinks, void* stream);
int qattn_mxfp4_decode_step_combine(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                                    long n, long splits, long q_heads, long kv_heads, int head_dim, void* stream);

/* The device-planned verify step (kv_cache_mxfp4.py VerifyStep): draft_tokens = K new tokens, 1 <= K <= 64, a
 * chain or a draft tree in topological order, for each of up to n listed sequences, appended and then attended
 * under the tree mask.  As in the decode step above no argument is computed by a host from the lengths: n, K,
 * splits and keys_per_split are fixed when the step is made, capacity = max_pages_per_seq * page_tokens, and the
 * host owns the pages (block_table holds the pages of positions lens[slot] .. lens[slot] + K - 1 of every listed
 * slot).  tree u64 [n * K] holds the ancestor word of every packed token: bit b of word t of an entry set iff
 * node b is an ancestor of node t or t itself.  Every reader cleans a word to (word & bits <= t) | bit t.
 *
 * qattn_mxfp4_verify_step_plan, one launch, reads slots i32 [n] (a slot per entry; any other value marks
 * padding), lens (the lengths BEFORE the append) and tree, and writes, with b = slots[i] and L = lens[b]:
 *   seq_tab i32 [n][4] = {b, K, i * K, 0} and tiles i32 [2 n][2], rows 2 i = {i, L / 64} and 2 i + 1 = {i,
 *     (L + K - 1) / 64} when that is another tile, else {-1, 0}: the arguments of
 *     qattn_mxfp4_paged_append_packed(_rope) at nseq = n, ntiles = 2 n, tokens = n * K;
 *   pos i32 [n * K]: L + popcount(cleaned word) - 1, the node's depth behind the cached keys (its rotary
 *     position, key and query);
 *   seq_rec i32 [n][8] = {b, i * K, K, ns, i * splits * kv_heads * group * K, 0, 0, K} for the length L + K, ns =
 *     ceil(ceil((L + K) / 64) * 64 / keys_per_split) held to splits: the host plan's record of K tree queries.
 * An entry with b outside [0, max_seqs), L < 0 or L + K > capacity is padding: seq_tab {-1, 0, i * K, 0}, both
 * tiles {-1, 0}, pos 0 and ns = 0.  No content of slots, lens or tree makes the kernel read or write outside its
 * tables.  Returns 1 for a NULL pointer, a keys_per_split that is no multiple of 64, K outside [1, 64], max_seqs,
 * kv_heads, group or splits < 1, splits > 65535, a capacity that is no multiple of 64 in [64, 2^25], n * splits *
 * kv_heads * group * K >= 2^31; 0 without a launch for n == 0.
 *
 * qattn_mxfp4_attn_fwd_verify_step is qattn_mxfp4_attn_fwd_varlen_paged_tree for those n sequences of K tree
 * queries over a grid fixed by n, K, group, splits and kv_heads: work i32 [n * nrb * splits][4], nrb = ceil(group
 * * K / 128), holds {i, row block, s, 0} for every entry, row block and split s < splits once, in any order, and a
 * workgroup whose s is >= ns of its entry returns at once without a store.  q4 / qscale: the n * K * kv_heads *
 * group quantised query rows, token-major; opart f32 [n * splits * kv_heads * group * K][128], ml as many rows;
 * entry i's rows are [split][kv head][g * K + t] from i * splits * kv_heads * group * K.  Every entry gets, bit
 * for bit, what the tree entry gives it at the same keys_per_split.  Returns 1 as that entry does for its pool,
 * and for the limits of the plan entry.
 *
 * qattn_mxfp4_verify_step_combine merges entry i's ns splits with qattn_mxfp4_varlen_combine's arithmetic into
 * out f16 [n * K][q_heads][128] and lse f32 [n * K][q_heads]; a padding entry (ns < 1) gets out = 0 and lse = -inf
 * in its K rows.  Only ns is read from seq_rec.  Nothing allocates. */
int qattn_mxfp4_verify_step_plan(const void* slots, const void* lens, const void* tree, void* seq_tab, void* tiles,
                                 void* seq_rec, void* pos, long n, long draft_tokens, long max_seqs, long capacity,
                                 long kv_heads, long group, int keys_per_split, long splits, void* stream);
int qattn_mxfp4_attn_fwd_verify_step(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    const void* tree_masks, long n, long draft_tokens, long splits, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int keys_per_split, int head_dim, float qks,
    void* stream);
int qattn_mxfp4_verify_step_combine(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                                    long n, long draft_tokens, long splits, long q_heads, long kv_heads,
                                    int head_dim, void* stream);

/* Merge of the splits, per row of rows_total = bhv*rows: M = max_s m_s, w_s = 2^(m_s - M) (exact; 0
 * for m_s = -inf), L = sum_s w_s l_s, out f16 [rows_total, 128] = (sum_s w_s O_s) * (1 / L), lse f32
 * [rows_total] = M + log2(L).  With nsplit == 1 this is the one-pass forward's epilogue bit for bit. */
int qattn_mxfp4_split_combine(const void* opart, const void* ml, void* out, void* lse, long rows_total,
                              int nsplit, int head_dim, void* stream);

/* ---------------------------------------------------------------- launch plans (csrc/plan.hip)
 * Host-only: no device, no stream, nothing launched.  Each answers a choice a host makes before it
 * calls an entry above; every answer gives bit-identical outputs and differs only in time and memory.
 * The Python drop-ins and the TORCH_LIBRARY operators take their plans from these functions, so a
 * host that does the same allocates and launches what they do.  The environment variables are read
 * on every call. */

/* keys per split of a decoding forward, a multiple of tile (32 int8, 64 MX-FP4); sk when one split
 * suffices or when there is no work (bhv * rows == 0); -1 for a bad tile / sk */
long qattn_split_keys(long bhv, long rows, long sk, int tile);

/* int8 record backward over bkv key/value heads of `group` query heads each.
 * chunk_req: key/value heads per chunk; < 0 = auto (QATTN_BWD_WS_CHUNK if set and >= 0, else the
 * measured rule), 0 = all heads.  cap: byte limit, < 0 = qattn_bwd_ws_cap().
 * Writes the chunk (1..bkv) to *kv_chunk; returns the workspace bytes of one chunk, 0 when the dQ
 * pass must recompute (a shape qattn_int8_attn_bwd_ws refuses: region >= 2 GiB per key/value head,
 * more than QATTN_WS_MAX_QUERY_TILES / _KEY_TILES tiles; or over the cap), -1 for bad shapes.
 * With bytes > 0: qattn_int8_attn_bwd_wsc(..., ws, *kv_chunk, ...); with 0: qattn_int8_attn_bwd_ex. */
long qattn_int8_bwd_plan(long bkv, int group, long sq_tok, long sk_tok, int causal,
                         long chunk_req, long cap, long* kv_chunk);

/* bf16 backward: bytes of the dS-record workspace (qattn_bf16_bwd_ws_ex), 0 = the recomputing entry
 * (qattn_bf16_bwd_ex), -1 for bad shapes.
 * force: < 0 auto (QATTN_BF16_BWD_WS = 1 / 0 if set, else records when causal), 0 off, 1 on.
 * cap as above. */
long qattn_bf16_bwd_plan(long bh, long sq_tok, long sk_tok, int causal, int force, long cap);

/* Fragment-layout probes and other diagnostics live in a separate development library
 * (libqattn_dev.so, include/qattn_dev.h); this library exports the product API only. */

#ifdef __cplusplus
}
#endif

#endif /* QATTN_H */
