// MX-FP4 attention forward for gfx950 inference (SageAttention3's FP4 path, which
// the reference names in README.md:49-55 but does not implement).  Everything below is defined
// here; oracle/restate.py mxfp4_fwd restates it and tests/test_gpu_mxfp4.py checks the kernels.
//
// Number format: OCP MX (v1.0) FP4 = e2m1 elements {0, ±0.5, ±1, ±1.5, ±2, ±3, ±4, ±6} sharing one
// power-of-two e8m0 scale per block of 32.  Block scale 2^e with e = floor(log2 amax) - 2 (amax = 0:
// e = -127); element = RNE(saturate(x / 2^e)) -- exactly v_cvt_scalef32_pk_fp4_f32.
//   Q, K: blocks of 32 along D per row  (the K dimension of S = Q K^T).
//   V   : blocks of 32 keys per column d (the K dimension of O = P V), stored transposed in operand
//         order: per 64-key tile g and column d, 2 x 16 bytes, half h holding the 32 keys
//         64g + 32(j>>4) + 8((j>>2)&3) + 4h + (j&3), j = 0..31 (nibble j, low nibble first) --
//         the key order in which a lane holds P after the swapped S^T = K Q^T product.
//   P   : per query row, one block per lane half: the 32 probabilities the lane holds of a 64-key
//         tile (same interleaved key set as V's block h), scale from their own max.
// Attention per 64-key tile: S = (deq Q)(deq K)^T exactly (block-scaled fp4 MFMA, fp32
// accumulation); m = ceil(rowmax(S * qks)) when that max exceeds the running m by more than 8
// (else m stays; m starts at -inf), O and l scaled by the exact power of two 2^(m_old - m_new);
// P = exp2(fma(S, qks, -m)) in fp32 (so P <= 2^8); P_fp4 = MX(P); l += sum(deq P_fp4);
// O += (deq P_fp4)(deq V).  Out: O / l (fp16), lse = m + log2(l) (fp32, base 2).  Because every
// rescale is a power of two, the fp4 codes of P do not depend on when m was raised.
// Causal (CAUSAL, key offset qoff): query row i sees key j iff j <= i + qoff (qoff = 0 top-left,
// Sk - Sq bottom-right).  Masked scores take no part in the row max (a lane whose 32 keys are all
// masked contributes -inf, which never raises m) and a masked key's P is exactly 0 before the MX
// quantisation -- a select, since exp2 of a masked score may be inf -- so the block's scale comes
// from the visible keys alone and a fully masked block is scale byte 0 with all-zero codes.  Key 0
// is visible to every row, so m is finite after tile 0.  A tile no row of a wave sees is the same
// as one with mx = -inf and P = 0: it is skipped (the workgroup's loop ends at its last row's
// diagonal tile), which changes no bit of O or lse.
// Key split (mxfp4_attn_split_kernel, the decoding forward of kv_cache_mxfp4.py): mx_tile, the tile
// body both kernels share, over a range of the keys, from m = -inf, writing the unnormalised (O_s, m_s,
// l_s); the merge weighs the splits by 2^(m_s - max_s m_s), exact because every m_s is an integer, and
// applies the epilogue above.  tests/mxfp4_split_ref.py restates it; tests/test_gpu_mxfp4_cache.py
// checks it.  Its LEN instantiation reads a preallocated cache with one length per sequence, which
// the "cache append" kernels below grow in place (tests/mxfp4_ragged_ref.py restates it,
// tests/test_gpu_mxfp4_ragged.py checks both).  Its PAGED instantiation reads the same tiles from a
// pool of pages through a block table ("paged pool" below; tests/test_gpu_mxfp4_paged.py holds it to
// the LEN instantiation bit for bit).  Its VARLEN instantiation runs a ragged batch of packed queries
// over that pool in one launch, from two host-built tables, with compact partials, a merge and a packed
// append of its own (tests/test_gpu_mxfp4_varlen.py holds every sequence to its run alone bit for bit).
// What these layers share stands once: mx_load_q and mx_tile (the tile body of every attention kernel);
// mx_merge_row (the merge of both combine kernels, which also defines the rounding to f16;
// tests/mxfp4_split_ref.py merge_bits restates it bit for bit); mx_requant_v_block and mx_append_k_block
// (the bodies of the padded, paged and packed append kernels, which differ in how a thread finds its
// sequence, head and source row); and on the host MxSplitCall + mx_split_launch (every key-split entry:
// its own argument checks, the call filled in, a dispatch on `causal`), mx_packed_call (the checks and the call of
// the packed entries without groups at every head_dim; mx_varlen_call for those of head_dim 128 alone),
// mx_varlen_paged (the plain and the windowed one), mx_append (the padded and the paged append) and, once for
// every head_dim in mxfp4_attn.h, mx_append_packed<D> (the packed append with and without rotary positions;
// mx_rope_block, the rotation both rope kernels put in front of the one quantiser body, is restated by
// tests/mxfp4_rope_ref.py and held bit for bit by tests/test_gpu_mxfp4_rope.py), mx_quant_rows_rope<D> and the
// launches of the two merges.  This file instantiates them at head_dim 128; head_dim 64 and 256 go to the
// instantiations in mxfp4_attn_d64.hip and mxfp4_attn_d256.hip, where mxfp4_attn_packed_kernel, the sibling of
// mxfp4_attn_split_kernel's VARLEN branch, runs over their rings.  The two rings here, MxRing and MxPagedRing, keep
// a piece plan each: holding one in common changed the paged kernels' instruction streams.
// Order: tools/asm_compare.py --labels compares two builds without the emission number a branch label carries, so
// no entry or kernel of these files has to keep its place for the comparison.
#include "mxfp4_attn.h"

using namespace qattn;

extern "C" int qattn_mxfp4_quant_rows(const void* x, const void* mean, void* q4, void* scale, long rows,
                                      long seq, int head_dim, void* stream) {
  if (head_dim != 64 && head_dim != 128 && head_dim != 256) return 1;
  if (mean && (seq <= 0 || rows % seq != 0)) return 1;
  const long nblk = rows * head_dim / 32;
  if (nblk == 0) return 0;
  if (head_dim == 256) return mx256_quant_rows(x, mean, q4, scale, nblk, seq, stream);
  dim3 grid((unsigned)((nblk + 255) / 256)), block(256);
  if (head_dim == 128)
    hipLaunchKernelGGL((mx_quant_rows_kernel<128>), grid, block, 0, (hipStream_t)stream,
                       (const _Float16*)x, (const _Float16*)mean, (uint8_t*)q4, (uint8_t*)scale, nblk, seq);
  else
    hipLaunchKernelGGL((mx_quant_rows_kernel<64>), grid, block, 0, (hipStream_t)stream,
                       (const _Float16*)x, (const _Float16*)mean, (uint8_t*)q4, (uint8_t*)scale, nblk, seq);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int qattn_mxfp4_quant_vt(const void* v, void* vt, void* vscale, long bh, long seq, int head_dim,
                                    void* stream) {
  if (seq % 64 != 0 || (head_dim != 64 && head_dim != 128)) return 1;
  const long nthr = bh * (seq / 64) * head_dim * 2;
  if (nthr == 0) return 0;
  dim3 grid((unsigned)((nthr + 255) / 256)), block(256);
  if (head_dim == 128)
    hipLaunchKernelGGL((mx_quant_vt_kernel<128>), grid, block, 0, (hipStream_t)stream,
                       (const _Float16*)v, (uint8_t*)vt, (uint8_t*)vscale, nthr, (int)seq);
  else
    hipLaunchKernelGGL((mx_quant_vt_kernel<64>), grid, block, 0, (hipStream_t)stream,
                       (const _Float16*)v, (uint8_t*)vt, (uint8_t*)vscale, nthr, (int)seq);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

template <bool CAUSAL>
static int mxfp4_attn_launch(const void* q4, const void* qscale, const void* k4, const void* kscale,
                             const void* vt, const void* vscale, void* out, void* lse, long bh, long sq,
                             long sk, int group, float qks, int qoff, void* stream) {
  using C = MxCfg<128>;
  const int nq = (int)((sq + C::QROWS - 1) / C::QROWS);
  const int lds = C::NSLOT * C::SLOT;
  { static LdsGrant granted_; lds_grant((const void*)mxfp4_attn_fwd_kernel<128, CAUSAL>, lds, granted_); }
  hipLaunchKernelGGL((mxfp4_attn_fwd_kernel<128, CAUSAL>), dim3((unsigned)(nq * bh)), dim3(256), lds,
                     (hipStream_t)stream, (const uint8_t*)q4, (const uint8_t*)qscale, (const uint8_t*)k4,
                     (const uint8_t*)kscale, (const uint8_t*)vt, (const uint8_t*)vscale, (_Float16*)out,
                     (float*)lse, (int)bh, (int)sq, (int)sk, group, qks, qoff);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// causal: 0 none, 1 top-left (row i sees keys <= i), 2 bottom-right (keys <= i + sk - sq; sk >= sq)
extern "C" int qattn_mxfp4_attn_fwd_ex(const void* q4, const void* qscale, const void* k4,
                                       const void* kscale, const void* vt, const void* vscale, void* out,
                                       void* lse, long bh, long sq, long sk, int group, int causal,
                                       int head_dim, float qks, void* stream) {
  if (sq % 32 != 0 || sk % 64 != 0 || group < 1 || bh % group != 0 || head_dim != 128) return 1;
  if (causal < 0 || causal > 2 || (causal == 2 && sk < sq)) return 1;
  if (bh == 0 || sq == 0) return 0;
  if (sk == 0) return 1;
  if (causal)
    return mxfp4_attn_launch<true>(q4, qscale, k4, kscale, vt, vscale, out, lse, bh, sq, sk, group, qks,
                                   causal == 2 ? (int)(sk - sq) : 0, stream);
  return mxfp4_attn_launch<false>(q4, qscale, k4, kscale, vt, vscale, out, lse, bh, sq, sk, group, qks, 0,
                                  stream);
}

extern "C" int qattn_mxfp4_attn_fwd(const void* q4, const void* qscale, const void* k4,
                                    const void* kscale, const void* vt, const void* vscale, void* out,
                                    void* lse, long bh, long sq, long sk, int group, int head_dim,
                                    float qks, void* stream) {
  return qattn_mxfp4_attn_fwd_ex(q4, qscale, k4, kscale, vt, vscale, out, lse, bh, sq, sk, group, 0,
                                 head_dim, qks, stream);
}

// what the padded key-split entries ask of their rows
static bool mx_rows_ok(long sq_head, long rows) { return sq_head >= 1 && rows % sq_head == 0; }

// the padded layouts' grid: (row blocks x key/value heads, splits of sk keys), false past the launch limits
static bool mx_split_grid(MxSplitCall& c, long sk) {
  const long nrb = (c.rows + MxCfg<128>::QROWS - 1) / MxCfg<128>::QROWS;
  const long nsplit = (sk + c.kps - 1) / c.kps;
  if (nrb * c.bhv > 0x7fffffffL || nsplit > 65535) return false;
  c.grid = dim3((unsigned)(nrb * c.bhv), (unsigned)nsplit);
  return true;
}

// the decoding layout: bhv key/value heads, each attended by one virtual head of rows = G * sq_head
// query rows; causal 0 or 2 (bottom-right over the cache: row r sees keys <= r % sq_head + sk - sq_head)
extern "C" int qattn_mxfp4_attn_fwd_split(const void* q4, const void* qscale, const void* k4,
                                          const void* kscale, const void* vt, const void* vscale,
                                          void* opart, void* ml, long bhv, long rows, long sq_head, long sk,
                                          int causal, int keys_per_split, int head_dim, float qks,
                                          void* stream) {
  if (!mx_split_ok(head_dim, keys_per_split) || bhv < 0 || rows < 0 || sk < 0 || sk % 64 != 0) return 1;
  if (!mx_rows_ok(sq_head, rows)) return 1;
  if ((causal != 0 && causal != 2) || (causal == 2 && sk < sq_head)) return 1;
  if (bhv == 0 || rows == 0) return 0;
  // 32-bit row indices inside a virtual head and 32-bit byte ranges of a key/value head
  if (sk == 0 || sk > (1L << 25) || rows > (1L << 30) || bhv > 0x7fffffffL) return 1;
  MxSplitCall c{q4, qscale, k4, kscale, vt, vscale, opart, ml, (int)bhv, (int)rows, (int)sq_head, (int)sk,
                keys_per_split, qks, (int)(sk - sq_head), nullptr, 1, nullptr, 0, 0, 0, MxVarlen{}, dim3()};
  if (!mx_split_grid(c, sk)) return 1;
  return causal ? mx_split_launch<true, false, false, false, false>(c, stream)
                : mx_split_launch<false, false, false, false, false>(c, stream);
}

// the same over a preallocated cache of cap tokens per head with one length per sequence (lens i32
// [bhv / heads_per_seq] on the device; the host guarantees 1 <= lens[b] <= sk_max and, causal,
// lens[b] >= sq_head); grid.y = ceil(sk_max / keys_per_split)
extern "C" int qattn_mxfp4_attn_fwd_split_len(const void* q4, const void* qscale, const void* k4,
                                              const void* kscale, const void* vt, const void* vscale,
                                              void* opart, void* ml, const void* lens, long bhv,
                                              long heads_per_seq, long rows, long sq_head, long cap,
                                              long sk_max, int causal, int keys_per_split, int head_dim,
                                              float qks, void* stream) {
  if (!mx_split_ok(head_dim, keys_per_split) || bhv < 0 || rows < 0 || !lens) return 1;
  if (cap % 64 != 0 || sk_max % 64 != 0 || sk_max < 64 || sk_max > cap || cap > (1L << 25)) return 1;
  if (!mx_rows_ok(sq_head, rows) || heads_per_seq < 1 || bhv % heads_per_seq != 0) return 1;
  if (causal != 0 && causal != 2) return 1;
  if (bhv == 0 || rows == 0) return 0;
  if (rows > (1L << 30) || bhv > 0x7fffffffL) return 1;
  MxSplitCall c{q4, qscale, k4, kscale, vt, vscale, opart, ml, (int)bhv, (int)rows, (int)sq_head, (int)cap,
                keys_per_split, qks, 0, lens, (int)heads_per_seq, nullptr, 0, 0, 0, MxVarlen{}, dim3()};
  if (!mx_split_grid(c, sk_max)) return 1;
  return causal ? mx_split_launch<true, true, false, false, false>(c, stream)
                : mx_split_launch<false, true, false, false, false>(c, stream);
}

// An append of n new tokens per sequence (kernels and format: "cache append" above), into the
// preallocated cache of cap tokens per head or, PAGED, through block_table into the pool; the three
// launches are stream-ordered, nothing is read back
template <bool PAGED>
static int mx_append(const void* k, const void* v, const void* k_mean, void* k4, void* kscale, void* vt,
                     void* vscale, void* vtail, void* lens, const void* counts, const void* block_table,
                     long batch, long kv_heads, long n, long cap, long mpp, int lgt, long npool, int head_dim,
                     void* stream) {
  if (head_dim != 128 || n < 1 || n > (1L << 25) || batch < 0 || batch > 0x7fffffffL) return 1;
  if (!k || !v || !k4 || !kscale || !vt || !vscale || !vtail || !lens) return 1;
  const long bhv = batch * kv_heads;
  if (bhv == 0 || cap == 0) return 0;
  const long ntile = (n + 62) / 64 + 1;   // tiles n tokens can touch from any start
  const long nthr = bhv * ntile * 128 * 2, nblk = bhv * n * (128 / 32);
  if ((nthr + 255) / 256 > 0x7fffffffL || (nblk + 255) / 256 > 0x7fffffffL) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((mx_append_vt_kernel<128, PAGED>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st,
                     (const _Float16*)v, (const _Float16*)vtail, (uint8_t*)vt, (uint8_t*)vscale,
                     (const int*)lens, (const int*)counts, nthr, (int)kv_heads, (int)n, (int)ntile, (int)cap,
                     (const int*)block_table, (int)mpp, lgt, (int)npool);
  hipLaunchKernelGGL((mx_append_k_kernel<128, PAGED>), dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st,
                     (const _Float16*)k, (const _Float16*)v, (const _Float16*)k_mean, (uint8_t*)k4,
                     (uint8_t*)kscale, (_Float16*)vtail, (const int*)lens, (const int*)counts, nblk,
                     (int)kv_heads, (int)n, (int)cap, (const int*)block_table, (int)mpp, lgt, (int)npool);
  hipLaunchKernelGGL(mx_append_len_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st,
                     (int*)lens, (const int*)counts, (int)batch, (int)n, (int)cap);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// append n new tokens per sequence to a preallocated cache
extern "C" int qattn_mxfp4_cache_append(const void* k, const void* v, const void* k_mean, void* k4,
                                        void* kscale, void* vt, void* vscale, void* vtail, void* lens,
                                        const void* counts, long batch, long kv_heads, long n, long cap,
                                        int head_dim, void* stream) {
  if (cap < 0 || cap % 64 != 0 || cap > (1L << 25) || kv_heads < 0 || kv_heads > 0x7fffffffL) return 1;
  return mx_append<false>(k, v, k_mean, k4, kscale, vt, vscale, vtail, lens, counts, nullptr, batch, kv_heads,
                          n, cap, 0, 0, 0, head_dim, stream);
}

// qattn_mxfp4_attn_fwd_split_len over the paged pool: the operands are pages of page_tokens tokens x
// heads_per_seq heads, block_table i32 [bhv / heads_per_seq][max_pages_per_seq] on the device
extern "C" int qattn_mxfp4_attn_fwd_split_paged(const void* q4, const void* qscale, const void* k4,
                                                const void* kscale, const void* vt, const void* vscale,
                                                void* opart, void* ml, const void* lens,
                                                const void* block_table, long bhv, long heads_per_seq,
                                                long rows, long sq_head, long num_pages, long page_tokens,
                                                long max_pages_per_seq, long sk_max, int causal,
                                                int keys_per_split, int head_dim, float qks, void* stream) {
  if (!mx_split_ok(head_dim, keys_per_split) || bhv < 0 || rows < 0 || !lens || !block_table) return 1;
  const int lgt = mx_page_lgt(page_tokens);
  if (!mx_pool_ok(num_pages, heads_per_seq, lgt, max_pages_per_seq)) return 1;
  if (sk_max % 64 != 0 || sk_max < 64 || sk_max > max_pages_per_seq * page_tokens) return 1;
  if (!mx_rows_ok(sq_head, rows) || bhv % heads_per_seq != 0) return 1;
  if (causal != 0 && causal != 2) return 1;
  if (bhv == 0 || rows == 0) return 0;
  if (rows > (1L << 30) || bhv > 0x7fffffffL) return 1;
  MxSplitCall c{q4, qscale, k4, kscale, vt, vscale, opart, ml, (int)bhv, (int)rows, (int)sq_head,
                (int)(max_pages_per_seq * page_tokens), keys_per_split, qks, 0, lens, (int)heads_per_seq,
                block_table, (int)max_pages_per_seq, lgt, (int)num_pages, MxVarlen{}, dim3()};
  if (!mx_split_grid(c, sk_max)) return 1;
  return causal ? mx_split_launch<true, true, true, false, false>(c, stream)
                : mx_split_launch<false, true, true, false, false>(c, stream);
}

// qattn_mxfp4_cache_append into the paged pool: the pages the new tokens need are in block_table already
extern "C" int qattn_mxfp4_paged_append(const void* k, const void* v, const void* k_mean, void* k4,
                                        void* kscale, void* vt, void* vscale, void* vtail, void* lens,
                                        const void* counts, const void* block_table, long batch,
                                        long kv_heads, long n, long num_pages, long page_tokens,
                                        long max_pages_per_seq, int head_dim, void* stream) {
  const int lgt = mx_page_lgt(page_tokens);
  if (!block_table || !mx_pool_ok(num_pages, kv_heads, lgt, max_pages_per_seq)) return 1;
  return mx_append<true>(k, v, k_mean, k4, kscale, vt, vscale, vtail, lens, counts, block_table, batch,
                         kv_heads, n, max_pages_per_seq * page_tokens, max_pages_per_seq, lgt, num_pages,
                         head_dim, stream);
}

// The two packed entries below.  window < 1: no window (the plain entry); else causal is 2.
static int mx_varlen_paged(const void* q4, const void* qscale, const void* k4, const void* kscale,
                           const void* vt, const void* vscale, void* opart, void* ml, const void* lens,
                           const void* block_table, const void* seq_rec, const void* work, long nseq,
                           long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
                           long num_pages, long page_tokens, long max_pages_per_seq, int causal,
                           int keys_per_split, int head_dim, float qks, long window, long sinks,
                           void* stream) {
  MxSplitCall c;
  const int rc = mx_packed_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec,
                                work, nseq, nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages,
                                page_tokens, max_pages_per_seq, causal, keys_per_split, head_dim, qks, window,
                                sinks, nullptr);
  if (rc >= 0) return rc;
  if (head_dim != 128) return mx_packed_wide<false, false>(c, head_dim, causal, window, stream);
  if (window < 1)
    return causal ? mx_split_launch<true, true, true, true, false>(c, stream)
                  : mx_split_launch<false, true, true, true, false>(c, stream);
  return mx_split_launch<true, true, true, true, true>(c, stream);
}

// the packed (varlen) step over the paged pool (kernel: mxfp4_attn_split_kernel VARLEN; the tables are
// the host plan of kv_cache_mxfp4.plan_varlen)
extern "C" int qattn_mxfp4_attn_fwd_varlen_paged(const void* q4, const void* qscale, const void* k4,
                                                 const void* kscale, const void* vt, const void* vscale,
                                                 void* opart, void* ml, const void* lens,
                                                 const void* block_table, const void* seq_rec,
                                                 const void* work, long nseq, long nwork, long tokens,
                                                 long part_rows, long max_seqs, long kv_heads, long group,
                                                 long num_pages, long page_tokens, long max_pages_per_seq,
                                                 int causal, int keys_per_split, int head_dim, float qks,
                                                 void* stream) {
  return mx_varlen_paged(q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, nseq,
                         nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages, page_tokens,
                         max_pages_per_seq, causal, keys_per_split, head_dim, qks, 0, 0, stream);
}

// the packed step with a sliding window and sinks (kernel: mxfp4_attn_split_kernel WINDOW): query i of
// sequence j at position p = L_j - n_j + i sees key k iff k <= p and (k > p - window or k < sinks).  The
// arguments and limits of the entry above; seq_rec[j][5], [6] carry the sequence's first window tile and
// its sink tiles (plan_varlen with a window).  The merge is qattn_mxfp4_varlen_combine.
extern "C" int qattn_mxfp4_attn_fwd_varlen_paged_window(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int causal, int keys_per_split, int head_dim,
    float qks, long window, long sinks, void* stream) {
  if (window < 1 || sinks < 0 || causal != 2) return 1;
  return mx_varlen_paged(q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, nseq,
                         nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages, page_tokens,
                         max_pages_per_seq, causal, keys_per_split, head_dim, qks, window, sinks, stream);
}

// the merge of the packed step's compact partials into O f16 [tokens][q_heads][head_dim], lse [tokens][q_heads];
// sink_logit f32 [q_heads] on the device, natural-log units (mx_merge_row SINK: lse then covers the visible keys
// and the sink), or null: none
static int mx_varlen_combine(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                             const void* sink_logit, long nseq, long tokens, long q_heads, long kv_heads,
                             long part_rows, int head_dim, void* stream) {
  if (head_dim != 64 && head_dim != 128 && head_dim != 256) return 1;
  if (nseq < 0 || tokens < 0 || part_rows < 0 || !seq_rec) return 1;
  if (kv_heads < 1 || q_heads < 1 || q_heads % kv_heads != 0 || q_heads > 0x7fffffffL) return 1;
  if (nseq == 0 || tokens == 0) return 0;
  if (nseq > tokens || part_rows < 1) return 1;
  if (tokens > 0x7fffffffL / q_heads || part_rows > 0x7fffffffL) return 1;
  const auto launch = head_dim == 64    ? mx_varlen_combine_launch<64>
                      : head_dim == 128 ? mx_varlen_combine_launch<128>
                                        : mx_varlen_combine_launch<256>;
  return launch(opart, ml, out, lse, seq_rec, sink_logit, nseq, tokens * q_heads, q_heads, kv_heads, part_rows,
                stream);
}

extern "C" int qattn_mxfp4_varlen_combine(const void* opart, const void* ml, void* out, void* lse,
                                          const void* seq_rec, long nseq, long tokens, long q_heads,
                                          long kv_heads, long part_rows, int head_dim, void* stream) {
  return mx_varlen_combine(opart, ml, out, lse, seq_rec, nullptr, nseq, tokens, q_heads, kv_heads, part_rows,
                           head_dim, stream);
}

extern "C" int qattn_mxfp4_varlen_combine_sink(const void* opart, const void* ml, void* out, void* lse,
                                               const void* seq_rec, const void* sink_logit, long nseq,
                                               long tokens, long q_heads, long kv_heads, long part_rows,
                                               int head_dim, void* stream) {
  if (!sink_logit) return 1;
  return mx_varlen_combine(opart, ml, out, lse, seq_rec, sink_logit, nseq, tokens, q_heads, kv_heads, part_rows,
                           head_dim, stream);
}

// the packed append (mx_append_packed<D>, mxfp4_attn.h) at the entry's head_dim
static int mx_append_packed_any(bool rope, bool had, const void* k, const void* v, const void* k_mean, void* k4,
                                void* kscale, void* vt, void* vscale, void* vtail, void* lens, const void* block_table,
                                const void* seq_tab, const void* tiles, long nseq, long ntiles, long tokens,
                                long max_seqs, long kv_heads, long num_pages, long page_tokens,
                                long max_pages_per_seq, int head_dim, const void* cos_sin, const void* pos,
                                long max_pos, int interleaved, void* stream) {
  if (head_dim != 64 && head_dim != 128 && head_dim != 256) return 1;
  const auto append = head_dim == 64 ? mx_append_packed<64> : head_dim == 128 ? mx_append_packed<128>
                                                                              : mx_append_packed<256>;
  return append(rope, had, k, v, k_mean, k4, kscale, vt, vscale, vtail, lens, block_table, seq_tab, tiles, nseq, ntiles,
                tokens, max_seqs, kv_heads, num_pages, page_tokens, max_pages_per_seq, cos_sin, pos, max_pos,
                interleaved, stream);
}

extern "C" int qattn_mxfp4_paged_append_packed(const void* k, const void* v, const void* k_mean, void* k4,
                                               void* kscale, void* vt, void* vscale, void* vtail,
                                               void* lens, const void* block_table, const void* seq_tab,
                                               const void* tiles, long nseq, long ntiles, long tokens,
                                               long max_seqs, long kv_heads, long num_pages,
                                               long page_tokens, long max_pages_per_seq, int head_dim,
                                               void* stream) {
  return mx_append_packed_any(false, false, k, v, k_mean, k4, kscale, vt, vscale, vtail, lens, block_table, seq_tab,
                              tiles, nseq, ntiles, tokens, max_seqs, kv_heads, num_pages, page_tokens,
                              max_pages_per_seq, head_dim, nullptr, nullptr, 0, 0, stream);
}

extern "C" int qattn_mxfp4_split_combine(const void* opart, const void* ml, void* out, void* lse,
                                         long rows_total, int nsplit, int head_dim, void* stream) {
  if (head_dim != 128 || rows_total < 0 || nsplit < 1) return 1;
  if (rows_total == 0) return 0;
  const long nthr = rows_total * (128 / 8);
  if ((nthr + 255) / 256 > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(mxfp4_split_combine_kernel<128>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)opart, (const float2*)ml, (_Float16*)out,
                     (float*)lse, rows_total, nsplit);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The packed step with shared prefixes (kernel: mxfp4_attn_split_kernel SHARED; the tables are the host
// plan of kv_cache_mxfp4.plan_varlen_shared): qattn_mxfp4_attn_fwd_varlen_paged with work records of two
// kinds, [j, row block, split, 0] as there and [g, row block of group g's stacked rows, split, 1], which
// one workgroup runs once for every member of the group (grp_rec i32 [ngroup][4], members i32
// [nmember][2] on the device).  Partials and merge are the plain entry's.
extern "C" int qattn_mxfp4_attn_fwd_varlen_paged_shared(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int causal, int keys_per_split, int head_dim,
    float qks, const void* grp_rec, const void* members, long ngroup, long nmember, void* stream) {
  if (!mx_split_ok(head_dim, keys_per_split) || nseq < 0 || nwork < 0 || tokens < 0 || part_rows < 0) return 1;
  if (!lens || !block_table || !seq_rec || !work || !grp_rec || !members) return 1;
  const int lgt = mx_page_lgt(page_tokens);
  if (!mx_pool_ok(num_pages, kv_heads, lgt, max_pages_per_seq)) return 1;
  if (max_seqs < 1 || group < 1 || group > 0x7fffffffL || (causal != 0 && causal != 2)) return 1;
  // at least one group, every group of at least two members, no sequence in two groups
  if (ngroup < 1 || nmember < 2 * ngroup || nmember > nseq) return 1;
  if (nwork == 0 || tokens == 0) return 0;
  if (nseq > max_seqs || nseq > tokens || part_rows < 1) return 1;
  // 32-bit packed rows, partial rows, workgroups and slot heads; a group's stacked rows are among the
  // packed rows
  if (tokens > 0x7fffffffL / (group * kv_heads) || part_rows > 0x7fffffffL) return 1;
  if (nwork > 0x7fffffffL / kv_heads || max_seqs > 0x7fffffffL / kv_heads) return 1;
  const MxVarlen vl{(const int*)work, (const int*)seq_rec, (int)nseq, (int)group, tokens * group * kv_heads,
                    part_rows, 0, 0, (const int*)grp_rec, (const int*)members, (int)ngroup, (int)nmember};
  const MxSplitCall c{q4, qscale, k4, kscale, vt, vscale, opart, ml, (int)(max_seqs * kv_heads), 0, 1,
                      (int)(max_pages_per_seq * page_tokens), keys_per_split, qks, 0, lens, (int)kv_heads,
                      block_table, (int)max_pages_per_seq, lgt, (int)num_pages, vl,
                      dim3((unsigned)(nwork * kv_heads))};
  return causal ? mx_split_launch<true, true, true, true, false, true>(c, stream)
                : mx_split_launch<false, true, true, true, false, true>(c, stream);
}

// The packed step with a tree mask on every sequence's last queries (kernel: mxfp4_attn_split_kernel TREE;
// kv_cache_mxfp4.attention_mxfp4_varlen_paged(tree=)): qattn_mxfp4_attn_fwd_varlen_paged at causal == 2
// with seq_rec[j][7] = nd_j tree nodes and tree_masks u64 [tokens] on the device, the ancestor word of
// every packed token (0 outside a tree).  Partials and merge are the plain entry's.
extern "C" int qattn_mxfp4_attn_fwd_varlen_paged_tree(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int causal, int keys_per_split, int head_dim,
    float qks, const void* tree_masks, void* stream) {
  if (causal != 2 || !tree_masks) return 1;
  MxSplitCall c;
  const int rc = mx_varlen_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec,
                                work, nseq, nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages,
                                page_tokens, max_pages_per_seq, causal, keys_per_split, head_dim, qks, 0, 0,
                                tree_masks);
  if (rc >= 0) return rc;
  return mx_split_launch<true, true, true, true, false, false, true>(c, stream);
}

// ---- rollback of the paged pool (kv_cache_mxfp4.py PagedKVFP4.rollback)
// recs i32 [nrec][4] = {slot, L0, row in saved, 0} (distinct slots); saved f16 [nsaved][Hkv][64][D] is the
// copy of the listed slots' vtail rows that PagedKVFP4.checkpoint took when sequence slot held L0 tokens.
// One thread per (record, head, column d, half h), in mx_append_vt_kernel's order: it puts the column's
// elements of vtail rows [0, L0 % 64) of its half's keys back, quantises its block of V tile L0 / 64 again
// FROM THE SAVED ROWS when L0 % 64 != 0 (mx_requant_v_block with no new token: the keys at or past L0 are
// zero, as after the appends that made L0), and thread (head 0, d 0, h 0) writes lens[slot] = L0.  The
// tile is written where the block table puts it; page L0 / P of the slot is still the sequence's.  A
// record whose slot, L0 or row lies outside [0, B), [0, cap] or [0, nsaved) writes nothing.
namespace qattn {
template <int D>
__global__ __launch_bounds__(256) void mx_rollback_kernel(const _Float16* __restrict__ saved,
                                                          _Float16* __restrict__ vtail,
                                                          uint8_t* __restrict__ vt, uint8_t* __restrict__ vs,
                                                          int* __restrict__ lens, const int* __restrict__ recs,
                                                          long nthr, int nsaved, int B, int Hkv, int cap,
                                                          const int* __restrict__ btab, int mpp, int lgt,
                                                          int npool) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nthr) return;
  const int h = (int)(i & 1);
  const int d = (int)((i >> 1) % D);
  const long rh = (i >> 1) / D;                 // record * Hkv + head
  const int hd = (int)(rh % Hkv);
  const int* rec = recs + 4 * (rh / Hkv);
  const int slot = rec[0], L0 = rec[1], row = rec[2];
  if (slot < 0 || slot >= B || L0 < 0 || L0 > cap || row < 0 || row >= nsaved) return;
  const _Float16* src = saved + (((long)row * Hkv + hd) * 64) * D + d;
  _Float16* dst = vtail + (((long)slot * Hkv + hd) * 64) * D + d;
  const int live = L0 % 64;
#pragma unroll 4
  for (int j = 0; j < 32; ++j) {
    const int key = 32 * (j >> 4) + 8 * ((j >> 2) & 3) + 4 * h + (j & 3);
    if (key < live) dst[(long)key * D] = src[(long)key * D];
  }
  if (live) {
    const long o = (mx_paged_tile(btab, slot, hd, L0 / 64, Hkv, mpp, lgt, npool) * D + d) * 2 + h;
    mx_requant_v_block<D>(src, src, 1, L0 / 64, L0, 0, h, reinterpret_cast<v4i*>(vt) + o, vs + o);
  }
  if (hd == 0 && d == 0 && h == 0) lens[slot] = L0;
}
}  // namespace qattn

extern "C" int qattn_mxfp4_paged_rollback(const void* saved, void* vtail, void* vt, void* vscale, void* lens,
                                          const void* block_table, const void* recs, long nrec, long nsaved,
                                          long max_seqs, long kv_heads, long num_pages, long page_tokens,
                                          long max_pages_per_seq, int head_dim, void* stream) {
  if (head_dim != 128 || nrec < 0 || nsaved < 0 || max_seqs < 1) return 1;
  if (!saved || !vtail || !vt || !vscale || !lens || !block_table || !recs) return 1;
  const int lgt = mx_page_lgt(page_tokens);
  if (!mx_pool_ok(num_pages, kv_heads, lgt, max_pages_per_seq)) return 1;
  if (nrec == 0) return 0;
  if (nrec > max_seqs || nsaved < 1 || nsaved > 0x7fffffffL || max_seqs > 0x7fffffffL / kv_heads) return 1;
  const long nthr = nrec * kv_heads * 128 * 2;
  if ((nthr + 255) / 256 > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(mx_rollback_kernel<128>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const _Float16*)saved, (_Float16*)vtail, (uint8_t*)vt,
                     (uint8_t*)vscale, (int*)lens, (const int*)recs, nthr, (int)nsaved, (int)max_seqs,
                     (int)kv_heads, (int)(max_pages_per_seq * page_tokens), (const int*)block_table,
                     (int)max_pages_per_seq, lgt, (int)num_pages);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// ------------------------------------------------------------------------------ rotary positions
// ("rotary positions" above) q quantised for the packed step with its rotation, and the packed append that
// rotates the new keys
extern "C" int qattn_mxfp4_quant_rows_rope(const void* x, void* q4, void* scale, const void* cos_sin,
                                           const void* pos, long tokens, long heads, long max_pos,
                                           int interleaved, int head_dim, void* stream) {
  if (head_dim != 64 && head_dim != 128 && head_dim != 256) return 1;
  const auto quant = head_dim == 64 ? mx_quant_rows_rope<64> : head_dim == 128 ? mx_quant_rows_rope<128>
                                                                               : mx_quant_rows_rope<256>;
  return quant(x, q4, scale, cos_sin, pos, tokens, heads, max_pos, interleaved, stream);
}

extern "C" int qattn_mxfp4_paged_append_packed_rope(
    const void* k, const void* v, const void* k_mean, void* k4, void* kscale, void* vt, void* vscale,
    void* vtail, void* lens, const void* block_table, const void* seq_tab, const void* tiles, long nseq,
    long ntiles, long tokens, long max_seqs, long kv_heads, long num_pages, long page_tokens,
    long max_pages_per_seq, int head_dim, const void* cos_sin, const void* pos, long max_pos, int interleaved,
    void* stream) {
  return mx_append_packed_any(true, false, k, v, k_mean, k4, kscale, vt, vscale, vtail, lens, block_table, seq_tab,
                              tiles, nseq, ntiles, tokens, max_seqs, kv_heads, num_pages, page_tokens,
                              max_pages_per_seq, head_dim, cos_sin, pos, max_pos, interleaved, stream);
}

// ------------------------------------------------------------------------------ Hadamard-rotated pools
// ("Hadamard-rotated Q and K" in mxfp4_attn.h) the two quantiser entries of a pool made with hadamard=True: the rope
// entries above with the transform between the f16 row and its scales; a null cos_sin: no rope
extern "C" int qattn_mxfp4_quant_rows_had(const void* x, void* q4, void* scale, const void* cos_sin,
                                          const void* pos, long tokens, long heads, long max_pos, int interleaved,
                                          int head_dim, void* stream) {
  if (head_dim != 64 && head_dim != 128 && head_dim != 256) return 1;
  const auto quant = head_dim == 64 ? mx_quant_rows_had<64> : head_dim == 128 ? mx_quant_rows_had<128>
                                                                              : mx_quant_rows_had<256>;
  return quant(x, q4, scale, cos_sin, pos, tokens, heads, max_pos, interleaved, stream);
}

extern "C" int qattn_mxfp4_paged_append_packed_had(
    const void* k, const void* v, const void* k_mean, void* k4, void* kscale, void* vt, void* vscale,
    void* vtail, void* lens, const void* block_table, const void* seq_tab, const void* tiles, long nseq,
    long ntiles, long tokens, long max_seqs, long kv_heads, long num_pages, long page_tokens,
    long max_pages_per_seq, int head_dim, const void* cos_sin, const void* pos, long max_pos, int interleaved,
    void* stream) {
  return mx_append_packed_any(cos_sin != nullptr, true, k, v, k_mean, k4, kscale, vt, vscale, vtail, lens,
                              block_table, seq_tab, tiles, nseq, ntiles, tokens, max_seqs, kv_heads, num_pages,
                              page_tokens, max_pages_per_seq, head_dim, cos_sin, pos, max_pos, interleaved, stream);
}

// ------------------------------------------------------------------------------ device-planned decode step
// (kv_cache_mxfp4.py DecodeStep) One new token for each of up to n listed sequences, with nothing in the
// launches that a host computed from the lengths: shapes, grids and pointers are fixed when the step is made,
// so the append and the attention can be captured once and replayed while the lengths move.
// mx_decode_plan_kernel, one thread per entry i < n, reads b = slots[i] and L = lens[b], the length BEFORE the
// append, and writes what the host plan would have uploaded (kv_cache_mxfp4.plan_decode_step restates it):
//   tab[i]     = {b, 1, i, 0}      the record of mx_append_*_packed_kernel: packed token i goes to slot b
//   tiles[i]   = {i, L / 64}       the one V tile that append touches
//   pos[i]     = L                 the rotary position of the new token, key and query
//   seq_rec[i] = {b, i, 1, ns, i * splits * hq, wt0, nst, 0} for the length L + 1: plan_varlen's expressions at
//                one query, nt = ceil((L + 1) / 64), ns = ceil(nt * 64 / kps) without a window; with one, wt0 =
//                max(0, L + 1 - W) / 64 and nst = ceil(min(S, L + 1) / 64) when wt0 > nst (a gap), else 0, 0,
//                and ns = (nst > 0) + ceil((nt - wt0) * 64 / kps); ns is held to `splits`, the grid's.
// An entry whose b lies outside [0, B) or whose L lies outside [0, cap) is padding: tab {-1, 0, i, 0}, which
// the append kernels skip, tiles {-1, 0}, pos 0 and ns = 0, so no workgroup runs for it and the merge writes
// O = 0, lse = -inf.  lens is read only at a checked b; every store goes to row i < n of a table of n rows.
namespace qattn {
template <int KT>
__global__ __launch_bounds__(256) void mx_decode_plan_kernel(const int* __restrict__ slots,
                                                             const int* __restrict__ lens, int* __restrict__ tab,
                                                             int* __restrict__ tiles, int* __restrict__ seq_rec,
                                                             int* __restrict__ pos, int n, int B, int cap, int kt,
                                                             int splits, int hq, int window, int sinks) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = slots[i];
  int L = -1;
  if (b >= 0 && b < B) L = lens[b];
  const bool ok = L >= 0 && L < cap;
  int ns = 0, wt0 = 0, nst = 0;
  if (ok) {
    const int L1 = L + 1, nt = (L1 + KT - 1) / KT;
    if (window > 0) {
      const int w0 = max(0, L1 - window) / KT, s0 = (min(sinks, L1) + KT - 1) / KT;
      if (w0 > s0) {
        wt0 = w0;
        nst = s0;
      }
    }
    ns = min((nst > 0) + (nt - wt0 + kt - 1) / kt, splits);
  }
  reinterpret_cast<v4i*>(tab)[i] = v4i{ok ? b : -1, ok ? 1 : 0, i, 0};
  reinterpret_cast<int2*>(tiles)[i] = make_int2(ok ? i : -1, ok ? L / KT : 0);
  pos[i] = ok ? L : 0;
  reinterpret_cast<v4i*>(seq_rec)[2 * i] = v4i{ok ? b : -1, i, 1, ns};
  reinterpret_cast<v4i*>(seq_rec)[2 * i + 1] = v4i{i * splits * hq, wt0, nst, 0};
}
}  // namespace qattn

// (No head_dim: the tables count 64-key tiles, splits, packed rows and partial rows, none of which depends on
// the width of a row, so a step of either head_dim is planned by the same launch.)
extern "C" int qattn_mxfp4_decode_step_plan(const void* slots, const void* lens, void* seq_tab, void* tiles,
                                            void* seq_rec, void* pos, long n, long max_seqs, long capacity,
                                            long kv_heads, long group, int keys_per_split, long splits,
                                            long window, long sinks, void* stream) {
  if (!mx_split_ok(128, keys_per_split) || n < 0 || max_seqs < 1 || max_seqs > 0x7fffffffL) return 1;
  if (capacity < 64 || capacity % 64 || capacity > (1L << 25) || !mx_step_window_ok(window, sinks)) return 1;
  if (kv_heads < 1 || group < 1 || splits < 1 || splits > 65535) return 1;
  if (kv_heads > 0x7fffffffL / group || n > 0x7fffffffL / (splits * kv_heads * group)) return 1;
  if (n == 0) return 0;
  if (!slots || !lens || !seq_tab || !tiles || !seq_rec || !pos) return 1;
  const long big = 1L << 26;
  hipLaunchKernelGGL(mx_decode_plan_kernel<64>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const int*)slots, (const int*)lens, (int*)seq_tab, (int*)tiles, (int*)seq_rec, (int*)pos,
                     (int)n, (int)max_seqs, (int)capacity, keys_per_split / 64, (int)splits,
                     (int)(kv_heads * group), (int)(window < big ? window : big), (int)(sinks < big ? sinks : big));
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The attention of the step over its fixed grid (kernel: mxfp4_attn_split_kernel STEP; head_dim 64 and 256:
// mxfp4_attn_packed_kernel STEP): n entries x splits
// work records x kv_heads workgroups, causal, with the window's instantiation for window >= 1.  seq_rec is
// mx_decode_plan_kernel's, work i32 [n * splits][4] = {i, 0, s, 0} in any order; the partials hold n * splits
// * kv_heads * group rows.
extern "C" int qattn_mxfp4_attn_fwd_decode_step(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work, long n,
    long splits, long max_seqs, long kv_heads, long group, long num_pages, long page_tokens,
    long max_pages_per_seq, int keys_per_split, int head_dim, float qks, long window, long sinks, void* stream) {
  if (n < 0 || splits < 1 || splits > 65535 || kv_heads < 1 || group < 1 || !mx_step_window_ok(window, sinks))
    return 1;
  if (kv_heads > 0x7fffffffL / group || n > 0x7fffffffL / (splits * kv_heads * group)) return 1;
  if (n > 0 && (!q4 || !qscale || !k4 || !kscale || !vt || !vscale || !opart || !ml)) return 1;
  MxSplitCall c;
  const int rc = mx_packed_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work,
                                n, n * splits, n, n * splits * kv_heads * group, max_seqs, kv_heads, group,
                                num_pages, page_tokens, max_pages_per_seq, 2, keys_per_split, head_dim, qks,
                                window, sinks, nullptr);
  if (rc >= 0) return rc;
  if (head_dim != 128) return mx_packed_wide<true, false>(c, head_dim, 2, window, stream);   // mxfp4_attn_packed_kernel STEP
  return window < 1 ? mx_split_launch<true, true, true, true, false, false, false, true>(c, stream)
                    : mx_split_launch<true, true, true, true, true, false, false, true>(c, stream);
}

// what the two merge entries of the step check: the entry's status when there is nothing to launch, else -1
static int mx_step_combine_check(const void* opart, const void* ml, const void* out, const void* lse,
                                 const void* seq_rec, long n, long splits, long q_heads, long kv_heads,
                                 int head_dim) {
  if ((head_dim != 128 && head_dim != 64 && head_dim != 256) || n < 0 || splits < 1 || splits > 65535) return 1;
  if (kv_heads < 1 || q_heads < 1 || q_heads % kv_heads != 0 || q_heads > 0x7fffffffL) return 1;
  if (n > 0x7fffffffL / (splits * q_heads)) return 1;
  if (n == 0) return 0;
  return !opart || !ml || !out || !lse || !seq_rec ? 1 : -1;
}

// the merge of the step (mxfp4_decode_step_combine_kernel); sink f32 [q_heads] on the device or null: none
static int mx_step_combine(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                           const void* sink, long n, long splits, long q_heads, long kv_heads, int head_dim,
                           void* stream) {
  const int rc = mx_step_combine_check(opart, ml, out, lse, seq_rec, n, splits, q_heads, kv_heads, head_dim);
  if (rc >= 0) return rc;
  const auto launch = head_dim == 64    ? mx_step_combine_launch<64>
                      : head_dim == 128 ? mx_step_combine_launch<128>
                                        : mx_step_combine_launch<256>;
  return launch(opart, ml, out, lse, seq_rec, sink, n * q_heads, q_heads, splits, stream);
}

extern "C" int qattn_mxfp4_decode_step_combine(const void* opart, const void* ml, void* out, void* lse,
                                               const void* seq_rec, long n, long splits, long q_heads,
                                               long kv_heads, int head_dim, void* stream) {
  return mx_step_combine(opart, ml, out, lse, seq_rec, nullptr, n, splits, q_heads, kv_heads, head_dim, stream);
}

// with a learned sink logit per query head, which joins the rows of listed entries only: a padding entry gets O =
// 0 and lse = -inf, not lse = z
extern "C" int qattn_mxfp4_decode_step_combine_sink(const void* opart, const void* ml, void* out, void* lse,
                                                    const void* seq_rec, const void* sink_logit, long n,
                                                    long splits, long q_heads, long kv_heads, int head_dim,
                                                    void* stream) {
  if (!sink_logit) return 1;
  return mx_step_combine(opart, ml, out, lse, seq_rec, sink_logit, n, splits, q_heads, kv_heads, head_dim, stream);
}

// ------------------------------------------------------------------------------ device-planned verify step
// (kv_cache_mxfp4.py VerifyStep) K draft tokens -- a chain or a tree, 1 <= K <= 64 -- for each of up to n listed
// sequences, appended and attended under the tree mask with launches fixed when the step is made, as the decode
// step above.  mx_verify_plan_kernel, one thread per packed token i * K + t, reads b = slots[i] and L = lens[b],
// the length BEFORE the append, and the token's ancestor word, cleaned as the TREE kernel cleans it: (word & (self
// | (self - 1))) | self with self = 1 << t.  It writes (kv_cache_mxfp4.plan_verify_step restates it):
//   pos[i * K + t] = L + popcount(cleaned word) - 1     the node's depth behind the cached keys
// and, the thread of t = 0,
//   tab[i]           = {b, K, i * K, 0}                 the record of mx_append_*_packed_kernel
//   tiles[2 i]       = {i, L / 64}                      the V tiles the K tokens touch: at most two, as K <= 64;
//   tiles[2 i + 1]   = {i, (L + K - 1) / 64} if that is another tile, else {-1, 0}, which the append skips
//   seq_rec[i]       = {b, i * K, K, ns, i * splits * hq * K, 0, 0, K} for the length L + K: plan_varlen's record
//                      of K queries that are all tree nodes, ns = ceil(ceil((L + K) / 64) * 64 / kps) held to
//                      `splits`; only the partial base differs, a fixed stride instead of compact.
// An entry whose b lies outside [0, B), whose L is negative or whose L + K passes cap is padding: tab {-1, 0, i *
// K, 0}, both tiles {-1, 0}, pos 0 and ns = 0 (slot -1 in the record).  lens is read only at a checked b, tree
// only at i * K + t < n * K; every store goes to row i of a table of n rows (2 i, 2 i + 1 of 2 n; i * K + t of n
// * K).
namespace qattn {
template <int KT>
__global__ __launch_bounds__(256) void mx_verify_plan_kernel(const int* __restrict__ slots,
                                                             const int* __restrict__ lens,
                                                             const unsigned long* __restrict__ tree,
                                                             int* __restrict__ tab, int* __restrict__ tiles,
                                                             int* __restrict__ seq_rec, int* __restrict__ pos, int n,
                                                             int K, int B, int cap, int kt, int splits, int hq) {
  const int tok = (int)blockIdx.x * 256 + threadIdx.x;
  if (tok >= n * K) return;
  const int i = tok / K, t = tok % K;
  const int b = slots[i];
  int L = -1;
  if (b >= 0 && b < B) L = lens[b];
  const bool ok = L >= 0 && L <= cap - K;
  const unsigned long self = 1ul << t;
  const unsigned long word = (tree[tok] & (self | (self - 1))) | self;
  pos[tok] = ok ? L + __builtin_popcountl(word) - 1 : 0;
  if (t != 0) return;
  const int g0 = ok ? L / KT : 0, g1 = ok ? (L + K - 1) / KT : 0;
  const int ns = ok ? min(((L + K + KT - 1) / KT + kt - 1) / kt, splits) : 0;
  reinterpret_cast<v4i*>(tab)[i] = v4i{ok ? b : -1, ok ? K : 0, i * K, 0};
  reinterpret_cast<v4i*>(tiles)[i] = v4i{ok ? i : -1, g0, ok && g1 != g0 ? i : -1, g1 != g0 ? g1 : 0};
  reinterpret_cast<v4i*>(seq_rec)[2 * i] = v4i{ok ? b : -1, i * K, K, ns};
  reinterpret_cast<v4i*>(seq_rec)[2 * i + 1] = v4i{i * splits * hq * K, 0, 0, K};
}

// The merge of the step: entry i owns the partial rows [i * splits * Hq * K, (i + 1) * splits * Hq * K), laid out
// [split][kv head][g * K + t] (the packed step's layout at K queries), so nothing but ns is read from the record
// and every address lies inside the partials.  mx_merge_row over the entry's ns splits, the arithmetic of
// mxfp4_varlen_combine_kernel in its order; an entry with ns < 1 (padding) gets O = 0 and lse = -inf in all its
// K rows.
template <int D>
__global__ __launch_bounds__(256) void mxfp4_verify_step_combine_kernel(const float* __restrict__ opart,
                                                                        const float2* __restrict__ ml,
                                                                        _Float16* __restrict__ out,
                                                                        float* __restrict__ lse,
                                                                        const int* __restrict__ seq_rec, long rows,
                                                                        int Hq, int G, int K, int splits) {
  constexpr int TPR = D / 8;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid / TPR;
  if (row >= rows) return;
  const int c = (int)(gid % TPR);
  const long token = row / Hq;
  const int head = (int)(row % Hq);
  const long i = token / K;
  const int t = (int)(token % K);
  const int ns = min(seq_rec[8 * i + 3], splits);
  if (ns < 1) {
    *reinterpret_cast<v8h*>(out + row * D + 8 * c) = v8h{};
    if (c == 0) lse[row] = -INFINITY;
    return;
  }
  const long step = (long)Hq * K;
  mx_merge_row<D>(opart, ml, i * splits * step + (long)(head / G) * G * K + (long)(head % G) * K + t, step, ns, c,
                  out + row * D, lse + row);
}
}  // namespace qattn

// what the three entries of the verify step hold their sizes to: 1 <= K <= 64 draft tokens per entry and fewer
// than 2^31 partial rows
static bool mx_verify_sizes_ok(long n, long draft_tokens, long splits, long kv_heads, long group) {
  if (n < 0 || draft_tokens < 1 || draft_tokens > 64 || splits < 1 || splits > 65535) return false;
  if (kv_heads < 1 || group < 1 || kv_heads > 0x7fffffffL / group) return false;
  return n <= 0x7fffffffL / (splits * kv_heads * group * draft_tokens);
}

extern "C" int qattn_mxfp4_verify_step_plan(const void* slots, const void* lens, const void* tree, void* seq_tab,
                                            void* tiles, void* seq_rec, void* pos, long n, long draft_tokens,
                                            long max_seqs, long capacity, long kv_heads, long group,
                                            int keys_per_split, long splits, void* stream) {
  if (!mx_split_ok(128, keys_per_split) || max_seqs < 1 || max_seqs > 0x7fffffffL) return 1;
  if (capacity < 64 || capacity % 64 || capacity > (1L << 25)) return 1;
  if (!mx_verify_sizes_ok(n, draft_tokens, splits, kv_heads, group)) return 1;
  if (n == 0) return 0;
  if (!slots || !lens || !tree || !seq_tab || !tiles || !seq_rec || !pos) return 1;
  const long nthr = n * draft_tokens;
  hipLaunchKernelGGL(mx_verify_plan_kernel<64>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const int*)slots, (const int*)lens, (const unsigned long*)tree,
                     (int*)seq_tab, (int*)tiles, (int*)seq_rec, (int*)pos, (int)n, (int)draft_tokens, (int)max_seqs,
                     (int)capacity, keys_per_split / 64, (int)splits, (int)(kv_heads * group));
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The attention of the step over its fixed grid (kernel: mxfp4_attn_split_kernel STEP with TREE): n entries x
// ceil(group * K / 128) row blocks x splits work records x kv_heads workgroups.  seq_rec is
// mx_verify_plan_kernel's, work i32 [n * row blocks * splits][4] = {i, row block, s, 0} in any order, tree_masks
// u64 [n * K] the words the plan read; the partials hold n * splits * kv_heads * group * K rows.
extern "C" int qattn_mxfp4_attn_fwd_verify_step(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    const void* tree_masks, long n, long draft_tokens, long splits, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int keys_per_split, int head_dim, float qks,
    void* stream) {
  if (!mx_verify_sizes_ok(n, draft_tokens, splits, kv_heads, group)) return 1;
  if (n > 0 && (!q4 || !qscale || !k4 || !kscale || !vt || !vscale || !opart || !ml || !tree_masks)) return 1;
  const long nrb = (group * draft_tokens + MxCfg<128>::QROWS - 1) / MxCfg<128>::QROWS;
  if (n > 0x7fffffffL / (nrb * splits * kv_heads)) return 1;
  MxSplitCall c;
  const int rc = mx_varlen_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work,
                                n, n * nrb * splits, n * draft_tokens,
                                n * splits * kv_heads * group * draft_tokens, max_seqs, kv_heads, group, num_pages,
                                page_tokens, max_pages_per_seq, 2, keys_per_split, head_dim, qks, 0, 0, tree_masks);
  if (rc >= 0) return rc;
  return mx_split_launch<true, true, true, true, false, false, true, true>(c, stream);
}

extern "C" int qattn_mxfp4_verify_step_combine(const void* opart, const void* ml, void* out, void* lse,
                                               const void* seq_rec, long n, long draft_tokens, long splits,
                                               long q_heads, long kv_heads, int head_dim, void* stream) {
  if (head_dim != 128 || kv_heads < 1 || q_heads < 1 || q_heads % kv_heads != 0) return 1;
  if (!mx_verify_sizes_ok(n, draft_tokens, splits, kv_heads, q_heads / kv_heads)) return 1;
  if (n == 0) return 0;
  if (!opart || !ml || !out || !lse || !seq_rec) return 1;
  const long rows = n * draft_tokens * q_heads, nthr = rows * (128 / 8);
  if ((nthr + 255) / 256 > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(mxfp4_verify_step_combine_kernel<128>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)opart, (const float2*)ml, (_Float16*)out, (float*)lse,
                     (const int*)seq_rec, rows, (int)q_heads, (int)(q_heads / kv_heads), (int)draft_tokens,
                     (int)splits);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// the packed append, the two packed quantisers and the two merges at head_dim 128
namespace qattn {
QA_MX_WIDTH(, 128)
}
