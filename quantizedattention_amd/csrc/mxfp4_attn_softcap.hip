// Logit soft-capping on the paged MX-FP4 cache (Gemma-2, Grok-1): the packed step and the decode step with the
// logit of a visible key cap * tanh(scale * s / cap) in place of scale * s, s = deq(q) . deq(k) the fp32 MFMA
// result.  Everything but the tile body is the uncapped call's: plan, tiles, splits, masks, skipped tiles,
// partials and merge (so `lse` is over the capped logits, and of the sink logit when the merge is given one).
//
// The tile body is mx_tile SOFTCAP (mxfp4_attn.h).  Per score it costs a multiply, an exp2, an add, a reciprocal
// and an fma in front of the fma and exp2 of the uncapped body: t = 1 - 2 / (1 + 2^(s c1)), P = 2^(C t - m) with
// c1 = 2 log2(e) scale / cap and C = cap log2(e), the two constants the entries below derive once on the host.  The
// row max needs one more tanh per lane and tile (tanh is monotonic), the masks none.  m stays the integer running
// max: mx_tile says why a fixed m = ceil(C) would not do.
//
// This file holds the head_dim 128 instantiations of mxfp4_attn_split_kernel (VARLEN + PAGED non-causal, causal
// and WINDOW, and the STEP form of the two causal ones) and the two C entries; head_dim 64 and 256 are the
// SOFTCAP instantiations of mxfp4_attn_packed_kernel in the files of those widths (mx_packed_wide).  The kernels
// stand in a file of their own because they are compiled without packed fp32 arithmetic, as those two files are: the 32 scores of a lane invite the
// vectoriser to pair the multiplies and fmas of the tanh, and mxfp4_attn.hip keeps the flags it was measured with.
#include "mxfp4_attn.h"

#include <cmath>

using namespace qattn;

// c1 and C of mx_tile SOFTCAP from qks = scale * log2(e) and the cap (natural-log units), each rounded once from
// the double; false unless both are finite and > 0
static bool mx_softcap_consts(float qks, float softcap, float& c1, float& capc) {
  if (!(qks > 0.f) || !(softcap > 0.f) || !std::isfinite(qks) || !std::isfinite(softcap)) return false;
  c1 = (float)(2.0 * (double)qks / (double)softcap);
  capc = (float)((double)softcap * 1.4426950408889634);
  return std::isfinite(c1) && c1 > 0.f && std::isfinite(capc);
}

// the packed step with a cap: qattn_mxfp4_attn_fwd_varlen_paged for window == 0 (then sinks == 0; causal 0 or 2)
// and qattn_mxfp4_attn_fwd_varlen_paged_window for window >= 1 (causal 2), with their arguments and limits.  The
// merge is qattn_mxfp4_varlen_combine or qattn_mxfp4_varlen_combine_sink.
extern "C" int qattn_mxfp4_attn_fwd_varlen_paged_softcap(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work,
    long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads, long group,
    long num_pages, long page_tokens, long max_pages_per_seq, int causal, int keys_per_split, int head_dim,
    float qks, long window, long sinks, float softcap, void* stream) {
  float c1, capc;
  if (!mx_softcap_consts(qks, softcap, c1, capc) || !mx_step_window_ok(window, sinks)) return 1;
  if (window >= 1 && causal != 2) return 1;
  MxSplitCall c;
  const int rc = mx_packed_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec,
                                work, nseq, nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages,
                                page_tokens, max_pages_per_seq, causal, keys_per_split, head_dim, qks, window,
                                sinks, nullptr, c1, capc);
  if (rc >= 0) return rc;
  if (head_dim != 128) return mx_packed_wide<false, true>(c, head_dim, causal, window, stream);
  if (window >= 1) return mx_split_launch<true, true, true, true, true, false, false, false, true>(c, stream);
  return causal ? mx_split_launch<true, true, true, true, false, false, false, false, true>(c, stream)
                : mx_split_launch<false, true, true, true, false, false, false, false, true>(c, stream);
}

// the decode step's attention with a cap: qattn_mxfp4_attn_fwd_decode_step with its arguments and limits, over the
// STEP instantiations of the capped kernels.  Plan and merge are the step's own.
extern "C" int qattn_mxfp4_attn_fwd_decode_step_softcap(
    const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt, const void* vscale,
    void* opart, void* ml, const void* lens, const void* block_table, const void* seq_rec, const void* work, long n,
    long splits, long max_seqs, long kv_heads, long group, long num_pages, long page_tokens,
    long max_pages_per_seq, int keys_per_split, int head_dim, float qks, long window, long sinks, float softcap,
    void* stream) {
  float c1, capc;
  if (!mx_softcap_consts(qks, softcap, c1, capc)) return 1;
  if (n < 0 || splits < 1 || splits > 65535 || kv_heads < 1 || group < 1 || !mx_step_window_ok(window, sinks))
    return 1;
  if (kv_heads > 0x7fffffffL / group || n > 0x7fffffffL / (splits * kv_heads * group)) return 1;
  if (n > 0 && (!q4 || !qscale || !k4 || !kscale || !vt || !vscale || !opart || !ml)) return 1;
  MxSplitCall c;
  const int rc = mx_packed_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work,
                                n, n * splits, n, n * splits * kv_heads * group, max_seqs, kv_heads, group,
                                num_pages, page_tokens, max_pages_per_seq, 2, keys_per_split, head_dim, qks, window,
                                sinks, nullptr, c1, capc);
  if (rc >= 0) return rc;
  if (head_dim != 128) return mx_packed_wide<true, true>(c, head_dim, 2, window, stream);
  return window < 1 ? mx_split_launch<true, true, true, true, false, false, false, true, true>(c, stream)
                    : mx_split_launch<true, true, true, true, true, false, false, true, true>(c, stream);
}
