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
// its own argument checks, the call filled in, a dispatch on `causal`), mx_varlen_call (the checks and the
// call of the three packed entries without groups), mx_varlen_paged (the plain and the windowed one),
// mx_append (the padded and the paged append) and mx_append_packed (the packed append with and without rotary
// positions; mx_rope_block, the rotation both rope kernels put in front of the one quantiser body, is
// restated by tests/mxfp4_rope_ref.py and held bit for bit by tests/test_gpu_mxfp4_rope.py).  The two rings, MxRing and MxPagedRing, keep a piece plan each: holding one in common changed the paged kernels' instruction streams.  The C entries
// stand in the order in which they first use their kernels, which is the order the kernels are emitted
// in; tools/asm_compare.py compares branch labels too, and those carry the function's number.
#include "common.h"

#include <type_traits>

namespace qattn {

typedef int v8i_t __attribute__((ext_vector_type(8)));

QA_DEVICE unsigned e8m0_of(float amax) {
  // floor(log2 amax) - 2 as a biased e8m0 byte (inputs are fp16, so amax is a normal fp32 or 0)
  if (!(amax > 0.f)) return 0u;
  const int e = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - 2;
  return (unsigned)min(max(e + 127, 0), 254);
}
QA_DEVICE float e8m0_value(unsigned b) {
  return b == 0 ? 5.877471754111438e-39f : __uint_as_float(b << 23);   // 2^-127 is a denormal
}

// Pack 32 floats into 4 dwords of e2m1 (element j at nibble j, low nibble first) with scale s.
QA_DEVICE v4i pack_fp4x32(const float* x, float s) {
  v4i w;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    unsigned u = 0;
    u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, x[8 * d + 0], x[8 * d + 1], s, 0);
    u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, x[8 * d + 2], x[8 * d + 3], s, 1);
    u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, x[8 * d + 4], x[8 * d + 5], s, 2);
    u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, x[8 * d + 6], x[8 * d + 7], s, 3);
    w[d] = (int)u;
  }
  return w;
}

// ------------------------------------------------------------------------------ quantisers
// One 32-element block of a Q / K row: src (and mu, the block of the mean, or null) -> 16 B of codes
// and the scale byte.  With mu the block is first f16(x - mu).
QA_DEVICE void mx_quant_row_block(const v8h* src, const v8h* mu, v4i* q4, uint8_t* sc) {
  float f[32];
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    v8h v = src[c];
    if (mu) {
      const v8h w = mu[c];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (_Float16)((float)v[j] - (float)w[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[8 * c + j] = (float)v[j];
      amax = fmaxf(amax, fabsf(f[8 * c + j]));
    }
  }
  const unsigned e = e8m0_of(amax);
  *q4 = pack_fp4x32(f, e8m0_value(e));
  *sc = (uint8_t)e;
}

// Q / K: one thread per 32-element block of a row.  x f16 [rows, D] -> q4 [rows, D/2], sc [rows, D/32].
// With ``mean`` (f16 [rows/seq, D], SageAttention smoothing) the row is first f16(x - mean[row/seq]).
template <int D>
__global__ __launch_bounds__(256) void mx_quant_rows_kernel(const _Float16* __restrict__ x,
                                                            const _Float16* __restrict__ mean,
                                                            uint8_t* __restrict__ q4,
                                                            uint8_t* __restrict__ sc, long nblk, long seq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nblk) return;
  constexpr int NB = D / 32;
  const v8h* mu = mean ? reinterpret_cast<const v8h*>(mean + (i / NB / seq) * D + (i % NB) * 32) : nullptr;
  mx_quant_row_block(reinterpret_cast<const v8h*>(x + i * 32), mu, reinterpret_cast<v4i*>(q4) + i, sc + i);
}

// V: one thread per (head, 64-key tile g, column d, half h).  v f16 [BH*Sk, D] ->
// vt [BH][Sk/64][D][32 B] (operand order, see the header) and vs [BH][Sk/64][D][2].
template <int D>
__global__ __launch_bounds__(256) void mx_quant_vt_kernel(const _Float16* __restrict__ v,
                                                          uint8_t* __restrict__ vt,
                                                          uint8_t* __restrict__ vs, long nthr, int Sk) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nthr) return;
  const int h = (int)(i & 1);
  const int d = (int)((i >> 1) % D);
  const long gt = (i >> 1) / D;                 // head * (Sk/64) + g
  const int ng = Sk / 64;
  const long bh = gt / ng;
  const int g = (int)(gt % ng);
  const _Float16* col = v + ((long)bh * Sk + 64L * g) * D + d;
  float f[32];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int key = 32 * (j >> 4) + 8 * ((j >> 2) & 3) + 4 * h + (j & 3);
    f[j] = (float)col[(long)key * D];
    amax = fmaxf(amax, fabsf(f[j]));
  }
  const unsigned e = e8m0_of(amax);
  reinterpret_cast<v4i*>(vt)[i] = pack_fp4x32(f, e8m0_value(e));
  vs[i] = (uint8_t)e;
}

// ------------------------------------------------------------------------------ cache append
// The preallocated cache (kv_cache_mxfp4.py PreallocatedKVFP4): k4 / ks / vt / vs in the layouts above
// with cap tokens per key/value head, len[b] of them valid for every head of sequence b, and vtail
// f16 [B*Hkv][64][D], the fp16 V rows of the sequence's last partial tile at slot token % 64.
// Invariant: rows [0, L) of k4 / ks and tiles [0, ceil(L / 64)) of vt / vs are, bit for bit, the
// quantisers' output for the sequence zero-padded to a multiple of 64; the rest is unspecified.
// An append of n new tokens (sequence b takes the first cnt = counts[b] <= n, null counts: n) is
// three launches in stream order: V (reads vtail), then K and vtail, then the lengths.

// The tokens sequence b takes of an append, with its length L before it: 0 (nothing is written) for a
// count outside [0, n] or a length that would pass cap, which the host refuses before it launches.
QA_DEVICE int mx_append_count(const int* lens, const int* counts, int b, int n, int cap, int& L) {
  L = lens[b];
  const int cnt = counts ? counts[b] : n;
  return cnt > 0 && cnt <= n && L >= 0 && L <= cap - cnt ? cnt : 0;
}

// ---- paged pool (kv_cache_mxfp4.py PagedKVFP4)
// The same four operands cut into pages of P = 64 << lgt tokens that hold every head of ONE sequence:
// k4 [npool][Hkv][P][D/2], ks [npool][Hkv][P][D/32], vt [npool][Hkv][P/64][D][32 B], vs [npool][Hkv][P/64]
// [D][2].  btab i32 [B][mpp] names the pages of sequence b in order, so logical tile g of head hd is
// physical tile (btab[b][g >> lgt] * Hkv + hd) << lgt | (g & (P/64 - 1)) of all four operands.  An
// entry is read only below ceil(L / P) (appends: of the length after the append) and is clamped to
// [0, npool): a wrong table gives a wrong answer, never an address outside the pool.  Tile indices are
// 64-bit products here; the C entries hold npool * Hkv * P/64 below 2^31.
QA_DEVICE long mx_paged_tile(const int* btab, int b, int hd, int g, int Hkv, int mpp, int lgt, int npool) {
  const int page = min(max(btab[(long)b * mpp + (g >> lgt)], 0), npool - 1);
  return (((long)page * Hkv + hd) << lgt) + (g & ((1 << lgt) - 1));
}

// A touched V tile g of a column, quantised again from its 32 keys per block in mx_quant_vt_kernel's
// order: token t < L from tail[t % 64] (tail, col: the column's element of vtail's row 0 and of the
// first new token; rstride: rows of D elements between two new tokens), t < L + cnt from col[t - L], else 0.
template <int D>
QA_DEVICE void mx_requant_v_block(const _Float16* tail, const _Float16* col, int rstride, int g, int L,
                                  int cnt, int h, v4i* q4, uint8_t* sc) {
  float f[32];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int key = 32 * (j >> 4) + 8 * ((j >> 2) & 3) + 4 * h + (j & 3);
    const int t = 64 * g + key;
    f[j] = t < L ? (float)tail[(long)key * D] : t < L + cnt ? (float)col[(long)(t - L) * rstride * D] : 0.f;
    amax = fmaxf(amax, fabsf(f[j]));
  }
  const unsigned e = e8m0_of(amax);
  *q4 = pack_fp4x32(f, e8m0_value(e));
  *sc = (uint8_t)e;
}

// One 32-element block of a new K row at token t: quantised as mx_quant_rows_kernel does (mu: the block of
// the mean, or null) into block o of k4 / ks; the same 32 elements of v go to vdst, their place in vtail,
// when the token lies in the new last partial tile (end = L + cnt, the length after the append).
QA_DEVICE void mx_append_k_block(const _Float16* ksrc, const _Float16* vsrc, const v8h* mu, uint8_t* k4,
                                 uint8_t* ks, long o, _Float16* vdst, int t, int end) {
  mx_quant_row_block(reinterpret_cast<const v8h*>(ksrc), mu, reinterpret_cast<v4i*>(k4) + o, ks + o);
  if (end % 64 != 0 && t / 64 == end / 64) {
    const v8h* src = reinterpret_cast<const v8h*>(vsrc);
    v8h* dst = reinterpret_cast<v8h*>(vdst);
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[c] = src[c];
  }
}

// V: one thread per (head, touched tile j, column d, half h) quantises tile g = L / 64 + j of the touched
// range [L / 64, (L + cnt - 1) / 64] again (mx_requant_v_block).  PAGED: cap = mpp * P and the tile is
// written where the block table puts it.
template <int D, bool PAGED = false>
__global__ __launch_bounds__(256) void mx_append_vt_kernel(const _Float16* __restrict__ v,
                                                           const _Float16* __restrict__ vtail,
                                                           uint8_t* __restrict__ vt, uint8_t* __restrict__ vs,
                                                           const int* __restrict__ lens,
                                                           const int* __restrict__ counts, long nthr,
                                                           int Hkv, int n, int ntile, int cap,
                                                           const int* __restrict__ btab, int mpp, int lgt,
                                                           int npool) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nthr) return;
  const int h = (int)(i & 1);
  const int d = (int)((i >> 1) % D);
  const long gt = (i >> 1) / D;                 // head * ntile + j
  const long bh = gt / ntile;
  const int b = (int)(bh / Hkv);
  int L;
  const int cnt = mx_append_count(lens, counts, b, n, cap, L);
  const int g = L / 64 + (int)(gt % ntile);
  if (cnt == 0 || 64 * g >= L + cnt) return;   // L + cnt <= cap = 64 * tiles: the tile lies inside
  long tile = bh * (cap / 64) + g;
  if constexpr (PAGED) tile = mx_paged_tile(btab, b, (int)(bh % Hkv), g, Hkv, mpp, lgt, npool);
  const long o = (tile * D + d) * 2 + h;
  mx_requant_v_block<D>(vtail + bh * 64 * D + d, v + bh * (long)n * D + d, 1, g, L, cnt, h,
                        reinterpret_cast<v4i*>(vt) + o, vs + o);
}

// K and vtail: one thread per 32-element block of a new row.  Row i < cnt of head bh goes to token
// L + i (mx_append_k_block; mean: f16 [B*Hkv, D] or null).  PAGED as above.
template <int D, bool PAGED = false>
__global__ __launch_bounds__(256) void mx_append_k_kernel(const _Float16* __restrict__ k,
                                                          const _Float16* __restrict__ v,
                                                          const _Float16* __restrict__ mean,
                                                          uint8_t* __restrict__ k4, uint8_t* __restrict__ ks,
                                                          _Float16* __restrict__ vtail,
                                                          const int* __restrict__ lens,
                                                          const int* __restrict__ counts, long nblk,
                                                          int Hkv, int n, int cap,
                                                          const int* __restrict__ btab, int mpp, int lgt,
                                                          int npool) {
  constexpr int NB = D / 32;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nblk) return;
  const int blk = (int)(i % NB);
  const int tok = (int)(i / NB % n);
  const long bh = i / NB / n;
  const int b = (int)(bh / Hkv);
  int L;
  const int cnt = mx_append_count(lens, counts, b, n, cap, L);
  const int t = L + tok;
  if (tok >= cnt) return;   // t < L + cnt <= cap
  const v8h* mu = mean ? reinterpret_cast<const v8h*>(mean + bh * D + blk * 32) : nullptr;
  long row = bh * cap + t;
  if constexpr (PAGED)
    row = mx_paged_tile(btab, b, (int)(bh % Hkv), t / 64, Hkv, mpp, lgt, npool) * 64 + t % 64;
  mx_append_k_block(k + i * 32, v + i * 32, mu, k4, ks, row * NB + blk,
                    vtail + (bh * 64 + t % 64) * D + blk * 32, t, L + cnt);
}

// lens[b] += cnt, one thread per sequence
__global__ __launch_bounds__(256) void mx_append_len_kernel(int* __restrict__ lens,
                                                            const int* __restrict__ counts, int B, int n,
                                                            int cap) {
  const int b = (int)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int L;
  const int cnt = mx_append_count(lens, counts, b, n, cap, L);
  if (cnt) lens[b] = L + cnt;
}

// ------------------------------------------------------------------------------ attention
template <int D>
struct MxCfg {
  static constexpr int WAVES = 4;
  static constexpr int QROWS = 32 * WAVES;
  static constexpr int KT = 64;                       // keys per tile / ring slot
  static constexpr int NSLOT = 4;
  static constexpr int KROWB = D / 2;                 // fp4 bytes per key row
  static constexpr int K_BYTES = KT * KROWB;          // 4 KiB at D = 128
  static constexpr int V_BYTES = D * 32;              // [D][32 B]
  static constexpr int KS_BYTES = KT * (D / 32);      // key scales of the tile
  static constexpr int VS_BYTES = D * 2;
  static constexpr int KOFF = 0, VOFF = K_BYTES, KSOFF = K_BYTES + V_BYTES, VSOFF = KSOFF + 256;
  static constexpr int SLOT = VSOFF + 256;
  static constexpr int P16 = (K_BYTES + V_BYTES) / 1024;   // 1-KiB pieces
  static constexpr int IPW16 = P16 / WAVES;
  static constexpr int IPW = IPW16 + 2;               // + the two 256-B scale blocks
  static constexpr int NKS = D / 64;                  // 32x32x64 k-steps of S
  static constexpr int NDB = D / 32;
  static constexpr float MSLACK = 8.f;                // P <= 2^MSLACK between max raises
  static_assert(KS_BYTES <= 256 && VS_BYTES <= 256 && P16 % WAVES == 0, "tile layout");
};

#ifndef QA_MX_OCC
#define QA_MX_OCC 2   // min waves per SIMD the register budget is sized for
#endif
#ifndef QA_MX_OCC_CAUSAL
#define QA_MX_OCC_CAUSAL QA_MX_OCC   // the same budget for the causal instantiation
#endif

// ---- what the one-pass and the key-split kernel share: the ring plan, the Q load and the tile body
// LDS-DMA plan of one wave: pieces 0..P16-1 of (K | V^T) and one dma4 each for the two scale blocks.
// The bases point at tile 0 of the ring; the buffer resources cover `tiles` tiles from there.
template <int D>
struct MxRing {
  using C = MxCfg<D>;
  unsigned voff[C::IPW16], loff[C::IPW16], stride[C::IPW16];
  v4u rs[C::IPW16], ks_rs, vs_rs;
  unsigned smem_lds;
  int lane;
  QA_DEVICE MxRing(const void* kbase, const void* ksbase, const void* vbase, const void* vsbase, int tiles,
                   const char* smem, int wave, int lane_)
      : lane(lane_) {
#pragma unroll
    for (int i = 0; i < C::IPW16; ++i) {
      const int p = wave + C::WAVES * i;
      const bool isv = p >= C::K_BYTES / 1024;
      const int piece = isv ? p - C::K_BYTES / 1024 : p;
      voff[i] = piece * 1024 + 16 * lane;
      loff[i] = (isv ? C::VOFF : C::KOFF) + piece * 1024;
      stride[i] = isv ? C::V_BYTES : C::K_BYTES;
      rs[i] = make_rsrc(isv ? vbase : kbase, (unsigned)(tiles * (isv ? C::V_BYTES : C::K_BYTES)));
    }
    ks_rs = make_rsrc(ksbase, (unsigned)(tiles * C::KS_BYTES));
    vs_rs = make_rsrc(vsbase, (unsigned)(tiles * C::VS_BYTES));
    smem_lds = lds_addr(smem);
  }
  // tile min(t, ntw - 1) into slot t & 3 (past the last tile the wave keeps its DMA count)
  QA_DEVICE void issue(int t, int ntw) const {
    const unsigned slot = smem_lds + (t & 3) * C::SLOT;
    t = min(t, ntw - 1);
#pragma unroll
    for (int i = 0; i < C::IPW16; ++i) dma16_buf(rs[i], voff[i], (unsigned)t * stride[i], slot + loff[i]);
    dma4_buf(ks_rs, 4 * lane, (unsigned)t * C::KS_BYTES, slot + C::KSOFF);
    dma4_buf(vs_rs, 4 * lane, (unsigned)t * C::VS_BYTES, slot + C::VSOFF);
  }
  QA_DEVICE void prologue(int ntw) const {
#pragma unroll
    for (int i = 0; i < C::NSLOT - 1; ++i) issue(i, ntw);
  }
};

// The same plan over the paged pool ("paged pool" above): the wave's tiles are t0 .. of head hd of the
// sequence whose table row is tbl, npages = ceil(L / P) entries of which may be read.  When the ring
// enters a page it rebases its four buffer resources: base = operand + (64-bit) first tile of the
// head's part of that page * bytes, bounds that part alone, so an operand may pass 4 GiB and no byte of
// another page or head can be fetched; inside the page the tile is the 32-bit soffset, as in MxRing.
// Tile indices are 32-bit (the C entry holds the pool below 2^31 tiles), byte offsets 64-bit.  The
// table is read through the constant address space (wave-uniform: scalar loads, which the ring's vmcnt
// counts do not see) and one page ahead: while the ring is in page i it holds the entry of page
// min(i + 1, npages - 1), loaded a tile before the rebase that needs it.  All of this is scalar ALU
// work on every wave's own instruction stream (tools/time_decode_paged.py measures what it costs).
template <int D>
struct MxPagedRing {
  using C = MxCfg<D>;
  typedef const __attribute__((address_space(4))) int* table_ptr;
  unsigned voff[C::IPW16], loff[C::IPW16], bytes[C::IPW16];
  const uint8_t* base[C::IPW16];
  const uint8_t *ksbase, *vsbase;
  v4u rs[C::IPW16], ks_rs, vs_rs;   // of the page the ring is in
  table_ptr tbl;
  int npages, lgt, hkv, hd, npool, t0;
  int cur, next;   // the page index the ring is in and the table entry after it
  unsigned smem_lds;
  int lane;
  QA_DEVICE void rebase(int id) {
    const unsigned long first = ((unsigned)min(max(id, 0), npool - 1) * (unsigned)hkv + hd) << lgt;
#pragma unroll
    for (int i = 0; i < C::IPW16; ++i) rs[i] = make_rsrc(base[i] + first * bytes[i], bytes[i] << lgt);
    ks_rs = make_rsrc(ksbase + first * C::KS_BYTES, (unsigned)C::KS_BYTES << lgt);
    vs_rs = make_rsrc(vsbase + first * C::VS_BYTES, (unsigned)C::VS_BYTES << lgt);
  }
  QA_DEVICE MxPagedRing(const uint8_t* k4, const uint8_t* ks, const uint8_t* vt, const uint8_t* vs,
                        const int* row, int npages_, int lgt_, int hkv_, int hd_, int npool_, int t0_,
                        const char* smem, int wave, int lane_)
      : ksbase(ks), vsbase(vs), tbl((table_ptr)(unsigned long)row), npages(npages_), lgt(lgt_), hkv(hkv_),
        hd(hd_), npool(npool_), t0(t0_), lane(lane_) {
#pragma unroll
    for (int i = 0; i < C::IPW16; ++i) {
      const int p = wave + C::WAVES * i;
      const bool isv = p >= C::K_BYTES / 1024;
      const int piece = isv ? p - C::K_BYTES / 1024 : p;
      voff[i] = piece * 1024 + 16 * lane;
      loff[i] = (isv ? C::VOFF : C::KOFF) + piece * 1024;
      bytes[i] = isv ? C::V_BYTES : C::K_BYTES;
      base[i] = isv ? vt : k4;
    }
    cur = t0 >> lgt;
    rebase(tbl[cur]);
    next = tbl[min(cur + 1, npages - 1)];
    smem_lds = lds_addr(smem);
  }
  // tile min(t, ntw - 1) of the wave into slot t & 3, from the page the ring is in; then the ring moves
  // to the page of the FOLLOWING issue, so that the rebase stands behind the DMA, where the scheduler
  // can sink it into the tile's matrix work, not between the barrier and the DMA
  QA_DEVICE void issue(int t, int ntw) {
    const unsigned slot = smem_lds + (t & 3) * C::SLOT;
    const unsigned in = (t0 + min(t, ntw - 1)) & ((1 << lgt) - 1);
#pragma unroll
    for (int i = 0; i < C::IPW16; ++i) dma16_buf(rs[i], voff[i], in * bytes[i], slot + loff[i]);
    dma4_buf(ks_rs, 4 * lane, in * C::KS_BYTES, slot + C::KSOFF);
    dma4_buf(vs_rs, 4 * lane, in * C::VS_BYTES, slot + C::VSOFF);
    const int g = t0 + min(t + 1, ntw - 1);
    if ((g >> lgt) != cur) {   // tiles advance one at a time: the page after cur
      cur = g >> lgt;
      rebase(next);
    }
    // every tile, without a branch: the loaded word is then the loop-carried register itself, and the
    // first instruction to wait for it is in the next issue (a load under `if` is copied, and waited
    // for, at once)
    next = tbl[min(cur + 1, npages - 1)];
  }
  QA_DEVICE void prologue(int ntw) {
#pragma unroll
    for (int i = 0; i < C::NSLOT - 1; ++i) issue(i, ntw);
  }
};

// what the split kernel declares in place of the ring it does not use
struct MxNoRing {
  template <class... A>
  QA_DEVICE MxNoRing(A...) {}
};

// Query fragments of row r (B operand of S^T): the lane holds Q[r][64s + 32h .. +32] and the row's
// D / 32 scale bytes packed into one word, which is returned.
template <int D>
QA_DEVICE unsigned mx_load_q(const uint8_t* q4, const uint8_t* qs, long r, int h, v4i (&qf)[MxCfg<D>::NKS]) {
  using C = MxCfg<D>;
#pragma unroll
  for (int s = 0; s < C::NKS; ++s) qf[s] = *reinterpret_cast<const v4i*>(q4 + r * C::KROWB + 32 * s + 16 * h);
  unsigned qsw = 0;   // byte b = the scale of block b, in one (unaligned) load
  __builtin_memcpy(&qsw, qs + r * (D / 32), D / 32);
  return qsw;
}

// One 64-key tile, landed in ring slot sl, into the running state (o, m, l) of the lane's query row.
// CAUSAL and diag (wave-uniform): the tile crosses the diagonal and the lane sees element r of half u
// iff 32u + 8(r>>2) + (r&3) <= lim; otherwise every key of the tile is visible.
// WINDOW (with CAUSAL; a sliding window with sinks): the mask has a lower edge too, element e is
// visible iff e <= lim && (e >= lo || e <= slim), lo the first element of the lane's window and slim
// the last sink element, both relative to the tile and the lane half as lim is.  The three limits are
// all a lane carries; every compare is against a constant e and feeds its select at once.
// TREE (with CAUSAL; the tree-masked verify step): the mask is a set, not an edge.  The lane brings the
// tile's visibility word, bit e of (vis1:vis0) set iff it sees element e (the word is shifted down by 4h
// already, so e is the constant of the other paths); every test is of a constant bit of one of the two
// registers and feeds its select at once.
template <int D, bool CAUSAL, bool WINDOW = false, bool TREE = false>
QA_DEVICE void mx_tile(const char* sl, const v4i (&qf)[MxCfg<D>::NKS], unsigned qsw,
                       v16f (&o)[MxCfg<D>::NDB], float& m, float& l, bool diag, int lim, float qks, int lane,
                       int h, int c32, int lo = 0, int slim = 0, unsigned vis0 = 0, unsigned vis1 = 0) {
  static_assert(CAUSAL || !WINDOW, "a window is causal");
  static_assert(!TREE || (CAUSAL && !WINDOW), "a tree mask is causal, without a window");
  // WINDOW, TREE: element e of the lane is visible
  const auto seen = [&](int e) {
    if constexpr (TREE) return (((e < 32 ? vis0 : vis1) >> (e & 31)) & 1u) != 0;
    else return e <= lim && (e >= lo || e <= slim);
  };
  using C = MxCfg<D>;
  // S^T for the two 32-key halves u: A = K rows 32u + c32, k = 64s + 32h .. +32
  v16f acc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    acc[u] = v16f{};
    const int key = 32 * u + c32;
    const unsigned ksw = *reinterpret_cast<const unsigned*>(sl + C::KSOFF + key * (D / 32));
#pragma unroll
    for (int s = 0; s < C::NKS; ++s) {
      const v4i ka = *reinterpret_cast<const v4i*>(sl + C::KOFF + key * C::KROWB + 32 * s + 16 * h);
      const v8i_t a = {ka[0], ka[1], ka[2], ka[3], 0, 0, 0, 0};
      const v8i_t b = {qf[s][0], qf[s][1], qf[s][2], qf[s][3], 0, 0, 0, 0};
      const int sa = (int)((ksw >> (8 * (2 * s + h))) & 0xff);
      const int sb = (int)((qsw >> (8 * (2 * s + h))) & 0xff);
      acc[u] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[u], 4, 4, 0, sa, 0, sb);
    }
  }
  // online softmax over the tile (fp32); the lane holds 32 keys of its query row.  m is an
  // integer (log2 units) raised only when the row max exceeds it by more than MSLACK, so every
  // rescale is an exact power of two and, between raises, P <= 2^MSLACK needs no rescale at all.
  float amx;
  if ((WINDOW || TREE) && diag) {
    amx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        amx = seen(32 * u + 8 * (r >> 2) + (r & 3)) ? fmaxf(amx, acc[u][r]) : amx;
  } else if (CAUSAL && diag) {
    amx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        amx = 32 * u + 8 * (r >> 2) + (r & 3) <= lim ? fmaxf(amx, acc[u][r]) : amx;
  } else {
    amx = acc[0][0];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = (u == 0 ? 1 : 0); r < 16; ++r) amx = fmaxf(amx, acc[u][r]);
  }
  const float lmx = amx * qks;                                  // this lane's max of S * qks
  const float mx = fmaxf(lmx, xor32_swap(lmx, lane));
  if (__ballot(mx > m + C::MSLACK)) {
    const float nm = mx > m + C::MSLACK ? ceilf(mx) : m;
    const float rsc = m == -INFINITY ? 0.f : __builtin_ldexpf(1.f, (int)(m - nm));
    m = nm;
    l *= rsc;
#pragma unroll
    for (int b = 0; b < C::NDB; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[b][i] = o[b][i] * rsc;
  }
  const float nm = -m;
  float x[32];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) x[16 * u + r] = exp2_f32(__builtin_fmaf(acc[u][r], qks, nm));
  if ((WINDOW || TREE) && diag) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        x[16 * u + r] = seen(32 * u + 8 * (r >> 2) + (r & 3)) ? x[16 * u + r] : 0.f;
  } else if (CAUSAL && diag) {   // masked P is exactly 0 (a select: exp2 of a masked score may be inf)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        x[16 * u + r] = 32 * u + 8 * (r >> 2) + (r & 3) <= lim ? x[16 * u + r] : 0.f;
  }
  // the block max is exp2 of the lane's max argument (exp2 and the fma are monotonic); with every
  // key of the lane masked amx = -inf and pmax = 0.  In a row still at m = -inf (a key split none of
  // whose keys the row sees) the argument is then -inf + inf = NaN, which e8m0_of maps to scale byte
  // 0 like pmax = 0 (its P is all zero)
  const float pmax = exp2_f32(__builtin_fmaf(amx, qks, nm));
  // P block of this lane half: its 32 values, nibble j = 16u + r
  const unsigned pe = e8m0_of(pmax);
  const v4i pk = pack_fp4x32(x, e8m0_value(pe));
  const v8i_t pb = {pk[0], pk[1], pk[2], pk[3], 0, 0, 0, 0};
  // row sum of the quantised P on the matrix core: every row of ONES . P^T is the column sum
  {
    const v8i_t ones = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};   // e2m1 1.0
    const v16f ts = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ones, pb, v16f{}, 4, 4, 0, 127, 0,
                                                                    (int)pe);
    l += ts[0];
  }
  // O^T[d][q] += V^T[d][keys] P^T[keys][q], A = V^T rows d = 32b + c32, k = the half-h key set
#pragma unroll
  for (int b = 0; b < C::NDB; ++b) {
    const int d = 32 * b + c32;
    const v4i va = *reinterpret_cast<const v4i*>(sl + C::VOFF + d * 32 + 16 * h);
    const v8i_t a = {va[0], va[1], va[2], va[3], 0, 0, 0, 0};
    const int sa = (int)*reinterpret_cast<const uint8_t*>(sl + C::VSOFF + 2 * d + h);
    o[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, o[b], 4, 4, 0, sa, 0, (int)pe);
  }
}

template <int D, bool CAUSAL>
__global__ __launch_bounds__(256, CAUSAL ? QA_MX_OCC_CAUSAL : QA_MX_OCC) void mxfp4_attn_fwd_kernel(
    const uint8_t* __restrict__ q4, const uint8_t* __restrict__ qs, const uint8_t* __restrict__ k4,
    const uint8_t* __restrict__ ks, const uint8_t* __restrict__ vt, const uint8_t* __restrict__ vs,
    _Float16* __restrict__ out, float* __restrict__ lse, int BH, int Sq, int Sk, int G, float qks,
    int qoff) {
  using C = MxCfg<D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nq = (Sq + C::QROWS - 1) / C::QROWS;
  int bh, qt;
  if constexpr (CAUSAL) xcd_remap_lpt(blockIdx.x, nq, BH, true, bh, qt);   // longest workgroups first
  else xcd_remap(blockIdx.x, nq, BH, bh, qt);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, h = lane >> 5, c32 = lane & 31;
  const int q0 = qt * C::QROWS + wave * 32;
  const bool active = q0 < Sq;
  const int qi = min(q0 + c32, Sq - 1);
  const long kvh = bh / G;
  const int nt = Sk / C::KT;
  // tiles this workgroup runs: up to the diagonal tile of its last real row (padding rows of a
  // partial workgroup do not extend it)
  int ntw = nt;
  if constexpr (CAUSAL) ntw = min(nt, (min(qt * C::QROWS + C::QROWS, Sq) - 1 + qoff) / C::KT + 1);
  const int wlast = q0 + 31 + qoff;   // last key any row of this wave sees

  const MxRing<D> ring(k4 + kvh * Sk * C::KROWB, ks + kvh * Sk * (D / 32), vt + kvh * (long)nt * C::V_BYTES,
                       vs + kvh * (long)nt * C::VS_BYTES, nt, smem, wave, lane);
  ring.prologue(ntw);

  v4i qf[C::NKS];
  const unsigned qsw = mx_load_q<D>(q4, qs, (long)bh * Sq + qi, h, qf);

  v16f o[C::NDB];
#pragma unroll
  for (int b = 0; b < C::NDB; ++b) o[b] = v16f{};
  float m = -INFINITY, l = 0.f;   // integer running max (log2 units), sum of the quantised P

  vmem_drain();
  __syncthreads();
  for (int t = 0; t < ntw; ++t) {
    ring_wait_barrier<2 * C::IPW>();   // tile t landed (t+1, t+2 may be in flight); slot (t+3)&3 is free
    ring.issue(t + 3, ntw);
    // causal: a wave past its own diagonal (or without rows) keeps its share of the DMA and the
    // barrier and skips the tile; `diag` (wave-uniform) marks the tiles that cross the diagonal
    bool diag = false;
    int lim = 0;
    if constexpr (CAUSAL) {
      if (!active || C::KT * t > wlast) continue;
      diag = C::KT * t + C::KT - 1 > q0 + qoff;
      lim = q0 + c32 + qoff - C::KT * t - 4 * h;
    }
    mx_tile<D, CAUSAL>(smem + (t & 3) * C::SLOT, qf, qsw, o, m, l, diag, lim, qks, lane, h, c32);
  }
  vmcnt_wait_all();
  __syncthreads();
  if (!active) return;
  const long row0 = (long)bh * Sq + q0;
  if (h == 0) lse[row0 + c32] = m + log2_f32(l);
  static_assert(C::WAVES * RowTile<D, _Float16>::BYTES <= C::NSLOT * C::SLOT, "staging fits the ring");
  store_rows<D, _Float16>(o, 1.0f / l, smem + wave * RowTile<D, _Float16>::BYTES, out + row0 * D, lane);
}

// ------------------------------------------------------------------------------ key-split forward
// The decoding layout of the forward above (kv_cache_mxfp4.py): the G query heads of a key/value
// head are consecutive [sq_head, D] blocks of q and run as ONE virtual head of rows = G * sq_head
// query rows against that key/value head, so a key/value tile is read once per group; and the keys
// are split over blockIdx.y, workgroup (x, y) running the tiles of keys [y * kps, min(Sk, y * kps +
// kps)) from m = -inf with a ring of its own.  Shared with the one-pass kernel: MxRing, mx_load_q and
// mx_tile; its own: the row mapping, the tile range, the causal prelude and the epilogue.  Written: the
// unnormalised state, opart f32 [nsplit][BHV * rows][D] = O_s and ml f32 x 2 [nsplit][BHV * rows] =
// {m_s, l_s}; mx_merge_row merges them.  Every m_s is an integer, so the merge's weights
// 2^(m_s - M) are exact and one split reproduces the one-pass result bit for bit.
// rows is any value >= 1: the lanes past the last row of a partial wave read a clamped row (as qi
// above) and store nothing.
// CAUSAL (bottom-right over the cache, qoff = Sk - sq_head): row r is query position r % sq_head and
// sees key j iff j <= r % sq_head + qoff.  A row that sees no key of a split keeps m = -inf, l = 0,
// O = 0: its scores never raise m, its P is selected to 0 before the quantisation (exp2 of a masked
// score is inf there) and the P block is scale byte 0 with zero codes; the merge gives it weight 0.
// LEN (the preallocated cache of kv_cache_mxfp4.py): Sk is the capacity, the stride of a key/value head,
// and sequence b = bh / hps holds L = lens[b] keys, 1 <= L <= Sk (causal: L >= sq_head; the host
// checks both).  The head has nt = ceil(L / 64) tiles; a split past them writes the empty state
// (-inf, 0, 0) and returns before any DMA or barrier; the ring's bounds end at the split's last tile
// of this sequence, so no byte of a tile >= nt is requested.  Row r sees key j iff j <= vis, vis =
// L - 1 non-causal and r % sq_head + L - sq_head causal: mx_tile's masked path, `diag` on the last
// tile when L % 64 != 0 and on the diagonal tiles.  K rows >= L of that tile may hold anything (their
// scores are selected away, NaN included); V tiles < nt are whole by the cache's invariant.
// PAGED (with LEN; the paged pool of kv_cache_mxfp4.py): the same tiles fetched through the block table
// btab i32 [B][mpp] by MxPagedRing, hps = Hkv heads per page, Sk = mpp * P (what a table row can hold).
// Only the ring differs: the prelude, the tile body and the epilogue are the LEN instantiation's.
// VARLEN (with PAGED; the packed step of kv_cache_mxfp4.py): a ragged batch in one launch.  The grid is
// one-dimensional, workgroup x = work record x / hps for key/value head x % hps; the record {j, 128-row
// block, split, 0} and sequence j's record {slot, first packed token, sq, splits, first partial row, ..}
// are read through the constant address space (wave-uniform: scalar loads).  From them: bh = slot * hps
// + head, sq_head = sq, rows = group * sq; len = lens[slot] as in LEN.  Two things differ from the PAGED
// instantiation: q is token-major, f16 [T][group * hps][D] quantised row by row, so virtual row r is
// packed row (first + r % sq) * (group * hps) + head * group + r / sq; and the partials are compact,
// row base = first partial row + (split * hps + head) * rows + q0 (opart f32 [part_rows][D], ml f32 x 2
// [part_rows]).  Slot, packed row and partial rows are clamped / bounded by the sizes in MxVarlen, so
// a wrong table gives a wrong answer, never an address outside q, the tables' slots or the partials.
// WINDOW (with VARLEN and CAUSAL; a sliding window of vl.window keys with vl.sinks sink keys): row r at
// position p = r % sq + len - sq sees key j iff j <= p and (j > p - window or j < sinks).  Three things
// differ from the VARLEN instantiation.  The mask has a lower edge (mx_tile WINDOW), `diag` being set
// when any row of the wave masks any key of the tile on either edge.  A wave also skips a tile that lies
// below the lower edge of all its rows and holds no sink key, as it skips one above its diagonal.  And
// the tile range need not start at 0: rec[5] = wt0 is the first tile of the window run and rec[6] = nsink
// the sink tiles when there is a gap between the two (else both are 0 and the tiles are VARLEN's); with
// sink tiles split 0 is the sink run [0, nsink) and split s >= 1 runs kps keys from tile wt0 + (s - 1) *
// kps / 64, without them split s starts at wt0 + s * kps / 64.  The workgroup still runs one contiguous
// range, so MxPagedRing starts at its first tile as it is and never enters a page of the gap (the host
// may have given those back: PagedKVFP4.trim).  Both numbers are clamped; a first tile past the
// sequence is the empty state.  tests/mxfp4_window_ref.py restates it, tests/test_gpu_mxfp4_window.py
// checks it.
// TREE (with VARLEN and CAUSAL, no window; the verify step of speculative decoding): rec[7] = nd, clamped
// to [0, min(sq, 64)], says that the sequence's last nd queries are the nodes of a draft tree, already
// appended at keys base = len - nd .. len - 1 in topological order.  Query i with t = i - (sq - nd) >= 0
// sees key k iff k < base or k = base + b with bit b of its word vl.tree[first packed token + i] set (the
// node's ancestors and itself); the lane loads the word once and clamps it to (word & bits <= t) | bit t,
// so the mask is a subset of the causal row that holds the query itself: a wrong word gives a wrong answer,
// never an empty row.  Queries with t < 0 and sequences with nd = 0 are plain causal.  Tiles, splits, the
// wave's causal skip, partial rows and the merge are the VARLEN instantiation's.  Its own: on a tile that
// crosses a causal diagonal of the wave or holds a key >= base (`diag`; at most two tiles of a sequence do
// the latter) every lane builds the tile's visibility word -- ones below base - k0 and the node's word
// shifted there, or the causal prefix for t < 0 -- shifted down by 4h, and mx_tile TREE tests its bits.
// The lane carries the word (two registers), t and the wave base.  tests/mxfp4_tree_ref.py restates it,
// tests/test_gpu_mxfp4_tree.py checks it.
// STEP (with VARLEN and CAUSAL, with or without WINDOW; the device-planned decode step at the end of this
// file): the grid is fixed when the step is made, `splits` work records {i, 0, s, 0} per entry i, and the
// records seq_rec[i] are written by mx_decode_plan_kernel from the device lengths.  A workgroup whose split
// s is >= rec[3] = ns_i -- a padding entry (ns = 0) or a sequence that needs fewer splits than the longest
// one could -- returns before it reads anything else and stores nothing; every other workgroup is the
// VARLEN (WINDOW) instantiation's statement for statement.  STEP with TREE (the device-planned verify step at
// the end of this file) is the same exit in front of the TREE instantiation: mx_verify_plan_kernel writes the
// records, rec[7] = K draft nodes of K queries, and the work records {i, row block, s, 0} cover ceil(G * K /
// 128) row blocks per entry.
struct MxVarlen {
  const int* work;      // i32 [nwork][4]
  const int* seq_rec;   // i32 [nseq][8]
  int nseq, group;      // sequences of the call, query heads per key/value head
  long qrows;           // T * group * hps packed query rows
  long part_rows;
  int window, sinks;    // WINDOW: W >= 1 keys a query looks back (itself included), S >= 0 sink keys
  // SHARED (at the end: the arguments of the other instantiations keep their places)
  const int* grp_rec;   // i32 [ngroup][4]
  const int* members;   // i32 [nmember][2]
  int ngroup, nmember;
  // TREE (after them, for the same reason)
  const unsigned long* tree;   // u64 [tokens]: the ancestor word of every packed token, 0 outside a tree
  long tokens;
};

// SHARED (with VARLEN; the shared-prefix step of kv_cache_mxfp4.py): one workgroup of a group record {g,
// 128-row block of the group's stacked rows, split, 1}.  grp_rec[g] = {first entry in members, member
// count, ns_g shared splits, R_g stacked rows}, members[e] = {j, first stacked row of sequence j}: stacked
// row r belongs to the last member whose first row is <= r and is virtual row r' = r - first of that
// sequence, in its own order g * sq_j + i.  The workgroup runs the split's kps / 64 tiles ONCE for all of
// its rows, through the table row of the group's first member (the host has found the pages equal in
// every member's row), and every lane writes its state where the VARLEN workgroup of its own sequence
// would have: partial row pbase_j + (split * hps + hd) * G * sq_j + r'.  The host shares only splits that
// lie wholly inside the common pages and below every member's first diagonal, so every key of every tile
// is visible to every row: no length is read and the tile body is mx_tile<D, false>, the statements the
// CAUSAL and LEN instantiations execute on such a tile (diag == false).  The ring is given npages =
// ceil(ns_g * kps / P), so its one-page-ahead table read stays inside the shared run.
// Every index is clamped (group, member slice, j, slot, row block, first tile, packed row) or checked
// (partial row): a wrong table gives a wrong answer, never an address outside q, the tables or the
// partials.  A wave's 32 rows may lie in several members, so the epilogue stores row by row
// (store_rows_indexed) from the 32 partial-row indices the lanes leave in LDS behind the ring; the state a
// lane keeps across the tile loop for this is that one index.
template <int D>
QA_DEVICE void mx_group_split(const uint8_t* __restrict__ q4, const uint8_t* __restrict__ qs,
                              const uint8_t* __restrict__ k4, const uint8_t* __restrict__ ks,
                              const uint8_t* __restrict__ vt, const uint8_t* __restrict__ vs,
                              float* __restrict__ opart, float2* __restrict__ ml, int nslot, int kps, float qks,
                              int hps, const int* __restrict__ btab, int mpp, int lgt, int npool,
                              const MxVarlen& vl, int g, int qt, int split, int hd, char* smem) {
  using C = MxCfg<D>;
  typedef const __attribute__((address_space(4))) int* table_ptr;
  const table_ptr grp = (table_ptr)(unsigned long)(vl.grp_rec + 4L * min(max(g, 0), vl.ngroup - 1));
  const int mfirst = min(max(grp[0], 0), vl.nmember - 1);
  const int mcnt = min(max(grp[1], 1), vl.nmember - mfirst);
  const int rows = max(grp[3], 1);
  const table_ptr mem = (table_ptr)(unsigned long)(vl.members + 2L * mfirst);
  const table_ptr recs = (table_ptr)(unsigned long)vl.seq_rec;
  // the shared run: gt >= 1 tiles from key 0 that the first member's table row can hold; this workgroup's
  // tiles [t0, t0 + ntw) of it, ntw >= 1
  const long gt = min((long)max(grp[2], 1) * (kps / C::KT), (long)mpp << lgt);
  const int t0 = (int)min((long)split * (kps / C::KT), gt - 1);
  const int ntw = (int)min((long)(kps / C::KT), gt - t0);
  const int slot0 = min(max(recs[8L * min(max(mem[0], 0), vl.nseq - 1)], 0), nslot - 1);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, h = lane >> 5, c32 = lane & 31;
  const int q0 = min(qt, (rows - 1) / C::QROWS) * C::QROWS + wave * 32;
  const int qi = min(q0 + c32, rows - 1);
  const bool active = q0 < rows;

  // the member of the lane's row: the last entry of the group's slice whose first row is <= qi
  int lo = 0, hi = mcnt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mem[2 * mid + 1] <= qi) lo = mid;
    else hi = mid - 1;
  }
  const table_ptr rec = recs + 8L * min(max(mem[2 * lo], 0), vl.nseq - 1);
  const int sq = max(rec[2], 1);
  const int rr = min(max(qi - mem[2 * lo + 1], 0), vl.group * sq - 1);   // virtual row of the member
  const long qrow = min(max(((long)rec[1] + rr % sq) * (vl.group * hps) + hd * vl.group + rr / sq, 0L),
                        vl.qrows - 1);
  const long prow = rec[4] + ((long)split * hps + hd) * ((long)vl.group * sq) + rr;
  // the lane's partial row, -1 for a lane without a row of its own or with one outside the partials
  const int dst = q0 + c32 < rows && prow >= 0 && prow < vl.part_rows ? (int)prow : -1;

  MxPagedRing<D> ring(k4, ks, vt, vs, btab + (long)slot0 * mpp, (int)((gt + (1 << lgt) - 1) >> lgt), lgt, hps,
                      hd, npool, t0, smem, wave, lane);
  ring.prologue(ntw);

  v4i qf[C::NKS];
  const unsigned qsw = mx_load_q<D>(q4, qs, qrow, h, qf);

  v16f o[C::NDB];
#pragma unroll
  for (int b = 0; b < C::NDB; ++b) o[b] = v16f{};
  float m = -INFINITY, l = 0.f;

  vmem_drain();
  __syncthreads();
  for (int t = 0; t < ntw; ++t) {
    ring_wait_barrier<2 * C::IPW>();
    ring.issue(t + 3, ntw);
    if (!active) continue;   // a wave without rows keeps its share of the DMA and the barrier
    mx_tile<D, false>(smem + (t & 3) * C::SLOT, qf, qsw, o, m, l, false, 0, qks, lane, h, c32);
  }
  vmcnt_wait_all();
  __syncthreads();
  if (!active) return;
  if (h == 0 && dst >= 0) ml[dst] = make_float2(m, l);
  int* rowidx = reinterpret_cast<int*>(smem + C::NSLOT * C::SLOT) + wave * 32;
  if (h == 0) rowidx[c32] = dst;
  store_rows_indexed<D, 2>(o, 1.0f, smem + wave * RowTile<D, float, 2>::BYTES, opart, rowidx, lane);
}
constexpr int MX_GROUP_LDS = MxCfg<128>::WAVES * 32 * (int)sizeof(int);   // rowidx, behind the ring

template <int D, bool CAUSAL, bool LEN = false, bool PAGED = false, bool VARLEN = false, bool WINDOW = false,
          bool SHARED = false, bool TREE = false, bool STEP = false>
__global__ __launch_bounds__(256, QA_MX_OCC) void mxfp4_attn_split_kernel(
    const uint8_t* __restrict__ q4, const uint8_t* __restrict__ qs, const uint8_t* __restrict__ k4,
    const uint8_t* __restrict__ ks, const uint8_t* __restrict__ vt, const uint8_t* __restrict__ vs,
    float* __restrict__ opart, float2* __restrict__ ml, int BHV, int rows, int sq_head, int Sk,
    int kps, float qks, int qoff, const int* __restrict__ lens, int hps, const int* __restrict__ btab,
    int mpp, int lgt, int npool, MxVarlen vl) {
  using C = MxCfg<D>;
  constexpr bool MASK = CAUSAL || LEN;
  static_assert(LEN || !PAGED, "the paged pool has a length per sequence");
  static_assert(PAGED || !VARLEN, "the packed step runs over the paged pool");
  static_assert(!WINDOW || (VARLEN && CAUSAL), "the window is the packed step's, and causal");
  static_assert(!SHARED || (VARLEN && !WINDOW), "shared prefixes are the packed step's, without a window");
  static_assert(!TREE || (VARLEN && CAUSAL && !WINDOW && !SHARED), "tree masks are the causal packed step's");
  static_assert(!STEP || (VARLEN && CAUSAL && !SHARED), "the fixed grid is the causal packed step's");
  static_assert(sizeof(float) == 4 && D == 128, "fp32 staging in two passes fills the ring exactly");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bh, qt, split = (int)blockIdx.y;
  long qbase = 0, pbase = 0;   // VARLEN: the sequence's first packed token and first partial row
  int wt0 = 0, nsink = 0;      // WINDOW: first tile of the window run; sink tiles when there is a gap, else 0
  [[maybe_unused]] int nd = 0; // TREE: the sequence's last nd queries are tree nodes
  if constexpr (VARLEN) {
    typedef const __attribute__((address_space(4))) int* table_ptr;
    const int hd = (int)(blockIdx.x % (unsigned)hps);
    const table_ptr w = (table_ptr)(unsigned long)(vl.work + 4L * (blockIdx.x / (unsigned)hps));
    if constexpr (SHARED) {
      if (w[3] == 1) {   // a group record (workgroup-uniform); every other record is the VARLEN path below
        mx_group_split<D>(q4, qs, k4, ks, vt, vs, opart, ml, BHV / hps, kps, qks, hps, btab, mpp, lgt, npool, vl,
                          w[0], max(w[1], 0), max(w[2], 0), hd, smem);
        return;
      }
    }
    const table_ptr rec =(table_ptr)(unsigned long)(vl.seq_rec + 8L * min(max(w[0], 0), vl.nseq - 1));
    if constexpr (STEP) {   // a surplus workgroup of the fixed grid: nothing fetched, nothing stored
      if (max(w[2], 0) >= rec[3]) return;
    }
    qt = max(w[1], 0);
    split = max(w[2], 0);
    bh = min(max(rec[0], 0), BHV / hps - 1) * hps + hd;
    qbase = rec[1];
    sq_head = max(rec[2], 1);
    pbase = rec[4];
    rows = vl.group * sq_head;
    if constexpr (WINDOW) {
      wt0 = max(rec[5], 0);
      nsink = max(rec[6], 0);
    }
    if constexpr (TREE) nd = min(max(rec[7], 0), min(sq_head, 64));
  } else {
    const int nrb = (rows + C::QROWS - 1) / C::QROWS;
    xcd_remap(blockIdx.x, nrb, BHV, bh, qt);
  }
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, h = lane >> 5, c32 = lane & 31;
  const int q0 = qt * C::QROWS + wave * 32;
  const int qi = min(q0 + c32, rows - 1);
  int len = Sk;   // keys of this head (workgroup-uniform)
  if constexpr (LEN) {
    len = min(__builtin_amdgcn_readfirstlane(lens[bh / hps]), Sk);   // never a tile past the capacity
    qoff = len - sq_head;
  }
  const int nt = LEN ? (len + C::KT - 1) / C::KT : Sk / C::KT;
  const int ntc = Sk / C::KT;   // tile stride of a key/value head in vt / vs
  // this workgroup's tiles [t0, t0 + ntw) of the key/value head: ntw >= 1 (nsplit = ceil(Sk / kps))
  // WINDOW: with a gap split 0 is the sink run [0, nsink) and split s >= 1 starts kps keys after split
  // s - 1 from tile wt0; without one (nsink = 0, wt0 = 0) the tiles are the ones below.  A first tile past
  // nt (a wrong table) is nt: the empty state.
  const bool sink_run = WINDOW && nsink > 0 && split == 0;
  const int t0 = !WINDOW ? split * (kps / C::KT)
                         : sink_run ? 0
                                    : (int)min((long)wt0 + (long)(split - (nsink > 0)) * (kps / C::KT), (long)nt);
  // the wave's first row of opart / ml
  const auto part_row0 = [&]() -> long {
    if constexpr (VARLEN) return pbase + ((long)split * hps + bh % hps) * rows + q0;
    else return ((long)split * BHV + bh) * rows + q0;
  };
  bool active = q0 < rows;
  if constexpr (VARLEN)   // a wave whose rows would pass the partials stores nothing
    active = active && part_row0() >= 0 && part_row0() + min(32, rows - q0) <= vl.part_rows;
  if constexpr (LEN) {
    if (t0 >= nt) {   // a split past the sequence: the empty state for the workgroup's rows
      if (!active) return;
      const long row0 = part_row0();
      const int nr = min(32, rows - q0);
      if (h == 0 && c32 < nr) ml[row0 + c32] = make_float2(-INFINITY, 0.f);
      v4f* dst = reinterpret_cast<v4f*>(opart + row0 * D);
#pragma unroll
      for (int i = 0; i < 32 * (D / 4) / 64; ++i)
        if (i * 64 + lane < nr * (D / 4)) dst[i * 64 + lane] = v4f{0.f, 0.f, 0.f, 0.f};
      return;
    }
  }
  const int ntw = sink_run ? min(nsink, nt) : min(nt - t0, kps / C::KT);
  // causal: query positions of the wave's rows (a wave that crosses a head boundary holds both ends)
  int wmin = 0, wmax = 0, pos = 0;
  if constexpr (CAUSAL) {
    const int nr = min(32, rows - q0), p0 = q0 % sq_head;
    const bool wraps = p0 + nr > sq_head;
    wmin = wraps ? 0 : p0;
    wmax = wraps ? sq_head - 1 : p0 + nr - 1;
    pos = qi % sq_head;
  }
  // TREE: the node of the lane's row (tnode < 0: a plain causal row), its cleaned word, the first tree key
  [[maybe_unused]] int tnode = -1, tbase = 0;
  [[maybe_unused]] unsigned long tword = 0;
  if constexpr (TREE) {
    tnode = nd > 0 ? pos - (sq_head - nd) : -1;
    tbase = max(len - nd, 0);
    if (tnode >= 0) {
      const unsigned long self = 1ul << tnode;
      tword = (vl.tree[min(max(qbase + pos, 0L), vl.tokens - 1)] & (self | (self - 1))) | self;
    }
  }

  // the ring over the split's own byte range: the buffer bounds end at its last tile
  const long kvh = bh;
  // (one of the two is an MxNoRing, which holds nothing; the LEN statement stays as it was)
  std::conditional_t<PAGED, MxNoRing, const MxRing<D>> lring(
      k4 + (kvh * Sk + (long)t0 * C::KT) * C::KROWB, ks + (kvh * Sk + (long)t0 * C::KT) * (D / 32),
      vt + (kvh * ntc + t0) * C::V_BYTES, vs + (kvh * ntc + t0) * C::VS_BYTES, ntw, smem, wave, lane);
  std::conditional_t<PAGED, MxPagedRing<D>, MxNoRing> pring(
      k4, ks, vt, vs, btab + (long)(bh / hps) * mpp, (nt + (1 << lgt) - 1) >> lgt, lgt, hps, bh % hps, npool,
      t0, smem, wave, lane);
  if constexpr (PAGED) pring.prologue(ntw);
  else lring.prologue(ntw);

  v4i qf[C::NKS];
  long qrow = (long)bh * rows + qi;
  if constexpr (VARLEN)   // token-major q: (token, query head) of virtual row qi
    qrow = min(max((qbase + qi % sq_head) * (vl.group * hps) + (bh % hps) * vl.group + qi / sq_head, 0L),
               vl.qrows - 1);
  const unsigned qsw = mx_load_q<D>(q4, qs, qrow, h, qf);

  v16f o[C::NDB];
#pragma unroll
  for (int b = 0; b < C::NDB; ++b) o[b] = v16f{};
  float m = -INFINITY, l = 0.f;

  vmem_drain();
  __syncthreads();
  for (int t = 0; t < ntw; ++t) {
    ring_wait_barrier<2 * C::IPW>();
    if constexpr (PAGED) pring.issue(t + 3, ntw);
    else lring.issue(t + 3, ntw);
    if (!active) continue;   // a wave without rows keeps its share of the DMA and the barrier
    bool diag = false;
    int lim = 0;
    [[maybe_unused]] int lo = 0, slim = 0;
    [[maybe_unused]] unsigned vis0 = 0, vis1 = 0;
    if constexpr (CAUSAL) {
      const int k0 = C::KT * (t0 + t);
      if (k0 > wmax + qoff) continue;           // no row of the wave sees the tile: m, l, O unchanged
      diag = k0 + C::KT - 1 > wmin + qoff;
      lim = pos + qoff - k0 - 4 * h;
      if constexpr (WINDOW) {
        // the tile lies below every row's window and holds no sink key: skipped like the one above
        if (k0 + C::KT - 1 < wmin + qoff - vl.window + 1 && k0 >= vl.sinks) continue;
        // some row's lower edge cuts the tile (the highest edge is the last row's), unless it is all sinks
        diag = diag || (k0 < wmax + qoff - vl.window + 1 && k0 + C::KT > vl.sinks);
        lo = pos + qoff - vl.window + 1 - k0 - 4 * h;
        slim = vl.sinks - 1 - k0 - 4 * h;
      }
      if constexpr (TREE) {
        // the tile holds a tree key: masked too.  d keys of the tile lie below the first tree key; the
        // tile starts below len <= tbase + 64, so a word is shifted by less than 64 either way
        const int d = tbase - k0;
        diag = diag || (nd > 0 && d < C::KT);
        if (diag) {
          const int c = pos + qoff - k0;   // the last element a causal row sees
          unsigned long vis = c >= C::KT - 1 ? ~0ul : c < 0 ? 0ul : (2ul << c) - 1;
          if (tnode >= 0)
            vis = d >= C::KT ? ~0ul : d >= 0 ? (tword << d) | ((1ul << d) - 1) : tword >> min(-d, C::KT - 1);
          vis >>= 4 * h;
          vis0 = (unsigned)vis;
          vis1 = (unsigned)(vis >> 32);
        }
      }
    } else if constexpr (LEN) {   // every row sees the keys <= len - 1
      const int k0 = C::KT * (t0 + t);
      diag = k0 + C::KT > len;
      lim = len - 1 - k0 - 4 * h;
    }
    if constexpr (WINDOW)
      mx_tile<D, MASK, true>(smem + (t & 3) * C::SLOT, qf, qsw, o, m, l, diag, lim, qks, lane, h, c32, lo, slim);
    else if constexpr (TREE)
      mx_tile<D, MASK, false, true>(smem + (t & 3) * C::SLOT, qf, qsw, o, m, l, diag, lim, qks, lane, h, c32, 0, 0,
                                    vis0, vis1);
    else
      mx_tile<D, MASK>(smem + (t & 3) * C::SLOT, qf, qsw, o, m, l, diag, lim, qks, lane, h, c32);
  }
  vmcnt_wait_all();
  __syncthreads();
  if (!active) return;
  const long row0 = part_row0();
  const int nr = min(32, rows - q0);
  if (h == 0 && c32 < nr) ml[row0 + c32] = make_float2(m, l);
  static_assert(C::WAVES * RowTile<D, float, 2>::BYTES <= C::NSLOT * C::SLOT, "staging fits the ring");
  store_rows<D, float, 2, false, true>(o, 1.0f, smem + wave * RowTile<D, float, 2>::BYTES, opart + row0 * D,
                                       lane, 0.f, nr);
}

// f16 of the exact product a * b, rounded once (v_fma_mixlo_f16 with fp32 sources)
QA_DEVICE _Float16 mul_f16_once(float a, float b) {
  unsigned r = 0;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(r) : "v"(a), "v"(b));
  return __builtin_bit_cast(_Float16, (unsigned short)r);
}

// Merge of the key splits of one output row, by the thread that owns its columns 8c .. 8c + 7: the row's
// nsplit partial rows are first, first + step, .. of opart / ml.  M = max_s m_s, w_s = 2^(m_s - M) (exact:
// every m_s is an integer or -inf, which weighs 0), L = sum_s w_s l_s, out = f16((sum_s w_s O_s) * (1 / L)),
// lse = M + log2(L): the one-pass epilogue on the merged state.
// The conversion to f16 is a definition, left to no heuristic of the compiler: the thread's columns 0 and 7
// are the exact product rounded to f16 once (mul_f16_once); its columns 1 .. 6 are the fp32 product,
// rounded, then converted (rounded twice; an empty asm keeps the product a value of its own, so it cannot
// be contracted into the conversion).  The two forms differ by one f16 ulp about once in 10^4 elements.
// tests/mxfp4_split_ref.py merge_bits restates this bit for bit.
template <int D>
QA_DEVICE void mx_merge_row(const float* __restrict__ opart, const float2* __restrict__ ml, long first,
                            long step, int nsplit, int c, _Float16* __restrict__ out_row,
                            float* __restrict__ lse_row) {
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ml[first + s * step].x);
  float L = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsplit; ++s) {
    const float2 v = ml[first + s * step];
    const float w = v.x == -INFINITY ? 0.f : __builtin_ldexpf(1.f, (int)(v.x - M));
    L = fmaf(w, v.y, L);
    const v4f* a = reinterpret_cast<const v4f*>(opart + (first + s * step) * D + 8 * c);
    const v4f a0 = a[0], a1 = a[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] = fmaf(w, a0[i], acc[i]);
      acc[4 + i] = fmaf(w, a1[i], acc[4 + i]);
    }
  }
  const float inv = 1.0f / L;
  v8h o;
  o[0] = mul_f16_once(acc[0], inv);
#pragma unroll
  for (int i = 1; i < 7; ++i) {
    float p = acc[i] * inv;
    asm volatile("" : "+v"(p));
    o[i] = (_Float16)p;
  }
  o[7] = mul_f16_once(acc[7], inv);
  *reinterpret_cast<v8h*>(out_row + 8 * c) = o;
  if (c == 0) *lse_row = M + log2_f32(L);
}

// The merge over the padded partials (opart f32 [nsplit][rows][D], ml [nsplit][rows]): one thread per 8
// columns of a row.
template <int D>
__global__ __launch_bounds__(256) void mxfp4_split_combine_kernel(const float* __restrict__ opart,
                                                                  const float2* __restrict__ ml,
                                                                  _Float16* __restrict__ out,
                                                                  float* __restrict__ lse, long rows,
                                                                  int nsplit) {
  constexpr int TPR = D / 8;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid / TPR;
  if (row >= rows) return;
  mx_merge_row<D>(opart, ml, row, rows, nsplit, (int)(gid % TPR), out + row * D, lse + row);
}

// The largest j in [0, n) with tab[j * stride + col] <= x (0 if there is none): the sequence of a
// packed token, from the ascending first-token column of a host-built table.
QA_DEVICE int mx_find_seq(const int* tab, int n, int stride, int col, int x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[(long)mid * stride + col] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The merge over the compact partials of the packed step (mxfp4_attn_split_kernel VARLEN): one thread per
// 8 columns of a packed output row (token, query head).  The thread finds its sequence j by binary search
// over the first-token column of seq_rec, and merges that sequence's own rec[3] splits, rows first + (s *
// Hkv + head / group) * group * sq + (head % group) * sq + token - first of opart / ml.  A row whose
// partial rows would pass part_rows (a wrong table) is not merged.
template <int D>
__global__ __launch_bounds__(256) void mxfp4_varlen_combine_kernel(const float* __restrict__ opart,
                                                                   const float2* __restrict__ ml,
                                                                   _Float16* __restrict__ out,
                                                                   float* __restrict__ lse,
                                                                   const int* __restrict__ seq_rec, int nseq,
                                                                   long rows, int Hq, int Hkv,
                                                                   long part_rows) {
  constexpr int TPR = D / 8;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid / TPR;
  if (row >= rows) return;
  const int token = (int)(row / Hq), head = (int)(row % Hq), G = Hq / Hkv;
  const int* rec = seq_rec + 8L * mx_find_seq(seq_rec, nseq, 8, 1, token);
  const int sq = max(rec[2], 1), nsplit = rec[3];
  const long rows_j = (long)G * sq, step = (long)Hkv * rows_j;
  const long first = rec[4] + (head / G) * rows_j + (long)(head % G) * sq + (token - rec[1]);
  if (nsplit < 1 || first < 0 || first + (nsplit - 1) * step >= part_rows) return;
  mx_merge_row<D>(opart, ml, first, step, nsplit, (int)(gid % TPR), out + row * D, lse + row);
}

// ---- packed append into the paged pool (kv_cache_mxfp4.py PagedKVFP4.append_packed)
// k, v f16 [T][Hkv][D] are token-major; tab i32 [nseq][4] = {slot, count, first packed token, 0} (first
// ascending, the slots distinct) says that packed tokens [first, first + count) go to tokens lens[slot]
// .. of sequence slot.  The same three launches as the padded append, the same quantisers, in the same
// order: V (reads vtail), then K and vtail, then the lengths.  A record whose slot is outside [0, B),
// whose count is < 1, whose tokens pass T or whose sequence would pass cap = mpp * P writes nothing
// (the host refuses all of these before it launches).

// the record j of a packed append with the sequence's length L before it -> its count, 0: nothing
QA_DEVICE int mx_packed_count(const int* tab, const int* lens, int j, int B, long T, int cap, int& slot,
                              int& first, int& L) {
  slot = tab[4L * j];
  const int cnt = tab[4L * j + 1];
  first = tab[4L * j + 2];
  if (slot < 0 || slot >= B || cnt < 1 || first < 0 || (long)first + cnt > T) return 0;
  L = lens[slot];
  return L >= 0 && L <= cap - cnt ? cnt : 0;
}

// V: one thread per (entry of tiles, head, column d, half h); tiles i32 [ntile][2] = {j, logical tile g}
// lists exactly the tiles the appends touch, g in [L / 64, (L + cnt - 1) / 64] (another g: nothing).
template <int D>
__global__ __launch_bounds__(256) void mx_append_vt_packed_kernel(
    const _Float16* __restrict__ v, const _Float16* __restrict__ vtail, uint8_t* __restrict__ vt,
    uint8_t* __restrict__ vs, const int* __restrict__ lens, const int* __restrict__ tab,
    const int* __restrict__ tiles, long nthr, int nseq, int B, int Hkv, long T, int cap,
    const int* __restrict__ btab, int mpp, int lgt, int npool) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nthr) return;
  const int h = (int)(i & 1);
  const int d = (int)((i >> 1) % D);
  const long gt = (i >> 1) / D;                 // entry * Hkv + head
  const int hd = (int)(gt % Hkv);
  const int j = tiles[2 * (gt / Hkv)], g = tiles[2 * (gt / Hkv) + 1];
  if (j < 0 || j >= nseq) return;
  int slot, first, L;
  const int cnt = mx_packed_count(tab, lens, j, B, T, cap, slot, first, L);
  if (cnt == 0 || g < L / 64 || 64L * g >= L + cnt) return;   // L + cnt <= cap: the tile lies inside
  const long bh = (long)slot * Hkv + hd;
  const long o = (mx_paged_tile(btab, slot, hd, g, Hkv, mpp, lgt, npool) * D + d) * 2 + h;
  mx_requant_v_block<D>(vtail + bh * 64 * D + d, v + ((long)first * Hkv + hd) * D + d, Hkv, g, L, cnt,
                        h, reinterpret_cast<v4i*>(vt) + o, vs + o);
}

// K and vtail: one thread per 32-element block of a packed row (token, head); its record is found by
// binary search over the first-token column of tab.
template <int D>
__global__ __launch_bounds__(256) void mx_append_k_packed_kernel(
    const _Float16* __restrict__ k, const _Float16* __restrict__ v, const _Float16* __restrict__ mean,
    uint8_t* __restrict__ k4, uint8_t* __restrict__ ks, _Float16* __restrict__ vtail,
    const int* __restrict__ lens, const int* __restrict__ tab, long nblk, int nseq, int B, int Hkv, long T,
    int cap, const int* __restrict__ btab, int mpp, int lgt, int npool) {
  constexpr int NB = D / 32;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nblk) return;
  const int blk = (int)(i % NB);
  const int hd = (int)(i / NB % Hkv);
  const int token = (int)(i / NB / Hkv);
  int slot, first, L;
  const int cnt = mx_packed_count(tab, lens, mx_find_seq(tab, nseq, 4, 2, token), B, T, cap, slot, first, L);
  const int tok = token - first;
  if (tok < 0 || tok >= cnt) return;   // t < L + cnt <= cap
  const int t = L + tok;
  const long bh = (long)slot * Hkv + hd;
  const v8h* mu = mean ? reinterpret_cast<const v8h*>(mean + bh * D + blk * 32) : nullptr;
  const long o = (mx_paged_tile(btab, slot, hd, t / 64, Hkv, mpp, lgt, npool) * 64 + t % 64) * NB + blk;
  mx_append_k_block(k + i * 32, v + i * 32, mu, k4, ks, o, vtail + (bh * 64 + t % 64) * D + blk * 32, t, L + cnt);
}

// lens[slot] += cnt, one thread per record
__global__ __launch_bounds__(256) void mx_append_len_packed_kernel(int* __restrict__ lens,
                                                                   const int* __restrict__ tab, int nseq,
                                                                   int B, long T, int cap) {
  const int j = (int)blockIdx.x * 256 + threadIdx.x;
  if (j >= nseq) return;
  int slot, first, L;
  const int cnt = mx_packed_count(tab, lens, j, B, T, cap, slot, first, L);
  if (cnt) lens[slot] = L + cnt;
}

// ---- rotary positions (kv_cache_mxfp4.py Rope): q on quantise, new keys on the packed append
// cos_sin f32 [max_pos][D]: row p holds cos theta(p, i) at [i] and sin theta(p, i) at [D/2 + i], pair i <
// D/2.  NeoX (IL false) pairs elements (i, i + D/2), interleaved (IL true) elements (2i, 2i + 1).  A pair
// (a, b) of f16 inputs becomes first = f16(f32(a c) - f32(b s)), second = f16(f32(b c) + f32(a s)): two
// rounded fp32 products, one rounded fp32 sum, one round-to-nearest-even to f16 and NO fused multiply-add,
// which is what separate fp32 tensor operations give (tests/mxfp4_rope_ref.py), so the rotated row is
// defined bit for bit and the quantisers take it unchanged.  The position is clamped to [0, max_pos): a
// wrong position gives a wrong answer, never an address outside the table.

// Block blk of the rotated row: row's own block and, NeoX, its partner blk ^ (D/64) -> out[4].
template <int D, bool IL>
QA_DEVICE void mx_rope_block(const _Float16* row, const float* cs, int blk, v8h* out) {
#pragma clang fp contract(off)
  constexpr int HALF = D / 2;
  const v8h* own = reinterpret_cast<const v8h*>(row + blk * 32);
  if constexpr (IL) {
    const v4f* co = reinterpret_cast<const v4f*>(cs + blk * 16);
    const v4f* si = reinterpret_cast<const v4f*>(cs + HALF + blk * 16);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const v8h v = own[c];
      const v4f cc = co[c], ss = si[c];
      v8h r;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float a = (float)v[2 * m], b = (float)v[2 * m + 1];
        const float ac = a * cc[m], bs = b * ss[m], bc = b * cc[m], as = a * ss[m];
        r[2 * m] = (_Float16)(ac - bs);
        r[2 * m + 1] = (_Float16)(bc + as);
      }
      out[c] = r;
    }
  } else {
    const bool second = blk * 32 >= HALF;             // the block holds the pairs' second elements
    const int pb = blk * 32 - (second ? HALF : 0);    // its first pair
    const v8h* par = reinterpret_cast<const v8h*>(row + (second ? pb : pb + HALF));
    const v4f* co = reinterpret_cast<const v4f*>(cs + pb);
    const v4f* si = reinterpret_cast<const v4f*>(cs + HALF + pb);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const v8h v = own[c], w = par[c];
      v8h r;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const v4f cc = co[2 * c + h], ss = si[2 * c + h];
#pragma unroll
        for (int m = 0; m < 4; ++m) {   // own c - partner s for a first element, own c + partner s for a second
          const float oc = (float)v[4 * h + m] * cc[m], ps = (float)w[4 * h + m] * ss[m];
          r[4 * h + m] = (_Float16)(second ? oc + ps : oc - ps);
        }
      }
      out[c] = r;
    }
  }
}

// Q: mx_quant_rows_kernel without a mean on packed rows x f16 [T][H][D], rotated first by pos[token]; one
// thread per 32-element block, the heads of a token adjacent (they read the same table row).
template <int D, bool IL>
__global__ __launch_bounds__(256) void mx_quant_rows_rope_kernel(const _Float16* __restrict__ x,
                                                                 uint8_t* __restrict__ q4,
                                                                 uint8_t* __restrict__ sc,
                                                                 const float* __restrict__ cos_sin,
                                                                 const int* __restrict__ pos, long nblk, int H,
                                                                 int max_pos) {
  constexpr int NB = D / 32;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nblk) return;
  const long row = i / NB;
  const int p = min(max(pos[row / H], 0), max_pos - 1);
  v8h r[4];
  mx_rope_block<D, IL>(x + row * D, cos_sin + (long)p * D, (int)(i % NB), r);
  mx_quant_row_block(r, nullptr, reinterpret_cast<v4i*>(q4) + i, sc + i);
}

// K and vtail: mx_append_k_packed_kernel with the K block rotated first by pos[packed token]; V is not rotated.
template <int D, bool IL>
__global__ __launch_bounds__(256) void mx_append_k_packed_rope_kernel(
    const _Float16* __restrict__ k, const _Float16* __restrict__ v, const _Float16* __restrict__ mean,
    uint8_t* __restrict__ k4, uint8_t* __restrict__ ks, _Float16* __restrict__ vtail,
    const int* __restrict__ lens, const int* __restrict__ tab, long nblk, int nseq, int B, int Hkv, long T,
    int cap, const int* __restrict__ btab, int mpp, int lgt, int npool, const float* __restrict__ cos_sin,
    const int* __restrict__ pos, int max_pos) {
  constexpr int NB = D / 32;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nblk) return;
  const int blk = (int)(i % NB);
  const int hd = (int)(i / NB % Hkv);
  const int token = (int)(i / NB / Hkv);
  int slot, first, L;
  const int cnt = mx_packed_count(tab, lens, mx_find_seq(tab, nseq, 4, 2, token), B, T, cap, slot, first, L);
  const int tok = token - first;
  if (tok < 0 || tok >= cnt) return;   // t < L + cnt <= cap
  const int t = L + tok;
  const long bh = (long)slot * Hkv + hd;
  const v8h* mu = mean ? reinterpret_cast<const v8h*>(mean + bh * D + blk * 32) : nullptr;
  const long o = (mx_paged_tile(btab, slot, hd, t / 64, Hkv, mpp, lgt, npool) * 64 + t % 64) * NB + blk;
  const int p = min(max(pos[token], 0), max_pos - 1);
  v8h r[4];
  mx_rope_block<D, IL>(k + (i / NB) * D, cos_sin + (long)p * D, blk, r);
  mx_append_k_block(reinterpret_cast<const _Float16*>(r), v + i * 32, mu, k4, ks, o,
                    vtail + (bh * 64 + t % 64) * D + blk * 32, t, L + cnt);
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_mxfp4_quant_rows(const void* x, const void* mean, void* q4, void* scale, long rows,
                                      long seq, int head_dim, void* stream) {
  if (head_dim != 64 && head_dim != 128) return 1;
  if (mean && (seq <= 0 || rows % seq != 0)) return 1;
  const long nblk = rows * head_dim / 32;
  if (nblk == 0) return 0;
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

// log2(page_tokens / 64) of a page size 64 * 2^k in [64, 1024], else -1
static int mx_page_lgt(long page_tokens) {
  for (int k = 0; k <= 4; ++k)
    if (page_tokens == 64L << k) return k;
  return -1;
}

// the pool's limits every paged entry shares: a physical tile index below 2^31 and 32-bit token indices
// inside a sequence
static bool mx_pool_ok(long num_pages, long kv_heads, int lgt, long mpp) {
  if (lgt < 0 || num_pages < 1 || kv_heads < 1 || mpp < 1 || num_pages > 0x7fffffffL) return false;
  if (kv_heads > 0x7fffffffL || mpp > (1L << 25) || mpp * (64L << lgt) > (1L << 25)) return false;
  return num_pages * kv_heads <= (0x7fffffffL >> lgt);
}

// what every key-split entry asks of its head_dim and keys_per_split, and the padded ones of their rows
static bool mx_split_ok(int head_dim, int keys_per_split) {
  return head_dim == 128 && keys_per_split >= 64 && keys_per_split % 64 == 0;
}
static bool mx_rows_ok(long sq_head, long rows) { return sq_head >= 1 && rows % sq_head == 0; }

// One call of mxfp4_attn_split_kernel: its arguments as the kernel takes them (Sk: the key stride of a
// key/value head, which is the key count without lens) and its grid.
struct MxSplitCall {
  const void *q4, *qscale, *k4, *kscale, *vt, *vscale;
  void *opart, *ml;
  int bhv, rows, sq_head, Sk, kps;
  float qks;
  int qoff;
  const void* lens;
  int hps;
  const void* btab;
  int mpp, lgt, npool;
  MxVarlen vl;
  dim3 grid;
};

// the padded layouts' grid: (row blocks x key/value heads, splits of sk keys), false past the launch limits
static bool mx_split_grid(MxSplitCall& c, long sk) {
  const long nrb = (c.rows + MxCfg<128>::QROWS - 1) / MxCfg<128>::QROWS;
  const long nsplit = (sk + c.kps - 1) / c.kps;
  if (nrb * c.bhv > 0x7fffffffL || nsplit > 65535) return false;
  c.grid = dim3((unsigned)(nrb * c.bhv), (unsigned)nsplit);
  return true;
}

template <bool CAUSAL, bool LEN, bool PAGED, bool VARLEN, bool WINDOW, bool SHARED = false, bool TREE = false,
          bool STEP = false>
static int mx_split_launch(const MxSplitCall& c, void* stream) {
  using C = MxCfg<128>;
  const auto kernel = mxfp4_attn_split_kernel<128, CAUSAL, LEN, PAGED, VARLEN, WINDOW, SHARED, TREE, STEP>;
  const int lds = C::NSLOT * C::SLOT + (SHARED ? MX_GROUP_LDS : 0);
  { static LdsGrant granted_; if (!lds_grant((const void*)kernel, lds, granted_)) return 1; }
  hipLaunchKernelGGL(kernel, c.grid, dim3(256), lds, (hipStream_t)stream, (const uint8_t*)c.q4,
                     (const uint8_t*)c.qscale, (const uint8_t*)c.k4, (const uint8_t*)c.kscale,
                     (const uint8_t*)c.vt, (const uint8_t*)c.vscale, (float*)c.opart, (float2*)c.ml, c.bhv,
                     c.rows, c.sq_head, c.Sk, c.kps, c.qks, c.qoff, (const int*)c.lens, c.hps,
                     (const int*)c.btab, c.mpp, c.lgt, c.npool, c.vl);
  return hipGetLastError() == hipSuccess ? 0 : 2;
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

// What the packed entries without groups share: their argument checks and the call filled in (nwork work
// records x kv_heads workgroups in one launch; rows, sq_head and qoff come from the records).  Returns the
// entry's status when there is nothing to launch, -1 when `c` is to be launched.  tree: the ancestor words
// of the tree entry, else null.
static int mx_varlen_call(MxSplitCall& c, const void* q4, const void* qscale, const void* k4,
                          const void* kscale, const void* vt, const void* vscale, void* opart, void* ml,
                          const void* lens, const void* block_table, const void* seq_rec, const void* work,
                          long nseq, long nwork, long tokens, long part_rows, long max_seqs, long kv_heads,
                          long group, long num_pages, long page_tokens, long max_pages_per_seq, int causal,
                          int keys_per_split, int head_dim, float qks, long window, long sinks,
                          const void* tree) {
  if (!mx_split_ok(head_dim, keys_per_split) || nseq < 0 || nwork < 0 || tokens < 0 || part_rows < 0) return 1;
  if (!lens || !block_table || !seq_rec || !work) return 1;
  const int lgt = mx_page_lgt(page_tokens);
  if (!mx_pool_ok(num_pages, kv_heads, lgt, max_pages_per_seq)) return 1;
  if (max_seqs < 1 || group < 1 || group > 0x7fffffffL || (causal != 0 && causal != 2)) return 1;
  if (nseq == 0 || nwork == 0 || tokens == 0) return 0;
  if (nseq > max_seqs || nseq > tokens || part_rows < 1) return 1;
  // 32-bit packed rows, partial rows, workgroups and slot heads
  if (tokens > 0x7fffffffL / (group * kv_heads) || part_rows > 0x7fffffffL) return 1;
  if (nwork > 0x7fffffffL / kv_heads || max_seqs > 0x7fffffffL / kv_heads) return 1;
  // a sequence holds at most 2^25 keys (mx_pool_ok): a larger window or sink count means the same, and
  // the kernel's 32-bit edges cannot overflow
  const long big = 1L << 26;
  const MxVarlen vl{(const int*)work, (const int*)seq_rec, (int)nseq, (int)group, tokens * group * kv_heads,
                    part_rows, (int)(window < big ? window : big), (int)(sinks < big ? sinks : big),
                    nullptr, nullptr, 0, 0, (const unsigned long*)tree, tokens};
  c = MxSplitCall{q4, qscale, k4, kscale, vt, vscale, opart, ml, (int)(max_seqs * kv_heads), 0, 1,
                  (int)(max_pages_per_seq * page_tokens), keys_per_split, qks, 0, lens, (int)kv_heads,
                  block_table, (int)max_pages_per_seq, lgt, (int)num_pages, vl,
                  dim3((unsigned)(nwork * kv_heads))};
  return -1;
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
  const int rc = mx_varlen_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec,
                                work, nseq, nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages,
                                page_tokens, max_pages_per_seq, causal, keys_per_split, head_dim, qks, window,
                                sinks, nullptr);
  if (rc >= 0) return rc;
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

// the merge of the packed step's compact partials into O f16 [tokens][q_heads][128], lse [tokens][q_heads]
extern "C" int qattn_mxfp4_varlen_combine(const void* opart, const void* ml, void* out, void* lse,
                                          const void* seq_rec, long nseq, long tokens, long q_heads,
                                          long kv_heads, long part_rows, int head_dim, void* stream) {
  if (head_dim != 128 || nseq < 0 || tokens < 0 || part_rows < 0 || !seq_rec) return 1;
  if (kv_heads < 1 || q_heads < 1 || q_heads % kv_heads != 0 || q_heads > 0x7fffffffL) return 1;
  if (nseq == 0 || tokens == 0) return 0;
  if (nseq > tokens || part_rows < 1) return 1;
  if (tokens > 0x7fffffffL / q_heads || part_rows > 0x7fffffffL) return 1;
  const long rows = tokens * q_heads, nthr = rows * (128 / 8);
  hipLaunchKernelGGL(mxfp4_varlen_combine_kernel<128>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)opart, (const float2*)ml, (_Float16*)out,
                     (float*)lse, (const int*)seq_rec, (int)nseq, rows, (int)q_heads, (int)kv_heads,
                     part_rows);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// what the rotary entries hold their table to ("rotary positions" above)
static bool mx_rope_ok(const void* cos_sin, const void* pos, long max_pos, int interleaved) {
  return cos_sin && pos && max_pos >= 1 && max_pos <= 0x7fffffffL && (interleaved == 0 || interleaved == 1);
}

// a packed append into the paged pool ("packed append" above): seq_tab i32 [nseq][4] and tiles i32
// [ntiles][2] on the device, the pages the new tokens need in block_table already.  ROPE: the keys are
// rotated first (interleaved picks the pairing), V and the lengths as without.
template <bool ROPE>
static int mx_append_packed(const void* k, const void* v, const void* k_mean, void* k4, void* kscale, void* vt,
                            void* vscale, void* vtail, void* lens, const void* block_table,
                            const void* seq_tab, const void* tiles, long nseq, long ntiles, long tokens,
                            long max_seqs, long kv_heads, long num_pages, long page_tokens,
                            long max_pages_per_seq, int head_dim, const void* cos_sin, const void* pos,
                            long max_pos, int interleaved, void* stream) {
  if (head_dim != 128 || nseq < 0 || ntiles < 0 || tokens < 0 || max_seqs < 1) return 1;
  if (ROPE && !mx_rope_ok(cos_sin, pos, max_pos, interleaved)) return 1;
  if (!k || !v || !k4 || !kscale || !vt || !vscale || !vtail || !lens || !block_table || !seq_tab || !tiles)
    return 1;
  const int lgt = mx_page_lgt(page_tokens);
  if (!mx_pool_ok(num_pages, kv_heads, lgt, max_pages_per_seq)) return 1;
  if (nseq == 0 || tokens == 0) return 0;
  if (nseq > max_seqs || nseq > tokens || ntiles < nseq) return 1;
  if (tokens > 0x7fffffffL / kv_heads || max_seqs > 0x7fffffffL / kv_heads) return 1;
  const long cap = max_pages_per_seq * page_tokens;
  const long nthr = ntiles * kv_heads * 128 * 2, nblk = tokens * kv_heads * (128 / 32);
  if ((nthr + 255) / 256 > 0x7fffffffL || (nblk + 255) / 256 > 0x7fffffffL) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mx_append_vt_packed_kernel<128>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st,
                     (const _Float16*)v, (const _Float16*)vtail, (uint8_t*)vt, (uint8_t*)vscale,
                     (const int*)lens, (const int*)seq_tab, (const int*)tiles, nthr, (int)nseq, (int)max_seqs,
                     (int)kv_heads, tokens, (int)cap, (const int*)block_table, (int)max_pages_per_seq, lgt,
                     (int)num_pages);
  const dim3 kgrid((unsigned)((nblk + 255) / 256));
  if constexpr (ROPE) {
    auto kern = interleaved ? mx_append_k_packed_rope_kernel<128, true> : mx_append_k_packed_rope_kernel<128, false>;
    hipLaunchKernelGGL(kern, kgrid, dim3(256), 0, st, (const _Float16*)k, (const _Float16*)v,
                       (const _Float16*)k_mean, (uint8_t*)k4, (uint8_t*)kscale, (_Float16*)vtail,
                       (const int*)lens, (const int*)seq_tab, nblk, (int)nseq, (int)max_seqs, (int)kv_heads,
                       tokens, (int)cap, (const int*)block_table, (int)max_pages_per_seq, lgt, (int)num_pages,
                       (const float*)cos_sin, (const int*)pos, (int)max_pos);
  } else {
    hipLaunchKernelGGL(mx_append_k_packed_kernel<128>, kgrid, dim3(256), 0, st,
                       (const _Float16*)k, (const _Float16*)v, (const _Float16*)k_mean, (uint8_t*)k4,
                       (uint8_t*)kscale, (_Float16*)vtail, (const int*)lens, (const int*)seq_tab, nblk,
                       (int)nseq, (int)max_seqs, (int)kv_heads, tokens, (int)cap, (const int*)block_table,
                       (int)max_pages_per_seq, lgt, (int)num_pages);
  }
  hipLaunchKernelGGL(mx_append_len_packed_kernel, dim3((unsigned)((nseq + 255) / 256)), dim3(256), 0, st,
                     (int*)lens, (const int*)seq_tab, (int)nseq, (int)max_seqs, tokens, (int)cap);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int qattn_mxfp4_paged_append_packed(const void* k, const void* v, const void* k_mean, void* k4,
                                               void* kscale, void* vt, void* vscale, void* vtail,
                                               void* lens, const void* block_table, const void* seq_tab,
                                               const void* tiles, long nseq, long ntiles, long tokens,
                                               long max_seqs, long kv_heads, long num_pages,
                                               long page_tokens, long max_pages_per_seq, int head_dim,
                                               void* stream) {
  return mx_append_packed<false>(k, v, k_mean, k4, kscale, vt, vscale, vtail, lens, block_table, seq_tab, tiles,
                                 nseq, ntiles, tokens, max_seqs, kv_heads, num_pages, page_tokens,
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
// [nmember][2] on the device).  Partials and merge are the plain entry's.  It stands last: its kernels
// are emitted after every other one of this file.
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
// every packed token (0 outside a tree).  Partials and merge are the plain entry's.  It stands behind
// every older entry, as its kernel is emitted behind theirs.
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
  if (head_dim != 128 || tokens < 0 || heads < 0 || !mx_rope_ok(cos_sin, pos, max_pos, interleaved)) return 1;
  if (tokens == 0 || heads == 0) return 0;
  if (!x || !q4 || !scale || tokens > 0x7fffffffL / heads) return 1;
  const long nblk = tokens * heads * (128 / 32);
  auto kern = interleaved ? mx_quant_rows_rope_kernel<128, true> : mx_quant_rows_rope_kernel<128, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const _Float16*)x, (uint8_t*)q4, (uint8_t*)scale, (const float*)cos_sin, (const int*)pos,
                     nblk, (int)heads, (int)max_pos);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int qattn_mxfp4_paged_append_packed_rope(
    const void* k, const void* v, const void* k_mean, void* k4, void* kscale, void* vt, void* vscale,
    void* vtail, void* lens, const void* block_table, const void* seq_tab, const void* tiles, long nseq,
    long ntiles, long tokens, long max_seqs, long kv_heads, long num_pages, long page_tokens,
    long max_pages_per_seq, int head_dim, const void* cos_sin, const void* pos, long max_pos, int interleaved,
    void* stream) {
  return mx_append_packed<true>(k, v, k_mean, k4, kscale, vt, vscale, vtail, lens, block_table, seq_tab, tiles,
                                nseq, ntiles, tokens, max_seqs, kv_heads, num_pages, page_tokens,
                                max_pages_per_seq, head_dim, cos_sin, pos, max_pos, interleaved, stream);
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
// (A template over the tile's keys, so that it is emitted where it is first used, behind every older kernel.)
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

// The merge of the step: entry i owns the partial rows [i * splits * Hq, (i + 1) * splits * Hq), laid out
// [split][query head] (one query: the virtual head order is the head order), so nothing but ns is read from
// the record and every address lies inside the partials.  mx_merge_row over the entry's ns splits, the
// arithmetic of mxfp4_varlen_combine_kernel in its order; an entry with ns < 1 (padding) gets O = 0 and lse =
// -inf.
template <int D>
__global__ __launch_bounds__(256) void mxfp4_decode_step_combine_kernel(const float* __restrict__ opart,
                                                                        const float2* __restrict__ ml,
                                                                        _Float16* __restrict__ out,
                                                                        float* __restrict__ lse,
                                                                        const int* __restrict__ seq_rec, long rows,
                                                                        int Hq, int splits) {
  constexpr int TPR = D / 8;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid / TPR;
  if (row >= rows) return;
  const int c = (int)(gid % TPR);
  const long token = row / Hq;
  const int ns = min(seq_rec[8 * token + 3], splits);
  if (ns < 1) {
    *reinterpret_cast<v8h*>(out + row * D + 8 * c) = v8h{};
    if (c == 0) lse[row] = -INFINITY;
    return;
  }
  mx_merge_row<D>(opart, ml, token * splits * Hq + row % Hq, Hq, ns, c, out + row * D, lse + row);
}
}  // namespace qattn

// window 0: none (then sinks must be 0); the kernels' 32-bit edges as in mx_varlen_call
static bool mx_step_window_ok(long window, long sinks) {
  return window >= 0 && sinks >= 0 && (window > 0 || sinks == 0);
}

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

// The attention of the step over its fixed grid (kernel: mxfp4_attn_split_kernel STEP): n entries x splits
// work records x kv_heads workgroups, causal, with the window's instantiation for window >= 1.  seq_rec is
// mx_decode_plan_kernel's, work i32 [n * splits][4] = {i, 0, s, 0} in any order; the partials hold n * splits
// * kv_heads * group rows.  It stands behind every older entry, as its kernels are emitted behind theirs.
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
  const int rc = mx_varlen_call(c, q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work,
                                n, n * splits, n, n * splits * kv_heads * group, max_seqs, kv_heads, group,
                                num_pages, page_tokens, max_pages_per_seq, 2, keys_per_split, head_dim, qks,
                                window, sinks, nullptr);
  if (rc >= 0) return rc;
  return window < 1 ? mx_split_launch<true, true, true, true, false, false, false, true>(c, stream)
                    : mx_split_launch<true, true, true, true, true, false, false, true>(c, stream);
}

extern "C" int qattn_mxfp4_decode_step_combine(const void* opart, const void* ml, void* out, void* lse,
                                               const void* seq_rec, long n, long splits, long q_heads,
                                               long kv_heads, int head_dim, void* stream) {
  if (head_dim != 128 || n < 0 || splits < 1 || splits > 65535) return 1;
  if (kv_heads < 1 || q_heads < 1 || q_heads % kv_heads != 0 || q_heads > 0x7fffffffL) return 1;
  if (n > 0x7fffffffL / (splits * q_heads)) return 1;
  if (n == 0) return 0;
  if (!opart || !ml || !out || !lse || !seq_rec) return 1;
  const long rows = n * q_heads, nthr = rows * (128 / 8);
  hipLaunchKernelGGL(mxfp4_decode_step_combine_kernel<128>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)opart, (const float2*)ml, (_Float16*)out, (float*)lse,
                     (const int*)seq_rec, rows, (int)q_heads, (int)splits);
  return hipGetLastError() == hipSuccess ? 0 : 2;
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
// u64 [n * K] the words the plan read; the partials hold n * splits * kv_heads * group * K rows.  It stands behind
// every older entry, as its kernels are emitted behind theirs.
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
