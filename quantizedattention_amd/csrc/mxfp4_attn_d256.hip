// The packed step and the decode step over the paged MX-FP4 cache at head_dim 256 (Gemma-2 / Gemma-3 layers).
// Format, tile body (mx_tile<256>), masks, partials and merge arithmetic are those of mxfp4_attn.hip
// (mxfp4_attn.h) at D = 256: NKS = 4 k-steps of S per 32-key half, NDB = 8 output blocks, 8 scale bytes per Q /
// K row, carried as one 64-bit word (MxCfg<256>::scale_t) of which k-step s, half h picks byte 2s + h.  What is
// this file's own is the tile schedule and the register budget.
//
// A 64-key tile at D = 256 is 8 KiB of K codes, 8 KiB of V^T codes and 512 B + 512 B of scales, twice the D = 128
// tile for the same barrier.  LDS image of a slot (MxCfg<256>): K | V^T | key scales | V scales, 17 KiB; the ring
// has four slots, 68 KiB, so two workgroups of a CU share its 160 KiB.  (Three slots would admit a third
// workgroup by LDS, but the register budget below holds a SIMD to two waves, and the fp32 staging of the final
// store, 66 KiB in two passes, would no longer fit the ring.)
// Piece plan of wave w per tile: the 1-KiB pieces w and w + 4 of K, the same two of V^T, and ONE 256-B scale
// block: the low (w & 1 = 0) or high half of the key scales (w < 2) or of the V scales (w >= 2).  Five VMEM ops
// per wave and tile, so the ring waits with vmcnt(2 * 5); one barrier per tile.  Every byte of the tile is
// requested exactly once.  Pages: one tile per slot, fetched through buffer resources that cover the head's
// part of the page the ring is in and are rebased when it enters the next one; the table entry is read one page
// ahead, as in MxPagedRing.
//
// Registers: the output accumulator is 8 x 16 = 128 fp32 per lane, the Q fragments 16, S and P 64 more while
// live; __launch_bounds__(256, QA_MX_OCC) gives the 256 registers of two waves per SIMD, which every
// instantiation holds without scratch (DESIGN.md has the figures of each).
//
// STEP is the fixed grid of the device-planned decode step, as in mxfp4_attn_varlen64_kernel: a surplus
// workgroup returns behind the two record reads, in front of the ring's constructor; every other workgroup is
// the instantiation without STEP statement for statement.
#include "mxfp4_attn.h"

namespace qattn {

struct MxRing256 {
  using C = MxCfg<256>;
  static_assert(C::K_BYTES == 8192 && C::V_BYTES == 8192 && C::KS_BYTES == 512 && C::VS_BYTES == 512 &&
                    C::SLOT == 17408, "tile image");
  static constexpr int IPW = 5;   // VMEM ops of a wave per tile
  typedef const __attribute__((address_space(4))) int* table_ptr;
  const uint8_t *kbase, *vbase, *scbase;   // scbase: the operand of the wave's scale block
  unsigned voff16[2], loff16[2], voffsc, loffsc;
  v4u k_rs, v_rs, sc_rs;                   // of the page the ring is in
  table_ptr tbl;
  int npages, lgt, hkv, hd, npool, t0;
  int cur, next;   // the page index the ring is in and the table entry after it
  unsigned smem_lds;
  QA_DEVICE void rebase(int id) {
    const unsigned long first = ((unsigned)min(max(id, 0), npool - 1) * (unsigned)hkv + hd) << lgt;
    k_rs = make_rsrc(kbase + first * C::K_BYTES, (unsigned)C::K_BYTES << lgt);
    v_rs = make_rsrc(vbase + first * C::V_BYTES, (unsigned)C::V_BYTES << lgt);
    sc_rs = make_rsrc(scbase + first * C::KS_BYTES, (unsigned)C::KS_BYTES << lgt);
  }
  QA_DEVICE MxRing256(const uint8_t* k4, const uint8_t* ks, const uint8_t* vt, const uint8_t* vs, const int* row,
                      int npages_, int lgt_, int hkv_, int hd_, int npool_, int t0_, const char* smem, int wave,
                      int lane)
      : kbase(k4), vbase(vt), scbase(wave < 2 ? ks : vs), tbl((table_ptr)(unsigned long)row), npages(npages_),
        lgt(lgt_), hkv(hkv_), hd(hd_), npool(npool_), t0(t0_) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      loff16[i] = (wave + C::WAVES * i) * 1024;
      voff16[i] = loff16[i] + 16 * lane;
    }
    voffsc = (wave & 1) * 256 + 4 * lane;
    loffsc = (wave < 2 ? C::KSOFF : C::VSOFF) + (wave & 1) * 256;
    cur = t0 >> lgt;
    rebase(tbl[cur]);
    next = tbl[min(cur + 1, npages - 1)];
    smem_lds = lds_addr(smem);
  }
  // tile min(t, ntw - 1) of the wave's run into slot t & 3, from the page the ring is in; then the ring moves to
  // the page of the following issue, so the rebase stands behind the DMA (MxPagedRing::issue)
  QA_DEVICE void issue(int t, int ntw) {
    const unsigned slot = smem_lds + (t & 3) * C::SLOT;
    const unsigned in = (t0 + min(t, ntw - 1)) & ((1 << lgt) - 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      dma16_buf(k_rs, voff16[i], in * C::K_BYTES, slot + C::KOFF + loff16[i]);
      dma16_buf(v_rs, voff16[i], in * C::V_BYTES, slot + C::VOFF + loff16[i]);
    }
    dma4_buf(sc_rs, voffsc, in * C::KS_BYTES, slot + loffsc);
    const int g = t0 + min(t + 1, ntw - 1);
    if ((g >> lgt) != cur) {   // tiles advance one at a time: the page after cur
      cur = g >> lgt;
      rebase(next);
    }
    next = tbl[min(cur + 1, npages - 1)];   // every tile, without a branch (MxPagedRing::issue)
  }
  QA_DEVICE void prologue(int ntw) {
#pragma unroll
    for (int i = 0; i < C::NSLOT - 1; ++i) issue(i, ntw);
  }
};

// mxfp4_attn_varlen64_kernel at D = 256: the work and sequence records, the row mapping, the tile range of a
// split, the masks, the skipped tiles, the empty state and the compact partials are that kernel's, statement for
// statement; the ring is MxRing256 and one barrier publishes one tile.
template <bool CAUSAL, bool WINDOW, bool STEP = false, bool SOFTCAP = false>
__global__ __launch_bounds__(256, QA_MX_OCC) void mxfp4_attn_varlen256_kernel(
    const uint8_t* __restrict__ q4, const uint8_t* __restrict__ qs, const uint8_t* __restrict__ k4,
    const uint8_t* __restrict__ ks, const uint8_t* __restrict__ vt, const uint8_t* __restrict__ vs,
    float* __restrict__ opart, float2* __restrict__ ml, int BHV, int Sk, int kps, float qks,
    const int* __restrict__ lens, int hps, const int* __restrict__ btab, int mpp, int lgt, int npool,
    MxVarlen vl) {
  constexpr int D = 256;
  using C = MxCfg<D>;
  using R = MxRing256;
  static_assert(CAUSAL || !WINDOW, "a window is causal");
  static_assert(CAUSAL || !STEP, "the fixed grid is the causal packed step's");
  static_assert(C::WAVES * RowTile<D, float, 2>::BYTES <= C::NSLOT * C::SLOT, "fp32 staging in two passes fits the ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef const __attribute__((address_space(4))) int* table_ptr;
  const int hd = (int)(blockIdx.x % (unsigned)hps);
  const table_ptr w = (table_ptr)(unsigned long)(vl.work + 4L * (blockIdx.x / (unsigned)hps));
  const table_ptr rec = (table_ptr)(unsigned long)(vl.seq_rec + 8L * min(max(w[0], 0), vl.nseq - 1));
  if constexpr (STEP) {   // a surplus workgroup of the fixed grid: nothing fetched, nothing stored
    if (max(w[2], 0) >= rec[3]) return;
  }
  const int qt = max(w[1], 0), split = max(w[2], 0);
  const int bh = min(max(rec[0], 0), BHV / hps - 1) * hps + hd;
  const long qbase = rec[1], pbase = rec[4];
  const int sq_head = max(rec[2], 1);
  const int rows = vl.group * sq_head;
  const int wt0 = WINDOW ? max(rec[5], 0) : 0, nsink = WINDOW ? max(rec[6], 0) : 0;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, h = lane >> 5, c32 = lane & 31;
  const int q0 = qt * C::QROWS + wave * 32;
  const int qi = min(q0 + c32, rows - 1);
  const int len = min(__builtin_amdgcn_readfirstlane(lens[bh / hps]), Sk);   // never a tile past the capacity
  const int qoff = len - sq_head;
  const int nt = (len + C::KT - 1) / C::KT;
  const bool sink_run = WINDOW && nsink > 0 && split == 0;
  const int t0 = !WINDOW ? split * (kps / C::KT)
                         : sink_run ? 0
                                    : (int)min((long)wt0 + (long)(split - (nsink > 0)) * (kps / C::KT), (long)nt);
  const long row0 = pbase + ((long)split * hps + hd) * rows + q0;   // the wave's first row of opart / ml
  const int nr = min(32, rows - q0);
  // a wave without rows, or whose rows would pass the partials, stores nothing
  const bool active = q0 < rows && row0 >= 0 && row0 + nr <= vl.part_rows;
  if (t0 >= nt) {   // a split past the sequence: the empty state for the workgroup's rows
    if (!active) return;
    if (h == 0 && c32 < nr) ml[row0 + c32] = make_float2(-INFINITY, 0.f);
    v4f* dst = reinterpret_cast<v4f*>(opart + row0 * D);
#pragma unroll
    for (int i = 0; i < 32 * (D / 4) / 64; ++i)
      if (i * 64 + lane < nr * (D / 4)) dst[i * 64 + lane] = v4f{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const int ntw = sink_run ? min(nsink, nt) : min(nt - t0, kps / C::KT);
  // causal: query positions of the wave's rows (a wave that crosses a head boundary holds both ends)
  int wmin = 0, wmax = 0, pos = 0;
  if constexpr (CAUSAL) {
    const int p0 = q0 % sq_head;
    const bool wraps = p0 + nr > sq_head;
    wmin = wraps ? 0 : p0;
    wmax = wraps ? sq_head - 1 : p0 + nr - 1;
    pos = qi % sq_head;
  }

  R ring(k4, ks, vt, vs, btab + (long)(bh / hps) * mpp, (nt + (1 << lgt) - 1) >> lgt, lgt, hps, hd, npool, t0, smem,
         wave, lane);
  ring.prologue(ntw);

  v4i qf[C::NKS];
  const long qrow = min(max((qbase + qi % sq_head) * (vl.group * hps) + hd * vl.group + qi / sq_head, 0L),
                        vl.qrows - 1);
  const C::scale_t qsw = mx_load_q<D>(q4, qs, qrow, h, qf);

  v16f o[C::NDB];
#pragma unroll
  for (int b = 0; b < C::NDB; ++b) o[b] = v16f{};
  float m = -INFINITY, l = 0.f;

  vmem_drain();
  __syncthreads();
  for (int t = 0; t < ntw; ++t) {
    ring_wait_barrier<2 * R::IPW>();   // tile t landed (t + 1, t + 2 may be in flight); slot (t + 3) & 3 is free
    ring.issue(t + 3, ntw);
    if (!active) continue;   // a wave without rows keeps its share of the DMA and the barrier
    const int k0 = C::KT * (t0 + t);
    bool diag;
    int lim, lo = 0, slim = 0;
    if constexpr (CAUSAL) {
      if (k0 > wmax + qoff) continue;             // no row of the wave sees the tile: m, l, O unchanged
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
    } else {   // every row sees the keys <= len - 1
      diag = k0 + C::KT > len;
      lim = len - 1 - k0 - 4 * h;
    }
    mx_tile<D, true, WINDOW, false, SOFTCAP>(smem + (t & 3) * C::SLOT, qf, qsw, o, m, l, diag, lim, qks, lane, h, c32,
                                             lo, slim, 0, 0, vl.cap_c1, vl.cap_c);
  }
  vmcnt_wait_all();
  __syncthreads();
  if (!active) return;
  if (h == 0 && c32 < nr) ml[row0 + c32] = make_float2(m, l);
  store_rows<D, float, 2, false, true>(o, 1.0f, smem + wave * RowTile<D, float, 2>::BYTES, opart + row0 * D, lane,
                                       0.f, nr);
}

// mxfp4_varlen_combine_kernel / mxfp4_varlen_combine_sink_kernel at D = 256 (mx_merge_row<256, SINK>; sink is
// read only with SINK)
template <bool SINK>
__global__ __launch_bounds__(256) void mxfp4_varlen_combine256_kernel(
    const float* __restrict__ opart, const float2* __restrict__ ml, _Float16* __restrict__ out,
    float* __restrict__ lse, const int* __restrict__ seq_rec, const float* __restrict__ sink, int nseq, long rows,
    int Hq, int Hkv, long part_rows) {
  constexpr int D = 256, TPR = D / 8;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid / TPR;
  if (row >= rows) return;
  const int token = (int)(row / Hq), head = (int)(row % Hq), G = Hq / Hkv;
  const int* rec = seq_rec + 8L * mx_find_seq(seq_rec, nseq, 8, 1, token);
  const int sq = max(rec[2], 1), nsplit = rec[3];
  const long rows_j = (long)G * sq, step = (long)Hkv * rows_j;
  const long first = rec[4] + (head / G) * rows_j + (long)(head % G) * sq + (token - rec[1]);
  if (nsplit < 1 || first < 0 || first + (nsplit - 1) * step >= part_rows) return;
  mx_merge_row<D, SINK>(opart, ml, first, step, nsplit, (int)(gid % TPR), out + row * D, lse + row,
                        SINK ? sink[head] : 0.f);
}

// mxfp4_decode_step_combine_kernel / mxfp4_decode_step_combine_sink_kernel at D = 256: entry i owns the partial
// rows [i * splits * Hq, (i + 1) * splits * Hq); an entry with ns < 1 (padding) gets O = 0 and lse = -inf
template <bool SINK>
__global__ __launch_bounds__(256) void mxfp4_decode_step_combine256_kernel(
    const float* __restrict__ opart, const float2* __restrict__ ml, _Float16* __restrict__ out,
    float* __restrict__ lse, const int* __restrict__ seq_rec, const float* __restrict__ sink, long rows, int Hq,
    int splits) {
  constexpr int D = 256, TPR = D / 8;
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
  mx_merge_row<D, SINK>(opart, ml, token * splits * Hq + row % Hq, Hq, ns, c, out + row * D, lse + row,
                        SINK ? sink[row % Hq] : 0.f);
}

template <bool CAUSAL, bool WINDOW, bool STEP, bool SOFTCAP>
static int mx256_launch(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                        const void* vscale, void* opart, void* ml, int bhv, int Sk, int kps, float qks,
                        const void* lens, int hps, const void* btab, int mpp, int lgt, int npool,
                        const MxVarlen& vl, unsigned grid, void* stream) {
  const auto kernel = mxfp4_attn_varlen256_kernel<CAUSAL, WINDOW, STEP, SOFTCAP>;
  const int lds = MxCfg<256>::NSLOT * MxCfg<256>::SLOT;
  { static LdsGrant granted_; if (!lds_grant((const void*)kernel, lds, granted_)) return 1; }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, (const uint8_t*)q4,
                     (const uint8_t*)qscale, (const uint8_t*)k4, (const uint8_t*)kscale, (const uint8_t*)vt,
                     (const uint8_t*)vscale, (float*)opart, (float2*)ml, bhv, Sk, kps, qks, (const int*)lens, hps,
                     (const int*)btab, mpp, lgt, npool, vl);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// the checks of mx64_packed (mxfp4_attn_d64.hip) and its dispatch, at head_dim 256; STEP: the fixed grid of the
// decode step (causal); SOFTCAP: the capped tile body with its two constants
template <bool STEP, bool SOFTCAP = false>
static int mx256_packed(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                        const void* vscale, void* opart, void* ml, const void* lens, const void* block_table,
                        const void* seq_rec, const void* work, long nseq, long nwork, long tokens, long part_rows,
                        long max_seqs, long kv_heads, long group, long num_pages, long page_tokens,
                        long max_pages_per_seq, int causal, int keys_per_split, float qks, long window, long sinks,
                        void* stream, float cap_c1 = 0.f, float cap_c = 0.f) {
  if (keys_per_split < 64 || keys_per_split % 64 != 0) return 1;
  if (nseq < 0 || nwork < 0 || tokens < 0 || part_rows < 0) return 1;
  if (!lens || !block_table || !seq_rec || !work) return 1;
  const int lgt = mx_page_lgt(page_tokens);
  if (!mx_pool_ok(num_pages, kv_heads, lgt, max_pages_per_seq)) return 1;
  if (max_seqs < 1 || group < 1 || group > 0x7fffffffL || (causal != 0 && causal != 2)) return 1;
  if (nseq == 0 || nwork == 0 || tokens == 0) return 0;
  if (nseq > max_seqs || nseq > tokens || part_rows < 1) return 1;
  if (tokens > 0x7fffffffL / (group * kv_heads) || part_rows > 0x7fffffffL) return 1;
  if (nwork > 0x7fffffffL / kv_heads || max_seqs > 0x7fffffffL / kv_heads) return 1;
  const long big = 1L << 26;
  const MxVarlen vl{(const int*)work, (const int*)seq_rec, (int)nseq, (int)group, tokens * group * kv_heads,
                    part_rows, (int)(window < big ? window : big), (int)(sinks < big ? sinks : big),
                    nullptr, nullptr, 0, 0, nullptr, tokens, cap_c1, cap_c};
  const int bhv = (int)(max_seqs * kv_heads), Sk = (int)(max_pages_per_seq * page_tokens);
  const unsigned grid = (unsigned)(nwork * kv_heads);
#define QA_MX256_ARGS q4, qscale, k4, kscale, vt, vscale, opart, ml, bhv, Sk, keys_per_split, qks, lens, \
                      (int)kv_heads, block_table, (int)max_pages_per_seq, lgt, (int)num_pages, vl, grid, stream
  if (window >= 1) return mx256_launch<true, true, STEP, SOFTCAP>(QA_MX256_ARGS);
  if constexpr (STEP) return mx256_launch<true, false, true, SOFTCAP>(QA_MX256_ARGS);
  else if (causal) return mx256_launch<true, false, false, SOFTCAP>(QA_MX256_ARGS);
  else return mx256_launch<false, false, false, SOFTCAP>(QA_MX256_ARGS);
#undef QA_MX256_ARGS
}

int mx256_varlen_paged(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                       const void* vscale, void* opart, void* ml, const void* lens, const void* block_table,
                       const void* seq_rec, const void* work, long nseq, long nwork, long tokens, long part_rows,
                       long max_seqs, long kv_heads, long group, long num_pages, long page_tokens,
                       long max_pages_per_seq, int causal, int keys_per_split, float qks, long window, long sinks,
                       void* stream) {
  return mx256_packed<false>(q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, nseq,
                             nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages, page_tokens,
                             max_pages_per_seq, causal, keys_per_split, qks, window, sinks, stream);
}

// The attention of the decode step at head_dim 256 (qattn_mxfp4_attn_fwd_decode_step, which has checked n, splits
// and the products below): the packed call at nseq = tokens = n one-token sequences, n * splits work records and
// n * splits * kv_heads * group partial rows, causal, over the STEP instantiations.
int mx256_decode_step(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                      const void* vscale, void* opart, void* ml, const void* lens, const void* block_table,
                      const void* seq_rec, const void* work, long n, long splits, long max_seqs, long kv_heads,
                      long group, long num_pages, long page_tokens, long max_pages_per_seq, int keys_per_split,
                      float qks, long window, long sinks, void* stream) {
  return mx256_packed<true>(q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, n,
                            n * splits, n, n * splits * kv_heads * group, max_seqs, kv_heads, group, num_pages,
                            page_tokens, max_pages_per_seq, 2, keys_per_split, qks, window, sinks, stream);
}

// mx_append_packed (mxfp4_attn.hip) at head_dim 256: the same checks, the same three launches
int mx256_append_packed(bool rope, const void* k, const void* v, const void* k_mean, void* k4, void* kscale,
                        void* vt, void* vscale, void* vtail, void* lens, const void* block_table,
                        const void* seq_tab, const void* tiles, long nseq, long ntiles, long tokens, long max_seqs,
                        long kv_heads, long num_pages, long page_tokens, long max_pages_per_seq,
                        const void* cos_sin, const void* pos, long max_pos, int interleaved, void* stream) {
  constexpr int D = 256;
  if (nseq < 0 || ntiles < 0 || tokens < 0 || max_seqs < 1) return 1;
  if (rope && !mx_rope_ok(cos_sin, pos, max_pos, interleaved)) return 1;
  if (!k || !v || !k4 || !kscale || !vt || !vscale || !vtail || !lens || !block_table || !seq_tab || !tiles)
    return 1;
  const int lgt = mx_page_lgt(page_tokens);
  if (!mx_pool_ok(num_pages, kv_heads, lgt, max_pages_per_seq)) return 1;
  if (nseq == 0 || tokens == 0) return 0;
  if (nseq > max_seqs || nseq > tokens || ntiles < nseq) return 1;
  if (tokens > 0x7fffffffL / kv_heads || max_seqs > 0x7fffffffL / kv_heads) return 1;
  const long cap = max_pages_per_seq * page_tokens;
  if (ntiles > 0x7fffffffL / kv_heads) return 1;
  const long nthr = ntiles * kv_heads * D * 2, nblk = tokens * kv_heads * (D / 32);
  if ((nthr + 255) / 256 > 0x7fffffffL || (nblk + 255) / 256 > 0x7fffffffL) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mx_append_vt_packed_kernel<D>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st,
                     (const _Float16*)v, (const _Float16*)vtail, (uint8_t*)vt, (uint8_t*)vscale,
                     (const int*)lens, (const int*)seq_tab, (const int*)tiles, nthr, (int)nseq, (int)max_seqs,
                     (int)kv_heads, tokens, (int)cap, (const int*)block_table, (int)max_pages_per_seq, lgt,
                     (int)num_pages);
  const dim3 kgrid((unsigned)((nblk + 255) / 256));
  if (rope) {
    auto kern = interleaved ? mx_append_k_packed_rope_kernel<D, true> : mx_append_k_packed_rope_kernel<D, false>;
    hipLaunchKernelGGL(kern, kgrid, dim3(256), 0, st, (const _Float16*)k, (const _Float16*)v,
                       (const _Float16*)k_mean, (uint8_t*)k4, (uint8_t*)kscale, (_Float16*)vtail,
                       (const int*)lens, (const int*)seq_tab, nblk, (int)nseq, (int)max_seqs, (int)kv_heads,
                       tokens, (int)cap, (const int*)block_table, (int)max_pages_per_seq, lgt, (int)num_pages,
                       (const float*)cos_sin, (const int*)pos, (int)max_pos);
  } else {
    hipLaunchKernelGGL(mx_append_k_packed_kernel<D>, kgrid, dim3(256), 0, st,
                       (const _Float16*)k, (const _Float16*)v, (const _Float16*)k_mean, (uint8_t*)k4,
                       (uint8_t*)kscale, (_Float16*)vtail, (const int*)lens, (const int*)seq_tab, nblk,
                       (int)nseq, (int)max_seqs, (int)kv_heads, tokens, (int)cap, (const int*)block_table,
                       (int)max_pages_per_seq, lgt, (int)num_pages);
  }
  hipLaunchKernelGGL(mx_append_len_packed_kernel, dim3((unsigned)((nseq + 255) / 256)), dim3(256), 0, st,
                     (int*)lens, (const int*)seq_tab, (int)nseq, (int)max_seqs, tokens, (int)cap);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// qattn_mxfp4_quant_rows at head_dim 256, behind that entry's checks of mean and seq; nblk = rows * 8 >= 1
int mx256_quant_rows(const void* x, const void* mean, void* q4, void* scale, long nblk, long seq, void* stream) {
  if ((nblk + 255) / 256 > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(mx_quant_rows_kernel<256>, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const _Float16*)x, (const _Float16*)mean, (uint8_t*)q4, (uint8_t*)scale,
                     nblk, seq);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int mx256_quant_rows_rope(const void* x, void* q4, void* scale, const void* cos_sin, const void* pos, long tokens,
                          long heads, long max_pos, int interleaved, void* stream) {
  if (tokens < 0 || heads < 0 || !mx_rope_ok(cos_sin, pos, max_pos, interleaved)) return 1;
  if (tokens == 0 || heads == 0) return 0;
  if (!x || !q4 || !scale || tokens > 0x7fffffffL / heads) return 1;
  const long nblk = tokens * heads * (256 / 32);
  if ((nblk + 255) / 256 > 0x7fffffffL) return 1;
  auto kern = interleaved ? mx_quant_rows_rope_kernel<256, true> : mx_quant_rows_rope_kernel<256, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const _Float16*)x, (uint8_t*)q4, (uint8_t*)scale, (const float*)cos_sin, (const int*)pos,
                     nblk, (int)heads, (int)max_pos);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// the packed step's merge at head_dim 256 with the checks of mx_varlen_combine_ext; sink_logit null: none
int mx256_varlen_combine(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                         const void* sink_logit, long nseq, long tokens, long q_heads, long kv_heads,
                         long part_rows, void* stream) {
  if (nseq < 0 || tokens < 0 || part_rows < 0 || !seq_rec) return 1;
  if (kv_heads < 1 || q_heads < 1 || q_heads % kv_heads != 0 || q_heads > 0x7fffffffL) return 1;
  if (nseq == 0 || tokens == 0) return 0;
  if (nseq > tokens || part_rows < 1) return 1;
  if (tokens > 0x7fffffffL / q_heads || part_rows > 0x7fffffffL) return 1;
  const long rows = tokens * q_heads;
  const auto kernel = sink_logit ? mxfp4_varlen_combine256_kernel<true> : mxfp4_varlen_combine256_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((rows * (256 / 8) + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)opart, (const float2*)ml, (_Float16*)out, (float*)lse, (const int*)seq_rec,
                     (const float*)sink_logit, (int)nseq, rows, (int)q_heads, (int)kv_heads, part_rows);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// the decode step's merge at head_dim 256, behind mx_step_combine_check (mxfp4_attn.hip); sink null: none
int mx256_step_combine(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                       const void* sink, long n, long splits, long q_heads, void* stream) {
  const long rows = n * q_heads;
  const auto kernel = sink ? mxfp4_decode_step_combine256_kernel<true> : mxfp4_decode_step_combine256_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((rows * (256 / 8) + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)opart, (const float2*)ml, (_Float16*)out, (float*)lse, (const int*)seq_rec,
                     (const float*)sink, rows, (int)q_heads, (int)splits);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// mx64_softcap (mxfp4_attn_d64.hip) at head_dim 256; it stands last, as its kernels are emitted behind every older one
int mx256_softcap(bool step, const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                  const void* vscale, void* opart, void* ml, const void* lens, const void* block_table,
                  const void* seq_rec, const void* work, long nseq, long nwork, long tokens, long part_rows,
                  long max_seqs, long kv_heads, long group, long num_pages, long page_tokens, long max_pages_per_seq,
                  int causal, int keys_per_split, long window, long sinks, float cap_c1, float cap_c, void* stream) {
#define QA_MX256_CAP q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, nseq, nwork, \
                     tokens, part_rows, max_seqs, kv_heads, group, num_pages, page_tokens, max_pages_per_seq,      \
                     causal, keys_per_split, 0.f, window, sinks, stream, cap_c1, cap_c
  return step ? mx256_packed<true, true>(QA_MX256_CAP) : mx256_packed<false, true>(QA_MX256_CAP);
#undef QA_MX256_CAP
}

}  // namespace qattn
