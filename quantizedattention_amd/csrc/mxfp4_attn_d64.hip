// The packed step over the paged MX-FP4 cache at head_dim 64, and the learned sink logit of the packed step's
// merge at both head dims.  Format, tile body (mx_tile<64>), masks, partials and merge are those of
// mxfp4_attn.hip (mxfp4_attn.h) at D = 64: NKS = 1 k-step of S per 32-key half, NDB = 2 output blocks, 2 scale
// bytes per Q / K row.  What is this file's own is the tile schedule.
//
// A 64-key tile at D = 64 is 2 KiB of K codes, 2 KiB of V^T codes and 128 B + 128 B of scales, half of the D =
// 128 tile for the same barrier and the same exp2 / pack work per score.  So a ring slot here holds TPS = 2
// consecutive tiles (the pair ring): 128 keys per barrier, the 8 one-KiB pieces per barrier of the D = 128 ring.
// LDS image of a slot: TPS images of MxCfg<64> one after the other (K | V^T | key scales | V scales, 4608 B
// each), so the tile body takes `slot + j * 4608` as it takes a slot of the one-tile ring.
// Piece plan of wave w per slot: piece w & 1 of K (w < 2) or of V^T (w >= 2) of tile 2i, the same piece of tile
// 2i + 1, and ONE scale block: the key (w < 2) or V (w >= 2) scales of tile 2i + (w & 1).  Three VMEM ops per
// wave and slot, as at one tile per slot (one piece, both scale blocks), so both rings wait with vmcnt(6).  A
// scale DMA moves 256 B for a 128-B block; lanes 32 .. 63 fetch the block again (into the unused half of the
// 256-B LDS block), so no byte past the tile's own scales is requested.
// A key run of an odd tile count leaves the last slot with one live tile: the dead half is fetched from the
// run's last tile (in bounds, never read).  Pages: every tile is fetched through the buffer resources of its own
// page, rebased when the ring enters it, so the two tiles of a slot may lie in two pages (always, at page_tokens
// = 64, or when a split starts on an odd tile); the table entry is read one page ahead per tile, as in
// MxPagedRing.
// Both schedules are built; -DQA_MX64_TPS=1 makes one tile per slot the default, and the environment variable
// QATTN_MX64_TPS (1 or 2, read at every launch) picks one for a process, which is how tools/time_decode_varlen.py
// --head-dim 64 measures the two side by side.
//
// STEP (causal, with or without WINDOW) is the fixed grid of the device-planned decode step (kv_cache_mxfp4.py
// DecodeStep, mxfp4_attn_split_kernel STEP at D = 128): `splits` work records {i, 0, s, 0} per entry i, the
// records seq_rec[i] written by mx_decode_plan_kernel from the device lengths.  A workgroup with s >= rec[3] =
// ns_i -- a padding entry (ns = 0, slot -1) or a sequence that needs fewer splits than the longest could --
// returns behind the two record reads: no length, no table entry (the ring's constructor reads one, so the exit
// stands in front of it), no DMA, no barrier, no store.  Every other workgroup is the instantiation without STEP
// statement for statement, so pair ring, page rebasing, the lone last tile, masks and the compact partials (at
// the fixed stride the plan writes into rec[4]) are the host-planned call's, and so are the bits.
#include "mxfp4_attn.h"

#include <cstdlib>

#ifndef QA_MX64_TPS
#define QA_MX64_TPS 2   // 64-key tiles per ring slot: 2 (the pair ring) or 1
#endif

namespace qattn {

template <int TPS>
struct MxRing64 {
  using C = MxCfg<64>;
  static_assert(TPS == 1 || TPS == 2, "one tile or a pair of tiles per slot");
  static_assert(C::K_BYTES == 2048 && C::V_BYTES == 2048 && C::KS_BYTES == 128 && C::VS_BYTES == 128, "tile image");
  static constexpr int SLOT = TPS * C::SLOT;
  static constexpr int IPW = 3;   // VMEM ops of a wave per slot
  typedef const __attribute__((address_space(4))) int* table_ptr;
  const uint8_t *base16, *ksbase, *vsbase;   // the wave's piece operand; TPS 2: ksbase is its scale operand
  unsigned voff16, loff16, voffsc, loffsc;
  int sctile;                                // TPS 2: the tile of the pair whose scale block the wave fetches
  v4u rs16, ks_rs, vs_rs;                    // of the page the ring is in (TPS 2: ks_rs is the wave's scale operand)
  table_ptr tbl;
  int npages, lgt, hkv, hd, npool, t0;
  int cur, next;   // the page index the ring is in and the table entry after it
  unsigned smem_lds;
  QA_DEVICE void rebase(int id) {
    const unsigned long first = ((unsigned)min(max(id, 0), npool - 1) * (unsigned)hkv + hd) << lgt;
    rs16 = make_rsrc(base16 + first * 2048, 2048u << lgt);
    ks_rs = make_rsrc(ksbase + first * 128, 128u << lgt);
    if constexpr (TPS == 1) vs_rs = make_rsrc(vsbase + first * 128, 128u << lgt);
  }
  QA_DEVICE MxRing64(const uint8_t* k4, const uint8_t* ks, const uint8_t* vt, const uint8_t* vs, const int* row,
                     int npages_, int lgt_, int hkv_, int hd_, int npool_, int t0_, const char* smem, int wave,
                     int lane)
      : tbl((table_ptr)(unsigned long)row), npages(npages_), lgt(lgt_), hkv(hkv_), hd(hd_), npool(npool_),
        t0(t0_) {
    const bool isv = wave >= 2;
    base16 = isv ? vt : k4;
    voff16 = (wave & 1) * 1024 + 16 * lane;
    loff16 = (isv ? C::VOFF : C::KOFF) + (wave & 1) * 1024;
    ksbase = TPS == 2 && isv ? vs : ks;
    vsbase = vs;
    loffsc = TPS == 2 && isv ? C::VSOFF : C::KSOFF;
    voffsc = 4 * (lane & 31);
    sctile = wave & 1;
    cur = t0 >> lgt;
    rebase(tbl[cur]);
    next = tbl[min(cur + 1, npages - 1)];
    smem_lds = lds_addr(smem);
  }
  // the ring moves to the page of tile g, which is the page it is in or the one after; the entry behind it is
  // loaded every time, without a branch (MxPagedRing::issue)
  QA_DEVICE void enter(int g) {
    if ((g >> lgt) != cur) {
      cur = g >> lgt;
      rebase(next);
    }
    next = tbl[min(cur + 1, npages - 1)];
  }
  // tiles min(TPS * p + j, ntw - 1), j < TPS, of the wave's run into slot p & 3; after every tile the ring
  // enters the page of the next one, so a rebase stands behind the DMA it follows
  QA_DEVICE void issue(int p, int ntw) {
    const unsigned slot = smem_lds + (p & 3) * SLOT;
#pragma unroll
    for (int j = 0; j < TPS; ++j) {
      const unsigned in = (t0 + min(TPS * p + j, ntw - 1)) & ((1 << lgt) - 1);
      const unsigned sl = slot + j * C::SLOT;
      dma16_buf(rs16, voff16, in * 2048u, sl + loff16);
      if constexpr (TPS == 1) {
        dma4_buf(ks_rs, voffsc, in * 128u, sl + C::KSOFF);
        dma4_buf(vs_rs, voffsc, in * 128u, sl + C::VSOFF);
      } else if (j == sctile) {   // wave-uniform
        dma4_buf(ks_rs, voffsc, in * 128u, sl + loffsc);
      }
      enter(t0 + min(TPS * p + j + 1, ntw - 1));
    }
  }
  QA_DEVICE void prologue(int ntw) {
#pragma unroll
    for (int i = 0; i < C::NSLOT - 1; ++i) issue(i, ntw);
  }
};

// mxfp4_attn_split_kernel's VARLEN instantiation (and, WINDOW, its windowed one) at D = 64: the work and
// sequence records, the row mapping, the tile range of a split, the masks, the skipped tiles, the empty state
// and the compact partials are that kernel's, statement for statement; the ring is MxRing64<TPS>, and one
// barrier publishes TPS tiles, which the wave runs through mx_tile<64> one after the other.
template <bool CAUSAL, bool WINDOW, int TPS, bool STEP = false, bool SOFTCAP = false>
__global__ __launch_bounds__(256, QA_MX_OCC) void mxfp4_attn_varlen64_kernel(
    const uint8_t* __restrict__ q4, const uint8_t* __restrict__ qs, const uint8_t* __restrict__ k4,
    const uint8_t* __restrict__ ks, const uint8_t* __restrict__ vt, const uint8_t* __restrict__ vs,
    float* __restrict__ opart, float2* __restrict__ ml, int BHV, int Sk, int kps, float qks,
    const int* __restrict__ lens, int hps, const int* __restrict__ btab, int mpp, int lgt, int npool,
    MxVarlen vl) {
  constexpr int D = 64;
  using C = MxCfg<D>;
  using R = MxRing64<TPS>;
  static_assert(CAUSAL || !WINDOW, "a window is causal");
  static_assert(CAUSAL || !STEP, "the fixed grid is the causal packed step's");
  static_assert(C::WAVES * RowTile<D, float, 2>::BYTES <= C::NSLOT * R::SLOT, "fp32 staging in two passes fits the ring");
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
  const unsigned qsw = mx_load_q<D>(q4, qs, qrow, h, qf);

  v16f o[C::NDB];
#pragma unroll
  for (int b = 0; b < C::NDB; ++b) o[b] = v16f{};
  float m = -INFINITY, l = 0.f;

  // tile t of the run, landed at sl (the masks and the skips of mxfp4_attn_split_kernel)
  const auto tile = [&](int t, const char* sl) {
    const int k0 = C::KT * (t0 + t);
    bool diag;
    int lim, lo = 0, slim = 0;
    if constexpr (CAUSAL) {
      if (k0 > wmax + qoff) return;             // no row of the wave sees the tile: m, l, O unchanged
      diag = k0 + C::KT - 1 > wmin + qoff;
      lim = pos + qoff - k0 - 4 * h;
      if constexpr (WINDOW) {
        // the tile lies below every row's window and holds no sink key: skipped like the one above
        if (k0 + C::KT - 1 < wmin + qoff - vl.window + 1 && k0 >= vl.sinks) return;
        // some row's lower edge cuts the tile (the highest edge is the last row's), unless it is all sinks
        diag = diag || (k0 < wmax + qoff - vl.window + 1 && k0 + C::KT > vl.sinks);
        lo = pos + qoff - vl.window + 1 - k0 - 4 * h;
        slim = vl.sinks - 1 - k0 - 4 * h;
      }
    } else {   // every row sees the keys <= len - 1
      diag = k0 + C::KT > len;
      lim = len - 1 - k0 - 4 * h;
    }
    mx_tile<D, true, WINDOW, false, SOFTCAP>(sl, qf, qsw, o, m, l, diag, lim, qks, lane, h, c32, lo, slim, 0, 0,
                                             vl.cap_c1, vl.cap_c);
  };

  vmem_drain();
  __syncthreads();
  const int np = (ntw + TPS - 1) / TPS;
  for (int p = 0; p < np; ++p) {
    ring_wait_barrier<2 * R::IPW>();   // slot p landed (p + 1, p + 2 may be in flight); slot (p + 3) & 3 is free
    ring.issue(p + 3, ntw);
    if (!active) continue;   // a wave without rows keeps its share of the DMA and the barrier
    const char* sl = smem + (p & 3) * R::SLOT;
    tile(TPS * p, sl);
    if constexpr (TPS == 2) {
      if (2 * p + 1 < ntw) tile(2 * p + 1, sl + C::SLOT);   // an odd run: the last slot holds one live tile
    }
  }
  vmcnt_wait_all();
  __syncthreads();
  if (!active) return;
  if (h == 0 && c32 < nr) ml[row0 + c32] = make_float2(m, l);
  store_rows<D, float, 2, false, true>(o, 1.0f, smem + wave * RowTile<D, float, 2>::BYTES, opart + row0 * D, lane,
                                       0.f, nr);
}

// mxfp4_varlen_combine_kernel with the learned sink logit of the row's query head (mx_merge_row SINK)
template <int D>
__global__ __launch_bounds__(256) void mxfp4_varlen_combine_sink_kernel(
    const float* __restrict__ opart, const float2* __restrict__ ml, _Float16* __restrict__ out,
    float* __restrict__ lse, const int* __restrict__ seq_rec, const float* __restrict__ sink, int nseq, long rows,
    int Hq, int Hkv, long part_rows) {
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
  mx_merge_row<D, true>(opart, ml, first, step, nsplit, (int)(gid % TPR), out + row * D, lse + row, sink[head]);
}

template <bool CAUSAL, bool WINDOW, int TPS, bool STEP, bool SOFTCAP>
static int mx64_launch_tps(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                       const void* vscale, void* opart, void* ml, int bhv, int Sk, int kps, float qks,
                       const void* lens, int hps, const void* btab, int mpp, int lgt, int npool, const MxVarlen& vl,
                       unsigned grid, void* stream) {
  const auto kernel = mxfp4_attn_varlen64_kernel<CAUSAL, WINDOW, TPS, STEP, SOFTCAP>;
  const int lds = MxCfg<64>::NSLOT * MxRing64<TPS>::SLOT;
  { static LdsGrant granted_; if (!lds_grant((const void*)kernel, lds, granted_)) return 1; }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, (const uint8_t*)q4,
                     (const uint8_t*)qscale, (const uint8_t*)k4, (const uint8_t*)kscale, (const uint8_t*)vt,
                     (const uint8_t*)vscale, (float*)opart, (float2*)ml, bhv, Sk, kps, qks, (const int*)lens, hps,
                     (const int*)btab, mpp, lgt, npool, vl);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// tiles per slot of this launch: QATTN_MX64_TPS when it is 1 or 2, else the build's default
static int mx64_tps() {
  const char* e = std::getenv("QATTN_MX64_TPS");
  return e && (e[0] == '1' || e[0] == '2') && !e[1] ? e[0] - '0' : QA_MX64_TPS;
}

template <bool CAUSAL, bool WINDOW, bool STEP, bool SOFTCAP, class... A>
static int mx64_launch(A... a) {
  return mx64_tps() == 2 ? mx64_launch_tps<CAUSAL, WINDOW, 2, STEP, SOFTCAP>(a...)
                         : mx64_launch_tps<CAUSAL, WINDOW, 1, STEP, SOFTCAP>(a...);
}

// the checks of mx_varlen_call (mxfp4_attn.hip) and the dispatch of mx_varlen_paged, at head_dim 64; STEP: the
// fixed grid of the decode step (causal); SOFTCAP: the capped tile body with its two constants
template <bool STEP, bool SOFTCAP = false>
static int mx64_packed(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
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
#define QA_MX64_ARGS q4, qscale, k4, kscale, vt, vscale, opart, ml, bhv, Sk, keys_per_split, qks, lens, \
                     (int)kv_heads, block_table, (int)max_pages_per_seq, lgt, (int)num_pages, vl, grid, stream
  if (window >= 1) return mx64_launch<true, true, STEP, SOFTCAP>(QA_MX64_ARGS);
  if constexpr (STEP) return mx64_launch<true, false, true, SOFTCAP>(QA_MX64_ARGS);
  else if (causal) return mx64_launch<true, false, false, SOFTCAP>(QA_MX64_ARGS);
  else return mx64_launch<false, false, false, SOFTCAP>(QA_MX64_ARGS);
#undef QA_MX64_ARGS
}

int mx64_varlen_paged(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                      const void* vscale, void* opart, void* ml, const void* lens, const void* block_table,
                      const void* seq_rec, const void* work, long nseq, long nwork, long tokens, long part_rows,
                      long max_seqs, long kv_heads, long group, long num_pages, long page_tokens,
                      long max_pages_per_seq, int causal, int keys_per_split, float qks, long window, long sinks,
                      void* stream) {
  return mx64_packed<false>(q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, nseq,
                            nwork, tokens, part_rows, max_seqs, kv_heads, group, num_pages, page_tokens,
                            max_pages_per_seq, causal, keys_per_split, qks, window, sinks, stream);
}

// The attention of the decode step at head_dim 64 (qattn_mxfp4_attn_fwd_decode_step, which has checked n, splits
// and the products below): the packed call at nseq = tokens = n one-token sequences, n * splits work records and
// n * splits * kv_heads * group partial rows, causal, over the STEP instantiations.
int mx64_decode_step(const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                     const void* vscale, void* opart, void* ml, const void* lens, const void* block_table,
                     const void* seq_rec, const void* work, long n, long splits, long max_seqs, long kv_heads,
                     long group, long num_pages, long page_tokens, long max_pages_per_seq, int keys_per_split,
                     float qks, long window, long sinks, void* stream) {
  return mx64_packed<true>(q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, n,
                           n * splits, n, n * splits * kv_heads * group, max_seqs, kv_heads, group, num_pages,
                           page_tokens, max_pages_per_seq, 2, keys_per_split, qks, window, sinks, stream);
}

// mx_append_packed (mxfp4_attn.hip) at head_dim 64: the same checks, the same three launches
int mx64_append_packed(bool rope, const void* k, const void* v, const void* k_mean, void* k4, void* kscale,
                       void* vt, void* vscale, void* vtail, void* lens, const void* block_table,
                       const void* seq_tab, const void* tiles, long nseq, long ntiles, long tokens, long max_seqs,
                       long kv_heads, long num_pages, long page_tokens, long max_pages_per_seq,
                       const void* cos_sin, const void* pos, long max_pos, int interleaved, void* stream) {
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
  const long nthr = ntiles * kv_heads * 64 * 2, nblk = tokens * kv_heads * (64 / 32);
  if ((nthr + 255) / 256 > 0x7fffffffL || (nblk + 255) / 256 > 0x7fffffffL) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mx_append_vt_packed_kernel<64>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st,
                     (const _Float16*)v, (const _Float16*)vtail, (uint8_t*)vt, (uint8_t*)vscale,
                     (const int*)lens, (const int*)seq_tab, (const int*)tiles, nthr, (int)nseq, (int)max_seqs,
                     (int)kv_heads, tokens, (int)cap, (const int*)block_table, (int)max_pages_per_seq, lgt,
                     (int)num_pages);
  const dim3 kgrid((unsigned)((nblk + 255) / 256));
  if (rope) {
    auto kern = interleaved ? mx_append_k_packed_rope_kernel<64, true> : mx_append_k_packed_rope_kernel<64, false>;
    hipLaunchKernelGGL(kern, kgrid, dim3(256), 0, st, (const _Float16*)k, (const _Float16*)v,
                       (const _Float16*)k_mean, (uint8_t*)k4, (uint8_t*)kscale, (_Float16*)vtail,
                       (const int*)lens, (const int*)seq_tab, nblk, (int)nseq, (int)max_seqs, (int)kv_heads,
                       tokens, (int)cap, (const int*)block_table, (int)max_pages_per_seq, lgt, (int)num_pages,
                       (const float*)cos_sin, (const int*)pos, (int)max_pos);
  } else {
    hipLaunchKernelGGL(mx_append_k_packed_kernel<64>, kgrid, dim3(256), 0, st,
                       (const _Float16*)k, (const _Float16*)v, (const _Float16*)k_mean, (uint8_t*)k4,
                       (uint8_t*)kscale, (_Float16*)vtail, (const int*)lens, (const int*)seq_tab, nblk,
                       (int)nseq, (int)max_seqs, (int)kv_heads, tokens, (int)cap, (const int*)block_table,
                       (int)max_pages_per_seq, lgt, (int)num_pages);
  }
  hipLaunchKernelGGL(mx_append_len_packed_kernel, dim3((unsigned)((nseq + 255) / 256)), dim3(256), 0, st,
                     (int*)lens, (const int*)seq_tab, (int)nseq, (int)max_seqs, tokens, (int)cap);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int mx64_quant_rows_rope(const void* x, void* q4, void* scale, const void* cos_sin, const void* pos, long tokens,
                         long heads, long max_pos, int interleaved, void* stream) {
  if (tokens < 0 || heads < 0 || !mx_rope_ok(cos_sin, pos, max_pos, interleaved)) return 1;
  if (tokens == 0 || heads == 0) return 0;
  if (!x || !q4 || !scale || tokens > 0x7fffffffL / heads) return 1;
  const long nblk = tokens * heads * (64 / 32);
  auto kern = interleaved ? mx_quant_rows_rope_kernel<64, true> : mx_quant_rows_rope_kernel<64, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const _Float16*)x, (uint8_t*)q4, (uint8_t*)scale, (const float*)cos_sin, (const int*)pos,
                     nblk, (int)heads, (int)max_pos);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

template <int D>
static void mx_combine_ext_launch(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                                  const void* sink, long nseq, long rows, long q_heads, long kv_heads,
                                  long part_rows, void* stream) {
  const dim3 grid((unsigned)((rows * (D / 8) + 255) / 256));
  if (sink)
    hipLaunchKernelGGL(mxfp4_varlen_combine_sink_kernel<D>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const float*)opart, (const float2*)ml, (_Float16*)out, (float*)lse, (const int*)seq_rec,
                       (const float*)sink, (int)nseq, rows, (int)q_heads, (int)kv_heads, part_rows);
  else
    hipLaunchKernelGGL(mxfp4_varlen_combine_kernel<D>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const float*)opart, (const float2*)ml, (_Float16*)out, (float*)lse, (const int*)seq_rec,
                       (int)nseq, rows, (int)q_heads, (int)kv_heads, part_rows);
}

int mx_varlen_combine_ext(const void* opart, const void* ml, void* out, void* lse, const void* seq_rec,
                          const void* sink_logit, long nseq, long tokens, long q_heads, long kv_heads,
                          long part_rows, int head_dim, void* stream) {
  if ((head_dim != 64 && head_dim != 128) || nseq < 0 || tokens < 0 || part_rows < 0 || !seq_rec) return 1;
  if (head_dim == 128 && !sink_logit) return 1;   // that call is qattn_mxfp4_varlen_combine's own
  if (kv_heads < 1 || q_heads < 1 || q_heads % kv_heads != 0 || q_heads > 0x7fffffffL) return 1;
  if (nseq == 0 || tokens == 0) return 0;
  if (nseq > tokens || part_rows < 1) return 1;
  if (tokens > 0x7fffffffL / q_heads || part_rows > 0x7fffffffL) return 1;
  if (head_dim == 64)
    mx_combine_ext_launch<64>(opart, ml, out, lse, seq_rec, sink_logit, nseq, tokens * q_heads, q_heads, kv_heads,
                              part_rows, stream);
  else
    mx_combine_ext_launch<128>(opart, ml, out, lse, seq_rec, sink_logit, nseq, tokens * q_heads, q_heads,
                               kv_heads, part_rows, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The capped packed call (step false: the arguments of mx64_varlen_paged) and the capped decode step (step true:
// those that mx64_decode_step hands to mx64_packed) at head_dim 64, for the entries of mxfp4_attn_softcap.hip.  It
// stands last: its kernels are emitted behind every older one.
int mx64_softcap(bool step, const void* q4, const void* qscale, const void* k4, const void* kscale, const void* vt,
                 const void* vscale, void* opart, void* ml, const void* lens, const void* block_table,
                 const void* seq_rec, const void* work, long nseq, long nwork, long tokens, long part_rows,
                 long max_seqs, long kv_heads, long group, long num_pages, long page_tokens, long max_pages_per_seq,
                 int causal, int keys_per_split, long window, long sinks, float cap_c1, float cap_c, void* stream) {
#define QA_MX64_CAP q4, qscale, k4, kscale, vt, vscale, opart, ml, lens, block_table, seq_rec, work, nseq, nwork, \
                    tokens, part_rows, max_seqs, kv_heads, group, num_pages, page_tokens, max_pages_per_seq,      \
                    causal, keys_per_split, 0.f, window, sinks, stream, cap_c1, cap_c
  return step ? mx64_packed<true, true>(QA_MX64_CAP) : mx64_packed<false, true>(QA_MX64_CAP);
#undef QA_MX64_CAP
}

}  // namespace qattn

// qattn_mxfp4_varlen_combine with a learned sink logit per query head (sink_logit f32 [q_heads] on the device,
// natural-log units; mx_merge_row SINK): lse covers the visible keys and the sink
extern "C" int qattn_mxfp4_varlen_combine_sink(const void* opart, const void* ml, void* out, void* lse,
                                               const void* seq_rec, const void* sink_logit, long nseq,
                                               long tokens, long q_heads, long kv_heads, long part_rows,
                                               int head_dim, void* stream) {
  if (!sink_logit) return 1;
  if (head_dim == 256)   // mxfp4_attn_d256.hip
    return qattn::mx256_varlen_combine(opart, ml, out, lse, seq_rec, sink_logit, nseq, tokens, q_heads, kv_heads,
                                       part_rows, stream);
  return qattn::mx_varlen_combine_ext(opart, ml, out, lse, seq_rec, sink_logit, nseq, tokens, q_heads, kv_heads,
                                      part_rows, head_dim, stream);
}
