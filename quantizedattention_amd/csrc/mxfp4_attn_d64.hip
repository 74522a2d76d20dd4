// The packed step over the paged MX-FP4 cache at head_dim 64: its ring, and the instantiations of what
// mxfp4_attn.h defines once for every head_dim (mxfp4_attn_packed_kernel and its host path mx_packed, the packed
// append, the rope quantiser and the two merges), which stand here because this file's flags are the ones they
// were measured with.  Format, tile body (mx_tile<64>), masks, partials and merge are those of mxfp4_attn.hip at D
// = 64: NKS = 1 k-step of S per 32-key half, NDB = 2 output blocks, 2 scale bytes per Q / K row.  What is this
// file's own is the tile schedule.
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
// DecodeStep): the surplus workgroup's exit of mxfp4_attn_packed_kernel stands in front of this ring's constructor,
// which reads a table entry; every other workgroup is the instantiation without STEP, so pair ring, page
// rebasing, the lone last tile, masks and the compact partials are the host-planned call's, and so are the bits.
#include "mxfp4_attn.h"

#include <cstdlib>

#ifndef QA_MX64_TPS
#define QA_MX64_TPS 2   // 64-key tiles per ring slot: 2 (the pair ring) or 1
#endif

namespace qattn {

template <int TPS_>
struct MxRing64 {
  using C = MxCfg<64>;
  static constexpr int TPS = TPS_;   // 64-key tiles per slot
  static constexpr bool TILE_IN_LOOP = false;
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

// tiles per slot of this launch: QATTN_MX64_TPS when it is 1 or 2, else the build's default
static int mx64_tps() {
  const char* e = std::getenv("QATTN_MX64_TPS");
  return e && (e[0] == '1' || e[0] == '2') && !e[1] ? e[0] - '0' : QA_MX64_TPS;
}

template <bool STEP, bool SOFTCAP>
int mx64_packed(const MxSplitCall& c, int causal, long window, void* stream) {
  return mx64_tps() == 2 ? mx_packed<MxRing64<2>, STEP, SOFTCAP>(c, causal, window, stream)
                         : mx_packed<MxRing64<1>, STEP, SOFTCAP>(c, causal, window, stream);
}
template int mx64_packed<false, false>(const MxSplitCall&, int, long, void*);   // the packed step
template int mx64_packed<true, false>(const MxSplitCall&, int, long, void*);    // the decode step
template int mx64_packed<false, true>(const MxSplitCall&, int, long, void*);    // and the two with a cap
template int mx64_packed<true, true>(const MxSplitCall&, int, long, void*);

// the packed append, the two packed quantisers and the two merges at head_dim 64
QA_MX_WIDTH(, 64)

}  // namespace qattn
