// The packed step and the decode step over the paged MX-FP4 cache at head_dim 256 (Gemma-2 / Gemma-3 layers): its
// ring, and the instantiations of what mxfp4_attn.h defines once for every head_dim (mxfp4_attn_packed_kernel and
// its host path mx_packed, the packed append, the quantisers and the two merges), which stand here because this
// file's flags are the ones they were measured with.  Format, tile body (mx_tile<256>), masks, partials and merge
// arithmetic are those of mxfp4_attn.hip at D = 256: NKS = 4 k-steps of S per 32-key half, NDB = 8 output blocks,
// 8 scale bytes per Q / K row, carried as one 64-bit word (MxCfg<256>::scale_t) of which k-step s, half h picks
// byte 2s + h.  What is this file's own is the tile schedule and the register budget.
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
// STEP is the fixed grid of the device-planned decode step: a surplus workgroup of mxfp4_attn_packed_kernel returns
// behind the two record reads, in front of this ring's constructor.
#include "mxfp4_attn.h"

namespace qattn {

struct MxRing256 {
  using C = MxCfg<256>;
  static_assert(C::K_BYTES == 8192 && C::V_BYTES == 8192 && C::KS_BYTES == 512 && C::VS_BYTES == 512 &&
                    C::SLOT == 17408, "tile image");
  static constexpr int SLOT = C::SLOT, TPS = 1;   // one tile per slot
  static constexpr bool TILE_IN_LOOP = true;
  static constexpr int IPW = 5;                   // VMEM ops of a wave per tile
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

template <bool STEP, bool SOFTCAP>
int mx256_packed(const MxSplitCall& c, int causal, long window, void* stream) {
  return mx_packed<MxRing256, STEP, SOFTCAP>(c, causal, window, stream);
}
template int mx256_packed<false, false>(const MxSplitCall&, int, long, void*);   // the packed step
template int mx256_packed<true, false>(const MxSplitCall&, int, long, void*);    // the decode step
template int mx256_packed<false, true>(const MxSplitCall&, int, long, void*);    // and the two with a cap
template int mx256_packed<true, true>(const MxSplitCall&, int, long, void*);

// the packed append, the two packed quantisers and the two merges at head_dim 256
QA_MX_WIDTH(, 256)

// qattn_mxfp4_quant_rows at head_dim 256, behind that entry's checks of mean and seq; nblk = rows * 8 >= 1
int mx256_quant_rows(const void* x, const void* mean, void* q4, void* scale, long nblk, long seq, void* stream) {
  if ((nblk + 255) / 256 > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(mx_quant_rows_kernel<256>, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const _Float16*)x, (const _Float16*)mean, (uint8_t*)q4, (uint8_t*)scale,
                     nblk, seq);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace qattn
