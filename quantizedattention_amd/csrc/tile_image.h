// The LDS images of a 32-row operand tile (table: DESIGN.md "LDS tile images").  The writer is the
// LDS-DMA in 1-KiB pieces, lane-linear in LDS, with the XOR swizzle of a row's 16-B chunks applied to
// the source offset (dma_src); the readers are row_off (row reads) and tr_off / tr_load
// (ds_read_b64_tr_b16).  The static_asserts hold the two sides together for D = 64 and 128.
#pragma once
#include "common.h"

namespace qattn {

// A tile of ROWB-byte rows whose 16-B chunk c of row r lies at chunk slot c ^ SW::sw(r).
template <int ROWB_, typename SW>
struct TileImage {
  static constexpr int ROWB = ROWB_;       // bytes per row
  static constexpr int NCH = ROWB / 16;    // 16-B chunks per row
  static constexpr int RPP = 64 / NCH;     // rows per 1-KiB piece
  static constexpr int TILE = 32 * ROWB;   // bytes per 32-row tile
  static constexpr int NP = TILE / 1024;   // pieces per tile
  static constexpr int NDB = ROWB / 64;    // 32-wide blocks of 16-bit columns
  static_assert(RPP * ROWB == 1024, "a piece is whole rows, so it lands lane-linear in LDS");

  static QA_IMG int sw(int row) { return SW::sw(row); }
  static constexpr bool period(int n) {   // the swizzle does not change under row + n
    for (int row = 0; row < 32; ++row)
      if (SW::sw(row + n) != SW::sw(row)) return false;
    return true;
  }
  // Byte offset of a row's chunk / 16-bit column d under swizzle value sw (a region whose image
  // depends on the wave passes the one it chose): the reader's LDS position, and the writer's source.
  static QA_IMG int chunk_at(int row, int chunk, int sw) { return row * ROWB + 16 * (chunk ^ sw); }
  static QA_IMG int elem_at(int row, int d, int sw) { return chunk_at(row, d / 8, sw) + (d % 8) * 2; }

  // writer: lane's row in a piece (past NP: the next tile of a stage) and its source byte offset
  static QA_IMG int piece_row(int piece, int lane) { return piece * RPP + lane / NCH; }
  static QA_IMG int dma_src(int piece, int lane) { return row_off(piece_row(piece, lane), lane % NCH); }
  // reader by rows: chunk 2s + h of row l & 31 is lane l's operand of k-step s
  static QA_IMG int row_off(int row, int chunk) { return chunk_at(row, chunk, SW::sw(row)); }

  // reader, transposed: lane 32h + l addresses row 4h + (l & 15) / 4 of an 8-row group and columns
  // 16 gg + 4 (l & 3) .. + 3 of each d block; a kernel forms TrLane once.  tr_off: rows row0 .. + 7.
  struct TrLane { int gg, i16, row; };
  static QA_IMG TrLane tr_lane(int lane, int h) {
    return TrLane{(lane >> 4) & 1, lane & 15, 4 * h + ((lane & 15) >> 2)};
  }
  static QA_IMG int tr_d(TrLane p, int b) { return 32 * b + 16 * p.gg + 4 * (p.i16 & 3); }
  static QA_IMG int tr_off(TrLane p, int b, int row0 = 0) {
    return elem_at(row0 + p.row, tr_d(p, b), SW::sw(row0 + p.row));
  }
  // one MFMA A operand (d on the lane): rows r .. r+3 and r+8 .. r+11 of a 16-row group, one offset
  static QA_DEVICE v8bf tr_frag(const char* a) {
    static_assert(period(8), "rows r and r + 8 must share an offset");
    return __builtin_bit_cast(v8bf, ds_read_tr16_x2(a, a + 8 * ROWB));
  }
  // the 2 * NDB operands of a tile, ta[s * NDB + b] = rows 16s .. 16s + 15 of d block b, from
  // troff[b] = tr_off(p, b) ...
  static QA_DEVICE void tr_load(const char* base, const int* troff, v8bf* ta) {
    static_assert(period(16), "rows r and r + 16 must share an offset");
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int b = 0; b < NDB; ++b) ta[s * NDB + b] = tr_frag(base + troff[b] + 16 * s * ROWB);
  }
  // ... or, for any swizzle, from troff[s][half][b] = tr_off(p, b, 16s + 8 half)
  static QA_DEVICE void tr_load(const char* base, const int (*troff)[2][NDB], v8bf* ta) {
#pragma unroll
    for (int i = 0; i < 2 * NDB; ++i)
      ta[i] = __builtin_bit_cast(v8bf, ds_read_tr16_x2(base + troff[i / NDB][0][i % NDB],
                                                       base + troff[i / NDB][1][i % NDB]));
  }
};

enum ImageKind { I8_ROWS, B16_ROWS, B16_TR };
template <int D, ImageKind K>
struct ImageSw {
  static QA_IMG int sw(int row) {
    return K == I8_ROWS    ? (row >> (D == 128 ? 1 : 2)) & (D / 16 - 1)
           : K == B16_ROWS ? (D == 128 ? row & 15 : (row >> 1) & 7)
                           : (row & 3) << (D == 128 ? 2 : 1);
  }
};
template <int D>
using I8Rows = TileImage<D, ImageSw<D, I8_ROWS>>;        // int8 rows, read by rows
template <int D>
using B16Rows = TileImage<2 * D, ImageSw<D, B16_ROWS>>;  // 16-bit rows, read by rows
template <int D>
using B16Tr = TileImage<2 * D, ImageSw<D, B16_TR>>;      // 16-bit rows, read transposed

// Source byte (inside the tile) that the DMA plan puts at LDS byte x of image I.
template <typename I>
constexpr int lds_to_src(int x) {
  return I::dma_src(x / 1024, x % 1024 / 16) + x % 16;
}
// the swizzle stays inside the row, repeats every 32 rows (a multi-tile stage is tiles back to
// back), and every chunk read by rows is the chunk the DMA plan put there
template <typename I>
constexpr bool row_reads_agree() {
  for (int row = 0; row < 32; ++row)
    for (int c = 0; c < I::NCH; ++c)
      if (I::sw(row) < 0 || I::sw(row) >= I::NCH || lds_to_src<I>(I::row_off(row, c)) != row * I::ROWB + 16 * c)
        return false;
  return I::period(32);
}
// every transposed read (lane, d block, 8-row group) starts at its element (row, d) of the source
template <typename I>
constexpr bool tr_reads_agree() {
  for (int lane = 0; lane < 64; ++lane)
    for (int b = 0; b < I::NDB; ++b)
      for (int row0 = 0; row0 < 32; row0 += 8) {
        const int row = row0 + 4 * (lane >> 5) + (lane & 15) / 4, d = 32 * b + 16 * (lane / 16 % 2) + 4 * (lane % 4);
        if (lds_to_src<I>(I::tr_off(I::tr_lane(lane, lane >> 5), b, row0)) != row * I::ROWB + 2 * d) return false;
      }
  return true;
}
template <int D>
constexpr bool images_agree() {
  return row_reads_agree<I8Rows<D>>() && row_reads_agree<B16Rows<D>>() && row_reads_agree<B16Tr<D>>() &&
         tr_reads_agree<B16Tr<D>>() && B16Tr<D>::period(8) && B16Tr<D>::period(16);
}
static_assert(images_agree<64>() && images_agree<128>(), "an image's DMA plan and reader disagree");

// LDS-DMA plan of ring slots that hold one B16Tr image each, filled by WAVES waves, IPK pieces per
// wave: extra waves re-issue a piece (the same bytes to the same place), so all have IPK in flight.
template <int D, int WAVES>
struct TrImageDma {
  using T = B16Tr<D>;
  static constexpr int IPK = (T::NP + WAVES - 1) / WAVES;
  unsigned voff[IPK], lds_off[IPK];
  v4u rsrc;
  QA_DEVICE void init(int wave, int lane, const void* rows, unsigned nrows) {
#pragma unroll
    for (int i = 0; i < IPK; ++i) {
      int pc = wave + WAVES * i;
      if (pc >= T::NP) pc = wave % T::NP;
      voff[i] = T::dma_src(pc, lane);
      lds_off[i] = pc * 1024;
    }
    rsrc = make_rsrc(rows, nrows * T::ROWB);
  }
  QA_DEVICE void issue(unsigned slot_lds, unsigned soff) const {   // soff: the tile's source offset
#pragma unroll
    for (int i = 0; i < IPK; ++i) dma16_buf(rsrc, voff[i], soff, slot_lds + lds_off[i]);
  }
};

}  // namespace qattn
