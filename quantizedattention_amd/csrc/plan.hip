// Launch plans (host code only, no kernels): the choices a host makes before it calls a kernel entry
// of include/qattn.h -- how many keys a split of a decoding forward takes, how many key/value heads
// the int8 record backward handles per workspace chunk, and whether a backward writes dS records or
// recomputes.  Every choice gives bit-identical outputs and differs only in time and memory, so no
// parity test can tell two copies of a rule apart: the rules live here alone, and the Python drop-ins,
// the TORCH_LIBRARY operators and the C host (tests/c_abi/int8_step.cpp) all ask these functions.
// The environment switches are read on every call.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "qattn.h"

namespace qattn {

// The dK+dV kernel addresses the records of one key/value head (its G query heads) with 32-bit
// buffer offsets: that region, G * (sq/32) * (sk/32) KiB, must stay below 2^31 bytes.  Both record
// kernels also keep per-tile tables in LDS beside their tile rings (int8_bwd.hip, launch_bwd_c and
// launch_dqw_c): dK+dV 36 bytes per streamed query tile of the key/value head (its scales and one dS
// scale per wave), dQ 32 bytes per key tile.  Past QATTN_WS_MAX_QUERY_TILES = G * sq/32 or QATTN_WS_MAX_KEY_TILES =
// sk/32 the 160 KiB of a workgroup do not hold them and the launch would be refused, so such shapes
// recompute (int8_bwd.hip asserts both constants against its configurations).
bool ws_region_fits(long group, long sq_tok, long sk_tok) {
  return group * (sq_tok / 32) <= QATTN_WS_MAX_QUERY_TILES && sk_tok / 32 <= QATTN_WS_MAX_KEY_TILES &&
         group * (sq_tok / 32) * (sk_tok / 32) * 1024 < (1L << 31);
}

}  // namespace qattn

using qattn::ws_region_fits;

// (LONG_MIN when the variable is unset or empty)
static long env_long(const char* name) {
  const char* s = getenv(name);
  return (s != nullptr && *s != 0) ? strtol(s, nullptr, 10) : LONG_MIN;
}

// Largest dS-record workspace either backward (int8 or bf16) allocates before it falls back to
// recomputation: QATTN_BWD_WS_MAX bytes if set, else 16 GiB.  A fixed figure, not the device's free
// memory: hipMemGetInfo does not see what the caller's caching allocator holds reserved, so a free-
// memory cap would depend on allocator history; an allocation that fails falls back to the
// recomputing backward instead (same results).
extern "C" long qattn_bwd_ws_cap(void) {
  const long v = env_long("QATTN_BWD_WS_MAX");
  return v != LONG_MIN ? v : 16L << 30;
}

extern "C" long qattn_int8_bwd_ws_bytes(long bh, long sq_tok, long sk_tok) {
  if (sq_tok % 32 != 0 || sk_tok % 32 != 0 || bh < 0) return -1;
  if (!ws_region_fits(1, sq_tok, sk_tok)) return -1;   // too large even ungrouped: recompute instead
  return bh * (sq_tok / 32) * (sk_tok / 32) * (1024 + 4);
}

// Enough workgroups for two per CU (512), no split shorter than 1024 keys (a workgroup's fixed
// prologue / epilogue cost is worth ~20 tiles of 32 keys); the measurements behind both constants are
// in the docstrings of kv_cache._split_plan and kv_cache_mxfp4._split_plan_fp4.
extern "C" long qattn_split_keys(long bhv, long rows, long sk, int tile) {
  if ((tile != 32 && tile != 64) || bhv < 0 || rows < 0 || sk < 0 || sk % tile != 0) return -1;
  const long wgs = bhv * ((rows + 127) / 128);
  if (wgs == 0) return sk;
  const long nsplit = std::max(1L, std::min(sk / 1024, (512 + wgs - 1) / wgs));
  return (sk / tile + nsplit - 1) / nsplit * tile;
}

// Auto chunk: non-causal, chunks of >= 512 dK+dV workgroups (two per CU; a workgroup covers 256
// keys), measured 2-4 % faster than one pass at config 3 with a quarter of the workspace; causal, one
// pass, since a causal chunk's uneven workgroups leave a longer tail per launch, measured 10-170 %
// slower in chunks.
extern "C" long qattn_int8_bwd_plan(long bkv, int group, long sq_tok, long sk_tok, int causal,
                                    long chunk_req, long cap, long* kv_chunk) {
  if (bkv < 0 || group < 1 || sq_tok < 0 || sk_tok < 0 || sq_tok % 32 != 0 || sk_tok % 32 != 0)
    return -1;
  long chunk = chunk_req;
  if (chunk < 0) chunk = env_long("QATTN_BWD_WS_CHUNK");   // (unset, or negative: auto)
  if (chunk < 0) {
    const long wgs_per_head = std::max(1L, sk_tok / 256);
    chunk = causal ? 0 : (512 + wgs_per_head - 1) / wgs_per_head;
  }
  chunk = chunk == 0 ? bkv : std::min(chunk, bkv);
  if (kv_chunk != nullptr) *kv_chunk = chunk;
  if (cap < 0) cap = qattn_bwd_ws_cap();
  if (!ws_region_fits(group, sq_tok, sk_tok)) return 0;
  const long bytes = qattn_int8_bwd_ws_bytes(chunk * group, sq_tok, sk_tok);
  return bytes <= cap ? bytes : 0;
}

extern "C" long qattn_bf16_bwd_plan(long bh, long sq_tok, long sk_tok, int causal, int force,
                                    long cap) {
  const long bytes = qattn_bf16_bwd_ws_bytes(bh, sq_tok, sk_tok);
  if (bytes < 0) return -1;
  if (force < 0) {
    const long v = env_long("QATTN_BF16_BWD_WS");
    force = v < 0 ? causal != 0 : v == 1;   // (unset, or negative: auto)
  }
  if (cap < 0) cap = qattn_bwd_ws_cap();
  return force != 0 && bytes <= cap ? bytes : 0;
}
