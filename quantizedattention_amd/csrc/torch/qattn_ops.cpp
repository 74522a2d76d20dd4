// TORCH_LIBRARY(qattn) operator layer over the C-ABI kernel library ("C++ op layer").
//
// Each operator allocates its outputs on the inputs' device, enters a HIP device guard on that
// device (c10::hip::HIPGuardMasqueradingAsCUDA: ROCm torch reports HIP devices as 'cuda') and
// enqueues the kernels of include/qattn.h on torch's current stream of that device
// (c10::hip::getCurrentHIPStream, c10/hip/HIPStream.h:245).  The kernel sequences are those of the
// Python drop-in functions (attention_int8.py / attention_bf16.py / attention_jvp.py /
// attention_mxfp4.py), so an operator's outputs are bit-identical to the drop-in's
// (tests/test_gpu_ops.py).  Registered for the CUDA dispatch key only: there is no CPU kernel, as
// in the drop-ins; the Python side (quantizedattention_amd/ops.py) adds the fake (meta)
// implementations and the autograd rules of int8_fwd / bf16_fwd.
//
// Schemas (reference file:line of the computation each replaces):
//   int8_quant(Tensor x, int block) -> (Tensor, Tensor)                 attention_int8.py:178-186
//   int8_fwd(Tensor q, Tensor k, Tensor v, bool smooth, bool causal)   attention_int8.py:20-65, 97-262
//       -> (O, lse, q_i8, k_i8, v_i8, sq, sk, sv)        (k_i8 row-major [B*Hkv*Sk, D])
//   int8_bwd(dO, q_i8, sq, k_i8, sk, v_i8, sv, O, lse, bool causal, int kv_heads)
//       -> (dq, dk, dv)                                                  attention_int8.py:264-432
//   bf16_fwd(q, k, v, bool causal) -> (O, lse)                           attention_bf16.py:107-296
//   bf16_bwd(q, k, v, O, lse, bool causal, dO) -> (dq, dk, dv)           attention_bf16.py:299-448
//   jvp_fwd(q, k, v, tq, tk, tv) -> (O, tO, lse)                         attention_jvp.py:24-195
//   mxfp4_fwd(q, k, v) -> O                                  (README.md:49-55)
//   mxfp4_fwd_ex(q, k, v, causal) -> O                       (the same with a mask: 0 / 1 / 2)
//   mxfp4_cached(q, k4, ks, vt, vs, causal, keys_per_split) -> (O, lse)
//       kv_cache_mxfp4.attention_mxfp4_cached on the cache's four operands (causal 0 / 1 bottom-right
//       over the cache; keys_per_split 0: the plan of qattn_split_keys)
//   mxfp4_decode(q, k4, ks, vt, vs, lens, sk_max, causal, keys_per_split) -> (O, lse)
//       kv_cache_mxfp4.attention_mxfp4_decode on a preallocated cache's operands and device lengths
//   mxfp4_decode_paged(q, k4, ks, vt, vs, lens, block_table, sk_max, causal, keys_per_split) -> (O, lse)
//       kv_cache_mxfp4.attention_mxfp4_decode_paged on a page pool's operands, lengths and block table
//   mxfp4_varlen_paged_window(.. the arguments of mxfp4_varlen_paged .., window, sinks) -> (O, lse)
//       the same with a sliding window and sinks (causal only)
//   mxfp4_varlen_paged(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal,
//                      keys_per_split) -> (O, lse)
//       kv_cache_mxfp4.attention_mxfp4_varlen_paged: packed q [T, Hq, 128] and the two plan tables
//   mxfp4_varlen_paged_tree(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, tree_masks, part_rows,
//                           causal, keys_per_split) -> (O, lse)      the same with a tree mask (verify step)
//   mxfp4_varlen_paged_shared(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, grp_rec, members,
//                             part_rows, causal, keys_per_split) -> (O, lse)
//       the same with shared prefixes: the four tables of kv_cache_mxfp4.plan_varlen_shared
//   mxfp4_quant_rows_rope(x, cos_sin, pos, interleaved) -> (q4, qs)
//       attention_mxfp4.mxfp4_quantize_rows_rope: packed x [T, H, 128] rotated by pos i32 [T] through the
//       table cos_sin f32 [max_pos, 128], then quantised
//   mxfp4_varlen_paged_rope(.. the arguments of mxfp4_varlen_paged .., cos_sin, pos, interleaved) -> (O, lse)
//       the same with q rotated inside its quantiser (attention_mxfp4_varlen_paged(rope=))
//   mxfp4_decode_step_plan(slots, lens, capacity, kv_heads, group, keys_per_split, splits, window, sinks)
//       -> (seq_tab, tiles, pos, seq_rec): kv_cache_mxfp4.DecodeStep's tables, derived on the device
//   mxfp4_decode_step(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, splits, keys_per_split, window,
//       sinks) -> (O, lse): kv_cache_mxfp4.DecodeStep.attend over its fixed grid
//   mxfp4_verify_step_plan(slots, lens, tree, draft_tokens, capacity, kv_heads, group, keys_per_split, splits)
//       -> (seq_tab, tiles, pos, seq_rec): kv_cache_mxfp4.VerifyStep's tables, derived on the device
//   mxfp4_verify_step(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, tree, draft_tokens, splits,
//       keys_per_split) -> (O, lse): kv_cache_mxfp4.VerifyStep.attend over its fixed grid
// Workspaces, head chunks and key splits are planned by the library (csrc/plan.hip), as in the drop-ins.
// Errors: TORCH_CHECK (c10::Error, RuntimeError in Python) with the drop-ins' messages; int8_quant's
// argument checks raise ValueError (TORCH_CHECK_VALUE) as its Python predecessor did.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <c10/hip/HIPCachingAllocator.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <tuple>

#include "qattn.h"

namespace {

using at::Tensor;
using T3 = std::tuple<Tensor, Tensor, Tensor>;

// The address of a kernel argument: the kernels read 16-byte vectors and LDS-DMA dwordx4 from every
// base address, so one that is no multiple of 16 never reaches them (_lib.ptr)
void* P(const Tensor& t) {
  if (!t.defined()) return nullptr;
  void* p = t.data_ptr();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "qattn: a tensor at an address that is not a "
              "multiple of 16 (storage offset ", t.storage_offset(), ")");
  return p;
}

// A tensor in the form a kernel reads (_lib.kernel_input): dtype dt, contiguous, at a 16-byte aligned
// address; a contiguous view at a misaligned storage offset is copied
Tensor kin(const Tensor& t, at::ScalarType dt) {
  Tensor x = t.to(dt).contiguous();
  if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0) x = x.clone(at::MemoryFormat::Contiguous);
  return x;
}
Tensor kin(const Tensor& t) { return kin(t, t.scalar_type()); }

// Every query keeps a key: Sk = 0 with rows > 0 is refused on every path, before anything is allocated
// (status 1 of the C entries, include/qattn.h)
void refuse_empty_keys(const char* what, int64_t rows, int64_t sk) {
  TORCH_CHECK(!(rows > 0 && sk == 0), "qattn ", what, ": an empty key sequence (Sk = 0) with ", rows,
              " query rows; every query keeps a key");
}

struct Ctx {   // device guard + the current stream of the inputs' device
  c10::hip::HIPGuardMasqueradingAsCUDA guard;
  void* stream;
  explicit Ctx(const Tensor& t)
      : guard(t.device()), stream((void*)c10::hip::getCurrentHIPStream(t.device().index()).stream()) {}
};

void call(int rc, const char* what) {
  TORCH_CHECK(rc != 1, "qattn: ", what, ": unsupported shape");
  TORCH_CHECK(rc == 0, "qattn: ", what, ": kernel launch failed");
}

void require_gpu(std::initializer_list<const Tensor*> ts) {
  for (const Tensor* t : ts)
    TORCH_CHECK(t->is_cuda(), "qattn kernels run on the GPU only; got a tensor on ", t->device(),
                " (no CPU fallback by design)");
}

// fp32(1/sqrt(D) * log2(e)) and fp32(1/sqrt(D)): the Python double rounded once to fp32
float qk_scale(int64_t D) { return (float)(1.0 / std::sqrt((double)D) * 1.44269504); }
float sm_scale(int64_t D) { return (float)(1.0 / std::sqrt((double)D)); }

Tensor empty(at::IntArrayRef shape, at::ScalarType dt, const Tensor& like) {
  return at::empty(shape, like.options().dtype(dt));
}

// A backward workspace of `bytes`, undefined when the allocator refuses.  torch's caching allocator
// frees every cached block and retries before it raises, so after one refusal a workspace that large
// is tried again only when the device has room for it (hipMemGetInfo free bytes plus the allocator's
// reserved-but-unused bytes): a training loop whose workspace never fits does not flush the cache in
// every backward (the same rule as _lib.try_workspace).
Tensor try_empty(int64_t bytes, const Tensor& like) {
  static std::mutex mu;
  static std::map<int, int64_t> refused;   // device -> smallest refused size
  const int dev = like.device().index();
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = refused.find(dev);
    if (it != refused.end() && bytes >= it->second) {
      size_t free_b = 0, total_b = 0;
      const auto st = c10::hip::HIPCachingAllocator::getDeviceStats(dev);
      const int64_t spare = st.reserved_bytes[0].current - st.allocated_bytes[0].current;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (int64_t)free_b + spare < bytes)
        return Tensor();
    }
  }
  try {
    Tensor t = at::empty({bytes}, like.options().dtype(at::kByte));
    std::lock_guard<std::mutex> g(mu);
    auto it = refused.find(dev);
    if (it != refused.end() && bytes >= it->second) refused.erase(it);
    return t;
  } catch (const c10::OutOfMemoryError&) {
    std::lock_guard<std::mutex> g(mu);
    auto it = refused.find(dev);
    if (it == refused.end() || bytes < it->second) refused[dev] = bytes;
    return Tensor();
  }
}

// ------------------------------------------------------------------------------------ int8
std::tuple<Tensor, Tensor> int8_quant(const Tensor& x, int64_t block) {
  TORCH_CHECK_VALUE(block == 32, "qattn::int8_quant supports block = 32 (the reference's Bq = Bkv)");
  TORCH_CHECK_VALUE(x.dim() >= 2 && x.size(-2) % 32 == 0 && (x.size(-1) == 64 || x.size(-1) == 128),
              "qattn::int8_quant needs x [..., S, D] with S % 32 == 0 and D in (64, 128)");
  require_gpu({&x});
  Ctx c(x);
  const Tensor xh = kin(x, at::kHalf);
  const int64_t D = x.size(-1), rows = xh.numel() / D, S = x.size(-2);
  Tensor idx = empty(xh.sizes(), at::kChar, xh);
  std::vector<int64_t> ss(xh.sizes().begin(), xh.sizes().end() - 2);
  ss.push_back(S / 32);
  Tensor scale = empty(ss, at::kHalf, xh);
  if (rows == 0) return {idx, scale};
  call(qattn_int8_quant(P(xh), P(idx), P(scale), nullptr, nullptr, rows, (int)S, (int)D, c.stream),
       "int8_quant");
  return {idx, scale};
}

void check_int8(const Tensor& q, const Tensor& k, const Tensor& v) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "qattn int8: q, k, v must be [B, H, S, D]");
  TORCH_CHECK(k.size(2) == v.size(2), "k and v tokens are different");          // int8:126
  TORCH_CHECK(k.size(3) == v.size(3), "k head_dim and v head_dim are different");  // int8:127
  TORCH_CHECK(q.size(0) == k.size(0) && k.sizes().slice(0, 2) == v.sizes().slice(0, 2) &&
                  q.size(3) == k.size(3) && q.size(1) % k.size(1) == 0,
              "qattn int8: batch and head_dim must match and q heads must be a multiple of k/v heads");
  TORCH_CHECK(q.size(2) % 32 == 0 && k.size(2) % 32 == 0, "qattn int8: token counts must be multiples of 32");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128, "qattn int8: head_dim must be 64 or 128");
}

using T8 = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// attention_int8._int8_forward
T8 int8_fwd(const Tensor& q_in, const Tensor& k_in, const Tensor& v_in, bool smooth, bool causal) {
  check_int8(q_in, k_in, v_in);
  require_gpu({&q_in, &k_in, &v_in});
  refuse_empty_keys("int8", q_in.size(0) * q_in.size(1) * q_in.size(2), k_in.size(2));
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf), k = kin(k_in, at::kHalf), v = kin(v_in, at::kHalf);
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int64_t Hkv = k.size(1), Sk = k.size(2), N = B * H * S, Nkv = B * Hkv * Sk;
  Tensor q_i8 = empty({N, D}, at::kChar, q), k_i8 = empty({Nkv, D}, at::kChar, q),
         v_i8 = empty({Nkv, D}, at::kChar, q);
  Tensor sq = empty({N / 32}, at::kHalf, q), sk = empty({Nkv / 32}, at::kHalf, q),
         sv = empty({Nkv / 32}, at::kHalf, q);
  Tensor vt = empty({Nkv, D}, at::kChar, q);   // the int8 V^T operand image
  Tensor O = empty({B, H, S, D}, at::kHalf, q), lse = empty({N}, at::kHalf, q);
  Tensor k_mean;
  if (smooth) {
    k_mean = empty({B, Hkv, 1, D}, at::kHalf, q);
    call(qattn_kmean(P(k), P(k_mean), B * Hkv, Sk, (int)D, c.stream), "kmean");
  }

  const float qks = qk_scale(D);
  call(qattn_int8_quant(P(k), P(k_i8), P(sk), nullptr, P(k_mean), Nkv, (int)Sk, (int)D, c.stream),
       "quantise k");
  call(qattn_int8_quant_vt(P(v), P(v_i8), P(sv), P(vt), Nkv, (int)D, c.stream), "quantise v");
  if (N == 0) return {O, lse, q_i8, k_i8, v_i8, sq, sk, sv};   // no query rows: empty O, lse, q_i8, sq
  call(qattn_int8_attn_fwd_qf(P(q), P(q_i8), P(sq), nullptr, P(k_i8), P(sk), P(vt), P(sv), P(O), P(lse),
                              B * H, S, Sk, (int)(H / Hkv), causal ? 1 : 0, (int)D, qks, c.stream),
       "int8 forward");
  return {O, lse, q_i8, k_i8, v_i8, sq, sk, sv};
}

// attention_int8._int8_backward: dS-record workspace (in head chunks when not causal) by default,
// recomputation when the workspace does not fit
T3 int8_bwd(const Tensor& dO_in, const Tensor& q_i8_in, const Tensor& sq, const Tensor& k_i8_in,
            const Tensor& sk, const Tensor& v_i8_in, const Tensor& sv, const Tensor& O_in,
            const Tensor& lse_in, bool causal, int64_t kv_heads) {
  require_gpu({&dO_in, &q_i8_in, &O_in});
  TORCH_CHECK(O_in.dim() == 4, "qattn int8 backward: O must be [B, H, S, D]");
  refuse_empty_keys("int8 backward", O_in.numel() / std::max<int64_t>(O_in.size(3), 1), k_i8_in.size(0));
  Ctx c(O_in);
  const Tensor O = kin(O_in, at::kHalf), dO = kin(dO_in, at::kHalf);
  const int64_t B = O.size(0), H = O.size(1), S = O.size(2), D = O.size(3), Hkv = kv_heads;
  const int64_t Nkv = k_i8_in.size(0);
  if (B * H * S == 0) {   // no query rows: dq is empty, dk and dv are zero
    TORCH_CHECK(Hkv > 0, "qattn int8 backward: inconsistent key/value heads");
    const int64_t Sk0 = B * Hkv ? Nkv / (B * Hkv) : 0;
    auto z = O_in.options().dtype(at::kHalf);
    return {at::zeros({B, H, S, D}, z), at::zeros({B, Hkv, Sk0, D}, z), at::zeros({B, Hkv, Sk0, D}, z)};
  }
  TORCH_CHECK(Hkv > 0 && H % Hkv == 0 && Nkv % (B * Hkv) == 0,
              "qattn int8 backward: inconsistent key/value heads");
  const int64_t Sk = Nkv / (B * Hkv), N = B * H * S, G = H / Hkv;
  const Tensor q_i8 = kin(q_i8_in), k_i8 = kin(k_i8_in), v_i8 = kin(v_i8_in);
  const Tensor sqc = kin(sq), skc = kin(sk), svc = kin(sv);
  const Tensor lse = kin(lse_in, at::kHalf);
  Tensor dO_i8 = empty({N, D}, at::kChar, O), sdO = empty({N / 32}, at::kHalf, O);
  Tensor LD = empty({N, 2}, at::kFloat, O), dO_bf = empty({N, D}, at::kBFloat16, O);
  call(qattn_int8_bwd_prep(P(dO), P(O), P(lse), P(dO_i8), P(sdO), P(LD), P(dO_bf), B * H, S, (int)D,
                           c.stream),
       "int8 backward prep");
  Tensor q_bf = empty({N, D}, at::kBFloat16, O), k_bf = empty({Nkv, D}, at::kBFloat16, O);
  call(qattn_i8_to_bf16(P(q_i8), P(q_bf), N * D, c.stream), "q image");
  call(qattn_i8_to_bf16(P(k_i8), P(k_bf), Nkv * D, c.stream), "k image");
  Tensor dq = empty({B, H, S, D}, at::kHalf, O), dk = empty({B, Hkv, Sk, D}, at::kHalf, O),
         dv = empty({B, Hkv, Sk, D}, at::kHalf, O);
  const float qks = qk_scale(D), sms = sm_scale(D);
  long chunk = 0;
  const long ws_bytes = qattn_int8_bwd_plan(B * Hkv, (int)G, S, Sk, causal ? 1 : 0, -1, -1, &chunk);
  Tensor ws;
  if (ws_bytes > 0) ws = try_empty(ws_bytes, O);
  if (ws.defined()) {
    call(qattn_int8_attn_bwd_wsc(P(dO_i8), P(sdO), P(q_i8), P(sqc), P(k_i8), P(skc), P(v_i8), P(svc),
                                 P(LD), P(q_bf), P(k_bf), P(dO_bf), P(dq), P(dk), P(dv), P(ws), chunk,
                                 B * H, S, Sk, (int)G, causal ? 1 : 0, (int)D, qks, sms, c.stream),
         "int8 backward");
  } else {
    call(qattn_int8_attn_bwd_ex(P(dO_i8), P(sdO), P(q_i8), P(sqc), P(k_i8), P(skc), P(v_i8), P(svc),
                                P(LD), P(q_bf), P(k_bf), P(dO_bf), P(dq), P(dk), P(dv), B * H, S, Sk,
                                (int)G, causal ? 1 : 0, (int)D, qks, sms, c.stream),
         "int8 backward");
  }
  return {dq, dk, dv};
}

// ------------------------------------------------------------------------------------ bf16
void check_bf16(const Tensor& q, const Tensor& k, const Tensor& v) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "qattn bf16: q, k, v must be [B, H, S, D]");
  TORCH_CHECK(k.size(2) == v.size(2), "input k_tokens must match v_tokens");   // bf16:154
  TORCH_CHECK(q.size(3) == k.size(3) && k.size(3) == v.size(3),
              "all head dimensions must match for q, k, v tensors");          // bf16:155
  TORCH_CHECK(q.size(0) == k.size(0) && k.sizes().slice(0, 2) == v.sizes().slice(0, 2) &&
                  q.size(1) % k.size(1) == 0,
              "qattn bf16: batch must match and q heads must be a multiple of k/v heads");
  TORCH_CHECK(q.size(2) % 32 == 0 && k.size(2) % 32 == 0, "qattn bf16: token counts must be multiples of 32");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128, "qattn bf16: head_dim must be 64 or 128");
}

std::tuple<Tensor, Tensor> bf16_fwd(const Tensor& q_in, const Tensor& k_in, const Tensor& v_in,
                                    bool causal) {
  check_bf16(q_in, k_in, v_in);
  require_gpu({&q_in, &k_in, &v_in});
  refuse_empty_keys("bf16", q_in.size(0) * q_in.size(1) * q_in.size(2), k_in.size(2));
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf), k = kin(k_in, at::kHalf), v = kin(v_in, at::kBFloat16);
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3), Sk = k.size(2);
  Tensor O = empty({B, H, S, D}, at::kFloat, q), lse = empty({B * H, S}, at::kFloat, q);
  if (O.numel() == 0) return {O, lse};   // no query rows: empty outputs
  // causal: the per-head V suffix sums stand in for the fully masked key tiles (include/qattn.h);
  // without room for them the kernel runs the whole masked tile loop (same results)
  Tensor ws;
  if (causal) ws = try_empty(qattn_bf16_fwd_ws_bytes(B * k.size(1), Sk, (int)D), q);
  call(qattn_bf16_fwd_ws_ex(P(q), P(k), P(v), P(O), P(lse), B * H, S, Sk, (int)(H / k.size(1)),
                            causal ? 1 : 0, (int)D, qk_scale(D), P(ws), c.stream),
       "bf16 forward");
  return {O, lse};
}

// attention_bf16.helion_flash_atten_2_algo_4_bwd (entry "auto": causal -> dS records)
T3 bf16_bwd(const Tensor& q_in, const Tensor& k_in, const Tensor& v_in, const Tensor& O_in,
            const Tensor& lse_in, bool causal, const Tensor& dO_in) {
  check_bf16(q_in, k_in, v_in);
  require_gpu({&q_in, &k_in, &v_in, &O_in, &lse_in, &dO_in});
  refuse_empty_keys("bf16 backward", q_in.size(0) * q_in.size(1) * q_in.size(2), k_in.size(2));
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf), k = kin(k_in, at::kHalf), v = kin(v_in, at::kBFloat16),
               O = kin(O_in, at::kFloat), dO = kin(dO_in, at::kFloat), lse = kin(lse_in, at::kFloat);
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int64_t Hkv = k.size(1), Sk = k.size(2);
  if (q.numel() == 0) {   // no query rows: dq is empty, dk and dv are zero
    auto z = q.options().dtype(at::kFloat);
    return {at::zeros(q.sizes(), z), at::zeros(k.sizes(), z), at::zeros(v.sizes(), z)};
  }
  Tensor dO_bf = empty({B, H, S, D}, at::kBFloat16, q), LD = empty({B * H, S, 2}, at::kFloat, q);
  call(qattn_bf16_bwd_prep(P(dO), P(O), P(lse), P(dO_bf), P(LD), B * H, S, (int)D, c.stream),
       "bf16 backward prep");
  Tensor q_bf = empty(q.sizes(), at::kBFloat16, q), k_bf = empty(k.sizes(), at::kBFloat16, q);
  call(qattn_f16_to_bf16(P(q), P(q_bf), q.numel(), c.stream), "q image");
  call(qattn_f16_to_bf16(P(k), P(k_bf), k.numel(), c.stream), "k image");
  Tensor dq = empty({B, H, S, D}, at::kFloat, q), dk = empty({B, Hkv, Sk, D}, at::kFloat, q),
         dv = empty({B, Hkv, Sk, D}, at::kFloat, q);
  const float qks = qk_scale(D), sms = sm_scale(D);
  const long ws_bytes = qattn_bf16_bwd_plan(B * H, S, Sk, causal ? 1 : 0, -1, -1);
  Tensor ws;
  if (ws_bytes > 0) ws = try_empty(ws_bytes, q);
  if (ws.defined())
    call(qattn_bf16_bwd_ws_ex(P(q), P(k), P(v), P(dO_bf), P(LD), P(q_bf), P(k_bf), P(dq), P(dk), P(dv),
                              B * H, S, Sk, (int)(H / Hkv), causal ? 1 : 0, (int)D, qks, sms, P(ws),
                              c.stream),
         "bf16 backward");
  else
    call(qattn_bf16_bwd_ex(P(q), P(k), P(v), P(dO_bf), P(LD), P(q_bf), P(k_bf), P(dq), P(dk), P(dv),
                           B * H, S, Sk, (int)(H / Hkv), causal ? 1 : 0, (int)D, qks, sms, c.stream),
         "bf16 backward");
  return {dq, dk, dv};
}

// ------------------------------------------------------------------------------------- jvp
// attention_jvp._jvp: bf16 inputs on the bf16 MFMA, other dtypes as fp32 split into bf16 hi/lo
T3 jvp_fwd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& tq, const Tensor& tk,
           const Tensor& tv) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "qattn jvp: q, k, v must be [B, H, S, D]");
  TORCH_CHECK(k.size(2) == v.size(2), "input k_tokens must match v_tokens");   // jvp:78
  TORCH_CHECK(q.size(3) == k.size(3) && k.size(3) == v.size(3),
              "all head dimensions must match for q, k, v tensors");          // jvp:79
  require_gpu({&q, &k, &v, &tq, &tk, &tv});
  TORCH_CHECK(q.size(2) % 32 == 0 && k.size(2) % 32 == 0, "qattn jvp: q and k tokens must be multiples of 32");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128, "qattn jvp: head_dim must be 64 or 128");
  TORCH_CHECK(tq.sizes() == q.sizes() && tk.sizes() == k.sizes() && tv.sizes() == v.sizes(),
              "qattn jvp: tangents must have the primals' shapes");
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3), Hkv = k.size(1);
  const int64_t Sk = k.size(2);
  TORCH_CHECK(k.size(0) == B && v.size(0) == B && v.size(1) == Hkv && H % Hkv == 0,
              "qattn jvp: k and v need q's batch and a head count dividing q's");
  refuse_empty_keys("jvp", B * H * S, Sk);
  Ctx c(q);
  Tensor O = empty({B, H, S, D}, at::kFloat, q), tO = empty({B, H, S, D}, at::kFloat, q),
         lse = empty({B * H, S}, at::kFloat, q);
  if (O.numel() == 0) return {O, tO, lse};   // no query rows: empty outputs
  const float qks = qk_scale(D), sm = sm_scale(D);
  const int G = (int)(H / Hkv);
  const Tensor* ins[6] = {&q, &k, &v, &tq, &tk, &tv};
  bool all_bf16 = true;
  for (const Tensor* t : ins) all_bf16 = all_bf16 && t->scalar_type() == at::kBFloat16;
  if (all_bf16) {
    TORCH_CHECK(Sk % 64 == 0, "qattn jvp: k tokens must be a multiple of 64 for bf16 inputs");
    Tensor x[6];
    for (int i = 0; i < 6; ++i) x[i] = kin(*ins[i]);
    call(qattn_jvp_fwd_ex(P(x[0]), P(x[1]), P(x[2]), P(x[3]), P(x[4]), P(x[5]), P(O), P(tO), P(lse), B * H,
                          S, Sk, G, (int)D, qks, sm, c.stream),
         "jvp forward");
    return {O, tO, lse};
  }
  Tensor hi[6], lo[6];
  for (int i = 0; i < 6; ++i) {
    const Tensor x = kin(*ins[i], at::kFloat);
    hi[i] = empty(x.sizes(), at::kBFloat16, x);
    lo[i] = empty(x.sizes(), at::kBFloat16, x);
    call(qattn_split_bf16(P(x), P(hi[i]), P(lo[i]), x.numel(), c.stream), "split fp32");
  }
  call(qattn_jvp_fwd_x3_ex(P(hi[0]), P(lo[0]), P(hi[1]), P(lo[1]), P(hi[2]), P(lo[2]), P(hi[3]), P(lo[3]),
                           P(hi[4]), P(lo[4]), P(hi[5]), P(lo[5]), P(O), P(tO), P(lse), B * H, S, Sk, G,
                           (int)D, qks, sm, c.stream),
       "jvp forward");
  return {O, tO, lse};
}

// ----------------------------------------------------------------------------------- mxfp4
// attention_mxfp4.mxfp4_attn_fwd with k smoothing (sage_attention_3_fp4); causal 0 none, 1 top-left,
// 2 bottom-right (Sk >= Sq)
Tensor mxfp4_fwd_ex(const Tensor& q_in, const Tensor& k_in, const Tensor& v_in, int64_t causal) {
  TORCH_CHECK(q_in.dim() == 4 && k_in.sizes() == v_in.sizes() && q_in.size(0) == k_in.size(0) &&
                  q_in.size(-1) == k_in.size(-1),
              "qattn mxfp4: q [B,H,Sq,D], k = v [B,Hkv,Sk,D] expected");
  TORCH_CHECK(q_in.size(1) % k_in.size(1) == 0, "qattn mxfp4: query heads must be a multiple of key/value heads");
  TORCH_CHECK(q_in.size(-1) == 128, "qattn mxfp4: head_dim must be 128");
  TORCH_CHECK(q_in.size(2) % 32 == 0 && k_in.size(2) % 64 == 0,
              "qattn mxfp4: q tokens must be a multiple of 32, k tokens of 64");
  TORCH_CHECK(causal >= 0 && causal <= 2, "qattn mxfp4: causal must be 0, 1 (top-left) or 2 (bottom-right)");
  TORCH_CHECK(causal != 2 || q_in.size(2) <= k_in.size(2), "qattn mxfp4: causal=2 (bottom-right) needs Sk >= Sq");
  require_gpu({&q_in, &k_in, &v_in});
  refuse_empty_keys("mxfp4", q_in.size(0) * q_in.size(1) * q_in.size(2), k_in.size(2));
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf), k = kin(k_in, at::kHalf), v = kin(v_in, at::kHalf);
  const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), D = q.size(3), Hkv = k.size(1),
                Sk = k.size(2);
  if (q.numel() == 0) return empty({B, H, Sq, D}, at::kHalf, q);   // no query rows: an empty output
  Tensor k_mean = empty({B, Hkv, 1, D}, at::kHalf, q);
  call(qattn_kmean(P(k), P(k_mean), B * Hkv, Sk, (int)D, c.stream), "kmean");
  Tensor q4 = empty({B * H * Sq, D / 2}, at::kByte, q), qs = empty({B * H * Sq, D / 32}, at::kByte, q);
  Tensor k4 = empty({B * Hkv * Sk, D / 2}, at::kByte, q), ks = empty({B * Hkv * Sk, D / 32}, at::kByte, q);
  call(qattn_mxfp4_quant_rows(P(q), nullptr, P(q4), P(qs), B * H * Sq, Sq, (int)D, c.stream), "quantise q");
  call(qattn_mxfp4_quant_rows(P(k), P(k_mean), P(k4), P(ks), B * Hkv * Sk, Sk, (int)D, c.stream),
       "quantise k");
  Tensor vt = empty({B * Hkv, Sk / 64, D, 32}, at::kByte, q), vs = empty({B * Hkv, Sk / 64, D, 2}, at::kByte, q);
  call(qattn_mxfp4_quant_vt(P(v), P(vt), P(vs), B * Hkv, Sk, (int)D, c.stream), "quantise v");
  Tensor out = empty({B, H, Sq, D}, at::kHalf, q), lse = empty({B * H, Sq}, at::kFloat, q);
  call(qattn_mxfp4_attn_fwd_ex(P(q4), P(qs), P(k4), P(ks), P(vt), P(vs), P(out), P(lse), B * H, Sq, Sk,
                               (int)(H / Hkv), (int)causal, (int)D, qk_scale(D), c.stream),
       "mxfp4 forward");
  return out;
}

Tensor mxfp4_fwd(const Tensor& q, const Tensor& k, const Tensor& v) { return mxfp4_fwd_ex(q, k, v, 0); }

// What the cache operators check of the four quantised operands (k4 [n0, Hkv, S, 64]; `paged`: a page pool,
// whose vt / vs keep k4's two leading dimensions) and of lens i32 [B] (null: the operator has none).
void check_fp4_operands(const Tensor& k4, const Tensor& ks, const Tensor& vt, const Tensor& vs,
                        const Tensor* lens, int64_t B, bool paged) {
  const char* what = paged ? "qattn mxfp4 paged cache: " : "qattn mxfp4 kv cache: ";
  for (const Tensor* t : {&k4, &ks, &vt, &vs})
    TORCH_CHECK(t->scalar_type() == at::kByte && t->is_contiguous(), what,
                "the quantised operands must be contiguous uint8");
  const int64_t n0 = k4.size(0), H = k4.size(1), S = k4.size(2), D = 128;
  TORCH_CHECK(ks.sizes() == at::IntArrayRef({n0, H, S, D / 32}) &&
                  (paged ? vt.sizes() == at::IntArrayRef({n0, H, S / 64, D, 32}) &&
                               vs.sizes() == at::IntArrayRef({n0, H, S / 64, D, 2})
                         : vt.sizes() == at::IntArrayRef({n0 * H, S / 64, D, 32}) &&
                               vs.sizes() == at::IntArrayRef({n0 * H, S / 64, D, 2})),
              what, "ks / vt / vs do not match k4");
  if (lens)
    TORCH_CHECK(lens->scalar_type() == at::kInt && lens->is_contiguous() && lens->dim() == 1 && lens->size(0) == B,
                what, "lens must be contiguous int32 [B]");
}

// The tail of mxfp4_cached, mxfp4_decode and mxfp4_decode_paged after their checks: the split plan at sk
// keys, the outputs, q quantised, the key-split entry -- split(q4, qs, opart, ml, bhv, rows, kps, stream),
// named `name` in an error -- and the merge.
template <class Split>
std::tuple<Tensor, Tensor> fp4_split_and_merge(const Tensor& q_in, int64_t Hkv, int64_t sk, int64_t keys_per_split,
                                               bool paged, const char* name, Split split) {
  const int64_t B = q_in.size(0), Hq = q_in.size(1), Sq = q_in.size(2), D = 128;
  const int64_t bhv = B * Hkv, rows = (Hq / Hkv) * Sq;
  int64_t kps = keys_per_split == 0 ? qattn_split_keys(bhv, rows, sk, 64) : keys_per_split;
  TORCH_CHECK(kps >= 64 && kps % 64 == 0, paged ? "qattn mxfp4 paged cache: " : "qattn mxfp4 kv cache: ",
              "keys_per_split must be a multiple of 64");
  kps = std::min(kps, sk);
  const int64_t nsplit = (sk + kps - 1) / kps;
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf);
  Tensor q4 = empty({B * Hq * Sq, D / 2}, at::kByte, q), qs = empty({B * Hq * Sq, D / 32}, at::kByte, q);
  Tensor out = empty({B, Hq, Sq, D}, at::kHalf, q), lse = empty({B * Hq, Sq}, at::kFloat, q);
  if (out.numel() == 0) return {out, lse};
  call(qattn_mxfp4_quant_rows(P(q), nullptr, P(q4), P(qs), B * Hq * Sq, Sq, (int)D, c.stream), "quantise q");
  Tensor opart = empty({nsplit, bhv * rows, D}, at::kFloat, q), ml = empty({nsplit, bhv * rows, 2}, at::kFloat, q);
  call(split(P(q4), P(qs), P(opart), P(ml), bhv, rows, (int)kps, c.stream), name);
  call(qattn_mxfp4_split_combine(P(opart), P(ml), P(out), P(lse), bhv * rows, (int)nsplit, (int)D, c.stream),
       "mxfp4 split merge");
  return {out, lse};
}

// kv_cache_mxfp4.attention_mxfp4_cached: q of any Sq >= 1 against an MX-FP4 cache in the decoding
// layout (split over the keys, then merged)
std::tuple<Tensor, Tensor> mxfp4_cached(const Tensor& q_in, const Tensor& k4, const Tensor& ks,
                                        const Tensor& vt, const Tensor& vs, int64_t causal,
                                        int64_t keys_per_split) {
  require_gpu({&q_in, &k4, &ks, &vt, &vs});
  TORCH_CHECK(q_in.dim() == 4 && k4.dim() == 4 && q_in.size(3) == 128 && k4.size(3) == 64,
              "qattn mxfp4 kv cache: head_dim must be 128 in q and in the cache");
  const int64_t B = k4.size(0), Hkv = k4.size(1), Sk = k4.size(2);
  TORCH_CHECK(q_in.size(0) == B && Hkv > 0 && q_in.size(1) % Hkv == 0,
              "qattn mxfp4 kv cache: q must be [B, G*Hkv, Sq, D] for the cache's B, Hkv");
  const int64_t Sq = q_in.size(2);
  TORCH_CHECK(Sq >= 1 && Sk >= 64 && Sk % 64 == 0,
              "qattn mxfp4 kv cache: Sq >= 1 and a cache of 64*n tokens expected");
  TORCH_CHECK(causal == 0 || causal == 1, "qattn mxfp4 kv cache: causal must be 0 or 1");
  TORCH_CHECK(!causal || Sq <= Sk, "qattn mxfp4 kv cache: causal attention needs Sq <= the cached tokens");
  check_fp4_operands(k4, ks, vt, vs, nullptr, B, false);
  return fp4_split_and_merge(
      q_in, Hkv, Sk, keys_per_split, false, "mxfp4 split forward",
      [&](void* q4, void* qs, void* opart, void* ml, int64_t bhv, int64_t rows, int kps, void* stream) {
        return qattn_mxfp4_attn_fwd_split(q4, qs, P(k4), P(ks), P(vt), P(vs), opart, ml, bhv, rows, Sq, Sk,
                                          causal ? 2 : 0, kps, 128, qk_scale(128), stream);
      });
}

// kv_cache_mxfp4.attention_mxfp4_decode on a preallocated cache's operands: k4 [B, Hkv, cap, 64] with
// lens i32 [B] on the device.  The operator cannot read lens without a synchronisation, so the caller
// guarantees 1 <= lens[b] <= sk_max (a multiple of 64, <= cap) and, causal, lens[b] >= Sq; the Python
// wrapper ops.mxfp4_decode checks them on the cache's host mirror.
std::tuple<Tensor, Tensor> mxfp4_decode(const Tensor& q_in, const Tensor& k4, const Tensor& ks,
                                        const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                        int64_t sk_max, int64_t causal, int64_t keys_per_split) {
  require_gpu({&q_in, &k4, &ks, &vt, &vs, &lens});
  TORCH_CHECK(q_in.dim() == 4 && k4.dim() == 4 && q_in.size(3) == 128 && k4.size(3) == 64,
              "qattn mxfp4 kv cache: head_dim must be 128 in q and in the cache");
  const int64_t B = k4.size(0), Hkv = k4.size(1), cap = k4.size(2);
  TORCH_CHECK(q_in.size(0) == B && Hkv > 0 && q_in.size(1) % Hkv == 0,
              "qattn mxfp4 kv cache: q must be [B, G*Hkv, Sq, D] for the cache's B, Hkv");
  const int64_t Sq = q_in.size(2);
  TORCH_CHECK(Sq >= 1 && cap >= 64 && cap % 64 == 0,
              "qattn mxfp4 kv cache: Sq >= 1 and a capacity of 64*n tokens expected");
  TORCH_CHECK(sk_max >= 64 && sk_max % 64 == 0 && sk_max <= cap,
              "qattn mxfp4 kv cache: sk_max must be a multiple of 64 in [64, capacity]");
  TORCH_CHECK(causal == 0 || causal == 1, "qattn mxfp4 kv cache: causal must be 0 or 1");
  TORCH_CHECK(!causal || Sq <= sk_max, "qattn mxfp4 kv cache: causal attention needs Sq <= the cached tokens");
  check_fp4_operands(k4, ks, vt, vs, &lens, B, false);
  return fp4_split_and_merge(
      q_in, Hkv, sk_max, keys_per_split, false, "mxfp4 decode forward",
      [&](void* q4, void* qs, void* opart, void* ml, int64_t bhv, int64_t rows, int kps, void* stream) {
        return qattn_mxfp4_attn_fwd_split_len(q4, qs, P(k4), P(ks), P(vt), P(vs), opart, ml, P(lens), bhv, Hkv,
                                              rows, Sq, cap, sk_max, causal ? 2 : 0, kps, 128, qk_scale(128),
                                              stream);
      });
}

// kv_cache_mxfp4.attention_mxfp4_decode_paged on a page pool's operands: k4 [num_pages, Hkv, P, 64] with
// lens i32 [B] and block_table i32 [B, max_pages_per_seq] on the device.  As for mxfp4_decode the caller
// guarantees what the operator cannot read: 1 <= lens[b] <= sk_max, the pages of every sequence named in
// its table row and, causal, lens[b] >= Sq; the Python wrapper ops.mxfp4_decode_paged checks the lengths
// on the cache's host mirror.
std::tuple<Tensor, Tensor> mxfp4_decode_paged(const Tensor& q_in, const Tensor& k4, const Tensor& ks,
                                              const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                              const Tensor& block_table, int64_t sk_max, int64_t causal,
                                              int64_t keys_per_split) {
  require_gpu({&q_in, &k4, &ks, &vt, &vs, &lens, &block_table});
  TORCH_CHECK(q_in.dim() == 4 && k4.dim() == 4 && q_in.size(3) == 128 && k4.size(3) == 64,
              "qattn mxfp4 paged cache: head_dim must be 128 in q and in the pool");
  const int64_t NP = k4.size(0), Hkv = k4.size(1), PT = k4.size(2);
  TORCH_CHECK(PT >= 64 && PT <= 1024 && (PT & (PT - 1)) == 0,
              "qattn mxfp4 paged cache: page_tokens must be 64 * 2^k in [64, 1024]");
  TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.is_contiguous() && block_table.dim() == 2 &&
                  block_table.size(1) >= 1,
              "qattn mxfp4 paged cache: block_table must be contiguous int32 [B, max_pages_per_seq]");
  const int64_t B = block_table.size(0), mpp = block_table.size(1);
  TORCH_CHECK(q_in.size(0) == B && Hkv > 0 && NP > 0 && q_in.size(1) % Hkv == 0,
              "qattn mxfp4 paged cache: q must be [B, G*Hkv, Sq, D] for the table's B and the pool's Hkv");
  const int64_t Sq = q_in.size(2);
  TORCH_CHECK(Sq >= 1, "qattn mxfp4 paged cache: Sq >= 1 expected");
  TORCH_CHECK(sk_max >= 64 && sk_max % 64 == 0 && sk_max <= mpp * PT,
              "qattn mxfp4 paged cache: sk_max must be a multiple of 64 in [64, max_pages_per_seq * page_tokens]");
  TORCH_CHECK(causal == 0 || causal == 1, "qattn mxfp4 paged cache: causal must be 0 or 1");
  TORCH_CHECK(!causal || Sq <= sk_max, "qattn mxfp4 paged cache: causal attention needs Sq <= the cached tokens");
  check_fp4_operands(k4, ks, vt, vs, &lens, B, true);
  return fp4_split_and_merge(
      q_in, Hkv, sk_max, keys_per_split, true, "mxfp4 paged decode forward",
      [&](void* q4, void* qs, void* opart, void* ml, int64_t bhv, int64_t rows, int kps, void* stream) {
        return qattn_mxfp4_attn_fwd_split_paged(q4, qs, P(k4), P(ks), P(vt), P(vs), opart, ml, P(lens),
                                                P(block_table), bhv, Hkv, rows, Sq, NP, PT, mpp, sk_max,
                                                causal ? 2 : 0, kps, 128, qk_scale(128), stream);
      });
}

// The rotary arguments of an operator (attention_mxfp4.Rope and device positions), checked
struct RopeArgs {
  const Tensor& cos_sin;
  const Tensor& pos;
  bool interleaved;
};
void check_rope(const RopeArgs& r, int64_t tokens) {
  require_gpu({&r.cos_sin, &r.pos});
  TORCH_CHECK(r.cos_sin.scalar_type() == at::kFloat && r.cos_sin.is_contiguous() && r.cos_sin.dim() == 2 &&
                  r.cos_sin.size(1) == 128 && r.cos_sin.size(0) >= 1,
              "qattn mxfp4 rope: the table must be a contiguous fp32 tensor [max_pos >= 1, 128]");
  TORCH_CHECK(r.pos.scalar_type() == at::kInt && r.pos.is_contiguous() && r.pos.dim() == 1 &&
                  r.pos.size(0) == tokens,
              "qattn mxfp4 rope: positions must be a contiguous int32 tensor [T], one per packed token");
}

// attention_mxfp4.mxfp4_quantize_rows_rope: packed x [T, H, 128], each row rotated by pos[token] first
std::tuple<Tensor, Tensor> mxfp4_quant_rows_rope(const Tensor& x_in, const Tensor& cos_sin, const Tensor& pos,
                                                 bool interleaved) {
  require_gpu({&x_in});
  TORCH_CHECK(x_in.dim() == 3 && x_in.size(2) == 128, "qattn mxfp4 rope: packed rows must be x [T, H, 128]");
  const int64_t T = x_in.size(0), H = x_in.size(1), D = 128;
  const RopeArgs rope{cos_sin, pos, interleaved};
  check_rope(rope, T);
  Ctx c(x_in);
  const Tensor x = kin(x_in, at::kHalf), p = kin(pos);
  Tensor q4 = empty({T * H, D / 2}, at::kByte, x), qs = empty({T * H, D / 32}, at::kByte, x);
  call(qattn_mxfp4_quant_rows_rope(P(x), P(q4), P(qs), P(cos_sin), P(p), T, H, cos_sin.size(0), interleaved,
                                   (int)D, c.stream),
       "quantise rotated rows");
  return {q4, qs};
}

// kv_cache_mxfp4.attention_mxfp4_varlen_paged on a page pool's operands: packed q [T, Hq, 128], lens i32
// [B] and block_table i32 [B, max_pages_per_seq] on the device, and the two tables of
// kv_cache_mxfp4.plan_varlen as device tensors, seq_rec i32 [nseq, 8] and work i32 [nwork, 4], with the
// plan's part_rows and keys_per_split.  The operator cannot read any of them without a synchronisation:
// the caller guarantees that they are a plan of the pool's lengths (the Python wrapper
// ops.mxfp4_varlen_paged builds them from the cache's host mirror); the kernels keep every address a
// wrong table names inside the buffers.  With `windowed` the plan is plan_varlen's for (window, sinks) and
// the forward is qattn_mxfp4_attn_fwd_varlen_paged_window.  With `rope` q is rotated inside its quantiser.
std::tuple<Tensor, Tensor> mxfp4_varlen_paged_run(const Tensor& q_in, const Tensor& k4, const Tensor& ks,
                                                  const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                                  const Tensor& block_table, const Tensor& seq_rec,
                                                  const Tensor& work, int64_t part_rows, int64_t causal,
                                                  int64_t keys_per_split, bool windowed, int64_t window,
                                                  int64_t sinks, const Tensor* grp_rec = nullptr,
                                                  const Tensor* members = nullptr,
                                                  const Tensor* tree = nullptr,
                                                  const RopeArgs* rope = nullptr) {
  require_gpu({&q_in, &k4, &ks, &vt, &vs, &lens, &block_table, &seq_rec, &work});
  if (rope) check_rope(*rope, q_in.dim() == 3 ? q_in.size(0) : -1);
  if (tree) {   // the tree entry's ancestor words, one per packed token
    require_gpu({tree});
    TORCH_CHECK(tree->scalar_type() == at::kLong && tree->is_contiguous() && tree->dim() == 1 &&
                    q_in.dim() == 3 && tree->size(0) == q_in.size(0),
                "qattn mxfp4 paged cache: tree_masks must be contiguous int64 [T], one word per packed token");
  }
  if (grp_rec) {   // the shared-prefix plan's two further tables
    require_gpu({grp_rec, members});
    TORCH_CHECK(grp_rec->scalar_type() == at::kInt && grp_rec->is_contiguous() && grp_rec->dim() == 2 &&
                    grp_rec->size(1) == 4 && grp_rec->size(0) >= 1,
                "qattn mxfp4 paged cache: grp_rec must be contiguous int32 [ngroup >= 1, 4]");
    TORCH_CHECK(members->scalar_type() == at::kInt && members->is_contiguous() && members->dim() == 2 &&
                    members->size(1) == 2 && members->size(0) >= 2 * grp_rec->size(0) &&
                    members->size(0) <= seq_rec.size(0),
                "qattn mxfp4 paged cache: members must be contiguous int32 [nmember, 2], 2 * ngroup <= nmember "
                "<= nseq");
  }
  TORCH_CHECK(q_in.dim() == 3 && k4.dim() == 4 && q_in.size(2) == 128 && k4.size(3) == 64,
              "qattn mxfp4 paged cache: packed queries must be q [T, Hq, 128], head_dim 128 in the pool");
  const int64_t NP = k4.size(0), Hkv = k4.size(1), PT = k4.size(2), D = 128;
  TORCH_CHECK(PT >= 64 && PT <= 1024 && (PT & (PT - 1)) == 0,
              "qattn mxfp4 paged cache: page_tokens must be 64 * 2^k in [64, 1024]");
  TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.is_contiguous() && block_table.dim() == 2 &&
                  block_table.size(1) >= 1,
              "qattn mxfp4 paged cache: block_table must be contiguous int32 [B, max_pages_per_seq]");
  const int64_t B = block_table.size(0), mpp = block_table.size(1);
  const int64_t T = q_in.size(0), Hq = q_in.size(1);
  TORCH_CHECK(Hkv > 0 && NP > 0 && Hq > 0 && Hq % Hkv == 0,
              "qattn mxfp4 paged cache: q must have G * Hkv heads for the pool's Hkv");
  TORCH_CHECK(causal == 0 || causal == 1, "qattn mxfp4 paged cache: causal must be 0 or 1");
  check_fp4_operands(k4, ks, vt, vs, &lens, B, true);
  TORCH_CHECK(seq_rec.scalar_type() == at::kInt && seq_rec.is_contiguous() && seq_rec.dim() == 2 &&
                  seq_rec.size(1) == 8 && seq_rec.size(0) >= 1 && seq_rec.size(0) <= B,
              "qattn mxfp4 paged cache: seq_rec must be contiguous int32 [nseq, 8], 1 <= nseq <= B");
  TORCH_CHECK(work.scalar_type() == at::kInt && work.is_contiguous() && work.dim() == 2 && work.size(1) == 4,
              "qattn mxfp4 paged cache: work must be contiguous int32 [nwork, 4]");
  TORCH_CHECK(keys_per_split >= 64 && keys_per_split % 64 == 0,
              "qattn mxfp4 paged cache: keys_per_split must be a multiple of 64 (the plan's)");
  TORCH_CHECK(T >= seq_rec.size(0) && part_rows >= 1 && work.size(0) >= 1,
              "qattn mxfp4 paged cache: every listed sequence brings a token, a partial row and a work record");
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf);
  Tensor q4 = empty({T * Hq, D / 2}, at::kByte, q), qs = empty({T * Hq, D / 32}, at::kByte, q);
  Tensor out = empty({T, Hq, D}, at::kHalf, q), lse = empty({T, Hq}, at::kFloat, q);
  if (rope) {
    const Tensor p = kin(rope->pos);
    call(qattn_mxfp4_quant_rows_rope(P(q), P(q4), P(qs), P(rope->cos_sin), P(p), T, Hq, rope->cos_sin.size(0),
                                     rope->interleaved, (int)D, c.stream),
         "quantise rotated q");
  } else {
    call(qattn_mxfp4_quant_rows(P(q), nullptr, P(q4), P(qs), T * Hq, Hq, (int)D, c.stream), "quantise q");
  }
  Tensor opart = empty({part_rows, D}, at::kFloat, q), ml = empty({part_rows, 2}, at::kFloat, q);
  if (grp_rec)
    call(qattn_mxfp4_attn_fwd_varlen_paged_shared(
             P(q4), P(qs), P(k4), P(ks), P(vt), P(vs), P(opart), P(ml), P(lens), P(block_table), P(seq_rec),
             P(work), seq_rec.size(0), work.size(0), T, part_rows, B, Hkv, Hq / Hkv, NP, PT, mpp, causal ? 2 : 0,
             (int)keys_per_split, (int)D, qk_scale(D), P(*grp_rec), P(*members), grp_rec->size(0),
             members->size(0), c.stream),
         "mxfp4 shared-prefix varlen forward");
  else if (tree)
    call(qattn_mxfp4_attn_fwd_varlen_paged_tree(
             P(q4), P(qs), P(k4), P(ks), P(vt), P(vs), P(opart), P(ml), P(lens), P(block_table), P(seq_rec),
             P(work), seq_rec.size(0), work.size(0), T, part_rows, B, Hkv, Hq / Hkv, NP, PT, mpp, causal ? 2 : 0,
             (int)keys_per_split, (int)D, qk_scale(D), P(*tree), c.stream),
         "mxfp4 tree-masked varlen forward");
  else if (windowed)
    call(qattn_mxfp4_attn_fwd_varlen_paged_window(
             P(q4), P(qs), P(k4), P(ks), P(vt), P(vs), P(opart), P(ml), P(lens), P(block_table), P(seq_rec),
             P(work), seq_rec.size(0), work.size(0), T, part_rows, B, Hkv, Hq / Hkv, NP, PT, mpp, causal ? 2 : 0,
             (int)keys_per_split, (int)D, qk_scale(D), (long)window, (long)sinks, c.stream),
         "mxfp4 windowed varlen forward");
  else
    call(qattn_mxfp4_attn_fwd_varlen_paged(P(q4), P(qs), P(k4), P(ks), P(vt), P(vs), P(opart), P(ml), P(lens),
                                           P(block_table), P(seq_rec), P(work), seq_rec.size(0), work.size(0),
                                           T, part_rows, B, Hkv, Hq / Hkv, NP, PT, mpp, causal ? 2 : 0,
                                           (int)keys_per_split, (int)D, qk_scale(D), c.stream),
         "mxfp4 varlen forward");
  call(qattn_mxfp4_varlen_combine(P(opart), P(ml), P(out), P(lse), P(seq_rec), seq_rec.size(0), T, Hq, Hkv,
                                  part_rows, (int)D, c.stream),
       "mxfp4 varlen merge");
  return {out, lse};
}

std::tuple<Tensor, Tensor> mxfp4_varlen_paged(const Tensor& q, const Tensor& k4, const Tensor& ks,
                                              const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                              const Tensor& block_table, const Tensor& seq_rec,
                                              const Tensor& work, int64_t part_rows, int64_t causal,
                                              int64_t keys_per_split) {
  return mxfp4_varlen_paged_run(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal,
                                keys_per_split, false, 0, 0);
}

// the same with q rotated inside its quantiser (kv_cache_mxfp4.attention_mxfp4_varlen_paged(rope=)): cos_sin
// f32 [max_pos, 128] and pos i32 [T] on the device
std::tuple<Tensor, Tensor> mxfp4_varlen_paged_rope(const Tensor& q, const Tensor& k4, const Tensor& ks,
                                                   const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                                   const Tensor& block_table, const Tensor& seq_rec,
                                                   const Tensor& work, int64_t part_rows, int64_t causal,
                                                   int64_t keys_per_split, const Tensor& cos_sin,
                                                   const Tensor& pos, bool interleaved) {
  const RopeArgs rope{cos_sin, pos, interleaved};
  return mxfp4_varlen_paged_run(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal,
                                keys_per_split, false, 0, 0, nullptr, nullptr, nullptr, &rope);
}

// the same with a sliding window and sinks (kv_cache_mxfp4.attention_mxfp4_varlen_paged(window=, sinks=)):
// causal only; seq_rec and work are plan_varlen's for the same (window, sinks)
std::tuple<Tensor, Tensor> mxfp4_varlen_paged_window(const Tensor& q, const Tensor& k4, const Tensor& ks,
                                                     const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                                     const Tensor& block_table, const Tensor& seq_rec,
                                                     const Tensor& work, int64_t part_rows, int64_t causal,
                                                     int64_t keys_per_split, int64_t window, int64_t sinks) {
  TORCH_CHECK(window >= 1 && sinks >= 0, "qattn mxfp4 paged cache: window >= 1 and sinks >= 0 expected");
  TORCH_CHECK(causal == 1, "qattn mxfp4 paged cache: a window implies causal attention (causal must be 1)");
  return mxfp4_varlen_paged_run(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal,
                                keys_per_split, true, window, sinks);
}

// the same with shared prefixes (kv_cache_mxfp4.attention_mxfp4_varlen_paged(share_prefix=True)): the
// tables are plan_varlen_shared's, grp_rec i32 [ngroup, 4] and members i32 [nmember, 2] among them
std::tuple<Tensor, Tensor> mxfp4_varlen_paged_shared(const Tensor& q, const Tensor& k4, const Tensor& ks,
                                                     const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                                     const Tensor& block_table, const Tensor& seq_rec,
                                                     const Tensor& work, const Tensor& grp_rec,
                                                     const Tensor& members, int64_t part_rows, int64_t causal,
                                                     int64_t keys_per_split) {
  return mxfp4_varlen_paged_run(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal,
                                keys_per_split, false, 0, 0, &grp_rec, &members);
}

// the same with a tree mask on every sequence's last queries (kv_cache_mxfp4.attention_mxfp4_varlen_paged(
// tree=)): causal only; seq_rec is plan_varlen's with the tree lengths, tree_masks i64 [T] the ancestor word
// of every packed token (0 outside a tree)
std::tuple<Tensor, Tensor> mxfp4_varlen_paged_tree(const Tensor& q, const Tensor& k4, const Tensor& ks,
                                                   const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                                   const Tensor& block_table, const Tensor& seq_rec,
                                                   const Tensor& work, const Tensor& tree_masks,
                                                   int64_t part_rows, int64_t causal, int64_t keys_per_split) {
  TORCH_CHECK(causal == 1, "qattn mxfp4 paged cache: a tree mask implies causal attention (causal must be 1)");
  return mxfp4_varlen_paged_run(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal,
                                keys_per_split, false, 0, 0, nullptr, nullptr, &tree_masks);
}

// kv_cache_mxfp4.DecodeStep's plan as an operator: from slots i32 [n] and the pool's lens i32 [B] (the lengths
// BEFORE the step's append) the four device tables of qattn_mxfp4_decode_step_plan, seq_tab i32 [n, 4], tiles
// i32 [n, 2], pos i32 [n] and seq_rec i32 [n, 8].  Nothing is read back; window 0: none.
std::tuple<Tensor, Tensor, Tensor, Tensor> mxfp4_decode_step_plan(const Tensor& slots, const Tensor& lens,
                                                                  int64_t capacity, int64_t kv_heads,
                                                                  int64_t group, int64_t keys_per_split,
                                                                  int64_t splits, int64_t window, int64_t sinks) {
  require_gpu({&slots, &lens});
  TORCH_CHECK(slots.scalar_type() == at::kInt && slots.is_contiguous() && slots.dim() == 1 && slots.size(0) >= 1,
              "qattn mxfp4 decode step: slots must be contiguous int32 [n >= 1]");
  TORCH_CHECK(lens.scalar_type() == at::kInt && lens.is_contiguous() && lens.dim() == 1 && lens.size(0) >= 1,
              "qattn mxfp4 decode step: lens must be contiguous int32 [max_seqs]");
  TORCH_CHECK(keys_per_split >= 64 && keys_per_split % 64 == 0,
              "qattn mxfp4 decode step: keys_per_split must be a multiple of 64");
  const int64_t n = slots.size(0);
  Ctx c(slots);
  Tensor seq_tab = empty({n, 4}, at::kInt, slots), tiles = empty({n, 2}, at::kInt, slots);
  Tensor pos = empty({n}, at::kInt, slots), seq_rec = empty({n, 8}, at::kInt, slots);
  call(qattn_mxfp4_decode_step_plan(P(slots), P(lens), P(seq_tab), P(tiles), P(seq_rec), P(pos), n, lens.size(0),
                                    capacity, kv_heads, group, (int)keys_per_split, splits, window, sinks,
                                    c.stream),
       "mxfp4 decode step plan");
  return {seq_tab, tiles, pos, seq_rec};
}

// kv_cache_mxfp4.DecodeStep.attend as an operator: q [n, Hq, 128], the pool's operands, lens (AFTER the step's
// append) and block table, seq_rec i32 [n, 8] of the plan above and work i32 [n * splits, 4] = {i, 0, s, 0}.
std::tuple<Tensor, Tensor> mxfp4_decode_step(const Tensor& q_in, const Tensor& k4, const Tensor& ks,
                                             const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                             const Tensor& block_table, const Tensor& seq_rec, const Tensor& work,
                                             int64_t splits, int64_t keys_per_split, int64_t window,
                                             int64_t sinks) {
  require_gpu({&q_in, &k4, &ks, &vt, &vs, &lens, &block_table, &seq_rec, &work});
  TORCH_CHECK(q_in.dim() == 3 && k4.dim() == 4 && q_in.size(2) == 128 && k4.size(3) == 64,
              "qattn mxfp4 decode step: q must be [n, Hq, 128], head_dim 128 in the pool");
  const int64_t NP = k4.size(0), Hkv = k4.size(1), PT = k4.size(2), D = 128;
  TORCH_CHECK(PT >= 64 && PT <= 1024 && (PT & (PT - 1)) == 0,
              "qattn mxfp4 paged cache: page_tokens must be 64 * 2^k in [64, 1024]");
  TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.is_contiguous() && block_table.dim() == 2 &&
                  block_table.size(1) >= 1,
              "qattn mxfp4 paged cache: block_table must be contiguous int32 [B, max_pages_per_seq]");
  const int64_t B = block_table.size(0), mpp = block_table.size(1);
  const int64_t n = q_in.size(0), Hq = q_in.size(1);
  TORCH_CHECK(Hkv > 0 && NP > 0 && Hq > 0 && Hq % Hkv == 0 && n >= 1 && n <= B,
              "qattn mxfp4 decode step: q must have G * Hkv heads for the pool's Hkv and 1 <= n <= B rows");
  check_fp4_operands(k4, ks, vt, vs, &lens, B, true);
  TORCH_CHECK(splits >= 1 && splits <= 65535 && n * splits * Hq < (int64_t(1) << 31),
              "qattn mxfp4 decode step: splits in [1, 65535] and fewer than 2^31 partial rows expected");
  TORCH_CHECK(seq_rec.scalar_type() == at::kInt && seq_rec.is_contiguous() && seq_rec.dim() == 2 &&
                  seq_rec.size(1) == 8 && seq_rec.size(0) == n,
              "qattn mxfp4 decode step: seq_rec must be contiguous int32 [n, 8]");
  TORCH_CHECK(work.scalar_type() == at::kInt && work.is_contiguous() && work.dim() == 2 && work.size(1) == 4 &&
                  work.size(0) == n * splits,
              "qattn mxfp4 decode step: work must be contiguous int32 [n * splits, 4]");
  TORCH_CHECK(keys_per_split >= 64 && keys_per_split % 64 == 0,
              "qattn mxfp4 decode step: keys_per_split must be a multiple of 64");
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf);
  Tensor q4 = empty({n * Hq, D / 2}, at::kByte, q), qs = empty({n * Hq, D / 32}, at::kByte, q);
  Tensor out = empty({n, Hq, D}, at::kHalf, q), lse = empty({n, Hq}, at::kFloat, q);
  Tensor opart = empty({n * splits * Hq, D}, at::kFloat, q), ml = empty({n * splits * Hq, 2}, at::kFloat, q);
  call(qattn_mxfp4_quant_rows(P(q), nullptr, P(q4), P(qs), n * Hq, Hq, (int)D, c.stream), "quantise q");
  call(qattn_mxfp4_attn_fwd_decode_step(P(q4), P(qs), P(k4), P(ks), P(vt), P(vs), P(opart), P(ml), P(lens),
                                        P(block_table), P(seq_rec), P(work), n, splits, B, Hkv, Hq / Hkv, NP, PT,
                                        mpp, (int)keys_per_split, (int)D, qk_scale(D), window, sinks, c.stream),
       "mxfp4 decode step forward");
  call(qattn_mxfp4_decode_step_combine(P(opart), P(ml), P(out), P(lse), P(seq_rec), n, splits, Hq, Hkv, (int)D,
                                       c.stream),
       "mxfp4 decode step merge");
  return {out, lse};
}

// kv_cache_mxfp4.VerifyStep's plan as an operator: from slots i32 [n], the pool's lens i32 [B] (the lengths BEFORE
// the step's append) and the ancestor words tree i64 [n * K] the four device tables of
// qattn_mxfp4_verify_step_plan, seq_tab i32 [n, 4], tiles i32 [2 n, 2], pos i32 [n * K] and seq_rec i32 [n, 8].
// Nothing is read back.
std::tuple<Tensor, Tensor, Tensor, Tensor> mxfp4_verify_step_plan(const Tensor& slots, const Tensor& lens,
                                                                  const Tensor& tree, int64_t draft_tokens,
                                                                  int64_t capacity, int64_t kv_heads,
                                                                  int64_t group, int64_t keys_per_split,
                                                                  int64_t splits) {
  require_gpu({&slots, &lens, &tree});
  TORCH_CHECK(slots.scalar_type() == at::kInt && slots.is_contiguous() && slots.dim() == 1 && slots.size(0) >= 1,
              "qattn mxfp4 verify step: slots must be contiguous int32 [n >= 1]");
  TORCH_CHECK(lens.scalar_type() == at::kInt && lens.is_contiguous() && lens.dim() == 1 && lens.size(0) >= 1,
              "qattn mxfp4 verify step: lens must be contiguous int32 [max_seqs]");
  TORCH_CHECK(draft_tokens >= 1 && draft_tokens <= 64, "qattn mxfp4 verify step: draft_tokens must be in [1, 64]");
  const int64_t n = slots.size(0), K = draft_tokens;
  TORCH_CHECK(tree.scalar_type() == at::kLong && tree.is_contiguous() && tree.dim() == 1 && tree.size(0) == n * K,
              "qattn mxfp4 verify step: tree must be contiguous int64 [n * draft_tokens]");
  TORCH_CHECK(keys_per_split >= 64 && keys_per_split % 64 == 0,
              "qattn mxfp4 verify step: keys_per_split must be a multiple of 64");
  Ctx c(slots);
  Tensor seq_tab = empty({n, 4}, at::kInt, slots), tiles = empty({2 * n, 2}, at::kInt, slots);
  Tensor pos = empty({n * K}, at::kInt, slots), seq_rec = empty({n, 8}, at::kInt, slots);
  call(qattn_mxfp4_verify_step_plan(P(slots), P(lens), P(tree), P(seq_tab), P(tiles), P(seq_rec), P(pos), n, K,
                                    lens.size(0), capacity, kv_heads, group, (int)keys_per_split, splits, c.stream),
       "mxfp4 verify step plan");
  return {seq_tab, tiles, pos, seq_rec};
}

// kv_cache_mxfp4.VerifyStep.attend as an operator: q [n * K, Hq, 128], the pool's operands, lens (AFTER the step's
// append) and block table, seq_rec i32 [n, 8] of the plan above, work i32 [n * nrb * splits, 4] = {i, row block, s,
// 0} with nrb = ceil(G * K / 128), and the words tree i64 [n * K].
std::tuple<Tensor, Tensor> mxfp4_verify_step(const Tensor& q_in, const Tensor& k4, const Tensor& ks,
                                             const Tensor& vt, const Tensor& vs, const Tensor& lens,
                                             const Tensor& block_table, const Tensor& seq_rec, const Tensor& work,
                                             const Tensor& tree, int64_t draft_tokens, int64_t splits,
                                             int64_t keys_per_split) {
  require_gpu({&q_in, &k4, &ks, &vt, &vs, &lens, &block_table, &seq_rec, &work, &tree});
  TORCH_CHECK(q_in.dim() == 3 && k4.dim() == 4 && q_in.size(2) == 128 && k4.size(3) == 64,
              "qattn mxfp4 verify step: q must be [n * draft_tokens, Hq, 128], head_dim 128 in the pool");
  const int64_t NP = k4.size(0), Hkv = k4.size(1), PT = k4.size(2), D = 128, K = draft_tokens;
  TORCH_CHECK(PT >= 64 && PT <= 1024 && (PT & (PT - 1)) == 0,
              "qattn mxfp4 paged cache: page_tokens must be 64 * 2^k in [64, 1024]");
  TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.is_contiguous() && block_table.dim() == 2 &&
                  block_table.size(1) >= 1,
              "qattn mxfp4 paged cache: block_table must be contiguous int32 [B, max_pages_per_seq]");
  TORCH_CHECK(K >= 1 && K <= 64 && q_in.size(0) >= K && q_in.size(0) % K == 0,
              "qattn mxfp4 verify step: draft_tokens in [1, 64] and q rows a multiple of it expected");
  const int64_t B = block_table.size(0), mpp = block_table.size(1);
  const int64_t n = q_in.size(0) / K, Hq = q_in.size(1);
  TORCH_CHECK(Hkv > 0 && NP > 0 && Hq > 0 && Hq % Hkv == 0 && n <= B,
              "qattn mxfp4 verify step: q must have G * Hkv heads for the pool's Hkv and at most B entries");
  check_fp4_operands(k4, ks, vt, vs, &lens, B, true);
  TORCH_CHECK(splits >= 1 && splits <= 65535 && n * splits * Hq * K < (int64_t(1) << 31),
              "qattn mxfp4 verify step: splits in [1, 65535] and fewer than 2^31 partial rows expected");
  const int64_t nrb = (Hq / Hkv * K + 127) / 128;
  TORCH_CHECK(seq_rec.scalar_type() == at::kInt && seq_rec.is_contiguous() && seq_rec.dim() == 2 &&
                  seq_rec.size(1) == 8 && seq_rec.size(0) == n,
              "qattn mxfp4 verify step: seq_rec must be contiguous int32 [n, 8]");
  TORCH_CHECK(work.scalar_type() == at::kInt && work.is_contiguous() && work.dim() == 2 && work.size(1) == 4 &&
                  work.size(0) == n * nrb * splits,
              "qattn mxfp4 verify step: work must be contiguous int32 [n * row blocks * splits, 4]");
  TORCH_CHECK(tree.scalar_type() == at::kLong && tree.is_contiguous() && tree.dim() == 1 && tree.size(0) == n * K,
              "qattn mxfp4 verify step: tree must be contiguous int64 [n * draft_tokens]");
  TORCH_CHECK(keys_per_split >= 64 && keys_per_split % 64 == 0,
              "qattn mxfp4 verify step: keys_per_split must be a multiple of 64");
  Ctx c(q_in);
  const Tensor q = kin(q_in, at::kHalf);
  const int64_t T = n * K;
  Tensor q4 = empty({T * Hq, D / 2}, at::kByte, q), qs = empty({T * Hq, D / 32}, at::kByte, q);
  Tensor out = empty({T, Hq, D}, at::kHalf, q), lse = empty({T, Hq}, at::kFloat, q);
  Tensor opart = empty({n * splits * Hq * K, D}, at::kFloat, q), ml = empty({n * splits * Hq * K, 2}, at::kFloat, q);
  call(qattn_mxfp4_quant_rows(P(q), nullptr, P(q4), P(qs), T * Hq, Hq, (int)D, c.stream), "quantise q");
  call(qattn_mxfp4_attn_fwd_verify_step(P(q4), P(qs), P(k4), P(ks), P(vt), P(vs), P(opart), P(ml), P(lens),
                                        P(block_table), P(seq_rec), P(work), P(tree), n, K, splits, B, Hkv,
                                        Hq / Hkv, NP, PT, mpp, (int)keys_per_split, (int)D, qk_scale(D), c.stream),
       "mxfp4 verify step forward");
  call(qattn_mxfp4_verify_step_combine(P(opart), P(ml), P(out), P(lse), P(seq_rec), n, K, splits, Hq, Hkv, (int)D,
                                       c.stream),
       "mxfp4 verify step merge");
  return {out, lse};
}

}  // namespace

TORCH_LIBRARY(qattn, m) {
  m.def("int8_quant(Tensor x, int block) -> (Tensor, Tensor)");
  m.def("int8_fwd(Tensor q, Tensor k, Tensor v, bool smooth, bool causal) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("int8_bwd(Tensor dO, Tensor q_i8, Tensor sq, Tensor k_i8, Tensor sk, Tensor v_i8, Tensor sv, "
        "Tensor O, Tensor lse, bool causal, int kv_heads) -> (Tensor, Tensor, Tensor)");
  m.def("bf16_fwd(Tensor q, Tensor k, Tensor v, bool causal) -> (Tensor, Tensor)");
  m.def("bf16_bwd(Tensor q, Tensor k, Tensor v, Tensor O, Tensor lse, bool causal, Tensor dO) -> "
        "(Tensor, Tensor, Tensor)");
  m.def("jvp_fwd(Tensor q, Tensor k, Tensor v, Tensor tq, Tensor tk, Tensor tv) -> (Tensor, Tensor, Tensor)");
  m.def("mxfp4_fwd(Tensor q, Tensor k, Tensor v) -> Tensor");
  m.def("mxfp4_fwd_ex(Tensor q, Tensor k, Tensor v, int causal) -> Tensor");
  m.def("mxfp4_cached(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, int causal, int keys_per_split) -> "
        "(Tensor, Tensor)");
  m.def("mxfp4_decode(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, int sk_max, int causal, "
        "int keys_per_split) -> (Tensor, Tensor)");
  m.def("mxfp4_decode_paged(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, Tensor block_table, "
        "int sk_max, int causal, int keys_per_split) -> (Tensor, Tensor)");
  m.def("mxfp4_varlen_paged(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, Tensor block_table, "
        "Tensor seq_rec, Tensor work, int part_rows, int causal, int keys_per_split) -> (Tensor, Tensor)");
  m.def("mxfp4_varlen_paged_window(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, "
        "Tensor block_table, Tensor seq_rec, Tensor work, int part_rows, int causal, int keys_per_split, "
        "int window, int sinks) -> (Tensor, Tensor)");
  m.def("mxfp4_varlen_paged_shared(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, "
        "Tensor block_table, Tensor seq_rec, Tensor work, Tensor grp_rec, Tensor members, int part_rows, "
        "int causal, int keys_per_split) -> (Tensor, Tensor)");
  m.def("mxfp4_varlen_paged_tree(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, "
        "Tensor block_table, Tensor seq_rec, Tensor work, Tensor tree_masks, int part_rows, int causal, "
        "int keys_per_split) -> (Tensor, Tensor)");
  m.def("mxfp4_quant_rows_rope(Tensor x, Tensor cos_sin, Tensor pos, bool interleaved) -> (Tensor, Tensor)");
  m.def("mxfp4_varlen_paged_rope(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, "
        "Tensor block_table, Tensor seq_rec, Tensor work, int part_rows, int causal, int keys_per_split, "
        "Tensor cos_sin, Tensor pos, bool interleaved) -> (Tensor, Tensor)");
  m.def("mxfp4_decode_step_plan(Tensor slots, Tensor lens, int capacity, int kv_heads, int group, "
        "int keys_per_split, int splits, int window, int sinks) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("mxfp4_decode_step(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, Tensor block_table, "
        "Tensor seq_rec, Tensor work, int splits, int keys_per_split, int window, int sinks) -> (Tensor, Tensor)");
  m.def("mxfp4_verify_step_plan(Tensor slots, Tensor lens, Tensor tree, int draft_tokens, int capacity, "
        "int kv_heads, int group, int keys_per_split, int splits) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("mxfp4_verify_step(Tensor q, Tensor k4, Tensor ks, Tensor vt, Tensor vs, Tensor lens, Tensor block_table, "
        "Tensor seq_rec, Tensor work, Tensor tree, int draft_tokens, int splits, int keys_per_split) "
        "-> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(qattn, CUDA, m) {
  m.impl("int8_quant", &int8_quant);
  m.impl("int8_fwd", &int8_fwd);
  m.impl("int8_bwd", &int8_bwd);
  m.impl("bf16_fwd", &bf16_fwd);
  m.impl("bf16_bwd", &bf16_bwd);
  m.impl("jvp_fwd", &jvp_fwd);
  m.impl("mxfp4_fwd", &mxfp4_fwd);
  m.impl("mxfp4_fwd_ex", &mxfp4_fwd_ex);
  m.impl("mxfp4_cached", &mxfp4_cached);
  m.impl("mxfp4_decode", &mxfp4_decode);
  m.impl("mxfp4_decode_paged", &mxfp4_decode_paged);
  m.impl("mxfp4_varlen_paged", &mxfp4_varlen_paged);
  m.impl("mxfp4_varlen_paged_window", &mxfp4_varlen_paged_window);
  m.impl("mxfp4_varlen_paged_shared", &mxfp4_varlen_paged_shared);
  m.impl("mxfp4_varlen_paged_tree", &mxfp4_varlen_paged_tree);
  m.impl("mxfp4_quant_rows_rope", &mxfp4_quant_rows_rope);
  m.impl("mxfp4_varlen_paged_rope", &mxfp4_varlen_paged_rope);
  m.impl("mxfp4_decode_step_plan", &mxfp4_decode_step_plan);
  m.impl("mxfp4_decode_step", &mxfp4_decode_step);
  m.impl("mxfp4_verify_step_plan", &mxfp4_verify_step_plan);
  m.impl("mxfp4_verify_step", &mxfp4_verify_step);
}
