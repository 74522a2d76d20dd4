"""MX-FP4 key/value cache, its wire format and the key-split decoding forward.

The MX-FP4 forward (attention_mxfp4.py) quantises K along head_dim per key row and V along the keys
inside one 64-key tile, so the quantised operands of a sequence are the concatenation of the
operands of its 64-key tiles: they are the natural cache.  :class:`QuantizedKVFP4` keeps them in HBM
-- 136 B per key and key/value head at D = 128 (K 64 + 4, V 64 + 4) against about 256 B for the int8
cache of kv_cache.py -- grows them by 64-token tiles and moves them in one self-describing buffer.
:func:`attention_mxfp4_cached` runs fp16 queries of ANY length >= 1 against the cache in the decoding
layout: the grouped query heads of a key/value head form one virtual head of G * Sq rows (one
workgroup reads each key/value tile once for the whole group), long caches are split over the keys
(``qattn_mxfp4_attn_fwd_split``) and the splits are merged (``qattn_mxfp4_split_combine``).  The
splits keep the unnormalised fp32 state and integer running maxima, so the merge's weights are exact
powers of two; with one split the result is the one-pass forward's bit for bit.

Granularity: a :class:`QuantizedKVFP4` grows by 64 tokens and every ``append`` copies it (it is the
immutable form: what is quantised once, serialised and moved).  A decode loop uses
:class:`PreallocatedKVFP4`: the same four operands at a fixed capacity per key/value head, one length
per sequence on the device (``lens``) with a host mirror (``lengths``), and ``append`` of ANY token
count, a different one per sequence if wanted, written in place by ``qattn_mxfp4_cache_append``
without a host synchronisation.  K is quantised per key row, so a key is appended alone; V's blocks
lie inside one 64-key tile, so only the sequence's last partial tile is quantised again, from its fp16
rows kept in ``vtail``.  The invariant that defines the format: after any sequence of appends, rows
[0, L) of ``k4`` / ``ks`` and tiles [0, ceil(L / 64)) of ``vt`` / ``vs`` equal, bit for bit, what
``quantize_kv_fp4(k, v, smooth=False, k_mean=...)`` gives for the sequence zero-padded to the next
multiple of 64; K rows at or past L and V tiles at or past ceil(L / 64) are unspecified and never
influence a result.  :func:`attention_mxfp4_decode` attends to such a cache
(``qattn_mxfp4_attn_fwd_split_len``: the key-split forward with a length per sequence; a split past a
sequence's end exits at once).  ``lse`` (base 2) is returned so that results can still be merged with
attention over keys held elsewhere; with a smoothed cache it is that of the scores q . (k - k_mean).

Wire format (little-endian), the container of kv_cache.py with a magic of its own::

    offset 0   8 B   magic  b"QATTNKF4"
    offset 8   4 B   header length H (uint32)
    offset 12  H B   UTF-8 JSON header: {"format": "mxfp4", "batch", "kv_heads", "tokens", "head_dim",
                     "block": 64, "smoothed": bool, "sections": {name: [offset, nbytes, dtype, shape]}}
    then the sections, each 256-byte aligned, offsets from the start of the buffer:
      k4      uint8   [batch, kv_heads, tokens, head_dim/2]      e2m1 pairs, low nibble first
      ks      uint8   [batch, kv_heads, tokens, head_dim/32]     e8m0 scale per 32 elements of a row
      vt      uint8   [batch*kv_heads, tokens/64, head_dim, 32]  V^T in operand key order
      vs      uint8   [batch*kv_heads, tokens/64, head_dim, 2]   e8m0 scale per 32 keys of a column
      k_mean  float16 [batch, kv_heads, 1, head_dim]             only when "smoothed"

Causal attention against a cache is bottom-right: the Sq queries are the LAST Sq positions (query i
keeps the keys <= Sk - Sq + i), Sq <= Sk.
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .attention_mxfp4 import _qk_scale, mxfp4_quantize_rows, mxfp4_quantize_v

MAGIC = b"QATTNKF4"
BLOCK = 64
_ALIGN = 256
_DTYPES = {"uint8": torch.uint8, "float16": torch.float16}

__all__ = ["QuantizedKVFP4", "quantize_kv_fp4", "attention_mxfp4_cached", "PreallocatedKVFP4",
           "attention_mxfp4_decode"]


@dataclass
class QuantizedKVFP4:
    """MX-FP4 keys/values of ``batch x kv_heads`` heads with ``tokens`` tokens each.

    ``k4`` u8 [B, Hkv, S, D/2], ``ks`` u8 [B, Hkv, S, D/32], ``vt`` u8 [B*Hkv, S/64, D, 32], ``vs`` u8
    [B*Hkv, S/64, D, 2] (layouts: csrc/mxfp4_attn.hip); ``k_mean`` f16 [B, Hkv, 1, D] when the keys
    were smoothed before quantisation, else None.
    """

    k4: torch.Tensor
    ks: torch.Tensor
    vt: torch.Tensor
    vs: torch.Tensor
    k_mean: Optional[torch.Tensor] = None

    @property
    def shape(self):
        B, H, S, D2 = self.k4.shape
        return (B, H, S, 2 * D2)

    @property
    def kv(self):
        """The ``kv`` tuple of ``mxfp4_attn_fwd_kv``."""
        return (self.k4, self.ks, self.vt, self.vs)

    # ------------------------------------------------------------------------------ growth
    def append(self, k: torch.Tensor, v: torch.Tensor) -> "QuantizedKVFP4":
        """Quantise ``k, v`` [B, Hkv, n, D] (n % 64 == 0) and append them along the token axis.

        K's blocks lie inside one key row and V's inside one 64-key tile, so appended tiles are
        independent: for an unsmoothed cache the result is bit-identical to quantising the
        concatenated sequence.  A smoothed cache subtracts its stored ``k_mean`` (the mean of the
        tokens it was created from) from the new keys; softmax is invariant to that shift, but the
        codes differ from smoothing with the mean of the longer sequence.
        """
        B, H, S, D = self.shape
        if (k.dim() != 4 or tuple(k.shape[:2]) != (B, H) or k.shape[3] != D or k.shape != v.shape
                or k.shape[2] % BLOCK):
            raise _lib.QAttnError("qattn mxfp4 kv cache: appended tiles must be [B, Hkv, 64*n, D]")
        new = quantize_kv_fp4(k, v, smooth=False, k_mean=self.k_mean)
        return QuantizedKVFP4(torch.cat([self.k4, new.k4], 2), torch.cat([self.ks, new.ks], 2),
                              torch.cat([self.vt, new.vt], 1), torch.cat([self.vs, new.vs], 1),
                              self.k_mean)

    # ------------------------------------------------------------------------------ wire format
    def to_bytes(self) -> torch.Tensor:
        """Serialise into one uint8 tensor on the cache's device (see the module docstring)."""
        B, H, S, D = self.shape
        parts = [("k4", self.k4), ("ks", self.ks), ("vt", self.vt), ("vs", self.vs)]
        if self.k_mean is not None:
            parts.append(("k_mean", self.k_mean))
        sections, off = {}, 0
        for name, t in parts:
            nbytes = t.numel() * t.element_size()
            sections[name] = [off, nbytes, str(t.dtype).replace("torch.", ""), list(t.shape)]
            off += (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        header = {"format": "mxfp4", "batch": B, "kv_heads": H, "tokens": S, "head_dim": D,
                  "block": BLOCK, "smoothed": self.k_mean is not None, "sections": {}}
        hdr = json.dumps(header).encode()
        base = 0
        for _ in range(3):   # the header length depends on the offsets it holds
            base = (12 + len(hdr) + _ALIGN - 1) // _ALIGN * _ALIGN
            header["sections"] = {k_: [o + base, n, dt, sh] for k_, (o, n, dt, sh) in sections.items()}
            hdr = json.dumps(header).encode()
        assert (12 + len(hdr) + _ALIGN - 1) // _ALIGN * _ALIGN == base
        buf = torch.zeros(base + off, dtype=torch.uint8, device=self.k4.device)
        prefix = MAGIC + len(hdr).to_bytes(4, "little") + hdr
        buf[:len(prefix)] = torch.frombuffer(bytearray(prefix), dtype=torch.uint8).to(buf.device)
        for name, t in parts:
            o, n = header["sections"][name][:2]
            buf[o:o + n] = t.contiguous().view(-1).view(torch.uint8)
        return buf

    @staticmethod
    def from_bytes(buf: torch.Tensor, device=None) -> "QuantizedKVFP4":
        """Parse a buffer written by :meth:`to_bytes` (sections become views of ``buf``, moved to
        ``device`` if given); an int8 cache's buffer (kv_cache.py) is refused."""
        if device is not None:
            buf = buf.to(device)
        head = bytes(buf[:12].cpu().tolist())
        if head[:8] != MAGIC:
            raise _lib.QAttnError("qattn mxfp4 kv cache: bad magic (not a QATTNKF4 buffer)")
        hlen = int.from_bytes(head[8:12], "little")
        header = json.loads(bytes(buf[12:12 + hlen].cpu().tolist()).decode())
        if header.get("format") != "mxfp4" or header.get("block") != BLOCK:
            raise _lib.QAttnError("qattn mxfp4 kv cache: unsupported format or block size")
        t = {}
        for name, (o, n, dt, sh) in header["sections"].items():
            t[name] = buf[o:o + n].view(_DTYPES[dt]).view(sh)
        return QuantizedKVFP4(t["k4"], t["ks"], t["vt"], t["vs"], t.get("k_mean"))


def quantize_kv_fp4(k: torch.Tensor, v: torch.Tensor, smooth: bool = True,
                    k_mean: Optional[torch.Tensor] = None) -> QuantizedKVFP4:
    """Quantise fp16 ``k, v`` [B, Hkv, S, D] (S % 64 == 0, D = 128) to MX-FP4 on the GPU with the
    forward's quantisers.  ``smooth`` subtracts the per-head token mean from k first (SageAttention
    smoothing, as ``mxfp4_attn_fwd``); an explicit ``k_mean`` is used as given."""
    if k.dim() != 4 or k.shape != v.shape:
        raise _lib.QAttnError("qattn mxfp4 kv cache: k and v must be [B, Hkv, S, D] of one shape")
    B, H, S, D = k.shape
    if S % BLOCK or D != 128:
        raise _lib.QAttnError("qattn mxfp4 kv cache: tokens must be a multiple of 64, head_dim 128")
    _lib.require_gpu(k, v)
    k = k.to(torch.float16).contiguous()
    if smooth and k_mean is None:
        k_mean = torch.empty((B, H, 1, D), dtype=torch.float16, device=k.device)
        _lib.call("qattn_kmean", _lib.ptr(k), _lib.ptr(k_mean), B * H, S, D, _lib.stream_of(k))
    km = None if k_mean is None else k_mean.to(torch.float16).contiguous()
    k4, ks = mxfp4_quantize_rows(k, km)
    vt, vs = mxfp4_quantize_v(v)
    return QuantizedKVFP4(k4.view(B, H, S, D // 2), ks.view(B, H, S, D // 32), vt, vs, km)


MIN_SPLIT_KEYS = 1024   # (qattn_split_keys' constant, restated: the tests hold the plan to it)


def _split_plan_fp4(bhv: int, rows: int, sk: int) -> int:
    """Keys per split of the decoding forward, a multiple of 64: enough workgroups for two per CU
    (512), no split shorter than MIN_SPLIT_KEYS = 1024 keys (16 tiles); sk when one split suffices.
    kv_cache._split_plan's rule at 64-key tiles; its constants, measured for the int8 kernel, hold
    for this one.  Measured on MI355X (tools/time_decode_fp4.py --kps, D = 128, whole call, median of
    3 x 30 alternating calls): (B, Hq, Hkv, Sq, Sk) = (8, 32, 8, 32, 8192) 1024 keys 45 us (512: 53,
    2048: 49, 4096: 75, one pass 134); (8, 32, 32, 32, 8192) 4096 keys 93 us (1024: 92, 2048: 99,
    512: 106, one pass 160); (1, 32, 8, 32, 32768) 1024 keys 46 us (512: 59, 2048: 51, one pass
    481); (4, 32, 32, 128, 8192) 2048 keys 61 us (1024: 68, 4096: 77, one pass 130); (8, 32, 8, 1,
    8192) 1024 keys 47 us (256 to 2048: 47 to 48, 4096: 72).  Splits under 1024 keys lose at every
    shape with 32 or more query rows per head.  The rule itself is the library's (qattn_split_keys)."""
    return _lib.load().qattn_split_keys(bhv, rows, sk, BLOCK)


@torch.no_grad()
def attention_mxfp4_cached(q: torch.Tensor, kv: QuantizedKVFP4, causal: bool = False,
                           keys_per_split: Optional[int] = None):
    """MX-FP4 attention of fp16 queries [B, Hq, Sq, D] (any Sq >= 1) against a quantised cache ->
    (O fp16 [B, Hq, Sq, D], lse fp32 [B*Hq, Sq] base 2).  Inference; no autograd.

    Hq must be a multiple of the cache's heads.  ``causal``: the Sq queries are the LAST Sq positions
    (query i keeps keys <= Sk - Sq + i), Sq <= Sk.  ``keys_per_split`` (a multiple of 64) forces the
    split size; None takes ``_split_plan_fp4``.  A smoothed cache is queried as it is (softmax
    ignores the shift; lse is that of the smoothed scores, as ``mxfp4_attn_fwd`` returns it).
    """
    if not isinstance(kv, QuantizedKVFP4):
        raise _lib.QAttnError("qattn mxfp4 kv cache: kv must be a QuantizedKVFP4")
    _lib.require_gpu(q, kv.k4, kv.ks, kv.vt, kv.vs)
    B, Hkv, Sk, D = kv.shape
    if D != 128 or q.dim() != 4 or q.shape[3] != D:
        raise _lib.QAttnError("qattn mxfp4 kv cache: head_dim must be 128 in q and in the cache")
    if q.shape[0] != B or Hkv == 0 or q.shape[1] % Hkv:
        raise _lib.QAttnError("qattn mxfp4 kv cache: q must be [B, G*Hkv, Sq, D] for the cache's B, Hkv")
    Hq, Sq = q.shape[1], q.shape[2]
    if Sq < 1 or Sk < BLOCK or Sk % BLOCK:
        raise _lib.QAttnError("qattn mxfp4 kv cache: Sq >= 1 and a cache of 64*n tokens expected")
    if causal and Sq > Sk:
        raise _lib.QAttnError("qattn mxfp4 kv cache: causal attention needs Sq <= the cached tokens")
    if any(t.dtype != torch.uint8 or not t.is_contiguous() for t in kv.kv):
        raise _lib.QAttnError("qattn mxfp4 kv cache: the quantised operands must be contiguous uint8")
    if (tuple(kv.ks.shape) != (B, Hkv, Sk, D // 32) or tuple(kv.vt.shape) != (B * Hkv, Sk // 64, D, 32)
            or tuple(kv.vs.shape) != (B * Hkv, Sk // 64, D, 2)):
        raise _lib.QAttnError("qattn mxfp4 kv cache: ks / vt / vs do not match k4")
    bhv, rows = B * Hkv, (Hq // Hkv) * Sq
    kps = _split_plan_fp4(bhv, rows, Sk) if keys_per_split is None else int(keys_per_split)
    if kps < BLOCK or kps % BLOCK:
        raise _lib.QAttnError("qattn mxfp4 kv cache: keys_per_split must be a multiple of 64")
    kps = min(kps, Sk)
    nsplit = -(-Sk // kps)
    dev, st = q.device, _lib.stream_of(q)
    q4, qs = mxfp4_quantize_rows(q)
    O = torch.empty((B, Hq, Sq, D), dtype=torch.float16, device=dev)
    lse = torch.empty((B * Hq, Sq), dtype=torch.float32, device=dev)
    opart = torch.empty((nsplit, bhv * rows, D), dtype=torch.float32, device=dev)
    ml = torch.empty((nsplit, bhv * rows, 2), dtype=torch.float32, device=dev)
    _lib.call("qattn_mxfp4_attn_fwd_split", _lib.ptr(q4), _lib.ptr(qs), _lib.ptr(kv.k4), _lib.ptr(kv.ks),
              _lib.ptr(kv.vt), _lib.ptr(kv.vs), _lib.ptr(opart), _lib.ptr(ml), bhv, rows, Sq, Sk,
              2 if causal else 0, kps, D, _qk_scale(D), st)
    _lib.call("qattn_mxfp4_split_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(O), _lib.ptr(lse),
              bhv * rows, nsplit, D, st)
    return O, lse


# ------------------------------------------------------------------------------ preallocated cache
def _ceil64(n: int) -> int:
    return -(-n // BLOCK) * BLOCK


class PreallocatedKVFP4:
    """MX-FP4 keys/values of ``batch`` sequences x ``kv_heads`` heads at a fixed ``capacity`` (a
    multiple of 64) with one length per sequence; format and invariant: the module docstring.

    ``k4`` u8 [B, Hkv, cap, D/2], ``ks`` u8 [B, Hkv, cap, D/32], ``vt`` u8 [B*Hkv, cap/64, D, 32], ``vs``
    u8 [B*Hkv, cap/64, D, 2] (QuantizedKVFP4's layouts at S = cap), ``vtail`` f16 [B*Hkv, 64, D] (the
    fp16 V rows of each sequence's last partial tile), ``lens`` i32 [B] on the device and ``lengths``,
    its host mirror, which ``append`` and ``reset`` keep without reading the device; ``k_mean`` f16
    [B, Hkv, 1, D] or None is subtracted from every appended key.
    """

    def __init__(self, k4, ks, vt, vs, vtail, lens, lengths, k_mean=None):
        self.k4, self.ks, self.vt, self.vs = k4, ks, vt, vs
        self.vtail, self.lens, self.lengths, self.k_mean = vtail, lens, list(lengths), k_mean

    @classmethod
    def allocate(cls, batch: int, kv_heads: int, capacity: int, device,
                 k_mean: Optional[torch.Tensor] = None) -> "PreallocatedKVFP4":
        """An empty cache (every length 0), zero-filled."""
        D = 128
        if batch < 1 or kv_heads < 1 or capacity < BLOCK or capacity % BLOCK or capacity > 1 << 25:
            raise _lib.QAttnError("qattn mxfp4 kv cache: batch, kv_heads >= 1 and a capacity of 64*n "
                                  "tokens (at most 2^25) expected")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.QAttnError(f"qattn kernels run on the GPU only; got device {dev} "
                                  "(no CPU fallback by design)")
        if k_mean is not None:
            if tuple(k_mean.shape) != (batch, kv_heads, 1, D):
                raise _lib.QAttnError("qattn mxfp4 kv cache: k_mean must be [B, Hkv, 1, 128]")
            k_mean = k_mean.to(device=dev, dtype=torch.float16).contiguous()
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        return cls(z(batch, kv_heads, capacity, D // 2), z(batch, kv_heads, capacity, D // 32),
                   z(batch * kv_heads, capacity // BLOCK, D, 32), z(batch * kv_heads, capacity // BLOCK, D, 2),
                   z(batch * kv_heads, BLOCK, D, dt=torch.float16), z(batch, dt=torch.int32),
                   [0] * batch, k_mean)

    @property
    def shape(self):
        """(B, Hkv, capacity, D)"""
        B, H, S, D2 = self.k4.shape
        return (B, H, S, 2 * D2)

    @property
    def capacity(self) -> int:
        return self.k4.shape[2]

    @property
    def kv(self):
        return (self.k4, self.ks, self.vt, self.vs)

    def append(self, k: torch.Tensor, v: torch.Tensor, counts=None) -> "PreallocatedKVFP4":
        """Append fp16 ``k, v`` [B, Hkv, n, D] (any n >= 1) in place; with ``counts`` (B ints in
        [0, n]) sequence b takes only the first ``counts[b]`` tokens.  Raises before anything is
        launched if a length would pass the capacity.  Stream-ordered; returns ``self``."""
        B, H, cap, D = self.shape
        if (k.dim() != 4 or tuple(k.shape[:2]) != (B, H) or k.shape[3] != D or k.shape != v.shape
                or k.shape[2] < 1):
            raise _lib.QAttnError("qattn mxfp4 kv cache: appended tokens must be k, v [B, Hkv, n >= 1, D]")
        n = k.shape[2]
        if counts is None:
            cnt = [n] * B
        else:
            cnt = [int(c) for c in (counts.tolist() if isinstance(counts, torch.Tensor) else counts)]
            if len(cnt) != B or any(c < 0 or c > n for c in cnt):
                raise _lib.QAttnError("qattn mxfp4 kv cache: counts must be B values in [0, n]")
        if any(L + c > cap for L, c in zip(self.lengths, cnt)):
            raise _lib.QAttnError(f"qattn mxfp4 kv cache: append past the capacity of {cap} tokens "
                                  f"(lengths {self.lengths}, counts {cnt})")
        _lib.require_gpu(k, v, self.k4)
        k = k.to(torch.float16).contiguous()
        v = v.to(torch.float16).contiguous()
        cdev = None if counts is None else torch.tensor(cnt, dtype=torch.int32).to(k.device, non_blocking=True)
        _lib.call("qattn_mxfp4_cache_append", _lib.ptr(k), _lib.ptr(v), _lib.ptr(self.k_mean),
                  _lib.ptr(self.k4), _lib.ptr(self.ks), _lib.ptr(self.vt), _lib.ptr(self.vs),
                  _lib.ptr(self.vtail), _lib.ptr(self.lens), _lib.ptr(cdev), B, H, n, cap, D,
                  _lib.stream_of(k))
        self.lengths = [L + c for L, c in zip(self.lengths, cnt)]
        return self

    def reset(self, seqs) -> None:
        """Empty the sequences ``seqs`` (indices).  Their stale bytes are harmless by the invariant."""
        seqs = [int(b) for b in seqs]
        if any(b < 0 or b >= len(self.lengths) for b in seqs):
            raise _lib.QAttnError("qattn mxfp4 kv cache: reset of a sequence the cache does not have")
        for b in seqs:
            self.lengths[b] = 0
        self.lens.copy_(torch.tensor(self.lengths, dtype=torch.int32), non_blocking=True)

    def snapshot(self, b: int) -> QuantizedKVFP4:
        """A :class:`QuantizedKVFP4` copy (batch 1) of sequence ``b``, whose length must be a
        multiple of 64 (and not 0)."""
        B, H, cap, D = self.shape
        if not 0 <= b < B:
            raise _lib.QAttnError("qattn mxfp4 kv cache: snapshot of a sequence the cache does not have")
        L = self.lengths[b]
        if L == 0 or L % BLOCK:
            raise _lib.QAttnError(f"qattn mxfp4 kv cache: snapshot needs a length of 64*n tokens, got {L}")
        hs = slice(b * H, b * H + H)
        return QuantizedKVFP4(self.k4[b:b + 1, :, :L].clone(), self.ks[b:b + 1, :, :L].clone(),
                              self.vt[hs, :L // BLOCK].clone(), self.vs[hs, :L // BLOCK].clone(),
                              None if self.k_mean is None else self.k_mean[b:b + 1].clone())


def _decode_plan(q: torch.Tensor, cache: "PreallocatedKVFP4", causal: bool, keys_per_split):
    """The host checks of a decode call -> (bhv, rows, sk_max, kps, nsplit)."""
    if not isinstance(cache, PreallocatedKVFP4):
        raise _lib.QAttnError("qattn mxfp4 kv cache: cache must be a PreallocatedKVFP4")
    B, Hkv, cap, D = cache.shape
    if D != 128 or q.dim() != 4 or q.shape[3] != D:
        raise _lib.QAttnError("qattn mxfp4 kv cache: head_dim must be 128 in q and in the cache")
    if q.shape[0] != B or q.shape[1] == 0 or q.shape[1] % Hkv:
        raise _lib.QAttnError("qattn mxfp4 kv cache: q must be [B, G*Hkv, Sq, D] for the cache's B, Hkv")
    Hq, Sq = q.shape[1], q.shape[2]
    if Sq < 1:
        raise _lib.QAttnError("qattn mxfp4 kv cache: Sq >= 1 expected")
    if min(cache.lengths) < 1:
        raise _lib.QAttnError("qattn mxfp4 kv cache: every sequence needs at least one cached token "
                              f"(lengths {cache.lengths})")
    if causal and Sq > min(cache.lengths):
        raise _lib.QAttnError("qattn mxfp4 kv cache: causal attention needs Sq <= every sequence's "
                              "cached tokens")
    sk_max = _ceil64(max(cache.lengths))
    bhv, rows = B * Hkv, (Hq // Hkv) * Sq
    kps = _split_plan_fp4(bhv, rows, sk_max) if keys_per_split is None else int(keys_per_split)
    if kps < BLOCK or kps % BLOCK:
        raise _lib.QAttnError("qattn mxfp4 kv cache: keys_per_split must be a multiple of 64")
    kps = min(kps, sk_max)
    return bhv, rows, sk_max, kps, -(-sk_max // kps)


@torch.no_grad()
def attention_mxfp4_decode(q: torch.Tensor, cache: PreallocatedKVFP4, causal: bool = False,
                           keys_per_split: Optional[int] = None):
    """MX-FP4 attention of fp16 queries [B, Hq, Sq, D] (one Sq >= 1 for the batch) against a
    preallocated cache, sequence b over its own ``lengths[b]`` keys -> (O fp16 [B, Hq, Sq, D], lse
    fp32 [B*Hq, Sq] base 2).  Inference; no autograd; stream-ordered (the lengths come from the host
    mirror, the kernel reads ``lens``).

    ``causal``: the queries are each sequence's LAST Sq positions (query i of sequence b keeps the
    keys <= lengths[b] - Sq + i).  Raises for a sequence of length 0 and, causal, for Sq >
    min(lengths).  ``keys_per_split`` as in :func:`attention_mxfp4_cached`; the plan is taken at
    ceil64(max(lengths)).
    """
    bhv, rows, sk_max, kps, nsplit = _decode_plan(q, cache, causal, keys_per_split)
    _lib.require_gpu(q, cache.k4)
    B, Hkv, cap, D = cache.shape
    Hq, Sq = q.shape[1], q.shape[2]
    dev, st = q.device, _lib.stream_of(q)
    q4, qs = mxfp4_quantize_rows(q)
    O = torch.empty((B, Hq, Sq, D), dtype=torch.float16, device=dev)
    lse = torch.empty((B * Hq, Sq), dtype=torch.float32, device=dev)
    opart = torch.empty((nsplit, bhv * rows, D), dtype=torch.float32, device=dev)
    ml = torch.empty((nsplit, bhv * rows, 2), dtype=torch.float32, device=dev)
    _lib.call("qattn_mxfp4_attn_fwd_split_len", _lib.ptr(q4), _lib.ptr(qs), _lib.ptr(cache.k4),
              _lib.ptr(cache.ks), _lib.ptr(cache.vt), _lib.ptr(cache.vs), _lib.ptr(opart), _lib.ptr(ml),
              _lib.ptr(cache.lens), bhv, Hkv, rows, Sq, cap, sk_max, 2 if causal else 0, kps, D,
              _qk_scale(D), st)
    _lib.call("qattn_mxfp4_split_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(O), _lib.ptr(lse),
              bhv * rows, nsplit, D, st)
    return O, lse
