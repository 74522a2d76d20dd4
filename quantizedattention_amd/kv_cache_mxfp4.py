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

A server uses :class:`PagedKVFP4`: the preallocated cache reserves ``capacity`` tokens for every
sequence, cannot hand a finished sequence's memory to another and stores a shared prompt once per
sequence.  K is quantised per key row and V per 64-key tile, so a sequence's operands are a
concatenation of independent 64-key tiles, each four fixed-size blocks (4096 B of ``k4``, 256 B of
``ks``, 4096 B of ``vt``, 256 B of ``vs``), and can lie anywhere.  The pool cuts them into pages of
``page_tokens`` P = 64 * 2^k tokens, 64 <= P <= 1024; a page belongs to one sequence and holds all
``kv_heads`` heads::

    k4           uint8   [num_pages, Hkv, P, D/2]
    ks           uint8   [num_pages, Hkv, P, D/32]
    vt           uint8   [num_pages, Hkv, P/64, D, 32]
    vs           uint8   [num_pages, Hkv, P/64, D, 2]
    vtail        float16 [max_seqs, Hkv, 64, D]
    lens         int32   [max_seqs]                      host mirror: lengths
    block_table  int32   [max_seqs, max_pages_per_seq]   host mirror: table
    k_mean       float16 [max_seqs, Hkv, 1, D] or None

Logical tile t of head h of sequence b is physical tile ``(block_table[b][t // (P/64)] * Hkv + h) *
(P/64) + t % (P/64)`` of all four operands.  Invariant: gathering a sequence's pages through its table
gives exactly the bytes :class:`PreallocatedKVFP4` holds after the same appends, rows [0, L) of ``k4``
/ ``ks`` and tiles [0, ceil(L / 64)) of ``vt`` / ``vs``.  Everything else -- the tail of a sequence's
last page, pages it does not own, table entries at or past ceil(L / P) -- is unspecified and never
influences a result.  :class:`PageAllocator` keeps the free list, the reference counts and the page
lists on the host; ``append`` reserves pages there first and uploads the changed table in stream
order, ``fork`` shares a prefix's full pages by reference count, and
:func:`attention_mxfp4_decode_paged` (``qattn_mxfp4_attn_fwd_split_paged``) gives, bit for bit, what
:func:`attention_mxfp4_decode` gives on a preallocated cache with the same tokens.

A continuous-batching step is ragged: some slots are free, some sequences decode one token, one or two
prefill a chunk.  The packed ("varlen") step serves it without padding.  Queries and new keys/values
are token-major, as a model produces them: ``q`` fp16 [T, Hq, D] and ``k, v`` fp16 [T, Hkv, D] hold the
n_0 tokens of sequence ``seq_ids[0]`` first, then the n_1 of ``seq_ids[1]``, ...; ``seq_ids`` are
distinct slots of the pool and the slots that are not listed are never read (they may be empty).
:meth:`PagedKVFP4.append_packed` (``qattn_mxfp4_paged_append_packed``) writes the new tokens from a
host-built int32 table [nseq][4] = {slot, count, first packed token, 0} and a list of {j, logical
tile}, exactly the V tiles the appends touch; the pool keeps the invariant above.
:func:`attention_mxfp4_varlen_paged` is one attention launch
(``qattn_mxfp4_attn_fwd_varlen_paged``) and one merge (``qattn_mxfp4_varlen_combine``) from the two
tables of :func:`plan_varlen`, which is pure Python on the host mirror::

    seq_rec  int32 [nseq][8]   {slot, first packed token, n_j, ns_j, first partial row, 0, 0, 0}
    work     int32 [nwork][4]  {j, 128-row block, split < ns_j, 0}, one per workgroup and kv head,
                               longest split first
    opart    fp32  [part_rows][D], ml fp32 [part_rows][2]   the compact partials

One ``kps`` serves the call; sequence j has ns_j = ceil(ceil64(L_j) / kps) splits and owns ns_j * Hkv * G
* n_j partial rows from its first one, laid out [split][kv head][virtual row g * n_j + i] (the virtual
head order of the decoding layout), so a long sequence beside a large chunk pays for its own splits
only and no workgroup exists to write an empty state.  Virtual row r of key/value head h is packed row
(first + r % n_j) * Hq + h * G + r // n_j of ``q``.  Causal is bottom-right per sequence: query i of
sequence j keeps the keys <= L_j - n_j + i, what a prefill chunk needs after its own append.  Every
sequence gets, bit for bit, what :func:`attention_mxfp4_decode` gives for it alone with Sq = n_j and the
same keys per split.

A sliding window with sinks (``window=W >= 1, sinks=S >= 0``, Python ints, one pair per call since layers
differ; causal only) narrows the mask: query i of sequence j at position p = L_j - n_j + i sees key k
iff ``k <= p and (k > p - W or k < S)``; every query sees itself and ``lse`` is over the visible keys (a
smoothed cache needs nothing new).  The plan then runs only the tiles the call needs.  With nt =
ceil(L_j / 64), wt0 = max(0, L_j - n_j - W + 1) // 64 (the first tile any window of j reaches) and nst =
ceil(min(S, L_j) / 64) sink tiles: when wt0 <= nst the two runs touch and the splits are the causal
call's; when wt0 > nst there is a gap, split 0 is the sink run [0, nst) (one split whatever ``kps`` is;
no such split without sinks) and the next splits run kps keys each from tile wt0, so ns_j = (nst > 0) +
ceil((nt - wt0) * 64 / kps); ``seq_rec[j][5:7]`` = [wt0, nst] (0, 0 when they touch)
(``qattn_mxfp4_attn_fwd_varlen_paged_window``; the merge is unchanged).  The pages of the gap are never
fetched, so :meth:`PagedKVFP4.trim` may give them back: it makes the pages p with p * P >= S and (p + 1)
* P <= L - W + 1 -- those no query at a position >= L can see -- holes (None) in the host page list, one
reference less each, keeps the logical page count (``append`` and ``reserve`` go on as before) and
uploads nothing; the table entries of holes are unspecified.  Whatever would read a hole -- a call
without a window, with a larger window or more sinks, ``attention_mxfp4_decode_paged``, ``gather``,
``snapshot``, ``fork`` from that sequence -- raises :class:`QAttnError` naming "trimmed" before any
launch; ``free`` works.

Shared prefixes (``share_prefix=True``, not together with a window): sequences that ``fork`` made of one
prompt hold the same physical pages, and the packed call above fetches them once per sequence.  The
shared call keeps that call's splits exactly and changes only who computes them:
:meth:`PagedKVFP4.prefix_groups` finds the listed sequences whose leading pages are the same physical
pages, :func:`plan_varlen_shared` gives group g its first ns_g = min(common pages * P, min_j vis_j) //
kps splits (vis_j = L_j - n_j + 1 causal, L_j otherwise: wholly inside the common pages, no key masked for
any member row) as work records of a second kind, [g, 128-row block of the group's stacked rows, split,
1], and adds two tables::

    grp_rec  int32 [ngroup][4]   {first entry in members, member count, ns_g, R_g = G * sum of n_j}
    members  int32 [nmember][2]  {j, first stacked row of sequence j in its group}

A group workgroup (``qattn_mxfp4_attn_fwd_varlen_paged_shared``) runs the split's tiles once, through
the table row of the group's first member, for up to 128 rows of several sequences, and writes each row's
state into its own sequence's partial row at that split, the row the plain workgroup would have written;
``seq_rec``, the partial rows and the merge are unchanged, and the result is the plain call's bit for bit
at the same keys per split.  One level of sharing per call: a sub-group with a longer common prefix (a
fork of a fork) still shares only its group's common pages.

Speculative decoding: a step that verifies a draft (a chain from a small model, or a Medusa / EAGLE-style
token tree) appends the draft tokens and queries them in one packed step, as a prefill chunk, and then
keeps one root-to-leaf path.  Two things serve it.  The tree mask (``tree=``, causal only, not with a
window or ``share_prefix``): the last nd_j <= min(n_j, 64) query tokens of sequence j are the nodes of a
tree (or forest) in topological order, already appended at keys base_j = L_j - nd_j ..; node t sees key
k iff ``k < base_j`` or ``k = base_j + b`` with bit b of its 64-bit word set, the word holding the node's
ancestors and itself (:func:`tree_ancestor_masks`); the queries before the tree are plain causal,
``lse`` is over the visible keys, and a chain is the causal call bit for bit
(``qattn_mxfp4_attn_fwd_varlen_paged_tree``; ``seq_rec[j][7]`` = nd_j, the words travel as one int64 [T]
tensor behind the two tables, in their upload).  A draft token at tree depth d sits on a path whose
accepted form lands at position L0 + d, whatever its index in the packed step: ``rope=`` (below) places
draft keys and queries by depth itself.  Taking tokens back:
:meth:`PagedKVFP4.checkpoint` notes the listed sequences' lengths and pages and copies their ``vtail``
rows; :meth:`PagedKVFP4.rollback` restores those rows, quantises V tile L0 // 64 again from them (an
append that crossed the tile boundary overwrote ``vtail``, and the tile holds the drafts' scales),
writes the lengths back (``qattn_mxfp4_paged_rollback``) and returns the pages past ceil(L0 / P)
(:meth:`PageAllocator.shrink`).  Afterwards the pool holds, byte for byte, what it held at the
checkpoint -- rows [0, L0) of ``k4`` / ``ks``, tiles [0, ceil(L0 / 64)) of ``vt`` / ``vs``, ``vtail``
rows [0, L0 % 64), ``lens``, the page lists below ceil(L0 / P) and the free-page count -- so every later
``append`` gives the bytes of a pool that never saw the drafts.  :meth:`PagedKVFP4.accept` is that
followed by one ``append_packed`` of the surviving draft rows.

Rotary positions (``rope=``, a :class:`Rope`: an fp32 table [max_pos, 128] of cos and sin and the pairing,
NeoX or interleaved): the packed path rotates q and the new k inside its quantisers, which read every
element once anyway, so no rotated fp16 copy is written.  :meth:`PagedKVFP4.append_packed` rotates the new
keys (``qattn_mxfp4_paged_append_packed_rope``; V is never rotated), :func:`attention_mxfp4_varlen_paged`
the queries (``qattn_mxfp4_quant_rows_rope``), :meth:`PagedKVFP4.accept` the kept rows at their final
places.  The positions default to what the pool knows (:func:`rope_positions`): token i of an append to a
sequence of length L sits at L + i, a draft tree's node at (its first node's position) + depth, a kept row
of ``accept`` at L0, L0 + 1, ...; explicit ``positions`` (host, checked against the table; or a device
int32 tensor, used as given and clamped by the kernel) override them.  The rotation is defined bit for bit
-- per pair (a, b), ``f16(f32(a c) - f32(b s))`` and ``f16(f32(b c) + f32(a s))``, no fused multiply-add
-- so every ``rope=`` call gives exactly the bytes of the same call on rows rotated that way in torch.
Cached keys are never rotated again, and the padded entries take no ``rope``.

The device-planned decode step (:class:`DecodeStep`): the commonest step, one new token for each of N running
sequences, is bound by the host plan and its uploads, not by its kernels, and a plan made from the host mirror
cannot be captured in a graph (a replay would run stale lengths).  A ``DecodeStep`` fixes every shape, grid and
pointer when it is made; ``qattn_mxfp4_decode_step_plan`` derives the append record, the V tile, the rotary
position and ``seq_rec`` of every entry from ``slots`` and ``lens`` on the device (:func:`plan_decode_step`
restates it), the attention runs ``splits`` (:func:`decode_step_splits`) work records per entry whatever the
lengths are, and a workgroup whose split its sequence does not have exits at once.  The host keeps what only it
can do, in ``prepare``: the checks, the page reservation, the table upload when a page was added and the upload
of ``slots``.  Results are the host-planned pair's bit for bit at the same keys per split.  ``share_prefix``,
``trim`` and prefill chunks stay on the host-planned path.

The device-planned verify step (:class:`VerifyStep`) is the same for speculative decoding: every listed sequence
appends K draft tokens (1 <= K <= 64, a chain or a tree, K fixed when the step is made) and attends to them under
the tree mask.  ``qattn_mxfp4_verify_step_plan`` derives the append record, the at most two V tiles, the K rotary
positions (depth behind the cached keys) and ``seq_rec`` from ``slots``, ``lens`` and the uploaded ancestor words
(:func:`plan_verify_step` restates it); the attention is the tree instantiation over a fixed grid of N *
ceil(G K / 128) * ``splits`` work records.  ``prepare`` uploads ``slots`` and the words of all N * K tokens every
time, so another tree costs no new capture.  A round is ``checkpoint`` BEFORE ``prepare`` (prepare moves the
mirror lengths), then ``append`` / ``attend`` or their replay, then ``rollback`` or ``accept`` as on the
host-planned path.  No window, no ``share_prefix``, one K for every entry of a step.

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

import itertools
import json
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .attention_mxfp4 import (Rope, _device_positions, _host_positions, _qk_scale, mxfp4_quantize_rows,
                              mxfp4_quantize_rows_rope, mxfp4_quantize_v, rope_table)

MAGIC = b"QATTNKF4"
BLOCK = 64
_ALIGN = 256
_DTYPES = {"uint8": torch.uint8, "float16": torch.float16}

__all__ = ["QuantizedKVFP4", "quantize_kv_fp4", "attention_mxfp4_cached", "PreallocatedKVFP4",
           "attention_mxfp4_decode", "PageAllocator", "PagedKVFP4", "attention_mxfp4_decode_paged",
           "plan_varlen", "plan_varlen_shared", "attention_mxfp4_varlen_paged", "tree_ancestor_masks",
           "tree_path", "Checkpoint", "Rope", "rope_table", "rope_positions", "DecodeStep",
           "decode_step_splits", "plan_decode_step", "VerifyStep", "verify_step_splits", "plan_verify_step"]


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
    k = _lib.kernel_input(k, torch.float16)
    if smooth and k_mean is None:
        k_mean = torch.empty((B, H, 1, D), dtype=torch.float16, device=k.device)
        _lib.call("qattn_kmean", _lib.ptr(k), _lib.ptr(k_mean), B * H, S, D, _lib.stream_of(k))
    km = _lib.kernel_input(k_mean, torch.float16)
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


def _split_and_merge(q: torch.Tensor, kv, causal: bool, kps: int, nsplit: int, bhv: int, rows: int,
                     entry: str, *middle):
    """The tail the padded attention functions share, after their checks: quantise ``q`` [B, Hq, Sq, D],
    allocate O, lse and the ``nsplit`` partials, run the key-split entry ``entry`` on the operands ``kv``
    (``middle``: the entry's own arguments between ``ml`` and ``causal``) and merge -> (O, lse)."""
    B, Hq, Sq, D = q.shape
    dev, st = q.device, _lib.stream_of(q)
    q4, qs = mxfp4_quantize_rows(q)
    O = torch.empty((B, Hq, Sq, D), dtype=torch.float16, device=dev)
    lse = torch.empty((B * Hq, Sq), dtype=torch.float32, device=dev)
    opart = torch.empty((nsplit, bhv * rows, D), dtype=torch.float32, device=dev)
    ml = torch.empty((nsplit, bhv * rows, 2), dtype=torch.float32, device=dev)
    _lib.call(entry, _lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in kv), _lib.ptr(opart), _lib.ptr(ml),
              *middle, 2 if causal else 0, kps, D, _qk_scale(D), st)
    _lib.call("qattn_mxfp4_split_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(O), _lib.ptr(lse),
              bhv * rows, nsplit, D, st)
    return O, lse


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
    return _split_and_merge(q, kv.kv, causal, kps, nsplit, bhv, rows, "qattn_mxfp4_attn_fwd_split",
                            bhv, rows, Sq, Sk)


# ------------------------------------------------------------------------------ preallocated cache
def _ceil64(n: int) -> int:
    return -(-n // BLOCK) * BLOCK


def _append_counts(counts, B: int, n: int, error: str) -> list:
    """``counts`` of a padded ``append`` as B ints in [0, n] (None: n each); raises ``error`` otherwise."""
    if counts is None:
        return [n] * B
    cnt = [int(c) for c in (counts.tolist() if isinstance(counts, torch.Tensor) else counts)]
    if len(cnt) != B or any(c < 0 or c > n for c in cnt):
        raise _lib.QAttnError(error)
    return cnt


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
            k_mean = _lib.kernel_input(k_mean.to(device=dev), torch.float16)
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
        cnt = _append_counts(counts, B, n, "qattn mxfp4 kv cache: counts must be B values in [0, n]")
        if any(L + c > cap for L, c in zip(self.lengths, cnt)):
            raise _lib.QAttnError(f"qattn mxfp4 kv cache: append past the capacity of {cap} tokens "
                                  f"(lengths {self.lengths}, counts {cnt})")
        _lib.require_gpu(k, v, self.k4)
        k = _lib.kernel_input(k, torch.float16)
        v = _lib.kernel_input(v, torch.float16)
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


def _decode_plan(q: torch.Tensor, cache, causal: bool, keys_per_split, kind=None):
    """The host checks of a decode call on a cache of class ``kind`` (None: PreallocatedKVFP4) ->
    (bhv, rows, sk_max, kps, nsplit)."""
    kind = PreallocatedKVFP4 if kind is None else kind
    if not isinstance(cache, kind):
        raise _lib.QAttnError(f"qattn mxfp4 kv cache: cache must be a {kind.__name__}")
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
    _, Hkv, cap, _ = cache.shape
    return _split_and_merge(q, cache.kv, causal, kps, nsplit, bhv, rows, "qattn_mxfp4_attn_fwd_split_len",
                            _lib.ptr(cache.lens), bhv, Hkv, rows, q.shape[2], cap, sk_max)


# ------------------------------------------------------------------------------ paged cache
PAGE_TOKENS = (64, 128, 256, 512, 1024)


class PageAllocator:
    """The host side of a page pool: a free list, a reference count per page and the page list of
    every sequence, which ``table`` mirrors.  No tensors, no device: plain Python.

    ``free_order`` (a permutation of range(num_pages); default ascending) is the order in which the
    pages are first handed out; a page that returns to the pool is the next one handed out.
    ``table[b][i]`` is page i of sequence b for i < len(pages[b]); the entries past that keep
    whatever they held.  Every operation either happens completely or raises
    :class:`QAttnError` before anything has changed.
    """

    def __init__(self, num_pages: int, page_tokens: int, max_seqs: int, max_pages_per_seq: int,
                 free_order=None):
        if page_tokens not in PAGE_TOKENS:
            raise _lib.QAttnError("qattn mxfp4 paged cache: page_tokens must be 64 * 2^k in [64, 1024], "
                                  f"got {page_tokens}")
        if num_pages < 1 or max_seqs < 1 or max_pages_per_seq < 1:
            raise _lib.QAttnError("qattn mxfp4 paged cache: num_pages, max_seqs and max_pages_per_seq >= 1 "
                                  "expected")
        order = list(range(num_pages)) if free_order is None else [int(p) for p in free_order]
        if sorted(order) != list(range(num_pages)):
            raise _lib.QAttnError("qattn mxfp4 paged cache: free_order must be a permutation of the pages")
        self.num_pages, self.page_tokens = num_pages, page_tokens
        self.max_seqs, self.max_pages_per_seq = max_seqs, max_pages_per_seq
        self._free = order[::-1]                  # handed out from the end
        self.refcount = [0] * num_pages
        self.pages = [[] for _ in range(max_seqs)]
        self.nholes = [0] * max_seqs              # holes (``drop``) in each sequence's page list
        self.table = [[0] * max_pages_per_seq for _ in range(max_seqs)]

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def _seq(self, b) -> int:
        b = int(b)
        if not 0 <= b < self.max_seqs:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: no sequence {b} (max_seqs {self.max_seqs})")
        return b

    def pages_for(self, tokens: int) -> int:
        return -(-tokens // self.page_tokens)

    def _take(self, b: int, count: int) -> list:
        new = [self._free.pop() for _ in range(count)]
        for p in new:
            self.refcount[p] = 1
            self.table[b][len(self.pages[b])] = p
            self.pages[b].append(p)
        return new

    def reserve(self, requests) -> list:
        """Give every ``(seq, new_length)`` of ``requests`` the pages its new length needs (a
        sequence never shrinks here) -> the sequences whose page list grew.  All or nothing: raises,
        naming "pages", before anything changes when a sequence would pass ``max_pages_per_seq`` or the
        pool has too few free pages."""
        need = {}
        for b, length in requests:
            b = self._seq(b)
            need[b] = max(need.get(b, 0), self.pages_for(int(length)) - len(self.pages[b]), 0)
        over = [b for b, n in need.items() if len(self.pages[b]) + n > self.max_pages_per_seq]
        if over:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequences {over} would pass max_pages_per_seq = "
                                  f"{self.max_pages_per_seq} pages of {self.page_tokens} tokens")
        total = sum(need.values())
        if total > len(self._free):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: out of pages ({total} needed, "
                                  f"{len(self._free)} of {self.num_pages} free)")
        grown = sorted(b for b, n in need.items() if n)
        for b in grown:
            self._take(b, need[b])
        return grown

    def release(self, b) -> None:
        """Empty sequence ``b``: each of its pages loses a reference and returns to the free list at 0."""
        b = self._seq(b)
        for p in self.pages[b]:
            if p is None:   # a hole (``drop``): given back already
                continue
            self.refcount[p] -= 1
            if self.refcount[p] == 0:
                self._free.append(p)
        self.pages[b] = []
        self.nholes[b] = 0

    def drop(self, b, first_page: int, last_page: int) -> int:
        """Make pages ``[first_page, last_page)`` of sequence ``b`` holes -> the pages that returned to
        the free list.  ``pages[b][i]`` becomes None and the page loses one reference (a page shared by
        ``share`` just loses that one); ``len(pages[b])`` stays the logical page count, so ``reserve``
        goes on as before and ``nholes[b]`` counts the holes.  ``table[b][i]`` keeps what it held and means nothing.  A page that is a
        hole already is left alone.  All or nothing: a range outside the sequence's pages raises."""
        b = self._seq(b)
        first_page, last_page = int(first_page), int(last_page)
        if not 0 <= first_page <= last_page <= len(self.pages[b]):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequence {b} has no pages [{first_page}, "
                                  f"{last_page}) to drop ({len(self.pages[b])} pages)")
        freed = 0
        for i in range(first_page, last_page):
            p = self.pages[b][i]
            if p is None:
                continue
            self.pages[b][i] = None
            self.nholes[b] += 1
            self.refcount[p] -= 1
            if self.refcount[p] == 0:
                self._free.append(p)
                freed += 1
        return freed

    def shrink(self, b, pages: int) -> int:
        """Cut sequence ``b``'s page list to its first ``pages`` logical pages -> the pages that returned to
        the free list.  Each page past the cut loses one reference (a page shared by ``share`` just loses
        that one); a hole past the cut only stops being counted, the holes below it stay.  ``table[b]``
        keeps what it held past the cut and means nothing there.  All or nothing: ``pages`` outside [0,
        len(pages[b])] raises."""
        b, pages = self._seq(b), int(pages)
        if not 0 <= pages <= len(self.pages[b]):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequence {b} cannot shrink to {pages} pages "
                                  f"(it has {len(self.pages[b])})")
        freed = 0
        for p in reversed(self.pages[b][pages:]):   # last taken, first back: the free list as it was
            if p is None:
                self.nholes[b] -= 1
                continue
            self.refcount[p] -= 1
            if self.refcount[p] == 0:
                self._free.append(p)
                freed += 1
        del self.pages[b][pages:]
        return freed

    def holes(self, b, first_page: int = 0, last_page: Optional[int] = None) -> list:
        """The indices in ``[first_page, last_page)`` (default: all) of sequence ``b``'s pages that are
        holes."""
        pages = self.pages[self._seq(b)]
        last_page = len(pages) if last_page is None else min(int(last_page), len(pages))
        return [i for i in range(max(int(first_page), 0), last_page) if pages[i] is None]

    def share(self, src, dst, shared: int, fresh: int = 0) -> list:
        """Make the empty sequence ``dst`` the first ``shared`` pages of ``src`` (one more reference
        each) followed by ``fresh`` new pages -> the new pages.  All or nothing."""
        src, dst = self._seq(src), self._seq(dst)
        if self.pages[dst]:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequence {dst} is not empty "
                                  f"({len(self.pages[dst])} pages)")
        if not 0 <= shared <= len(self.pages[src]) or fresh < 0:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequence {src} has no {shared} pages to share")
        if None in self.pages[src][:shared]:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequence {src} has trimmed pages among its first "
                                  f"{shared}; they cannot be shared")
        if shared + fresh > self.max_pages_per_seq or fresh > len(self._free):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: out of pages ({fresh} needed, "
                                  f"{len(self._free)} of {self.num_pages} free, max_pages_per_seq "
                                  f"{self.max_pages_per_seq})")
        for p in self.pages[src][:shared]:
            self.refcount[p] += 1
            self.table[dst][len(self.pages[dst])] = p
            self.pages[dst].append(p)
        return self._take(dst, fresh)

    def prefix_groups(self, seq_ids) -> list:
        """The listed sequences that hold the same leading physical pages -> ``[(members, common_pages),
        ...]``: ``members`` are indices into ``seq_ids``, ascending, of the sequences whose page 0 is the
        same physical page, and ``common_pages`` the number of leading positions at which every member
        holds the same physical page.  Groups of one member or without a common page are not returned, a
        sequence with holes (``drop``) or without pages is never grouped, and the slots that are not
        listed are not looked at.  One level of sharing: members of a group that share a longer prefix
        among themselves (a fork of a fork) still get only the whole group's common pages.  Host only."""
        ids = [self._seq(b) for b in seq_ids]
        by_first = {}
        for i, b in enumerate(ids):
            if self.pages[b] and not self.nholes[b]:
                by_first.setdefault(self.pages[b][0], []).append(i)
        out = []
        for idxs in by_first.values():
            if len(idxs) < 2:
                continue
            lists = [self.pages[ids[i]] for i in idxs]
            head = lists[0][:min(len(x) for x in lists)]
            for x in lists[1:]:   # whole-slice compares: the lists of forks are equal up to their own pages
                if x[:len(head)] != head:
                    head = head[:next(i for i, p in enumerate(head) if x[i] != p)]
            out.append((idxs, len(head)))
        return out


@dataclass
class Checkpoint:
    """What :meth:`PagedKVFP4.checkpoint` notes of the sequences ``seq_ids`` (slots) of ``cache``: per
    sequence its length L0, its logical page count, its hole count and the slot's epoch, all host lists
    in the order of ``seq_ids``, and ``saved`` f16 [len(seq_ids), Hkv, 64, D], the copy of the slots'
    ``vtail`` rows on the device.  :meth:`PagedKVFP4.rollback` stamps ``epochs`` again."""

    cache: "PagedKVFP4"
    seq_ids: list
    lengths: list
    pages: list
    holes: list
    epochs: list
    saved: torch.Tensor


class PagedKVFP4:
    """MX-FP4 keys/values of up to ``max_seqs`` sequences x ``kv_heads`` heads in a pool of
    ``num_pages`` pages of ``page_tokens`` tokens; layout and invariant: the module docstring.

    ``k4``, ``ks``, ``vt``, ``vs`` are the pool, ``vtail``, ``lens`` and ``k_mean`` as in
    :class:`PreallocatedKVFP4` with one row per sequence slot, ``block_table`` i32 [max_seqs,
    max_pages_per_seq] on the device; ``alloc`` (:class:`PageAllocator`) and ``lengths`` are the host
    mirrors, kept without reading the device.  A sequence's memory is the pages it holds: ``free``
    gives them back, and ``fork`` lets two sequences hold the same full pages.  Shared pages are
    always full and ``append`` only writes at or past a sequence's length, so a shared page is never
    written and no copy-on-write is needed.
    """

    def __init__(self, k4, ks, vt, vs, vtail, lens, block_table, alloc: PageAllocator, k_mean=None):
        self.k4, self.ks, self.vt, self.vs = k4, ks, vt, vs
        self.vtail, self.lens, self.block_table, self.alloc, self.k_mean = vtail, lens, block_table, alloc, k_mean
        self.lengths = [0] * alloc.max_seqs
        self.epoch = [0] * alloc.max_seqs   # bumped by free, trim and rollback: what a Checkpoint is held to

    @classmethod
    def allocate(cls, num_pages: int, page_tokens: int, max_seqs: int, kv_heads: int, max_pages_per_seq: int,
                 device, k_mean: Optional[torch.Tensor] = None, free_order=None) -> "PagedKVFP4":
        """An empty pool (every length 0, every page free), zero-filled."""
        D = 128
        alloc = PageAllocator(num_pages, page_tokens, max_seqs, max_pages_per_seq, free_order)
        tpp = page_tokens // BLOCK
        if (kv_heads < 1 or num_pages * kv_heads * tpp >= 1 << 31
                or max_pages_per_seq * page_tokens > 1 << 25):
            raise _lib.QAttnError("qattn mxfp4 paged cache: kv_heads >= 1, fewer than 2^31 tiles in the pool "
                                  "and at most 2^25 tokens per sequence expected")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.QAttnError(f"qattn kernels run on the GPU only; got device {dev} "
                                  "(no CPU fallback by design)")
        if k_mean is not None:
            if tuple(k_mean.shape) != (max_seqs, kv_heads, 1, D):
                raise _lib.QAttnError("qattn mxfp4 paged cache: k_mean must be [max_seqs, Hkv, 1, 128]")
            k_mean = _lib.kernel_input(k_mean.to(device=dev), torch.float16)
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        return cls(z(num_pages, kv_heads, page_tokens, D // 2), z(num_pages, kv_heads, page_tokens, D // 32),
                   z(num_pages, kv_heads, tpp, D, 32), z(num_pages, kv_heads, tpp, D, 2),
                   z(max_seqs, kv_heads, BLOCK, D, dt=torch.float16), z(max_seqs, dt=torch.int32),
                   z(max_seqs, max_pages_per_seq, dt=torch.int32), alloc, k_mean)

    @property
    def shape(self):
        """(max_seqs, Hkv, max_pages_per_seq * page_tokens, D): what one table row can hold"""
        return (self.alloc.max_seqs, self.k4.shape[1], self.alloc.max_pages_per_seq * self.page_tokens, 128)

    @property
    def page_tokens(self) -> int:
        return self.alloc.page_tokens

    @property
    def num_pages(self) -> int:
        return self.alloc.num_pages

    @property
    def free_pages(self) -> int:
        return self.alloc.free_pages

    @property
    def table(self):
        """The host mirror of ``block_table`` (the allocator's)."""
        return self.alloc.table

    @property
    def kv(self):
        return (self.k4, self.ks, self.vt, self.vs)

    def capacity_tokens(self, b: int) -> int:
        """The tokens sequence ``b`` can hold in the pages it has."""
        return len(self.alloc.pages[self.alloc._seq(b)]) * self.page_tokens

    def _upload(self, table: bool) -> None:
        # from fresh pageable host tensors: the copies are staged before they return, so the mirrors
        # may change again at once
        if table:
            self.block_table.copy_(torch.tensor(self.alloc.table, dtype=torch.int32), non_blocking=True)
        self.lens.copy_(torch.tensor(self.lengths, dtype=torch.int32), non_blocking=True)

    def append(self, k: torch.Tensor, v: torch.Tensor, counts=None) -> "PagedKVFP4":
        """Append fp16 ``k, v`` [max_seqs, Hkv, n, D] (any n >= 1) in place; with ``counts`` (max_seqs
        ints in [0, n]) sequence b takes only the first ``counts[b]`` tokens.  The pages the new
        lengths need are reserved on the host first (all or nothing: out of pages, or a sequence past
        ``max_pages_per_seq``, raises before anything is launched or changed), the changed table is
        uploaded in stream order and ``qattn_mxfp4_paged_append`` writes in place.  No host
        synchronisation, nothing is read back; returns ``self``."""
        B, H, _, D = self.shape
        if (k.dim() != 4 or tuple(k.shape[:2]) != (B, H) or k.shape[3] != D or k.shape != v.shape
                or k.shape[2] < 1):
            raise _lib.QAttnError("qattn mxfp4 paged cache: appended tokens must be k, v [max_seqs, Hkv, "
                                  "n >= 1, D]")
        n = k.shape[2]
        cnt = _append_counts(counts, B, n, "qattn mxfp4 paged cache: counts must be max_seqs values in [0, n]")
        _lib.require_gpu(k, v, self.k4)
        grown = self.alloc.reserve([(b, L + c) for b, (L, c) in enumerate(zip(self.lengths, cnt)) if c])
        k = _lib.kernel_input(k, torch.float16)
        v = _lib.kernel_input(v, torch.float16)
        if grown:
            self.block_table.copy_(torch.tensor(self.alloc.table, dtype=torch.int32), non_blocking=True)
        cdev = None if counts is None else torch.tensor(cnt, dtype=torch.int32).to(k.device, non_blocking=True)
        _lib.call("qattn_mxfp4_paged_append", _lib.ptr(k), _lib.ptr(v), _lib.ptr(self.k_mean),
                  _lib.ptr(self.k4), _lib.ptr(self.ks), _lib.ptr(self.vt), _lib.ptr(self.vs),
                  _lib.ptr(self.vtail), _lib.ptr(self.lens), _lib.ptr(cdev), _lib.ptr(self.block_table), B, H,
                  n, self.num_pages, self.page_tokens, self.alloc.max_pages_per_seq, D, _lib.stream_of(k))
        self.lengths = [L + c for L, c in zip(self.lengths, cnt)]
        return self

    def append_packed(self, k: torch.Tensor, v: torch.Tensor, seq_ids, counts, rope: Optional[Rope] = None,
                      positions=None, tree=None) -> "PagedKVFP4":
        """Append packed fp16 ``k, v`` [T, Hkv, D], token-major as a model produces them: the first
        ``counts[0]`` tokens go to sequence ``seq_ids[0]``, the next ``counts[1]`` to ``seq_ids[1]``,
        ... (distinct slots, every count >= 1, T = sum(counts)); the slots that are not listed are
        not touched.  As :meth:`append`: the pages are reserved on the host first (all or nothing,
        raises before anything is launched or changed), the changed table is uploaded in stream
        order and ``qattn_mxfp4_paged_append_packed`` writes in place, over exactly the V tiles the
        appends touch (listed here from the host mirror).  No host synchronisation, nothing is read
        back; returns ``self``.

        ``rope`` (a :class:`Rope`; None: no rotation, the bits of the call without these arguments) rotates
        the new keys inside the K quantiser (``qattn_mxfp4_paged_append_packed_rope``; V is not rotated): ``k`` is the UNROTATED
        key.  ``positions`` defaults to ``rope_positions(self.lengths, seq_ids, counts, tree)``: token i of
        sequence j at L_j + i, and with ``tree`` (entries as in :func:`attention_mxfp4_varlen_paged`) a
        draft node at its depth.  A list or a host tensor is checked against [0, rope.max_pos) -- the call
        raises before any page is reserved -- and travels in the upload of the records; a device int32
        tensor [T] is used as given, never read back, and clamped to the table by the kernel.
        ``positions`` or ``tree`` without ``rope``, and ``positions`` together with ``tree``, raise."""
        _, H, _, D = self.shape
        ids, cnt = _packed_lists(self.alloc.max_seqs, seq_ids, counts, "counts")
        if (k.dim() != 3 or tuple(k.shape[1:]) != (H, D) or k.shape != v.shape or k.shape[0] != sum(cnt)):
            raise _lib.QAttnError("qattn mxfp4 paged cache: packed tokens must be k, v [sum(counts), Hkv, D]")
        if k.shape[0] * H >= 1 << 31:
            raise _lib.QAttnError("qattn mxfp4 paged cache: fewer than 2^31 packed rows expected")
        pos = _rope_args(rope, positions, tree, k.shape[0], lambda: (self.lengths, ids, cnt, tree))
        _lib.require_gpu(k, v, self.k4)
        grown = self.alloc.reserve([(b, self.lengths[b] + c) for b, c in zip(ids, cnt)])
        k = _lib.kernel_input(k, torch.float16)
        v = _lib.kernel_input(v, torch.float16)
        if grown:
            self.block_table.copy_(torch.tensor(self.alloc.table, dtype=torch.int32), non_blocking=True)
        tab, tiles, first = [], [], 0
        for j, (b, c) in enumerate(zip(ids, cnt)):
            L = self.lengths[b]
            tab += [b, c, first, 0]
            tiles += [x for g in range(L // BLOCK, (L + c - 1) // BLOCK + 1) for x in (j, g)]
            first += c
        # one upload: the records, then the tile list (the record block is a multiple of 16 bytes), then,
        # at the next multiple of 16 bytes, host positions
        if pos is None or pos.is_cuda:
            flat = torch.tensor(tab + tiles, dtype=torch.int32)
        else:
            flat = torch.cat([torch.tensor(tab + tiles + [0] * (-len(tiles) % 4), dtype=torch.int32), pos])
        dev = flat.to(k.device, non_blocking=True)
        args = (_lib.ptr(k), _lib.ptr(v), _lib.ptr(self.k_mean),
                _lib.ptr(self.k4), _lib.ptr(self.ks), _lib.ptr(self.vt), _lib.ptr(self.vs),
                _lib.ptr(self.vtail), _lib.ptr(self.lens), _lib.ptr(self.block_table), _lib.ptr(dev),
                _lib.ptr(dev[len(tab):]), len(ids), len(tiles) // 2, k.shape[0], self.alloc.max_seqs, H,
                self.num_pages, self.page_tokens, self.alloc.max_pages_per_seq, D)
        if rope is None:
            _lib.call("qattn_mxfp4_paged_append_packed", *args, _lib.stream_of(k))
        else:
            pos_d = _lib.kernel_input(pos) if pos.is_cuda else dev[len(dev) - k.shape[0]:]
            _lib.call("qattn_mxfp4_paged_append_packed_rope", *args, _lib.ptr(rope.table), _lib.ptr(pos_d),
                      rope.max_pos, int(rope.interleaved), _lib.stream_of(k))
        for b, c in zip(ids, cnt):
            self.lengths[b] += c
        return self

    def free(self, seqs) -> None:
        """Empty the sequences ``seqs`` (indices) and give their pages back to the pool."""
        seqs = [self.alloc._seq(b) for b in seqs]
        for b in seqs:
            self.lengths[b] = 0
            self.alloc.release(b)
            self.epoch[b] += 1
        self._upload(table=False)

    def _whole(self, b: int, what: str) -> None:
        """Raise when sequence ``b`` has had pages trimmed: ``what`` would read them."""
        if not self.alloc.nholes[b]:   # (a counter: this sits on every packed call's path)
            return
        holes = self.alloc.holes(b)
        if holes:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: {what} would read trimmed pages {holes} of "
                                  f"sequence {b} (PagedKVFP4.trim gave them back to the pool)")

    def trim(self, seq_ids, window: int, sinks: int = 0) -> int:
        """Give back the pages of the listed sequences that no query at a position >= the sequence's
        length L can see under ``(window, sinks)`` -- the queries of every later step, those of a chunk
        appended later included: the pages p with ``p * P >= sinks`` and ``(p + 1) * P <= L - window +
        1`` -> the number of pages that returned to the pool (a page still held by a fork does not).
        The pages become holes of the sequence (:meth:`PageAllocator.drop`); lengths, logical page
        counts and ``append`` are as before.  Host only: nothing is uploaded (the table entries of
        holes are unspecified and never used), nothing is launched or synchronised.  Afterwards every
        call that would read a hole raises :class:`QAttnError` naming "trimmed" before it launches: a
        windowed call needs ``window`` and ``sinks`` no larger than the holes allow."""
        W, S = _window_args(window, sinks, True)
        seqs = [self.alloc._seq(b) for b in seq_ids]
        P = self.page_tokens
        freed = 0
        for b in seqs:
            first, last = -(-S // P), (self.lengths[b] - W + 1) // P
            if last > first:
                freed += self.alloc.drop(b, first, last)
            self.epoch[b] += 1
        return freed

    # ------------------------------------------------------------------------------ speculative decoding
    def checkpoint(self, seq_ids) -> "Checkpoint":
        """Note where the listed sequences (distinct slots; a length of 0 is allowed) stand, so that
        :meth:`rollback` can take back what is appended after this: per sequence the slot, its length
        L0, its logical page count, its hole count and the slot's epoch on the host, and on the device a
        copy of the slots' ``vtail`` rows (rows [0, L0 % 64) are what matters: a later append that crosses
        a tile boundary overwrites them).  Stream-ordered, no synchronisation, nothing read back."""
        ids = [self.alloc._seq(b) for b in seq_ids]
        if not ids or len(set(ids)) != len(ids):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: checkpoint needs distinct slots, got {ids}")
        dev = self.vtail.device
        saved = self.vtail.index_select(0, torch.tensor(ids, dtype=torch.long).to(dev, non_blocking=True))
        a = self.alloc
        return Checkpoint(self, ids, [self.lengths[b] for b in ids], [len(a.pages[b]) for b in ids],
                          [a.nholes[b] for b in ids], [self.epoch[b] for b in ids], saved)

    def _rollback_check(self, ckpt: "Checkpoint", seq_ids) -> list:
        """The refusals of :meth:`rollback` -> the checkpoint's rows of the listed sequences."""
        if not isinstance(ckpt, Checkpoint) or ckpt.cache is not self:
            raise _lib.QAttnError("qattn mxfp4 paged cache: rollback needs a checkpoint of this pool")
        ids = ckpt.seq_ids if seq_ids is None else [self.alloc._seq(b) for b in seq_ids]
        if len(set(ids)) != len(ids) or any(b not in ckpt.seq_ids for b in ids):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: rollback of {ids}: distinct sequences of the "
                                  f"checkpoint ({ckpt.seq_ids}) expected")
        rows = [ckpt.seq_ids.index(b) for b in ids]
        a, P = self.alloc, self.page_tokens
        for r in rows:
            b, L0 = ckpt.seq_ids[r], ckpt.lengths[r]
            if self.epoch[b] != ckpt.epochs[r]:
                raise _lib.QAttnError(f"qattn mxfp4 paged cache: stale checkpoint of sequence {b}: it was "
                                      "freed, trimmed or rolled back through another checkpoint since")
            if self.lengths[b] < L0:
                raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequence {b} is shorter ({self.lengths[b]} "
                                      f"tokens) than its checkpoint ({L0})")
            page = a.pages[b][L0 // P] if L0 % P else None
            if page is not None and a.refcount[page] > 1:
                raise _lib.QAttnError(f"qattn mxfp4 paged cache: the page that holds position {L0} of sequence "
                                      f"{b} is shared (a fork after the checkpoint): rolling back would let "
                                      "later appends write into a page another sequence reads")
        return rows

    def rollback(self, ckpt: "Checkpoint", seq_ids=None) -> "PagedKVFP4":
        """Take the listed sequences (default: all of the checkpoint) back to their lengths L0 at
        ``ckpt``.  One launch (``qattn_mxfp4_paged_rollback``) restores ``vtail`` rows [0, L0 % 64),
        quantises V tile L0 // 64 again from the saved rows when L0 % 64 != 0 (the rows at or past L0 are
        zero) and writes ``lens``; the host gives the pages past ceil(L0 / P) back
        (:meth:`PageAllocator.shrink`) and mirrors the lengths.  K rows at or past L0 are left alone
        (unspecified by the invariant).  Afterwards the pool holds, byte for byte, what it held at the
        checkpoint (module docstring).  The checkpoint is stamped again, so it can serve the next draft
        round.  Raises before any launch or change, naming the reason: "stale" (the slot was freed, trimmed
        or rolled back through another checkpoint since), "shorter" (its length is below L0 now), "shared"
        (L0 % P != 0 and the page holding position L0 has a reference count above 1).  Stream-ordered, no
        synchronisation; returns ``self``.  Not for :class:`PreallocatedKVFP4`."""
        rows = self._rollback_check(ckpt, seq_ids)
        self._rollback(ckpt, rows)
        return self

    def _rollback(self, ckpt: "Checkpoint", rows) -> None:
        _, H, _, D = self.shape
        recs = [x for r in rows for x in (ckpt.seq_ids[r], ckpt.lengths[r], r, 0)]
        dev = torch.tensor(recs, dtype=torch.int32).to(self.vtail.device, non_blocking=True)
        _lib.call("qattn_mxfp4_paged_rollback", _lib.ptr(ckpt.saved), _lib.ptr(self.vtail), _lib.ptr(self.vt),
                  _lib.ptr(self.vs), _lib.ptr(self.lens), _lib.ptr(self.block_table), _lib.ptr(dev), len(rows),
                  len(ckpt.seq_ids), self.alloc.max_seqs, H, self.num_pages, self.page_tokens,
                  self.alloc.max_pages_per_seq, D, _lib.stream_of(self.vtail))
        for r in rows:
            b = ckpt.seq_ids[r]
            self.alloc.shrink(b, ckpt.pages[r])
            self.lengths[b] = ckpt.lengths[r]
            self.epoch[b] += 1
            ckpt.epochs[r] = self.epoch[b]

    def _accept_pages(self, ckpt: "Checkpoint", rows, ids, acc) -> None:
        """Raise unless the append that follows the rollback of :meth:`accept` will find its pages, so that
        a refused accept changes nothing.  The rollback returns a page past a sequence's cut only when the
        listed sequences hold all its references: a fork made after the drafts keeps it.  Those pages are
        counted only when the free ones do not suffice."""
        a = self.alloc
        full = [a.pages_for(ckpt.lengths[r] + len(kept)) for r, kept in zip(rows, acc)]
        if max(full) > a.max_pages_per_seq:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequences {ids} would pass max_pages_per_seq = "
                                  f"{a.max_pages_per_seq} pages with their accepted tokens")
        need = sum(max(0, n - ckpt.pages[r]) for n, r in zip(full, rows))
        if need <= a.free_pages:
            return
        past = {}
        for r, b in zip(rows, ids):
            for p in a.pages[b][ckpt.pages[r]:]:
                if p is not None:
                    past[p] = past.get(p, 0) + 1
        back = sum(1 for p, n in past.items() if a.refcount[p] == n)
        if need > a.free_pages + back:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: out of pages ({need} needed for the accepted tokens, "
                                  f"{a.free_pages} of {self.num_pages} free and {back} returned by the rollback: "
                                  "a fork made after the drafts still holds their pages)")

    def accept(self, ckpt: "Checkpoint", k: torch.Tensor, v: torch.Tensor, seq_ids, counts, accepted,
               rope: Optional[Rope] = None) -> "PagedKVFP4":
        """:meth:`rollback` of ``seq_ids`` followed by one :meth:`append_packed` of the draft rows that
        survive.  ``k``, ``v``, ``seq_ids`` and ``counts`` are those of the draft step's ``append_packed``;
        ``accepted[j]`` lists distinct token indices into sequence j's ``counts[j]`` tokens, in the order
        in which they are kept (a :func:`tree_path`, say); it may be empty, and a sequence that keeps
        nothing is only rolled back.  The kept rows are gathered from ``k``, ``v`` on the device with
        uploaded indices.  Every argument is checked before anything changes, the pages included: the
        kept tokens take the pages the rollback returns, and when a fork made after the drafts still
        holds those and the pool has no others, the call raises, naming "out of pages", before the
        rollback.  Stream-ordered; returns ``self``.

        ``rope`` goes to the inner ``append_packed`` with its default positions, so the kept rows of
        sequence j are rotated to L0_j, L0_j + 1, ...: for a :func:`tree_path` exactly where their depths
        put them in the draft step.  ``k`` is then the UNROTATED key of the draft step, the tensor that
        step's ``append_packed(..., rope=)`` was given."""
        _, H, _, D = self.shape
        if rope is not None and not isinstance(rope, Rope):
            raise _lib.QAttnError("qattn mxfp4 rope: rope must be a Rope")
        ids, cnt = _packed_lists(self.alloc.max_seqs, seq_ids, counts, "counts")
        if (k.dim() != 3 or tuple(k.shape[1:]) != (H, D) or k.shape != v.shape or k.shape[0] != sum(cnt)):
            raise _lib.QAttnError("qattn mxfp4 paged cache: packed tokens must be k, v [sum(counts), Hkv, D]")
        acc = [[int(i) for i in a] for a in accepted]
        if len(acc) != len(ids) or any(len(set(a)) != len(a) or any(not 0 <= i < c for i in a)
                                       for a, c in zip(acc, cnt)):
            raise _lib.QAttnError("qattn mxfp4 paged cache: accepted must list, per sequence, distinct token "
                                  f"indices below its count (counts {cnt}, accepted {acc})")
        rows = self._rollback_check(ckpt, ids)
        _lib.require_gpu(k, v, self.k4)
        self._accept_pages(ckpt, rows, ids, acc)
        self._rollback(ckpt, rows)
        first = list(itertools.accumulate([0] + cnt[:-1]))
        keep = [f + i for f, a in zip(first, acc) for i in a]
        if keep:
            idx = torch.tensor(keep, dtype=torch.long).to(k.device, non_blocking=True)
            kept = [(b, len(a)) for b, a in zip(ids, acc) if a]
            self.append_packed(k.index_select(0, idx), v.index_select(0, idx), [b for b, _ in kept],
                               [n for _, n in kept], rope=rope)
        return self

    def fork(self, src: int, dst: int) -> None:
        """Make the empty sequence ``dst`` a copy of ``src`` that shares its memory: the ``L // P``
        full pages by reference count; a partial last page is copied into a fresh page on the device
        (all heads, four operands), as are the ``vtail`` and ``k_mean`` rows.  Stream-ordered.  A
        trimmed ``src`` is refused."""
        src, dst = self.alloc._seq(src), self.alloc._seq(dst)
        self._whole(src, "fork")
        if self.lengths[dst]:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: fork into sequence {dst}, which is not empty "
                                  f"({self.lengths[dst]} tokens)")
        L, P = self.lengths[src], self.page_tokens
        fresh = self.alloc.share(src, dst, L // P, 1 if L % P else 0)
        if fresh:
            old = self.alloc.pages[src][L // P]
            for t in self.kv:
                t[fresh[0]].copy_(t[old])
        self.vtail[dst].copy_(self.vtail[src])
        if self.k_mean is not None:
            self.k_mean[dst].copy_(self.k_mean[src])
        self.lengths[dst] = L
        self._upload(table=True)

    def prefix_groups(self, seq_ids) -> list:
        """:meth:`PageAllocator.prefix_groups` of the pool: which of the listed sequences hold the same
        leading pages (after :meth:`fork`), as ``[(members, common_pages), ...]`` with ``members`` indices
        into ``seq_ids``.  One level of sharing per call: a sub-group that shares a longer prefix still
        gets only its group's common pages.  Host only, no tensor."""
        return self.alloc.prefix_groups(seq_ids)

    def gather(self, b: int):
        """Copies of sequence ``b``'s pages in order, per head: (k4 [Hkv, n*P, D/2], ks [Hkv, n*P, D/32],
        vt [Hkv, n*P/64, D, 32], vs [Hkv, n*P/64, D, 2]) for its n pages.  A trimmed sequence is refused."""
        self._whole(self.alloc._seq(b), "gather")
        pages = torch.tensor(self.alloc.pages[self.alloc._seq(b)], dtype=torch.long, device=self.k4.device)
        H = self.k4.shape[1]
        return tuple(t[pages].transpose(0, 1).reshape(H, -1, *t.shape[3:]) for t in self.kv)

    def snapshot(self, b: int) -> QuantizedKVFP4:
        """A :class:`QuantizedKVFP4` copy (batch 1) of sequence ``b``, whose length must be a
        multiple of 64 (and not 0)."""
        L = self.lengths[self.alloc._seq(b)]
        self._whole(int(b), "snapshot")
        if L == 0 or L % BLOCK:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: snapshot needs a length of 64*n tokens, got {L}")
        k4, ks, vt, vs = self.gather(b)
        return QuantizedKVFP4(k4[None, :, :L].contiguous(), ks[None, :, :L].contiguous(),
                              vt[:, :L // BLOCK].contiguous(), vs[:, :L // BLOCK].contiguous(),
                              None if self.k_mean is None else self.k_mean[b:b + 1].clone())


@torch.no_grad()
def attention_mxfp4_decode_paged(q: torch.Tensor, cache: PagedKVFP4, causal: bool = False,
                                 keys_per_split: Optional[int] = None):
    """:func:`attention_mxfp4_decode` against a paged cache: fp16 queries [max_seqs, Hq, Sq, D],
    sequence b over its own ``lengths[b]`` keys, found through ``block_table`` -> (O fp16 [max_seqs,
    Hq, Sq, D], lse fp32 [max_seqs*Hq, Sq] base 2), bit for bit what a preallocated cache with the same
    tokens gives.  The same contract: every sequence slot needs a length >= 1 (raises otherwise),
    causal needs Sq <= min(lengths); the plan is ``_split_plan_fp4`` at ceil64(max(lengths)), and
    ``keys_per_split`` is any multiple of 64, whatever the page size."""
    bhv, rows, sk_max, kps, nsplit = _decode_plan(q, cache, causal, keys_per_split, PagedKVFP4)
    if any(cache.alloc.nholes):   # this entry has no window: it reads every page
        for b in range(cache.alloc.max_seqs):
            cache._whole(b, "attention_mxfp4_decode_paged")
    _lib.require_gpu(q, cache.k4)
    return _split_and_merge(q, cache.kv, causal, kps, nsplit, bhv, rows, "qattn_mxfp4_attn_fwd_split_paged",
                            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), bhv, cache.shape[1], rows,
                            q.shape[2], cache.num_pages, cache.page_tokens, cache.alloc.max_pages_per_seq,
                            sk_max)


# ------------------------------------------------------------------------------ packed (varlen) step
QROWS = 128   # query rows of a workgroup (csrc/mxfp4_attn.hip MxCfg::QROWS)


def _packed_lists(max_seqs: int, seq_ids, counts, what: str):
    """``seq_ids`` and ``counts`` of a packed call as lists of ints, checked: nseq >= 1 distinct slots
    in [0, max_seqs), every count >= 1."""
    as_list = lambda x: [int(i) for i in (x.tolist() if isinstance(x, torch.Tensor) else x)]  # noqa: E731
    ids, cnt = as_list(seq_ids), as_list(counts)
    if not ids or len(ids) != len(cnt):
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: seq_ids and {what} must list the same nseq >= 1 "
                              "sequences")
    if any(not 0 <= b < max_seqs for b in ids) or len(set(ids)) != len(ids):
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: seq_ids must be distinct slots in [0, {max_seqs}), "
                              f"got {ids}")
    if any(c < 1 for c in cnt):
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: every entry of {what} must be >= 1, got {cnt}")
    return ids, cnt


def _window_args(window, sinks, required: bool = False):
    """``(window, sinks)`` of a call, checked -> (W, S) as ints, or (None, 0) without a window."""
    if window is None:
        if required:
            raise _lib.QAttnError("qattn mxfp4 paged cache: a window >= 1 expected")
        if sinks:
            raise _lib.QAttnError("qattn mxfp4 paged cache: sinks without a window (sinks keep the first "
                                  "keys visible below a window's lower edge)")
        return None, 0
    if not isinstance(window, int) or not isinstance(sinks, int) or window < 1 or sinks < 0:
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: window must be an int >= 1 and sinks an int >= 0, "
                              f"got window {window!r}, sinks {sinks!r}")
    return int(window), int(sinks)


def _window_tiles(L: int, n: int, W: int, S: int):
    """(wt0', nst', nt) of a sequence of L keys and n queries under window W and S sinks: the first tile
    of the window run and the sink tiles when there is a gap between the two runs, else (0, 0)."""
    nt = -(-L // BLOCK)
    wt0, nst = max(0, L - n - W + 1) // BLOCK, -(-min(S, L) // BLOCK)
    return (wt0, nst, nt) if wt0 > nst else (0, 0, nt)


def _window_pages(L: int, n: int, W: int, S: int, P: int) -> list:
    """The page indices a windowed call reads of a sequence of L keys and n queries: the pages of the
    tiles it runs (the sink run and the window run, or every tile when the two touch)."""
    wt0, nst, nt = _window_tiles(L, n, W, S)
    tpp = P // BLOCK
    pages = set(range(-(-nst // tpp))) if nst else set()
    return sorted(pages | set(range(wt0 // tpp, -(-nt // tpp))))


def _varlen_lists(lengths, seq_ids, q_lens, Hq: int, Hkv: int, causal: bool):
    """What every packed plan checks first -> (slots, q_lens, lengths of the listed slots) as ints."""
    lengths = [int(x) for x in lengths]
    ids, sq = _packed_lists(len(lengths), seq_ids, q_lens, "q_lens")
    if Hkv < 1 or Hq < 1 or Hq % Hkv:
        raise _lib.QAttnError("qattn mxfp4 paged cache: q must have G * Hkv heads for the cache's Hkv")
    Ls = [lengths[b] for b in ids]
    if min(Ls) < 1:
        raise _lib.QAttnError("qattn mxfp4 paged cache: every listed sequence needs at least one cached "
                              f"token (slots {ids}, lengths {Ls})")
    if causal and any(n > L for n, L in zip(sq, Ls)):
        raise _lib.QAttnError("qattn mxfp4 paged cache: causal attention needs q_lens[j] <= the cached "
                              f"tokens of every listed sequence (q_lens {sq}, lengths {Ls})")
    return ids, sq, Ls


TREE_NODES = 64   # nodes of one sequence's draft tree: the bits of its ancestor words


def _tree_parents(parents) -> list:
    par = [int(p) for p in (parents.tolist() if isinstance(parents, torch.Tensor) else parents)]
    if len(par) > TREE_NODES:
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: a draft tree of {len(par)} nodes; at most {TREE_NODES} "
                              "(one bit of the ancestor word each)")
    bad = [t for t, p in enumerate(par) if not -1 <= p < t]
    if bad:
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: draft tree nodes {bad} have a parent outside [-1, t): "
                              "nodes come in topological order (parent < child, -1 marks a root)")
    return par


def tree_ancestor_masks(parents) -> list:
    """The 64-bit ancestor words of a draft tree (or forest) given as ``parents``: ``parents[t]`` in [-1, t)
    is the parent of node t, -1 marks a root, so the nodes are in topological order -> ``anc`` with bit b of
    ``anc[t]`` set iff node b is an ancestor of node t or t itself.  Every word is a subset of bits <= t
    that holds bit t.  Pure Python, no device.  Raises :class:`QAttnError` for a parent >= t (or < -1) and
    for more than 64 nodes."""
    anc = []
    for t, p in enumerate(_tree_parents(parents)):
        anc.append((anc[p] if p >= 0 else 0) | 1 << t)
    return anc


def tree_path(parents, leaf: int) -> list:
    """The node indices from the root to ``leaf`` (both included), ascending: the ``accepted`` list of
    :meth:`PagedKVFP4.accept` for the path that ends at ``leaf``."""
    par, leaf = _tree_parents(parents), int(leaf)
    if not 0 <= leaf < len(par):
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: no node {leaf} in a draft tree of {len(par)} nodes")
    path = []
    while leaf >= 0:
        path.append(leaf)
        leaf = par[leaf]
    return path[::-1]


ARANGE_TOKENS = 32   # a run of more default positions than this is a torch.arange, not a Python list


def _default_positions(lengths_before, seq_ids, counts, tree=None):
    """:func:`rope_positions` as (host int32 tensor [T], lowest value, highest value): long runs are ranges,
    so a prefill chunk costs no Python per token."""
    lengths = [int(x) for x in lengths_before]
    ids, cnt = _packed_lists(len(lengths), seq_ids, counts, "counts")
    trees = [None] * len(ids) if tree is None else list(tree)
    if len(trees) != len(ids):
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: tree must have one entry (None or a parents list) per "
                              f"listed sequence, got {len(trees)} for {len(ids)}")
    parts, run, hi = [], [], -1

    def flush():
        if run:
            parts.append(torch.tensor(run, dtype=torch.int32))
            run.clear()

    for b, c, p in zip(ids, cnt, trees):
        depth = []
        for q in ([] if p is None else _tree_parents(p)):
            depth.append(depth[q] + 1 if q >= 0 else 0)
        if len(depth) > c:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: a tree of {len(depth)} nodes on a sequence of {c} "
                                  "tokens")
        L, plain = lengths[b], c - len(depth)
        if plain > ARANGE_TOKENS:
            flush()
            parts.append(torch.arange(L, L + plain, dtype=torch.int32))
        else:
            run.extend(range(L, L + plain))
        run.extend(L + plain + d for d in depth)
        hi = max(hi, L + plain - 1, L + plain + max(depth, default=-1))
    flush()
    lo = min(lengths[b] for b in ids)
    return (parts[0] if len(parts) == 1 else torch.cat(parts)), lo, hi


def rope_positions(lengths_before, seq_ids, counts, tree=None) -> list:
    """The default rotary positions of a packed step -> one int per packed token, from the host mirror
    alone (no device).  ``lengths_before`` holds one length per slot BEFORE the step's append; token i of
    the ``counts[j]`` tokens of slot ``seq_ids[j]`` gets L_j + i.  With ``tree`` (one entry per listed
    sequence, None or a ``parents`` list of nd_j <= counts[j] nodes, as in
    :func:`attention_mxfp4_varlen_paged`) the last nd_j tokens are draft nodes and get L_j + (counts[j] -
    nd_j) + depth, a root at depth 0: where the node lands when its path is accepted.  Raises
    :class:`QAttnError` as ``append_packed`` does for its lists and :func:`tree_ancestor_masks` for a tree,
    and for a tree list of another length or a tree of more nodes than the sequence has tokens."""
    return _default_positions(lengths_before, seq_ids, counts, tree)[0].tolist()


def _rope_args(rope, positions, tree, tokens: int, default):
    """The rotary arguments of a packed call, checked before anything is reserved or launched -> None
    without ``rope``, else an int32 tensor [tokens]: the device tensor given as ``positions``, or host
    positions inside the table (``positions``, else ``default()``, the arguments of
    :func:`_default_positions`)."""
    if rope is None:
        if positions is not None or tree is not None:
            raise _lib.QAttnError("qattn mxfp4 rope: positions or tree without rope (they place the rotation)")
        return None
    if not isinstance(rope, Rope):
        raise _lib.QAttnError("qattn mxfp4 rope: rope must be a Rope")
    if positions is None:
        pos, lo, hi = _default_positions(*default())
        if lo < 0 or hi >= rope.max_pos:
            raise _lib.QAttnError(f"qattn mxfp4 rope: the default positions [{lo}, {hi}] lie outside the table's "
                                  f"[0, {rope.max_pos})")
        return pos
    if tree is not None:
        raise _lib.QAttnError("qattn mxfp4 rope: explicit positions together with tree (tree only places the "
                              "default positions)")
    return positions if _device_positions(positions, tokens) else _host_positions(positions, tokens, rope.max_pos)


def plan_varlen(lengths, seq_ids, q_lens, Hq: int, Hkv: int, keys_per_split: Optional[int] = None,
                causal: bool = False, window: Optional[int] = None, sinks: int = 0, tree_lens=None):
    """The host plan of :func:`attention_mxfp4_varlen_paged` -> (kps, seq_rec, work, part_rows); pure
    Python on the host mirror ``lengths`` (one entry per slot), no device and no tensor.

    ``kps``: one key split size per call.  None takes ``qattn_split_keys(W, 1, sk_max, 64)``, the
    library's rule (two workgroups per CU, no split under 1024 keys) at the call's real workgroup count
    W = Hkv * sum_j ceil(G * q_lens[j] / 128) and sk_max = ceil64(max_j L_j), L_j the length of
    ``seq_ids[j]``.  Sequence j then has ns_j = ceil(ceil64(L_j) / kps) splits of its own.  The rule's
    constants (512 workgroups, 1024 keys) were measured on uniform batches only (``_split_plan_fp4``)
    and are not tuned for mixed ones.  What mixed batches gave on one MI355X (tools/time_decode_varlen.py,
    2026-10-20, 32 / 8 heads, P = 256, causal, whole call, median us of 3 x 20 alternating calls, pass
    medians within 0.1 to 2.3 %): a 2048-token chunk at 8192 cached beside 63 decodes over 512 .. 8192
    keys, rule 8192 keys (no split) 260.5, 4096 keys 237.2, 1024 keys 401.8 (kernel alone 230.8 against
    202.3 at 4096); a 512-token chunk beside 15 decodes, rule 2752 keys 114.9, 1408 keys 136.8, 5504
    keys 111.0, 1024 keys 151.7.  The rule loses to half its value on the first shape by more than the
    spread and wins on the second, so it is left as it is; the long chunk, whose workgroups the rule
    counts like a decode's, is what a better rule would split.

    ``seq_rec`` [nseq][8] = [slot, first packed token, q_lens[j], ns_j, first partial row, 0, 0, 0].
    Sequence j owns the ns_j * Hkv * G * q_lens[j] partial rows from its first one, laid out [split][kv
    head][virtual row g * q_lens[j] + i]; the blocks are dense in [0, ``part_rows``).
    ``work`` [nwork][4] = [j, 128-row block, split, 0]: one record per workgroup and key/value head,
    every split < ns_j of every row block of every sequence once, ordered by descending tile count of
    the split (the longest workgroups start first); results do not depend on the order.

    ``window`` (with ``sinks``; None: the plan above, unchanged): the windowed call's plan (module
    docstring).  seq_rec[j][5:7] = [wt0, nst] when sequence j has a gap between its sink tiles and its
    window's first tile, else [0, 0]; ns_j = (nst > 0) + ceil((nt - wt0) * 64 / kps); the sink split counts
    nst tiles in the order of ``work``; and ``kps`` (given or the rule's, the rule taken at this sk_max) is
    clamped to sk_max = 64 * max_j (tiles sequence j runs), not to the cached length.  Raises for window <
    1, sinks < 0, sinks without a window, and a window without ``causal``.  Measured on one MI355X
    (tools/time_decode_varlen.py --window 4096 --sinks 4, 2026-10-20, 64 decodes, 32 / 8 heads, P = 256, L
    = 32768, median us of 3 x 20 alternating calls, range of the pass medians): windowed 217.2
    (215.3..223.5), causal on the same pool 670.6 (669.2..671.5), causal on a pool of 4160 cached keys
    164.2 (163.9..165.3): 0.32 of the causal call, 53 us behind the short one, host-bound (128 work
    records against 64).  Kernels alone 91.2 / 653.8 / 84.7, the windowed one without sinks 90.3: the
    sink split costs 0.9 us, the rest of the 6.5 us is the windowed instantiation.
    ``free_pages`` before and after ``trim`` of that batch: 0 -> 7104 of 8192.

    ``tree_lens`` (None: no trees): one int per listed sequence, nd_j tree tokens among its q_lens[j] (module
    docstring); ``seq_rec[j][7]`` = nd_j and everything else -- splits, work records, partial rows -- is the
    causal plan's.  Raises, naming "tree", without ``causal``, with a window, and for nd_j outside [0,
    min(q_lens[j], 64)].

    Raises :class:`QAttnError` for an empty, duplicate or out-of-range slot list, a q_lens entry < 1, a
    listed slot of length 0, ``causal`` with q_lens[j] > L_j, Hq % Hkv != 0, a ``keys_per_split`` that
    is not a multiple of 64, and when T * Hq, part_rows or nwork * Hkv reach 2^31.  The slots that are
    not listed are not looked at.
    """
    W, S = _window_args(window, sinks)
    if W is not None and not causal:
        raise _lib.QAttnError("qattn mxfp4 paged cache: a window implies causal attention; pass causal=True")
    ids, sq, Ls = _varlen_lists(lengths, seq_ids, q_lens, Hq, Hkv, causal)
    nds = [0] * len(ids)
    if tree_lens is not None:
        nds = [int(x) for x in tree_lens]
        if not causal or W is not None:
            raise _lib.QAttnError("qattn mxfp4 paged cache: a tree mask needs causal=True and no window (every "
                                  "tree node sees the cached keys and its ancestors)")
        if len(nds) != len(ids) or any(not 0 <= nd <= min(n, TREE_NODES) for nd, n in zip(nds, sq)):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: tree lengths {nds} must be one per sequence, each "
                                  f"in [0, min(q_lens[j], {TREE_NODES})] (q_lens {sq})")
    G = Hq // Hkv
    nrb = [-(-G * n // QROWS) for n in sq]
    sk_max = _ceil64(max(Ls))
    if W is not None:   # (first window tile, sink tiles, tiles) per sequence; the tiles it actually runs
        wt = [_window_tiles(L, n, W, S) for L, n in zip(Ls, sq)]
        sk_max = BLOCK * max(nst + nt - wt0 for wt0, nst, nt in wt)
    if keys_per_split is None:
        kps = _lib.load().qattn_split_keys(Hkv * sum(nrb), 1, sk_max, BLOCK)
    else:
        kps = int(keys_per_split)
    if kps < BLOCK or kps % BLOCK:
        raise _lib.QAttnError("qattn mxfp4 paged cache: keys_per_split must be a multiple of 64")
    kps = min(kps, sk_max)
    nsp = [-(-_ceil64(L) // kps) for L in Ls]
    if W is not None:
        nsp = [(1 if nst else 0) + -(-(nt - wt0) * BLOCK // kps) for wt0, nst, nt in wt]
    if (sum(sq) * Hq >= 1 << 31 or sum(ns * Hkv * G * n for ns, n in zip(nsp, sq)) >= 1 << 31
            or sum(ns * r for ns, r in zip(nsp, nrb)) * Hkv >= 1 << 31):
        raise _lib.QAttnError("qattn mxfp4 paged cache: a packed call of 2^31 or more query rows, partial "
                              "rows or workgroups")
    seq_rec, work, first, base = [], [], 0, 0
    for j, (b, n, L, ns) in enumerate(zip(ids, sq, Ls, nsp)):
        wt0, nst = wt[j][:2] if W is not None else (0, 0)
        seq_rec.append([b, first, n, ns, base, wt0, nst, nds[j]])
        nt = -(-L // BLOCK)
        for s in range(ns):
            if nst and s == 0:   # a gap: the sink split, then the window splits from wt0
                tiles = nst
            elif W is not None:
                t0 = wt0 + (s - (1 if nst else 0)) * (kps // BLOCK)
                tiles = min(nt, t0 + kps // BLOCK) - t0
            else:
                tiles = min(nt, (s + 1) * (kps // BLOCK)) - s * (kps // BLOCK)
            work += [(tiles, [j, rb, s, 0]) for rb in range(nrb[j])]
        first += n
        base += ns * Hkv * G * n
    work.sort(key=lambda w: -w[0])   # stable: equal tile counts stay in sequence order
    return kps, seq_rec, [w for _, w in work], base


def plan_varlen_shared(lengths, seq_ids, q_lens, Hq: int, Hkv: int, groups, keys_per_split: Optional[int] = None,
                       causal: bool = False, *, page_tokens: int):
    """The host plan of :func:`attention_mxfp4_varlen_paged` with ``share_prefix=True`` -> (kps, seq_rec,
    work, part_rows, grp_rec, members); pure Python like :func:`plan_varlen`.  ``groups`` is what
    :meth:`PagedKVFP4.prefix_groups` gives for ``seq_ids``, ``[(members, common_pages), ...]`` with
    ``members`` ascending indices into ``seq_ids``, and ``page_tokens`` the pool's P.

    The shared call keeps the plain call's splits and changes only who computes them.  Sequence j has
    the splits [s * kps, (s + 1) * kps) of :func:`plan_varlen`; group g shares the first ``ns_g = min(
    common_pages * P, min_j vis_j) // kps`` of them, vis_j = L_j - n_j + 1 causal and L_j otherwise: the
    splits that lie wholly inside the common pages and on which no row of any member masks a key.  A
    group with ns_g == 0 dissolves into plain sequences.  ``seq_rec`` and ``part_rows`` are
    :func:`plan_varlen`'s for the same ``kps``.  ``work`` [nwork][4] holds [j, 128-row block, split, 0] for
    every split >= ns_g of a member (every split of an ungrouped sequence) and [g, 128-row block of the
    group's stacked rows, split, 1] for every split < ns_g, by descending tile count.  ``grp_rec``
    [ngroup][4] = [first entry in members, member count, ns_g, R_g], R_g = G * sum of the members' q_lens;
    ``members`` [nmember][2] = [j, first stacked row of sequence j in its group], ascending inside a
    group; stacked row r is row r - first of its member's virtual head, in that member's own order g *
    n_j + i.  The group workgroup writes each row's state into the member's own partial rows at split s,
    where the plain workgroup would have, so the merge is unchanged.

    ``kps`` when ``keys_per_split`` is None: ``qattn_split_keys`` at the shared call's own workgroup count,
    Hkv * (sum_g ceil(R_g / 128) + sum over ungrouped j of ceil(G * n_j / 128)), then lowered to the
    largest multiple of 64 that is <= the smallest group's shareable key count min(common_pages * P, min_j
    vis_j) when it exceeds that, so that every group shares at least one split (a group that cannot
    share 64 keys is left out of this minimum: it dissolves whatever kps is).  An explicit
    ``keys_per_split`` is used as given (a multiple of 64, clamped to sk_max as in :func:`plan_varlen`).
    This default began as a guess from byte counts.  What one MI355X gave (tools/time_decode_shared.py,
    2026-10-20, one new token per sequence, 32 / 8 heads, P = 256, causal, median us of 3 x 20 alternating
    calls, whole call | kernel alone, against the plain call at its own rule in the same run; pass
    medians within 0.2 to 3 % except the first shape's shared whole calls, 10 %): 64 forks of a 32768-key
    prompt + 256 own keys, plain 539.8 | 522.7, shared at the rule (1088 keys) 267.3 | 32.6, at 512 keys
    287.1 | 34.6, at 1024 keys 272.9 | 29.5; 8 forks of it, plain 114.7 | 67.7, shared at the rule (1088)
    110.7 | 22.2, at 512 118.6 | 15.2, at 1024 110.3 | 21.2; 64 forks of a 2048-key prompt, plain 171.6 |
    34.9, shared at the rule (1152) 209.1 | 27.0, at 576 210.0 | 16.6, at 1024 209.8 | 19.1; 16 forks of an
    8192-key prompt beside 16 unrelated decodes, plain 140.5 | 70.4, shared at the rule (2112) 161.2 |
    44.5, at 1024 177.5 | 25.9.  The kernel wins on all four; the whole call wins on the first (2.0 x) and
    barely on the second, and LOSES on the last two (host-bound: the groups and the longer plan are
    Python before the launch).  On the kernel alone the rule loses to a swept value by more than the
    spread on every shape (1024, 512, 576, 1024 keys); on the whole call it is level or ahead on all
    four, so it is left as it is.

    Raises as :func:`plan_varlen` (same messages, same 2^31 limits), and for a group with fewer than two
    members or no common page, a member out of range or not ascending, and a sequence in two groups.
    """
    ids, sq, Ls = _varlen_lists(lengths, seq_ids, q_lens, Hq, Hkv, causal)
    P, G, nseq = int(page_tokens), Hq // Hkv, len(ids)
    if P not in PAGE_TOKENS:
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: page_tokens must be 64 * 2^k in [64, 1024], got {P}")
    glist, grouped = [], set()
    for mem, common in groups:
        mem, common = [int(x) for x in mem], int(common)
        if len(mem) < 2 or common < 1:
            raise _lib.QAttnError("qattn mxfp4 paged cache: a prefix group needs at least two members and one "
                                  f"common page, got {mem}, {common}")
        if any(not 0 <= j < nseq for j in mem) or any(a >= b for a, b in zip(mem, mem[1:])):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: group members must be ascending indices into the "
                                  f"{nseq} listed sequences, got {mem}")
        if grouped.intersection(mem):
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: sequences {sorted(grouped.intersection(mem))} are "
                                  "in two prefix groups")
        grouped.update(mem)
        vis = min(Ls[j] - sq[j] + 1 if causal else Ls[j] for j in mem)
        glist.append((mem, min(common * P, vis)))   # (members, keys the group can share)
    nrb = [-(-G * n // QROWS) for n in sq]
    sk_max = _ceil64(max(Ls))
    if keys_per_split is None:
        wgs = sum(-(-G * sum(sq[j] for j in mem) // QROWS) for mem, _ in glist)
        wgs += sum(r for j, r in enumerate(nrb) if j not in grouped)
        kps = _lib.load().qattn_split_keys(Hkv * wgs, 1, sk_max, BLOCK)
        least = min((keys for _, keys in glist if keys >= BLOCK), default=kps)
        if kps > least:
            kps = least // BLOCK * BLOCK
    else:
        kps = int(keys_per_split)
    if kps < BLOCK or kps % BLOCK:
        raise _lib.QAttnError("qattn mxfp4 paged cache: keys_per_split must be a multiple of 64")
    kps = min(kps, sk_max)
    tps = kps // BLOCK
    nsp = [-(-_ceil64(L) // kps) for L in Ls]
    if (sum(sq) * Hq >= 1 << 31 or sum(ns * Hkv * G * n for ns, n in zip(nsp, sq)) >= 1 << 31
            or sum(ns * r for ns, r in zip(nsp, nrb)) * Hkv >= 1 << 31):
        raise _lib.QAttnError("qattn mxfp4 paged cache: a packed call of 2^31 or more query rows, partial "
                              "rows or workgroups")
    shared = [0] * nseq   # ns_g of the sequence's group, 0 for a plain sequence
    grp_rec, members, work = [], [], []
    for mem, keys in glist:
        ns_g = keys // kps
        if not ns_g:   # nothing to share at this kps: plain sequences
            continue
        rows = 0
        grp_rec.append([len(members), len(mem), ns_g, G * sum(sq[j] for j in mem)])
        for j in mem:
            shared[j] = ns_g
            members.append([j, rows])
            rows += G * sq[j]
        g = len(grp_rec) - 1
        work += [(tps, [g, rb, s, 1]) for s in range(ns_g) for rb in range(-(-rows // QROWS))]
    seq_rec, first, base = [], 0, 0
    for j, (b, n, L, ns) in enumerate(zip(ids, sq, Ls, nsp)):
        seq_rec.append([b, first, n, ns, base, 0, 0, 0])
        nt = -(-L // BLOCK)
        for s in range(shared[j], ns):
            work += [(min(nt, (s + 1) * tps) - s * tps, [j, rb, s, 0]) for rb in range(nrb[j])]
        first += n
        base += ns * Hkv * G * n
    work.sort(key=lambda w: -w[0])   # stable: group records first among the full splits
    return kps, seq_rec, [w for _, w in work], base, grp_rec, members


def _shared_plan(cache: "PagedKVFP4", ids, sq, Hq: int, keys_per_split, causal: bool, window):
    """The plan of a ``share_prefix=True`` call over the listed slots, or None when nothing is shared
    (no two listed sequences hold a common page, or no whole split fits the common pages): the caller
    then makes the plain call.  Raises for a window."""
    if window is not None:
        raise _lib.QAttnError("qattn mxfp4 paged cache: share_prefix with a window is not supported (a "
                              "window's lower edge masks keys of the shared prefix row by row)")
    groups = cache.prefix_groups(ids)
    if not groups:
        return None
    plan = plan_varlen_shared(cache.lengths, ids, sq, Hq, cache.shape[1], groups, keys_per_split, causal,
                              page_tokens=cache.page_tokens)
    return plan if plan[4] else None


def _check_trimmed(cache: "PagedKVFP4", ids, sq, W, S) -> None:
    """Raise when a packed call over ``ids`` with ``sq`` queries each and window ``(W, S)`` (W None: no
    window) would read a page that :meth:`PagedKVFP4.trim` gave back."""
    P = cache.page_tokens
    for b, n in zip(ids, sq):
        if W is None:
            cache._whole(b, "a call without a window")
            continue
        if not cache.alloc.nholes[b]:
            continue
        pages = cache.alloc.pages[b]
        bad = [p for p in _window_pages(cache.lengths[b], n, W, S, P) if p < len(pages) and pages[p] is None]
        if bad:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: window {W} with {S} sinks and {n} queries would "
                                  f"read trimmed pages {bad} of sequence {b} (it was trimmed for a smaller "
                                  "window or fewer sinks)")


def _tree_args(tree, sq, causal: bool, window, share_prefix: bool):
    """``tree`` of a packed call over sequences of ``sq`` queries, checked -> (tree lengths, the int64
    ancestor word of every packed token as a host int32 tensor [2 T], low half first), or None when no
    sequence has a tree (the plain causal call is then made).  Every refusal names "tree"."""
    if not causal or window is not None or share_prefix:
        raise _lib.QAttnError("qattn mxfp4 paged cache: tree needs causal=True and cannot be combined with a "
                              "window or share_prefix")
    tree = list(tree)
    if len(tree) != len(sq):
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: tree must have one entry (None or a parents list) per "
                              f"listed sequence, got {len(tree)} for {len(sq)}")
    # one host tensor of words per distinct parents list (a batch usually drafts one tree shape): the host
    # work per sequence is a dictionary look-up and, at the end, one concatenation
    seen, parts, nds = {}, [], []
    for p, n in zip(tree, sq):
        w = seen.get(id(p))
        if w is None:
            anc = [] if p is None else tree_ancestor_masks(p)
            w = seen[id(p)] = torch.tensor([x - (1 << 64) if x >> 63 else x for x in anc], dtype=torch.int64)
        nds.append(w.numel())
        if w.numel() > n:
            raise _lib.QAttnError(f"qattn mxfp4 paged cache: a tree of {w.numel()} nodes on a sequence of {n} "
                                  "query tokens")
        if n > w.numel():
            parts.append(torch.zeros(n - w.numel(), dtype=torch.int64))
        parts.append(w)
    if not any(nds):
        return None
    return nds, torch.cat(parts).view(torch.int32)


def _query_positions(cache: "PagedKVFP4", ids, sq, tree, rope, positions):
    """``_rope_args`` of a packed attention call: the default positions are those of the append that made
    the queries the sequences' last tokens (``tree`` is the call's mask, so explicit positions may come
    with it)."""
    def default():
        before = list(cache.lengths)
        for b, n in zip(ids, sq):
            before[b] -= n
        return before, ids, sq, tree
    return _rope_args(rope, positions, None, sum(sq), default)


@torch.no_grad()
def attention_mxfp4_varlen_paged(q: torch.Tensor, cache: PagedKVFP4, seq_ids, q_lens, causal: bool = False,
                                 keys_per_split: Optional[int] = None, window: Optional[int] = None,
                                 sinks: int = 0, share_prefix: bool = False, tree=None,
                                 rope: Optional[Rope] = None, positions=None):
    """A ragged batch against a paged cache in one attention launch and one merge: packed fp16 queries
    ``q`` [T, Hq, D], token-major, the ``q_lens[0]`` tokens of sequence ``seq_ids[0]`` first, then
    those of ``seq_ids[1]``, ... (nseq >= 1 distinct slots, every q_lens[j] >= 1, T = sum(q_lens)) ->
    (O fp16 [T, Hq, D], lse fp32 [T, Hq] base 2).  Sequence ``seq_ids[j]`` is attended over its own
    ``lengths[slot]`` keys through its table row; ``causal`` is bottom-right per sequence (query i of
    sequence j keeps the keys <= L_j - q_lens[j] + i: a prefill chunk after its own append).  The slots
    that are not listed may be empty or hold anything: their lengths, table rows and pages are never
    read.  Every sequence gets, bit for bit, what :func:`attention_mxfp4_decode` gives for it alone
    with Sq = q_lens[j] and the same keys per split.  ``window`` (with ``sinks``; causal only) is the
    sliding window with sinks of the module docstring, through
    ``qattn_mxfp4_attn_fwd_varlen_paged_window``; a window at least as long as every sequence gives the
    causal call's bits.  Raises before any launch (and before any tensor is made) as
    :func:`plan_varlen` does, for sum(q_lens) != T, and when a listed sequence has had a page trimmed
    that this call would read.  Stream-ordered: the plan comes from the host mirror, its two
    tables are uploaded without a synchronisation, nothing is read back.

    ``share_prefix=True`` reads the pages that listed sequences hold in common (after
    :meth:`PagedKVFP4.fork`: parallel sampling, beam search, a shared system prompt) once per group
    instead of once per sequence: :meth:`PagedKVFP4.prefix_groups` finds the groups on the host,
    :func:`plan_varlen_shared` gives the key splits inside the common pages to group workgroups whose 128
    rows come from several sequences (``qattn_mxfp4_attn_fwd_varlen_paged_shared``), and everything else
    runs as above.  The result is, bit for bit, that of the same call without ``share_prefix`` at the
    same ``keys_per_split`` (the default ``keys_per_split`` differs: :func:`plan_varlen_shared`); when
    nothing is shared the plain call is made.  One level of sharing per call, and no ``window``: the
    combination raises :class:`QAttnError` before any launch.

    ``tree`` (causal only) is the verify step of speculative decoding: a list with one entry per listed
    sequence, None or that sequence's ``parents`` list (:func:`tree_ancestor_masks`), whose length is
    nd_j: the last nd_j <= min(q_lens[j], 64) query tokens of the sequence are the nodes of a draft tree
    in topological order, appended already like a prefill chunk.  With base_j = L_j - nd_j, node t sees
    key k iff ``k < base_j`` or ``k = base_j + b`` for an ancestor b of t or b = t; the queries before
    the tree and the sequences with None are plain causal; ``lse`` is over the visible keys
    (``qattn_mxfp4_attn_fwd_varlen_paged_tree``; the words are uploaded with the two tables, in one
    upload).  A chain gives the causal call's bits, and with every entry None the plain causal call is
    made.  A draft token at tree depth d sits on a path whose accepted form lands at position L0 + d (L0
    the length before the drafts): ``rope=`` (below, and in :meth:`PagedKVFP4.append_packed`) places draft
    keys and queries by depth.  Raises before any launch, naming "tree": without ``causal``, together
    with ``window`` or ``share_prefix=True``, for more nodes than min(q_lens[j], 64), and for a parent
    that is not in [-1, t).

    ``rope`` (a :class:`Rope`; None: no rotation, the bits of the call without these arguments) rotates
    ``q``, given UNROTATED, inside its quantiser (``qattn_mxfp4_quant_rows_rope`` in place of ``qattn_mxfp4_quant_rows``); everything after
    that is unchanged, so ``window``, ``share_prefix`` and ``tree`` work with it.  ``positions`` defaults to
    L_j - q_lens[j] + i for query i of sequence j, and under ``tree=`` the nodes are placed by depth: the
    numbers :func:`rope_positions` gives for the ``append_packed`` that preceded this call (the queries
    are the sequence's last q_lens[j] tokens).  Explicit ``positions`` are as in ``append_packed``: a list
    or a host tensor, checked against the table before any launch, or a device int32 tensor [T], used as
    given.  ``positions`` without ``rope`` raises."""
    if not isinstance(cache, PagedKVFP4):
        raise _lib.QAttnError("qattn mxfp4 kv cache: cache must be a PagedKVFP4")
    _, Hkv, _, D = cache.shape
    if q.dim() != 3 or q.shape[2] != D:
        raise _lib.QAttnError("qattn mxfp4 paged cache: packed queries must be q [T, Hq, 128]")
    T, Hq = q.shape[0], q.shape[1]
    if Hq == 0 or Hq % Hkv:
        raise _lib.QAttnError("qattn mxfp4 paged cache: q must have G * Hkv heads for the cache's Hkv")
    ids, sq = _packed_lists(cache.alloc.max_seqs, seq_ids, q_lens, "q_lens")
    if sum(sq) != T:
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: q holds {T} tokens, q_lens sum to {sum(sq)}")
    trees = None if tree is None else _tree_args(tree, sq, causal, window, share_prefix)
    shared = _shared_plan(cache, ids, sq, Hq, keys_per_split, causal, window) if share_prefix else None
    if shared is not None:
        kps, seq_rec, work, part_rows, grp_rec, members = shared
    else:
        kps, seq_rec, work, part_rows = plan_varlen(cache.lengths, ids, sq, Hq, Hkv, keys_per_split, causal,
                                                    window, sinks, None if trees is None else trees[0])
    W, S = _window_args(window, sinks)
    _check_trimmed(cache, ids, sq, W, S)
    pos = _query_positions(cache, ids, sq, tree, rope, positions)
    _lib.require_gpu(q, cache.k4)
    dev, st = q.device, _lib.stream_of(q)
    # from fresh pageable host tensors, as PagedKVFP4._upload: staged before the copies return
    if trees is not None:   # one upload: the two tables, then the words (at a multiple of 16 bytes)
        flat = torch.tensor(list(itertools.chain.from_iterable(seq_rec + work)), dtype=torch.int32)
        rec_d = torch.cat([flat, trees[1]]).to(dev, non_blocking=True)
        work_d = rec_d[8 * len(seq_rec):]
        tree_d = work_d[4 * len(work):].view(torch.int64)
    elif shared is None:
        rec_d = torch.tensor(seq_rec, dtype=torch.int32).to(dev, non_blocking=True)
        work_d = torch.tensor(work, dtype=torch.int32).to(dev, non_blocking=True)
    else:   # one upload of the four tables, the longest records first
        flat = list(itertools.chain.from_iterable(seq_rec + work + grp_rec + members))
        rec_d = torch.tensor(flat, dtype=torch.int32).to(dev, non_blocking=True)
        work_d = rec_d[8 * len(seq_rec):]
        grp_d = work_d[4 * len(work):]
    q4, qs = mxfp4_quantize_rows(q) if rope is None else mxfp4_quantize_rows_rope(q, rope, pos)
    O = torch.empty((T, Hq, D), dtype=torch.float16, device=dev)
    lse = torch.empty((T, Hq), dtype=torch.float32, device=dev)
    opart = torch.empty((part_rows, D), dtype=torch.float32, device=dev)
    ml = torch.empty((part_rows, 2), dtype=torch.float32, device=dev)
    args = (_lib.ptr(q4), _lib.ptr(qs), _lib.ptr(cache.k4),
            _lib.ptr(cache.ks), _lib.ptr(cache.vt), _lib.ptr(cache.vs), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d), _lib.ptr(work_d), len(ids),
            len(work), T, part_rows, cache.alloc.max_seqs, Hkv, Hq // Hkv, cache.num_pages,
            cache.page_tokens, cache.alloc.max_pages_per_seq, 2 if causal else 0, kps, D, _qk_scale(D))
    if shared is not None:
        _lib.call("qattn_mxfp4_attn_fwd_varlen_paged_shared", *args, _lib.ptr(grp_d),
                  _lib.ptr(grp_d[4 * len(grp_rec):]), len(grp_rec), len(members), st)
    elif trees is not None:
        _lib.call("qattn_mxfp4_attn_fwd_varlen_paged_tree", *args, _lib.ptr(tree_d), st)
    elif W is None:
        _lib.call("qattn_mxfp4_attn_fwd_varlen_paged", *args, st)
    else:   # no sequence holds 2^25 keys or more: a larger window or sink count means the same
        _lib.call("qattn_mxfp4_attn_fwd_varlen_paged_window", *args, min(W, 1 << 26), min(S, 1 << 26), st)
    _lib.call("qattn_mxfp4_varlen_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(O), _lib.ptr(lse),
              _lib.ptr(rec_d), len(ids), T, Hq, Hkv, part_rows, D, st)
    return O, lse


# ------------------------------------------------------------------------------ device-planned decode step
def _step_plan(L1: int, kps: int, W, S: int):
    """(ns, wt0, nst) of one query over ``L1`` >= 1 keys at ``kps`` keys per split under window ``(W, S)`` (W
    None: no window): :func:`plan_varlen`'s expressions at q_len 1."""
    wt0, nst, nt = (0, 0, -(-L1 // BLOCK)) if W is None else _window_tiles(L1, 1, W, S)
    return (1 if nst else 0) + -(-(nt - wt0) * BLOCK // kps), wt0, nst


def _step_split_order(splits: int, W, S: int) -> list:
    """The order of the splits in a step's ``work`` table (results do not depend on it): ascending, except that
    under a window with sinks split 0 comes last.  With a gap it is the short sink run, and the host plan starts
    the longest workgroups first; measured on the 64-decode window case of DESIGN.md section 5."""
    return list(range(splits)) if W is None or not S or splits < 2 else list(range(1, splits)) + [0]


def decode_step_splits(max_keys: int, kps: int, window: Optional[int] = None, sinks: int = 0) -> int:
    """The largest number of key splits one query needs over any length in [1, ``max_keys``] at ``kps`` keys per
    split under ``(window, sinks)``: the ``splits`` of a :class:`DecodeStep`, whose grid is sized for it.  Pure
    Python.  Without a window it is ceil(ceil64(max_keys) / kps).  With one it does not grow with ``max_keys``:
    while the sink tiles and the window's first tile touch, the sequence is shorter than W + 64 * (ceil(S / 64)
    + 1) keys and runs every tile; beyond that (a gap) the window run holds at most ceil(W / 64) + 1 tiles
    whatever the length, so the count is at most 1 + the splits of the W-key run and repeats with period 64."""
    W, S = _window_args(window, sinks)
    max_keys, kps = int(max_keys), int(kps)
    if max_keys < 1 or kps < BLOCK or kps % BLOCK:
        raise _lib.QAttnError("qattn mxfp4 decode step: max_keys >= 1 and keys_per_split a multiple of 64 expected")
    if W is None:
        return _step_plan(max_keys, kps, None, 0)[0]
    gap = W + BLOCK * (-(-S // BLOCK) + 1)   # the first length with a gap; every longer one has it too
    best = _step_plan(min(max_keys, gap - 1), kps, W, S)[0]   # no gap: the count grows with the length
    return max([best] + [_step_plan(L1, kps, W, S)[0] for L1 in range(gap, min(max_keys, gap + BLOCK - 1) + 1)])


def plan_decode_step(lengths_before, slots, kps: int, splits: int, kv_heads: int, group: int,
                     window: Optional[int] = None, sinks: int = 0, capacity: Optional[int] = None):
    """The tables of one device-planned decode step -> (seq_tab, tiles, pos, seq_rec, work) as lists: the pure-
    Python statement of what ``qattn_mxfp4_decode_step_plan`` writes (and of ``work``, which a :class:`DecodeStep`
    writes once when it is made).  No device.  ``lengths_before`` holds one length per slot BEFORE the step's
    append and ``slots`` one slot per entry of the step, any value outside [0, len(lengths_before)) marking
    padding.  For entry i with b = slots[i] and L = lengths_before[b]:

        seq_tab[i] = [b, 1, i, 0]          the record of ``append_packed``: packed token i goes to slot b
        tiles[i]   = [i, L // 64]          the V tile that append touches
        pos[i]     = L                     the rotary position of the new key and of the query
        seq_rec[i] = [b, i, 1, ns, i * splits * kv_heads * group, wt0, nst, 0]

    with ns, wt0 and nst those of :func:`plan_varlen` for one sequence of L + 1 keys and one query at ``kps``
    under ``(window, sinks)`` (ns held to ``splits``, which :func:`decode_step_splits` makes large enough).  A
    padding entry -- b out of range, or L outside [0, ``capacity``) -- is seq_tab [-1, 0, i, 0], tiles [-1, 0],
    pos 0 and seq_rec [-1, i, 1, 0, i * splits * kv_heads * group, 0, 0, 0]: the append skips it, no workgroup
    runs for it and the merge writes O = 0, lse = -inf.  ``work`` = [i, 0, s, 0] for every s < ``splits`` and
    every entry, split by split (under a window with sinks split 0 last: the sink run is the short one)."""
    W, S = _window_args(window, sinks)
    lengths = [int(x) for x in lengths_before]
    slots = [int(b) for b in slots]
    kps, splits, hq = int(kps), int(splits), int(kv_heads) * int(group)
    if kps < BLOCK or kps % BLOCK or splits < 1 or hq < 1:
        raise _lib.QAttnError("qattn mxfp4 decode step: keys_per_split must be a multiple of 64, splits, kv_heads "
                              "and group >= 1")
    seq_tab, tiles, pos, seq_rec = [], [], [], []
    for i, b in enumerate(slots):
        L = lengths[b] if 0 <= b < len(lengths) else -1
        if L < 0 or (capacity is not None and L >= capacity):
            seq_tab.append([-1, 0, i, 0])
            tiles.append([-1, 0])
            pos.append(0)
            seq_rec.append([-1, i, 1, 0, i * splits * hq, 0, 0, 0])
            continue
        ns, wt0, nst = _step_plan(L + 1, kps, W, S)
        seq_tab.append([b, 1, i, 0])
        tiles.append([i, L // BLOCK])
        pos.append(L)
        seq_rec.append([b, i, 1, min(ns, splits), i * splits * hq, wt0, nst, 0])
    work = [[i, 0, s, 0] for s in _step_split_order(splits, W, S) for i in range(len(slots))]
    return seq_tab, tiles, pos, seq_rec, work


class DecodeStep:
    """One decode step -- one new token for each of up to ``max_batch`` running sequences of a
    :class:`PagedKVFP4` -- whose launches depend on nothing the host computed from the lengths, so ``append`` and
    ``attend`` can be captured in a graph once and replayed while the sequences grow, leave and join.

    Everything is allocated here, once, and nothing at call time: ``slots`` i32 [N] (the listed slots, -1 for
    padding), the append table ``seq_tab`` i32 [N, 4] and tile list ``tiles`` i32 [N, 2], ``seq_rec`` i32 [N, 8],
    ``pos`` i32 [N], ``work`` i32 [N * splits, 4] (written here and never again), the quantised queries ``q4`` /
    ``qs``, the partials ``opart`` f32 [N * splits * Hq, 128] / ``ml``, and the results ``O`` f16 [N, Hq, 128] /
    ``lse`` f32 [N, Hq], which ``attend`` returns and the next ``attend`` overwrites.  ``kps`` is fixed here:
    ``keys_per_split``, or ``qattn_split_keys(kv_heads * N, 1, ceil64(max_keys), 64)``; ``splits`` =
    :func:`decode_step_splits`, so the attention grid is N * splits * kv_heads workgroups whatever the lengths
    are.  ``window`` / ``sinks`` as in :func:`attention_mxfp4_varlen_paged`; under a window ``splits`` does not
    grow with ``max_keys``.

    ``prepare`` is the host's part, before every step or replay: the checks, the pages, ``slots``.  ``append``
    derives the step's tables from the device lengths (``qattn_mxfp4_decode_step_plan``) and appends;
    ``attend`` quantises ``q`` and runs the fixed grid (``qattn_mxfp4_attn_fwd_decode_step``), whose surplus
    workgroups exit, and the merge (``qattn_mxfp4_decode_step_combine``).  Every listed entry gets, bit for bit,
    what ``append_packed(k, v, ids, [1] * n)`` followed by ``attention_mxfp4_varlen_paged(q, cache, ids, [1] * n,
    causal=True, keys_per_split=step.kps[, window, sinks][, rope])`` gives.  One step object serves any number of
    pools, layer after layer, on one stream: each pool's ``append`` rewrites the tables from that pool's own
    ``lens``."""

    def __init__(self, max_batch: int, max_keys: int, q_heads: int, kv_heads: int, device,
                 keys_per_split: Optional[int] = None, window: Optional[int] = None, sinks: int = 0):
        N, max_keys, Hq, Hkv, D = int(max_batch), int(max_keys), int(q_heads), int(kv_heads), 128
        self.window, self.sinks = _window_args(window, sinks)
        if N < 1 or Hkv < 1 or Hq < 1 or Hq % Hkv or not 1 <= max_keys <= 1 << 25:
            raise _lib.QAttnError("qattn mxfp4 decode step: max_batch >= 1, q_heads = G * kv_heads and max_keys in "
                                  "[1, 2^25] expected")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.QAttnError(f"qattn kernels run on the GPU only; got device {dev} "
                                  "(no CPU fallback by design)")
        if keys_per_split is None:
            kps = _lib.load().qattn_split_keys(Hkv * N, 1, _ceil64(max_keys), BLOCK)
        else:
            kps = int(keys_per_split)
        if kps < BLOCK or kps % BLOCK:
            raise _lib.QAttnError("qattn mxfp4 decode step: keys_per_split must be a multiple of 64")
        self.N, self.max_keys, self.q_heads, self.kv_heads, self.kps = N, max_keys, Hq, Hkv, kps
        self.splits = decode_step_splits(max_keys, kps, self.window, self.sinks)
        if self.splits > 65535 or N * self.splits * Hq >= 1 << 31:
            raise _lib.QAttnError("qattn mxfp4 decode step: more than 65535 splits or 2^31 partial rows; raise "
                                  "keys_per_split")
        z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.slots = torch.full((N,), -1, dtype=torch.int32, device=dev)
        self.seq_tab, self.tiles, self.seq_rec, self.pos = z(N, 4), z(N, 2), z(N, 8), z(N)
        self.work = torch.tensor([[i, 0, s, 0] for s in _step_split_order(self.splits, self.window, self.sinks)
                                  for i in range(N)], dtype=torch.int32).to(dev)
        rows = N * self.splits * Hq
        self.opart, self.ml = z(rows, D, dt=torch.float32), z(rows, 2, dt=torch.float32)
        self.q4, self.qs = z(N * Hq, D // 2, dt=torch.uint8), z(N * Hq, D // 32, dt=torch.uint8)
        self.O, self.lse = z(N, Hq, D, dt=torch.float16), z(N, Hq, dt=torch.float32)
        self.listed = []   # the slots of the last prepare

    def _pool(self, cache: "PagedKVFP4") -> None:
        if not isinstance(cache, PagedKVFP4):
            raise _lib.QAttnError("qattn mxfp4 kv cache: cache must be a PagedKVFP4")
        if cache.shape[1] != self.kv_heads or cache.k4.device != self.slots.device:
            raise _lib.QAttnError(f"qattn mxfp4 decode step: a pool of {self.kv_heads} key/value heads on "
                                  f"{self.slots.device} expected")
        if self.N > cache.alloc.max_seqs:
            raise _lib.QAttnError(f"qattn mxfp4 decode step: a step of {self.N} entries on a pool of "
                                  f"{cache.alloc.max_seqs} sequence slots")

    def prepare(self, cache: "PagedKVFP4", seq_ids) -> "DecodeStep":
        """The host's part of a step over the slots ``seq_ids`` of ``cache`` (at most N, distinct, none empty),
        before ``append`` / ``attend`` or a replay of their graph; not capturable.  Raises :class:`QAttnError`
        before anything changes for duplicate or out-of-range slots, more than N of them, a listed slot of length
        0, a sequence whose length + 1 would pass ``max_keys`` or what its table row can hold, and a trimmed page
        the step would read.  Then it reserves the pages the lengths + 1 need (all or nothing: out of pages
        raises with nothing changed), uploads the table if it grew and ``seq_ids``, padded with -1, into
        ``slots``, and adds 1 to the listed ``cache.lengths``.  It builds no plan and no per-tile list;
        stream-ordered, nothing read back."""
        self._pool(cache)
        ids = [int(b) for b in (seq_ids.tolist() if isinstance(seq_ids, torch.Tensor) else seq_ids)]
        a = cache.alloc
        if len(ids) > self.N or len(set(ids)) != len(ids) or any(not 0 <= b < a.max_seqs for b in ids):
            raise _lib.QAttnError(f"qattn mxfp4 decode step: seq_ids must be at most {self.N} distinct slots in "
                                  f"[0, {a.max_seqs}), got {ids}")
        Ls = [cache.lengths[b] for b in ids]
        if any(L < 1 for L in Ls):
            raise _lib.QAttnError("qattn mxfp4 decode step: every listed sequence needs at least one cached token "
                                  f"(slots {ids}, lengths {Ls})")
        cap = min(self.max_keys, a.max_pages_per_seq * a.page_tokens)
        if any(L + 1 > cap for L in Ls):
            raise _lib.QAttnError(f"qattn mxfp4 decode step: a sequence would pass {cap} keys (the step's max_keys "
                                  f"{self.max_keys}, the pool's {a.max_pages_per_seq} pages of {a.page_tokens}; "
                                  f"slots {ids}, lengths {Ls})")
        for b in ids:   # the lengths the step attends at; taken back if it is refused
            cache.lengths[b] += 1
        try:
            _check_trimmed(cache, ids, [1] * len(ids), self.window, self.sinks)
            grown = a.reserve([(b, cache.lengths[b]) for b in ids])
        except _lib.QAttnError:
            for b in ids:
                cache.lengths[b] -= 1
            raise
        if grown:
            cache.block_table.copy_(torch.tensor(a.table, dtype=torch.int32), non_blocking=True)
        self.slots.copy_(torch.tensor(ids + [-1] * (self.N - len(ids)), dtype=torch.int32), non_blocking=True)
        self.listed = ids
        return self

    def _rope(self, cache: "PagedKVFP4", rope) -> None:
        if not isinstance(rope, Rope):
            raise _lib.QAttnError("qattn mxfp4 rope: rope must be a Rope")
        hi = max((cache.lengths[b] - 1 for b in self.listed), default=0)
        if hi >= rope.max_pos:   # (the mirror after prepare: a check only, no launch depends on it)
            raise _lib.QAttnError(f"qattn mxfp4 rope: the step's positions reach {hi}, outside the table's "
                                  f"[0, {rope.max_pos})")

    def append(self, cache: "PagedKVFP4", k: torch.Tensor, v: torch.Tensor, rope: Optional[Rope] = None):
        """Append ``k, v`` fp16 [N, Hkv, 128], row i the new token of entry i (rows of padding entries are not
        read), to the sequences ``slots`` names; capturable.  One launch derives the tables from ``cache.lens``
        (``qattn_mxfp4_decode_step_plan``), then ``qattn_mxfp4_paged_append_packed`` (``_rope`` with ``rope``:
        the keys rotated to ``pos``, their lengths before the append) runs on them as it is."""
        self._pool(cache)
        N, H, D = self.N, self.kv_heads, 128
        if tuple(k.shape) != (N, H, D) or k.shape != v.shape:
            raise _lib.QAttnError(f"qattn mxfp4 decode step: k, v must be [{N}, {H}, 128]")
        if rope is not None:
            self._rope(cache, rope)
        _lib.require_gpu(k, v, cache.k4)
        k = _lib.kernel_input(k, torch.float16)
        v = _lib.kernel_input(v, torch.float16)
        a, st = cache.alloc, _lib.stream_of(k)
        _lib.call("qattn_mxfp4_decode_step_plan", _lib.ptr(self.slots), _lib.ptr(cache.lens), _lib.ptr(self.seq_tab),
                  _lib.ptr(self.tiles), _lib.ptr(self.seq_rec), _lib.ptr(self.pos), N, a.max_seqs,
                  a.max_pages_per_seq * a.page_tokens, H, self.q_heads // H, self.kps, self.splits,
                  self.window or 0, self.sinks, st)
        args = (_lib.ptr(k), _lib.ptr(v), _lib.ptr(cache.k_mean), _lib.ptr(cache.k4), _lib.ptr(cache.ks),
                _lib.ptr(cache.vt), _lib.ptr(cache.vs), _lib.ptr(cache.vtail), _lib.ptr(cache.lens),
                _lib.ptr(cache.block_table), _lib.ptr(self.seq_tab), _lib.ptr(self.tiles), N, N, N, a.max_seqs, H,
                a.num_pages, a.page_tokens, a.max_pages_per_seq, D)
        if rope is None:
            _lib.call("qattn_mxfp4_paged_append_packed", *args, st)
        else:
            _lib.call("qattn_mxfp4_paged_append_packed_rope", *args, _lib.ptr(rope.table), _lib.ptr(self.pos),
                      rope.max_pos, int(rope.interleaved), st)
        return self

    def attend(self, cache: "PagedKVFP4", q: torch.Tensor, rope: Optional[Rope] = None):
        """Attention of ``q`` fp16 [N, Hq, 128], row i the query of entry i's new token, over the sequences after
        this step's ``append`` -> (``O`` fp16 [N, Hq, 128], ``lse`` fp32 [N, Hq] base 2), the step's own buffers;
        capturable.  ``q`` is quantised (rotated to ``pos`` first with ``rope``), one attention launch runs the
        fixed grid and one merge follows; the rows of padding entries come back as O = 0, lse = -inf."""
        self._pool(cache)
        N, Hq, H, D = self.N, self.q_heads, self.kv_heads, 128
        if tuple(q.shape) != (N, Hq, D):
            raise _lib.QAttnError(f"qattn mxfp4 decode step: q must be [{N}, {Hq}, 128]")
        if rope is not None:
            self._rope(cache, rope)
        _lib.require_gpu(q, cache.k4)
        q = _lib.kernel_input(q, torch.float16)
        a, st = cache.alloc, _lib.stream_of(q)
        if rope is None:
            _lib.call("qattn_mxfp4_quant_rows", _lib.ptr(q), None, _lib.ptr(self.q4), _lib.ptr(self.qs), N * Hq, Hq,
                      D, st)
        else:
            _lib.call("qattn_mxfp4_quant_rows_rope", _lib.ptr(q), _lib.ptr(self.q4), _lib.ptr(self.qs),
                      _lib.ptr(rope.table), _lib.ptr(self.pos), N, Hq, rope.max_pos, int(rope.interleaved), D, st)
        _lib.call("qattn_mxfp4_attn_fwd_decode_step", _lib.ptr(self.q4), _lib.ptr(self.qs), _lib.ptr(cache.k4),
                  _lib.ptr(cache.ks), _lib.ptr(cache.vt), _lib.ptr(cache.vs), _lib.ptr(self.opart),
                  _lib.ptr(self.ml), _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(self.seq_rec),
                  _lib.ptr(self.work), N, self.splits, a.max_seqs, H, Hq // H, a.num_pages, a.page_tokens,
                  a.max_pages_per_seq, self.kps, D, _qk_scale(D), self.window or 0, self.sinks, st)
        _lib.call("qattn_mxfp4_decode_step_combine", _lib.ptr(self.opart), _lib.ptr(self.ml), _lib.ptr(self.O),
                  _lib.ptr(self.lse), _lib.ptr(self.seq_rec), N, self.splits, Hq, H, D, st)
        return self.O, self.lse


# ------------------------------------------------------------------------------ device-planned verify step
_WORD = (1 << 64) - 1


def _signed64(x: int) -> int:
    return x - (1 << 64) if x >> 63 else x


def verify_step_splits(max_keys: int, kps: int) -> int:
    """The largest number of key splits a sequence of at most ``max_keys`` keys (the K draft tokens included) needs
    at ``kps`` keys per split: the ``splits`` of a :class:`VerifyStep`, ceil(ceil64(max_keys) / kps).  Pure Python."""
    max_keys, kps = int(max_keys), int(kps)
    if max_keys < 1 or kps < BLOCK or kps % BLOCK:
        raise _lib.QAttnError("qattn mxfp4 verify step: max_keys >= 1 and keys_per_split a multiple of 64 expected")
    return -(-_ceil64(max_keys) // kps)


def plan_verify_step(lengths_before, slots, K: int, words, kps: int, splits: int, kv_heads: int, group: int,
                     capacity: Optional[int] = None):
    """The tables of one device-planned verify step -> (seq_tab, tiles, pos, seq_rec, work) as lists: the pure-
    Python statement of what ``qattn_mxfp4_verify_step_plan`` writes (and of ``work``, which a :class:`VerifyStep`
    writes once when it is made).  No device.  ``lengths_before`` holds one length per slot BEFORE the step's
    append, ``slots`` one slot per entry of the step, any value outside [0, len(lengths_before)) marking padding,
    and ``words`` the len(slots) * K ancestor words (:func:`tree_ancestor_masks`, entry by entry; as unsigned or
    as int64 values), each cleaned as the kernels clean it: ``(word & (self | (self - 1))) | self`` with ``self = 1
    << t``.  For entry i with b = slots[i] and L = lengths_before[b]:

        seq_tab[i]       = [b, K, i * K, 0]         the record of ``append_packed``
        tiles[2 i]       = [i, L // 64]             the V tiles the K tokens touch: at most two, as K <= 64;
        tiles[2 i + 1]   = [i, (L + K - 1) // 64]   when that is another tile, else [-1, 0], which the append skips
        pos[i * K + t]   = L + popcount(cleaned word) - 1, the node's depth behind the cached keys
        seq_rec[i]       = [b, i * K, K, ns, i * splits * kv_heads * group * K, 0, 0, K]

    with ns = min(ceil(ceil64(L + K) / kps), splits): :func:`plan_varlen`'s record for a sequence of L + K keys and
    K queries that are all tree nodes, but for the partial base, a fixed stride.  A padding entry -- b out of range,
    or L + K > ``capacity`` -- is seq_tab [-1, 0, i * K, 0], both tiles [-1, 0], pos 0 and seq_rec [-1, i * K, K, 0,
    base, 0, 0, K].  ``work`` = [i, row block, s, 0] for every entry, every row block < ceil(group * K / 128) and
    every s < ``splits``, split by split."""
    lengths = [int(x) for x in lengths_before]
    slots = [int(b) for b in slots]
    K, kps, splits, hq, group = int(K), int(kps), int(splits), int(kv_heads) * int(group), int(group)
    if not 1 <= K <= TREE_NODES or kps < BLOCK or kps % BLOCK or splits < 1 or hq < 1:
        raise _lib.QAttnError(f"qattn mxfp4 verify step: draft_tokens in [1, {TREE_NODES}], keys_per_split a "
                              "multiple of 64, splits, kv_heads and group >= 1 expected")
    words = [int(w) & _WORD for w in words]
    if len(words) != len(slots) * K:
        raise _lib.QAttnError(f"qattn mxfp4 verify step: {len(slots) * K} ancestor words expected, got {len(words)}")
    seq_tab, tiles, pos, seq_rec = [], [], [], []
    for i, b in enumerate(slots):
        L = lengths[b] if 0 <= b < len(lengths) else -1
        base = i * splits * hq * K
        if L < 0 or (capacity is not None and L + K > capacity):
            seq_tab.append([-1, 0, i * K, 0])
            tiles += [[-1, 0], [-1, 0]]
            pos += [0] * K
            seq_rec.append([-1, i * K, K, 0, base, 0, 0, K])
            continue
        g0, g1 = L // BLOCK, (L + K - 1) // BLOCK
        seq_tab.append([b, K, i * K, 0])
        tiles += [[i, g0], [i, g1] if g1 != g0 else [-1, 0]]
        for t in range(K):
            w = (words[i * K + t] & ((2 << t) - 1)) | 1 << t
            pos.append(L + bin(w).count("1") - 1)
        seq_rec.append([b, i * K, K, min(-(-_ceil64(L + K) // kps), splits), base, 0, 0, K])
    nrb = -(-group * K // QROWS)
    work = [[i, rb, s, 0] for s in range(splits) for rb in range(nrb) for i in range(len(slots))]
    return seq_tab, tiles, pos, seq_rec, work


class VerifyStep:
    """One verify step of speculative decoding -- ``draft_tokens`` = K new tokens (1 <= K <= 64), a chain or a
    draft tree, for each of up to ``max_batch`` running sequences of a :class:`PagedKVFP4` -- planned on the device
    like :class:`DecodeStep`, so ``append`` and ``attend`` can be captured in a graph once and replayed while the
    sequences grow, are rolled back, leave and join, and while the trees change.

    Everything is allocated here, once: ``slots`` i32 [N] and ``tree`` int64 [N * K] (the ancestor words; one
    buffer, one upload per ``prepare``), the append table ``seq_tab`` i32 [N, 4] and tile list ``tiles`` i32 [2 N,
    2], ``seq_rec`` i32 [N, 8], ``pos`` i32 [N * K], ``work`` i32 [N * nrb * splits, 4] with nrb = ceil(G K / 128)
    (written here and never again), the quantised queries ``q4`` / ``qs``, the partials ``opart`` f32 [N * splits *
    Hq * K, 128] / ``ml``, and the results ``O`` f16 [N * K, Hq, 128] / ``lse`` f32 [N * K, Hq], which ``attend``
    returns and the next ``attend`` overwrites.  ``parents`` (None: a chain of K nodes) is the default topology, a
    ``parents`` list of exactly K nodes (:func:`tree_ancestor_masks`).  ``kps`` is fixed here: ``keys_per_split``,
    or ``qattn_split_keys(kv_heads * N * nrb, 1, ceil64(max_keys), 64)``; ``splits`` = :func:`verify_step_splits`,
    so the attention grid is N * nrb * splits * kv_heads workgroups whatever the lengths are.  ``max_keys`` bounds
    a sequence's length AFTER the K tokens.

    A round: ``ckpt = cache.checkpoint(ids)`` BEFORE ``prepare`` (``prepare`` moves the mirror lengths to L + K,
    and a checkpoint notes the mirror), then ``prepare``, then ``append`` and ``attend`` or the replay of their
    graph, then ``cache.rollback(ckpt)`` or ``cache.accept(ckpt, k[:n * K], v[:n * K], ids, [K] * n, accepted)`` as
    on the host-planned path.  Every listed entry gets, bit for bit, what ``append_packed(k, v, ids, [K] * n[,
    rope=rope, tree=trees])`` followed by ``attention_mxfp4_varlen_paged(q, cache, ids, [K] * n, causal=True,
    keys_per_split=step.kps, tree=trees[, rope=rope])`` gives, and the pool holds that pair's bytes.  No window
    and no ``share_prefix`` (a tree excludes both), one K for every entry; page reservation stays on the host."""

    def __init__(self, max_batch: int, max_keys: int, q_heads: int, kv_heads: int, device, draft_tokens: int,
                 parents=None, keys_per_split: Optional[int] = None):
        N, max_keys, Hq, Hkv, K, D = int(max_batch), int(max_keys), int(q_heads), int(kv_heads), int(draft_tokens), 128
        if N < 1 or Hkv < 1 or Hq < 1 or Hq % Hkv or not 1 <= max_keys <= 1 << 25:
            raise _lib.QAttnError("qattn mxfp4 verify step: max_batch >= 1, q_heads = G * kv_heads and max_keys in "
                                  "[1, 2^25] expected")
        if not 1 <= K <= TREE_NODES:
            raise _lib.QAttnError(f"qattn mxfp4 verify step: draft_tokens must be in [1, {TREE_NODES}] (one bit of "
                                  f"the ancestor word each), got {K}")
        self.K = K
        self.words, self.depth = self._tree(list(range(-1, K - 1)) if parents is None else parents)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.QAttnError(f"qattn kernels run on the GPU only; got device {dev} "
                                  "(no CPU fallback by design)")
        self.nrb = -(-(Hq // Hkv) * K // QROWS)
        if keys_per_split is None:
            kps = _lib.load().qattn_split_keys(Hkv * N * self.nrb, 1, _ceil64(max_keys), BLOCK)
        else:
            kps = int(keys_per_split)
        if kps < BLOCK or kps % BLOCK:
            raise _lib.QAttnError("qattn mxfp4 verify step: keys_per_split must be a multiple of 64")
        self.N, self.max_keys, self.q_heads, self.kv_heads, self.kps = N, max_keys, Hq, Hkv, kps
        self.splits = verify_step_splits(max_keys, kps)
        if self.splits > 65535 or N * self.splits * Hq * K >= 1 << 31:
            raise _lib.QAttnError("qattn mxfp4 verify step: more than 65535 splits or 2^31 partial rows; raise "
                                  "keys_per_split")
        z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        # one buffer for what prepare uploads: the words first, then, at a multiple of 16 bytes, the slots
        self._gap = -(2 * N * K) % 4
        self.args = z(2 * N * K + self._gap + N)
        self.tree, self.slots = self.args[:2 * N * K].view(torch.int64), self.args[2 * N * K + self._gap:]
        self.slots.fill_(-1)
        self.seq_tab, self.tiles, self.seq_rec, self.pos = z(N, 4), z(2 * N, 2), z(N, 8), z(N * K)
        self.work = torch.tensor([[i, rb, s, 0] for s in range(self.splits) for rb in range(self.nrb)
                                  for i in range(N)], dtype=torch.int32).to(dev)
        rows = N * self.splits * Hq * K
        self.opart, self.ml = z(rows, D, dt=torch.float32), z(rows, 2, dt=torch.float32)
        self.q4, self.qs = z(N * K * Hq, D // 2, dt=torch.uint8), z(N * K * Hq, D // 32, dt=torch.uint8)
        self.O, self.lse = z(N * K, Hq, D, dt=torch.float16), z(N * K, Hq, dt=torch.float32)
        self.listed = []    # the slots of the last prepare
        self.top = 0        # the highest rotary position of the last prepare

    def _tree(self, parents):
        """(int64 words, depth of the deepest node) of a ``parents`` list of exactly K nodes."""
        anc = tree_ancestor_masks(parents)
        if len(anc) != self.K:
            raise _lib.QAttnError(f"qattn mxfp4 verify step: a tree of {len(anc)} nodes on a step of {self.K} draft "
                                  "tokens (every entry's tree has exactly draft_tokens nodes)")
        return [_signed64(x) for x in anc], max(bin(x).count("1") for x in anc) - 1

    def _pool(self, cache: "PagedKVFP4") -> None:
        if not isinstance(cache, PagedKVFP4):
            raise _lib.QAttnError("qattn mxfp4 kv cache: cache must be a PagedKVFP4")
        if cache.shape[1] != self.kv_heads or cache.k4.device != self.slots.device:
            raise _lib.QAttnError(f"qattn mxfp4 verify step: a pool of {self.kv_heads} key/value heads on "
                                  f"{self.slots.device} expected")
        if self.N > cache.alloc.max_seqs:
            raise _lib.QAttnError(f"qattn mxfp4 verify step: a step of {self.N} entries on a pool of "
                                  f"{cache.alloc.max_seqs} sequence slots")

    def prepare(self, cache: "PagedKVFP4", seq_ids, trees=None) -> "VerifyStep":
        """The host's part of a step over the slots ``seq_ids`` of ``cache`` (at most N, distinct, none empty),
        before ``append`` / ``attend`` or a replay of their graph; not capturable.  ``trees`` (None: the step's
        default topology for every entry) lists one entry per listed sequence, None or a ``parents`` list of
        exactly K nodes.  Raises :class:`QAttnError` before anything changes for duplicate or out-of-range slots,
        more than N of them, a listed slot of length 0, a sequence whose length + K would pass ``max_keys`` or
        what its table row can hold, a trimmed sequence (there is no window), a ``trees`` list of another length,
        a tree that does not have K nodes or has a parent outside [-1, t).  Then it reserves the pages the lengths
        + K need (all or nothing: out of pages raises with nothing changed), uploads the table if it grew, and
        ``seq_ids``, padded with -1, together with the words of all N * K tokens in one upload, and adds K to the
        listed ``cache.lengths``.  Stream-ordered, nothing read back."""
        self._pool(cache)
        ids = [int(b) for b in (seq_ids.tolist() if isinstance(seq_ids, torch.Tensor) else seq_ids)]
        a, K = cache.alloc, self.K
        if len(ids) > self.N or len(set(ids)) != len(ids) or any(not 0 <= b < a.max_seqs for b in ids):
            raise _lib.QAttnError(f"qattn mxfp4 verify step: seq_ids must be at most {self.N} distinct slots in "
                                  f"[0, {a.max_seqs}), got {ids}")
        trees = [None] * len(ids) if trees is None else list(trees)
        if len(trees) != len(ids):
            raise _lib.QAttnError(f"qattn mxfp4 verify step: trees must have one entry (None or a parents list) "
                                  f"per listed sequence, got {len(trees)} for {len(ids)}")
        seen, per = {}, []   # a batch usually drafts one tree shape: one look-up per sequence
        for p in trees:
            w = (self.words, self.depth) if p is None else seen.get(id(p))
            if w is None:
                w = seen[id(p)] = self._tree(p)
            per.append(w)
        Ls = [cache.lengths[b] for b in ids]
        if any(L < 1 for L in Ls):
            raise _lib.QAttnError("qattn mxfp4 verify step: every listed sequence needs at least one cached token "
                                  f"(slots {ids}, lengths {Ls})")
        cap = min(self.max_keys, a.max_pages_per_seq * a.page_tokens)
        if any(L + K > cap for L in Ls):
            raise _lib.QAttnError(f"qattn mxfp4 verify step: a sequence would pass {cap} keys with its {K} draft "
                                  f"tokens (the step's max_keys {self.max_keys}, the pool's {a.max_pages_per_seq} "
                                  f"pages of {a.page_tokens}; slots {ids}, lengths {Ls})")
        for b in ids:
            cache._whole(b, "a verify step (it has no window)")
        grown = a.reserve([(b, L + K) for b, L in zip(ids, Ls)])
        if grown:
            cache.block_table.copy_(torch.tensor(a.table, dtype=torch.int32), non_blocking=True)
        words = list(itertools.chain.from_iterable(w for w, _ in per)) + [0] * (K * (self.N - len(ids)))
        host = torch.cat([torch.tensor(words, dtype=torch.int64).view(torch.int32),
                          torch.tensor([0] * self._gap + ids + [-1] * (self.N - len(ids)), dtype=torch.int32)])
        self.args.copy_(host, non_blocking=True)
        for b in ids:
            cache.lengths[b] += K
        self.listed = ids
        self.top = max((L + d for L, (_, d) in zip(Ls, per)), default=0)
        return self

    def _rope(self, rope) -> None:
        if not isinstance(rope, Rope):
            raise _lib.QAttnError("qattn mxfp4 rope: rope must be a Rope")
        if self.top >= rope.max_pos:   # (from the mirror at prepare: a check only, no launch depends on it)
            raise _lib.QAttnError(f"qattn mxfp4 rope: the step's positions reach {self.top}, outside the table's "
                                  f"[0, {rope.max_pos})")

    def append(self, cache: "PagedKVFP4", k: torch.Tensor, v: torch.Tensor, rope: Optional[Rope] = None):
        """Append ``k, v`` fp16 [N * K, Hkv, 128], rows i * K .. i * K + K - 1 the draft tokens of entry i in
        topological order (rows of padding entries are not read), to the sequences ``slots`` names; capturable.
        One launch derives the tables from ``cache.lens`` and ``tree`` (``qattn_mxfp4_verify_step_plan``), then
        ``qattn_mxfp4_paged_append_packed`` (``_rope`` with ``rope``: the keys rotated to ``pos``, the nodes'
        depths behind the cached keys) runs on them as it is."""
        self._pool(cache)
        N, K, H, D = self.N, self.K, self.kv_heads, 128
        if tuple(k.shape) != (N * K, H, D) or k.shape != v.shape:
            raise _lib.QAttnError(f"qattn mxfp4 verify step: k, v must be [{N * K}, {H}, 128]")
        if rope is not None:
            self._rope(rope)
        _lib.require_gpu(k, v, cache.k4)
        k = _lib.kernel_input(k, torch.float16)
        v = _lib.kernel_input(v, torch.float16)
        a, st = cache.alloc, _lib.stream_of(k)
        _lib.call("qattn_mxfp4_verify_step_plan", _lib.ptr(self.slots), _lib.ptr(cache.lens), _lib.ptr(self.tree),
                  _lib.ptr(self.seq_tab), _lib.ptr(self.tiles), _lib.ptr(self.seq_rec), _lib.ptr(self.pos), N, K,
                  a.max_seqs, a.max_pages_per_seq * a.page_tokens, H, self.q_heads // H, self.kps, self.splits, st)
        args = (_lib.ptr(k), _lib.ptr(v), _lib.ptr(cache.k_mean), _lib.ptr(cache.k4), _lib.ptr(cache.ks),
                _lib.ptr(cache.vt), _lib.ptr(cache.vs), _lib.ptr(cache.vtail), _lib.ptr(cache.lens),
                _lib.ptr(cache.block_table), _lib.ptr(self.seq_tab), _lib.ptr(self.tiles), N, 2 * N, N * K,
                a.max_seqs, H, a.num_pages, a.page_tokens, a.max_pages_per_seq, D)
        if rope is None:
            _lib.call("qattn_mxfp4_paged_append_packed", *args, st)
        else:
            _lib.call("qattn_mxfp4_paged_append_packed_rope", *args, _lib.ptr(rope.table), _lib.ptr(self.pos),
                      rope.max_pos, int(rope.interleaved), st)
        return self

    def attend(self, cache: "PagedKVFP4", q: torch.Tensor, rope: Optional[Rope] = None):
        """Attention of ``q`` fp16 [N * K, Hq, 128], row i * K + t the query of entry i's draft node t, over the
        sequences after this step's ``append``, node t seeing the cached keys, its ancestors and itself ->
        (``O`` fp16 [N * K, Hq, 128], ``lse`` fp32 [N * K, Hq] base 2), the step's own buffers; capturable.  ``q``
        is quantised (rotated to ``pos`` first with ``rope``), one attention launch runs the fixed grid
        (``qattn_mxfp4_attn_fwd_verify_step``) and one merge follows (``qattn_mxfp4_verify_step_combine``); the
        rows of padding entries come back as O = 0, lse = -inf."""
        self._pool(cache)
        N, K, Hq, H, D = self.N, self.K, self.q_heads, self.kv_heads, 128
        if tuple(q.shape) != (N * K, Hq, D):
            raise _lib.QAttnError(f"qattn mxfp4 verify step: q must be [{N * K}, {Hq}, 128]")
        if rope is not None:
            self._rope(rope)
        _lib.require_gpu(q, cache.k4)
        q = _lib.kernel_input(q, torch.float16)
        a, st = cache.alloc, _lib.stream_of(q)
        if rope is None:
            _lib.call("qattn_mxfp4_quant_rows", _lib.ptr(q), None, _lib.ptr(self.q4), _lib.ptr(self.qs), N * K * Hq,
                      Hq, D, st)
        else:
            _lib.call("qattn_mxfp4_quant_rows_rope", _lib.ptr(q), _lib.ptr(self.q4), _lib.ptr(self.qs),
                      _lib.ptr(rope.table), _lib.ptr(self.pos), N * K, Hq, rope.max_pos, int(rope.interleaved), D,
                      st)
        _lib.call("qattn_mxfp4_attn_fwd_verify_step", _lib.ptr(self.q4), _lib.ptr(self.qs), _lib.ptr(cache.k4),
                  _lib.ptr(cache.ks), _lib.ptr(cache.vt), _lib.ptr(cache.vs), _lib.ptr(self.opart),
                  _lib.ptr(self.ml), _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(self.seq_rec),
                  _lib.ptr(self.work), _lib.ptr(self.tree), N, K, self.splits, a.max_seqs, H, Hq // H, a.num_pages,
                  a.page_tokens, a.max_pages_per_seq, self.kps, D, _qk_scale(D), st)
        _lib.call("qattn_mxfp4_verify_step_combine", _lib.ptr(self.opart), _lib.ptr(self.ml), _lib.ptr(self.O),
                  _lib.ptr(self.lse), _lib.ptr(self.seq_rec), N, K, self.splits, Hq, H, D, st)
        return self.O, self.lse
