"""What the packed C entries of the paged MX-FP4 cache refuse, at head_dim 64, 128 and 256 alike.

One table of argument sets for the packed step (plain, windowed, capped), the decode step (plain, capped), the
packed append (plain, rope), the rope quantiser and the four merges.  Every case ends in the entry's argument
checks: a refused set returns 1, an empty call (no sequence, work record, token or entry) returns 0, and nothing
is launched, so the pointers are never read (a made-up non-null address stands for every operand).  The three
widths go through one host path (mxfp4_attn.h); this holds their refusal sets equal."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p(4096)   # a non-null operand that no case reads
BIG = 1 << 31

POOL = dict(num_pages=8, page_tokens=64, max_pages_per_seq=4)
OPERANDS = ("q4", "qscale", "k4", "kscale", "vt", "vscale", "opart", "ml", "lens", "block_table", "seq_rec", "work")
PACKED = OPERANDS + ("nseq", "nwork", "tokens", "part_rows", "max_seqs", "kv_heads", "group", "num_pages",
                     "page_tokens", "max_pages_per_seq", "causal", "keys_per_split", "head_dim", "qks")
PACKED_OK = dict(nseq=2, nwork=4, tokens=8, part_rows=64, max_seqs=4, kv_heads=2, group=2, causal=2,
                 keys_per_split=128, qks=0.1, **POOL)
STEP = OPERANDS + ("n", "splits", "max_seqs", "kv_heads", "group", "num_pages", "page_tokens",
                   "max_pages_per_seq", "keys_per_split", "head_dim", "qks", "window", "sinks")
STEP_OK = dict(n=2, splits=2, max_seqs=4, kv_heads=2, group=2, keys_per_split=128, qks=0.1, window=0, sinks=0,
               **POOL)
APPEND = ("k", "v", "k_mean", "k4", "kscale", "vt", "vscale", "vtail", "lens", "block_table", "seq_tab", "tiles",
          "nseq", "ntiles", "tokens", "max_seqs", "kv_heads", "num_pages", "page_tokens", "max_pages_per_seq",
          "head_dim")
APPEND_OK = dict(nseq=2, ntiles=2, tokens=8, max_seqs=4, kv_heads=2, **POOL)
ROPE_OK = dict(max_pos=16, interleaved=0)
QUANT = ("x", "q4", "scale", "cos_sin", "pos", "tokens", "heads", "max_pos", "interleaved", "head_dim")
MERGE = ("opart", "ml", "out", "lse", "seq_rec")
VARLEN_MERGE_OK = dict(nseq=2, tokens=8, q_heads=4, kv_heads=2, part_rows=64)
STEP_MERGE_OK = dict(n=2, splits=2, q_heads=4, kv_heads=2)

# entry -> (argument names in order, without the stream; a set of arguments the entry accepts)
ENTRIES = {
    "attn_fwd_varlen_paged": (PACKED, PACKED_OK),
    "attn_fwd_varlen_paged_window": (PACKED + ("window", "sinks"), dict(PACKED_OK, window=16, sinks=0)),
    "attn_fwd_varlen_paged_softcap": (PACKED + ("window", "sinks", "softcap"),
                                      dict(PACKED_OK, window=16, sinks=0, softcap=30.0)),
    "attn_fwd_decode_step": (STEP, STEP_OK),
    "attn_fwd_decode_step_softcap": (STEP + ("softcap",), dict(STEP_OK, softcap=30.0)),
    "paged_append_packed": (APPEND, APPEND_OK),
    "paged_append_packed_rope": (APPEND + ("cos_sin", "pos", "max_pos", "interleaved"), dict(APPEND_OK, **ROPE_OK)),
    "quant_rows_rope": (QUANT, dict(tokens=8, heads=4, **ROPE_OK)),
    "varlen_combine": (MERGE + ("nseq", "tokens", "q_heads", "kv_heads", "part_rows", "head_dim"), VARLEN_MERGE_OK),
    "varlen_combine_sink": (MERGE + ("sink_logit", "nseq", "tokens", "q_heads", "kv_heads", "part_rows", "head_dim"),
                            VARLEN_MERGE_OK),
    "decode_step_combine": (MERGE + ("n", "splits", "q_heads", "kv_heads", "head_dim"), STEP_MERGE_OK),
    "decode_step_combine_sink": (MERGE + ("sink_logit", "n", "splits", "q_heads", "kv_heads", "head_dim"),
                                 STEP_MERGE_OK),
}

# (what is wrong, the arguments that make it so, the status); a case goes to every entry that has all its arguments
TABLE = [
    ("null lens", dict(lens=None), 1),
    ("null block_table", dict(block_table=None), 1),
    ("null seq_rec", dict(seq_rec=None), 1),
    ("null work", dict(work=None), 1),
    ("null seq_tab", dict(seq_tab=None), 1),
    ("null tiles", dict(tiles=None), 1),
    ("null cos_sin", dict(cos_sin=None), 1),
    ("null pos", dict(pos=None), 1),
    ("null x", dict(x=None), 1),
    ("null sink_logit", dict(sink_logit=None), 1),
    ("keys_per_split 0", dict(keys_per_split=0), 1),
    ("keys_per_split 96", dict(keys_per_split=96), 1),
    ("page_tokens 96", dict(page_tokens=96), 1),
    ("nseq > max_seqs", dict(nseq=5, max_seqs=4), 1),
    ("n > max_seqs", dict(n=5, max_seqs=4), 1),
    ("nseq > tokens", dict(nseq=3, tokens=2), 1),
    ("causal 1", dict(causal=1), 1),
    ("a window with causal 0", dict(window=16, causal=0), 1),
    ("q_heads % kv_heads", dict(q_heads=5), 1),
    ("tokens x heads past 2^31", dict(tokens=BIG), 1),
    ("part_rows past 2^31", dict(part_rows=BIG), 1),
    ("n x splits x heads past 2^31", dict(n=BIG), 1),
    ("ntiles x kv_heads past 2^31", dict(ntiles=BIG, kv_heads=8), 1),
    ("splits 0", dict(splits=0), 1),
    ("max_pos 0", dict(max_pos=0), 1),
    ("interleaved 2", dict(interleaved=2), 1),
    ("head_dim 32", dict(head_dim=32), 1),
    ("no sequence", dict(nseq=0), 0),
    ("no work record", dict(nwork=0), 0),
    ("no token", dict(tokens=0), 0),
    ("no head", dict(heads=0), 0),
    ("no entry", dict(n=0), 0),
]


def cases():
    for entry, (names, ok) in ENTRIES.items():
        for what, bad, status in TABLE:
            if all(k in names for k in bad):
                yield entry, what, bad, status


def status_of(lib, entry, head_dim, bad):
    names, ok = ENTRIES[entry]
    values = dict({n: P for n in names}, **ok, head_dim=head_dim)
    values.update(bad)
    return getattr(lib, "qattn_mxfp4_" + entry)(*[values[n] for n in names], None)


@pytest.fixture(scope="module")
def lib():
    from quantizedattention_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("head_dim", [64, 128, 256])
def test_the_table(lib, head_dim):
    wrong = [(entry, what, got, want) for entry, what, bad, want in cases()
             if (got := status_of(lib, entry, head_dim, bad)) != want]
    assert not wrong, wrong


def test_the_table_reaches_every_entry_and_line():
    assert {entry for entry, *_ in cases()} == set(ENTRIES)
    assert {what for _, what, *_ in cases()} == {what for what, *_ in TABLE}
