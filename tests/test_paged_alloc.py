"""The host side of the paged MX-FP4 cache (kv_cache_mxfp4.PageAllocator), which holds no tensors and
needs no GPU, and the fake kernel of torch.ops.qattn.mxfp4_decode_paged."""
import copy

import pytest
import torch

from quantizedattention_amd._lib import QAttnError
from quantizedattention_amd.kv_cache_mxfp4 import PageAllocator


def _state(a):
    return copy.deepcopy((a._free, a.refcount, a.pages, a.table))


def _mirror_ok(a):
    for b, pages in enumerate(a.pages):
        assert a.table[b][:len(pages)] == pages, b
    owned = [p for pages in a.pages for p in pages]
    for p in range(a.num_pages):
        assert a.refcount[p] == owned.count(p), p
    assert sorted(a._free) == [p for p in range(a.num_pages) if a.refcount[p] == 0]
    assert a.free_pages == len(a._free)


def test_free_order_is_honoured_and_the_table_mirrors_the_page_lists():
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    a = PageAllocator(8, 64, 3, 4, free_order=order)
    assert a.free_pages == 8 and a.pages == [[], [], []]
    assert a.reserve([(0, 1), (2, 130)]) == [0, 2]      # 1 page and 3 pages
    assert a.pages == [[5], [], [2, 7, 0]] and a.free_pages == 4
    assert a.reserve([(0, 64), (2, 192)]) == []         # both still fit their pages
    assert a.reserve([(0, 65)]) == [0] and a.pages[0] == [5, 3]
    _mirror_ok(a)
    assert PageAllocator(4, 128, 1, 4).reserve([(0, 300)]) == [0]     # default: ascending
    assert PageAllocator(4, 128, 1, 4).pages_for(300) == 3
    for bad in ([0, 1, 2], [0, 1, 2, 2], [0, 1, 2, 4]):
        with pytest.raises(QAttnError, match="free_order"):
            PageAllocator(4, 64, 1, 4, free_order=bad)
    for p in (0, 32, 96, 2048):
        with pytest.raises(QAttnError, match="page_tokens"):
            PageAllocator(4, p, 1, 4)


def test_reservation_is_all_or_nothing():
    a = PageAllocator(4, 64, 3, 3)
    a.reserve([(0, 64), (1, 100)])                       # 1 + 2 pages, 1 free
    before = _state(a)
    with pytest.raises(QAttnError, match="pages"):       # the pool: 0 could grow alone, 2 cannot as well
        a.reserve([(0, 128), (2, 64)])
    assert _state(a) == before
    with pytest.raises(QAttnError, match="max_pages_per_seq"):   # 1 would need a fourth page
        a.reserve([(0, 128), (1, 193)])
    assert _state(a) == before
    with pytest.raises(QAttnError, match="sequence"):
        a.reserve([(0, 128), (3, 1)])
    assert _state(a) == before
    assert a.reserve([(0, 128)]) == [0] and a.free_pages == 0
    _mirror_ok(a)


def test_a_freed_page_is_handed_out_again():
    a = PageAllocator(3, 64, 2, 3, free_order=[2, 0, 1])
    a.reserve([(0, 128)])
    assert a.pages[0] == [2, 0] and a.free_pages == 1
    a.release(0)
    assert a.pages[0] == [] and a.free_pages == 3 and a.refcount == [0, 0, 0]
    a.reserve([(1, 192)])
    assert sorted(a.pages[1]) == [0, 1, 2] and a.pages[1][0] in (2, 0)   # a returned page first
    _mirror_ok(a)
    with pytest.raises(QAttnError, match="out of pages"):
        a.reserve([(0, 1)])


@pytest.mark.parametrize("first", ["src", "dst"])
def test_reference_counts_through_share_and_release(first):
    a = PageAllocator(6, 64, 3, 4)
    a.reserve([(0, 150)])                                # pages 0, 1, 2; the last one partial
    fresh = a.share(0, 1, 2, 1)                          # what fork does at L = 150
    assert a.pages[1][:2] == a.pages[0][:2] and a.pages[1][2:] == fresh and len(fresh) == 1
    assert fresh[0] not in a.pages[0]
    assert [a.refcount[p] for p in a.pages[0]] == [2, 2, 1] and a.refcount[fresh[0]] == 1
    assert a.free_pages == 2
    _mirror_ok(a)
    before = _state(a)
    with pytest.raises(QAttnError, match="not empty"):
        a.share(0, 1, 2, 1)
    with pytest.raises(QAttnError, match="pages"):       # 3 fresh pages, 2 free
        a.share(0, 2, 1, 3)
    with pytest.raises(QAttnError, match="pages"):       # 5 pages in a row of 4
        a.share(0, 2, 3, 2)
    assert _state(a) == before
    shared = a.pages[0][:2]
    a.release(0 if first == "src" else 1)
    assert [a.refcount[p] for p in shared] == [1, 1] and a.free_pages == 3   # only the unshared page returns
    _mirror_ok(a)
    a.release(1 if first == "src" else 0)
    assert a.free_pages == 6 and a.refcount == [0] * 6
    _mirror_ok(a)


def test_decode_paged_fake_kernel():
    """Shapes and dtypes of the operator under FakeTensorMode, beside test_ops.test_fake_shapes."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    import quantizedattention_amd.ops  # noqa: F401  (registers torch.ops.qattn.*)
    assert hasattr(torch.ops.qattn, "mxfp4_decode_paged")
    op = torch.ops.qattn.mxfp4_decode_paged.default
    assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU")
    with FakeTensorMode():
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")  # noqa: E731
        q = torch.empty((3, 8, 5, 128), dtype=torch.float16, device="cuda")
        lens = torch.empty((3,), dtype=torch.int32, device="cuda")
        table = torch.empty((3, 4), dtype=torch.int32, device="cuda")
        O, lse = torch.ops.qattn.mxfp4_decode_paged(q, u8(16, 2, 128, 64), u8(16, 2, 128, 4),
                                                    u8(16, 2, 2, 128, 32), u8(16, 2, 2, 128, 2), lens,
                                                    table, 256, 1, 0)
        assert O.shape == (3, 8, 5, 128) and O.dtype == torch.float16 and O.device.type == "cuda"
        assert lse.shape == (24, 5) and lse.dtype == torch.float32
