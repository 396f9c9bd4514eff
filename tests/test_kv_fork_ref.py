"""Copy-on-fork building blocks on the CPU: the reference semantics of
ops.kv_copy_blocks_ and the refcounts behind PagedKVCache.share."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import PagedKVCache

SHAPE = (2, 6, 1, 16, 8)


def _caches(dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    k = torch.randn(SHAPE, generator=g).to(dtype)
    v = torch.randn(SHAPE, generator=g).to(dtype)
    return k, v


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16,
                                   torch.float8_e4m3fn])
def test_ref_copy_semantics(dtype):
    k, v = _caches(dtype)
    k0, v0 = k.clone(), v.clone()
    # src repeats (one tail feeds several children); dst unique
    src, dst = [1, 1, 4], [0, 3, 5]
    ops.kv_copy_blocks_(k, v, _i32(src), _i32(dst))
    for c, c0 in ((k, k0), (v, v0)):
        raw, raw0 = c.view(torch.uint8), c0.view(torch.uint8)
        for layer in range(SHAPE[0]):
            for s, d in zip(src, dst):
                assert torch.equal(raw[layer, d], raw0[layer, s])
            for b in set(range(SHAPE[1])) - set(dst):
                assert torch.equal(raw[layer, b], raw0[layer, b])


def test_ref_copy_empty_is_a_noop():
    k, v = _caches()
    k0, v0 = k.clone(), v.clone()
    ops.kv_copy_blocks_(k, v, _i32([]), _i32([]))
    assert torch.equal(k, k0) and torch.equal(v, v0)


def test_ref_copy_length_mismatch_raises():
    k, v = _caches()
    with pytest.raises(ValueError):
        ops.kv_copy_blocks_(k, v, _i32([1, 2]), _i32([3]))


def test_cache_copy_blocks_uploads_and_copies():
    kv = PagedKVCache(2, 6, 1, 16, 8, dtype=torch.float32)
    kv.k.copy_(torch.arange(kv.k.numel()).view_as(kv.k))
    kv.v.copy_(-torch.arange(kv.v.numel()).view_as(kv.v))
    k0, v0 = kv.k.clone(), kv.v.clone()
    kv.copy_blocks([2, 2], [4, 5])
    kv.copy_blocks([], [])
    for d in (4, 5):
        assert torch.equal(kv.k[:, d], k0[:, 2])
        assert torch.equal(kv.v[:, d], v0[:, 2])
    for b in (0, 1, 2, 3):
        assert torch.equal(kv.k[:, b], k0[:, b])
        assert torch.equal(kv.v[:, b], v0[:, b])


def test_share_free_refcounts():
    kv = PagedKVCache(1, 4, 1, 16, 8, dtype=torch.float32)
    blocks = kv.allocate(2)
    assert kv.free_blocks == 2
    shared = kv.share(blocks)
    assert shared == blocks and shared is not blocks
    kv.share(blocks[:1])                       # third holder of block 0
    kv.free(blocks)                            # first holder leaves
    assert kv.free_blocks == 2                 # both still held
    kv.free(shared)
    assert kv.free_blocks == 3                 # blocks[1] is back
    assert blocks[1] in kv._free and blocks[0] not in kv._free
    kv.free(blocks[:1])
    assert kv.free_blocks == 4
    assert sorted(kv._free) == [0, 1, 2, 3]


def test_shared_keyed_block_goes_to_cached_free():
    kv = PagedKVCache(1, 4, 1, 16, 8, dtype=torch.float32)
    (b,) = kv.allocate(1)
    kv.register_block(b, b"key")
    kv.share([b])
    kv.free([b])
    assert b not in kv._cached_free and kv.free_blocks == 3
    kv.free([b])                               # last holder
    assert b in kv._cached_free and b not in kv._free
    assert kv.free_blocks == 4
    assert kv.lookup_prefix([b"key"]) == [b]   # still indexed, reusable


def test_share_of_a_free_block_asserts():
    kv = PagedKVCache(1, 4, 1, 16, 8, dtype=torch.float32)
    with pytest.raises(AssertionError):
        kv.share([0])
