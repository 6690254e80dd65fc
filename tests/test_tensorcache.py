"""The one rule of every tensor-identity cache (diffgfdn_amd/tensorcache.py), on CPU tensors."""
import gc
import weakref

import pytest
import torch

from diffgfdn_amd.tensorcache import TensorCache, tensor_key


class _Value:
    """a cached value a weakref can point at"""

    def __init__(self, tag):
        self.tag = tag


def _counting(value="v"):
    calls = []

    def build():
        calls.append(1)
        return value
    return build, calls


def test_key_fields():
    t = torch.arange(6.0).reshape(2, 3)
    assert tensor_key(None) is None
    assert tensor_key(t) == (t.data_ptr(), (2, 3), (3, 1), torch.float32, t.device, t._version)
    assert tensor_key(t) != tensor_key(t.T) and tensor_key(t) != tensor_key(t.view(torch.int32))
    hash(tensor_key(t))


def test_same_tensor_hits_and_builds_once():
    c, t = TensorCache(), torch.ones(4)
    build, calls = _counting()
    assert c.get((t,), 3, build) == "v" and c.get((t,), 3, build) == "v" and c.get((t.view(4),), 3, build) == "v"
    assert len(calls) == 1
    c.get((t,), 4, build)                                  # another ``extra``: another entry
    assert len(calls) == 2


@pytest.mark.parametrize("edit", [lambda t: t.mul_(2.0), lambda t: torch.autograd.graph.increment_version(t)])
def test_in_place_edit_misses(edit):
    c, t = TensorCache(), torch.ones(4)
    build, calls = _counting()
    c.get((t,), None, build)
    edit(t)
    c.get((t,), None, build)
    assert len(calls) == 2
    c.get((t,), None, build)
    assert len(calls) == 2


def test_equal_values_miss_by_identity_and_hit_by_value(monkeypatch):
    t = torch.arange(5.0)
    c = TensorCache()
    build, calls = _counting()
    c.get((t,), None, build)
    c.get((t.clone(),), None, build)
    assert len(calls) == 2

    c = TensorCache(by_value=True)
    build, calls = _counting(_Value(0))
    v = c.get((t, None), 7, build)
    u = t.clone()
    assert c.get((u, None), 7, build) is v and len(calls) == 1
    monkeypatch.setattr(torch, "equal", lambda *a: pytest.fail("an identity hit compares nothing"))
    assert c.get((u, None), 7, build) is v and len(calls) == 1            # re-keyed: the new tensor hits by identity
    monkeypatch.undo()
    # equal values are not enough: extra, dtype and shape belong to the match, and so does an edit of the copy's source
    c.get((u, None), 8, build)
    assert len(calls) == 2
    c.get((u.to(torch.float64), None), 8, build)
    assert len(calls) == 3
    w = u.to(torch.float64)
    c.get((w, None), 8, build)
    assert len(calls) == 3
    w[0] = 9.0
    c.get((w, None), 8, build)
    assert len(calls) == 4


def test_identity_hit_never_compares_values(monkeypatch):
    c, t = TensorCache(by_value=True), torch.ones(3)
    build, calls = _counting()
    c.get((t,), None, build)

    def boom(*a):
        raise AssertionError("torch.equal on an identity hit")
    monkeypatch.setattr(torch, "equal", boom)
    assert c.get((t,), None, build) == "v" and len(calls) == 1


def test_entry_keeps_its_key_tensor_alive():
    for drop in ("evict", "clear"):
        c, t = TensorCache(), torch.ones(4)
        ref = weakref.ref(t)
        c.get((t,), None, lambda: 1)
        del t
        gc.collect()
        assert ref() is not None, "the entry holds the tensor: its address stays its own"
        if drop == "evict":
            c.get((torch.zeros(2),), None, lambda: 2)
        else:
            c.clear()
        gc.collect()
        assert ref() is None, drop


def test_capacity_evicts_only_the_oldest():
    c = TensorCache(capacity=3)
    ts = [torch.full((2,), float(i)) for i in range(4)]
    build, calls = _counting()
    for t in ts:
        c.get((t,), None, build)
    assert len(calls) == 4 and len(c.values()) == 3
    c.get((ts[1],), None, build), c.get((ts[2],), None, build), c.get((ts[3],), None, build)
    assert len(calls) == 4, "the three younger entries still hit"
    c.get((ts[0],), None, build)
    assert len(calls) == 5, "the oldest was dropped"


@pytest.mark.parametrize("by_value", [False, True])
def test_capacity_one_releases_the_old_value_before_the_build(by_value):
    c = TensorCache(capacity=1, by_value=by_value)
    old = _Value("old")
    ref = weakref.ref(old)
    c.get((torch.ones(2),), None, lambda: old)
    del old
    gc.collect()
    assert ref() is not None
    seen = []

    def build():
        gc.collect()
        seen.append(ref())
        return _Value("new")
    assert c.get((torch.zeros(2),), None, build).tag == "new"
    assert seen == [None], "never two stores alive"


def test_none_among_the_tensors_and_none_as_value():
    for by_value in (False, True):
        c, t = TensorCache(by_value=by_value), torch.ones(2)
        build, calls = _counting(None)
        assert c.get((None, t, None), "x", build) is None
        assert c.get((None, t, None), "x", build) is None
        assert len(calls) == 1 and c.values() == [None]
        c.get((t, None, None), "x", build)                 # None is a position, not a wildcard
        assert len(calls) == 2
    c = TensorCache(by_value=True)
    c.get((None,), None, build)
    c.get((torch.ones(2),), None, build)                   # a tensor where the entry has None: no match, no comparison error
    assert len(calls) == 4


def test_no_capture(monkeypatch):
    c, t = TensorCache(capacity=4, no_capture="first use inside a capture"), torch.ones(2)
    build, calls = _counting()
    c.get((t,), None, build)
    # (without a device the query itself raises, so the cache asks an initialised runtime only: both are patched)
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert c.get((t,), None, build) == "v"                 # a hit is served inside a capture
    with pytest.raises(RuntimeError, match="first use inside a capture"):
        c.get((torch.ones(2),), None, build)
    assert len(calls) == 1
    plain = TensorCache()
    assert plain.get((torch.ones(2),), None, build) == "v"    # caches without the message build anywhere
