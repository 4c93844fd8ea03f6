"""``ops.PackedConvWeight`` on the host: when a cached image is served, when it is re-packed, and into which storage -- for one
weight and for a list of same-shape weights (a grouped launch's images one after another).  The pack functions the cache calls
are replaced by recorders, so neither the library nor a device is needed."""
import importlib

import pytest
import torch


@pytest.fixture
def cache(monkeypatch):
    """-> (a fresh PackedConvWeight, the list of pack calls it makes: (weights, key, transpose_flip, out))."""
    ops = importlib.import_module("speak-hack_amd").ops
    calls = []

    def pack_image(w, key, transpose_flip=False, out=None):
        calls.append(([w], key, transpose_flip, out))
        return out if out is not None else torch.empty(w.numel())

    def pack_conv_weights_list(ws, key, transpose_flip=False, out=None):
        calls.append((list(ws), key, transpose_flip, out))
        return out if out is not None else torch.empty(len(ws) * ws[0].numel())

    def pack_conv_weights_wino_into(ws, outs, transpose_flip=False):
        calls.append((list(ws), "wino", transpose_flip, list(outs)))

    def empty_image(key, Cin, Cout, device, count=1):
        return torch.empty(count * Cin * Cout * 16, device=device)

    monkeypatch.setattr(ops, "pack_image", pack_image)
    monkeypatch.setattr(ops, "pack_conv_weights_list", pack_conv_weights_list)
    monkeypatch.setattr(ops, "pack_conv_weights_wino_into", pack_conv_weights_wino_into)
    monkeypatch.setattr(ops, "empty_image", empty_image)
    return ops.PackedConvWeight(), calls


def _weights(kind):
    """One [8,4,3,3] weight, or a list of three (the last repeating the first, as a two-image group repeats its trunks)."""
    if kind == "one":
        return torch.randn(8, 4, 3, 3)
    ws = [torch.randn(8, 4, 3, 3) for _ in range(2)]
    return ws + ws[:1]


def _members(w):
    return w if isinstance(w, list) else [w]


def _ptrs(ws):
    return [t.data_ptr() for t in ws]


KINDS = ("one", "list")
KEYS = (3, "wino")


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("kind", KINDS)
def test_unchanged_weights_are_served_from_the_cache(cache, kind, key):
    pk, calls = cache
    w = _weights(kind)
    first = pk.get(w, key)
    assert len(calls) == 1 and _ptrs(calls[0][0]) == _ptrs(_members(w))
    assert pk.get(w, key) is first and len(calls) == 1


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("kind", KINDS)
def test_an_in_place_update_repacks(cache, kind, key):
    pk, calls = cache
    w = _weights(kind)
    pk.get(w, key)
    with torch.no_grad():
        _members(w)[0].add_(1.0)             # the optimizer's in-place step: the version counter moves
    pk.get(w, key)
    assert len(calls) == 2


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("kind", KINDS)
def test_another_tensor_with_the_same_pointer_version_and_shape_repacks(cache, kind, key):
    pk, calls = cache
    w = _weights(kind)
    pk.get(w, key)
    other = [t.detach() for t in _members(w)]             # same storage, version counter and shape; another object
    assert _ptrs(other) == _ptrs(_members(w)) and [t._version for t in other] == [t._version for t in _members(w)]
    pk.get(other if kind == "list" else other[0], key)
    assert len(calls) == 2


@pytest.mark.parametrize("key", KEYS)
def test_any_changed_member_repacks_the_whole_list(cache, key):
    pk, calls = cache
    ws = [torch.randn(8, 4, 3, 3) for _ in range(3)]
    pk.get(ws, key)
    with torch.no_grad():
        ws[1].mul_(2.0)
    pk.get(ws, key)
    assert len(calls) == 2 and _ptrs(calls[1][0]) == _ptrs(ws)
    ws2 = [ws[0], ws[1].detach(), ws[2]]                  # one member replaced by another object of the same address
    pk.get(ws2, key)
    assert len(calls) == 3 and _ptrs(calls[2][0]) == _ptrs(ws)


@pytest.mark.parametrize("kind", KINDS)
def test_key_and_transpose_flip_have_separate_entries(cache, kind):
    pk, calls = cache
    w = _weights(kind)
    keys = [(3, False), (3, True), (5, False), (5, 2), ("wino", False), ("wino", True)]
    images = [pk.get(w, k, tf) for k, tf in keys]
    assert len(calls) == len(keys) and len({id(t) for t in images}) == len(keys)
    assert [(c[1], c[2]) for c in calls] == keys
    assert all(pk.get(w, k, tf) is t for (k, tf), t in zip(keys, images)) and len(calls) == len(keys)
    assert pk.get_wino(w, transpose_flip=True) is images[-1]


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_stale_image_is_repacked_into_its_own_storage(cache, kind, key):
    pk, calls = cache
    w = _weights(kind)
    first = pk.get(w, key)
    with torch.no_grad():
        _members(w)[-1].add_(1.0)
    again = pk.get(w, key)
    assert again.data_ptr() == first.data_ptr() and len(calls) == 2
    if key == "wino" and kind == "list":           # the list's images are rows of that one buffer
        assert [o.data_ptr() for o in calls[1][3]] == [r.data_ptr() for r in first.view(len(w), -1)]
    else:
        assert calls[1][3] is first
    # new shapes (another size): fresh storage
    bigger = [torch.randn(16, 4, 3, 3) for _ in _members(w)]
    fresh = pk.get(bigger if kind == "list" else bigger[0], key)
    assert len(calls) == 3 and fresh.data_ptr() != first.data_ptr() and fresh.numel() == 2 * first.numel()


def test_prepack_wino_fills_only_stale_images_in_one_call(cache):
    ops = importlib.import_module("speak-hack_amd").ops
    pk, calls = cache
    pks = [pk, ops.PackedConvWeight()]
    ws = [torch.randn(8, 4, 3, 3), torch.randn(4, 8, 3, 3)]
    served = pks[0].get_wino(ws[0])                               # already fresh: not packed again
    del calls[:]
    ops.prepack_wino([(pks[0], ws[0], False), (pks[0], ws[0], True), (pks[1], ws[1], False), (pks[1], ws[1], True)])
    assert len(calls) == 1 and _ptrs(calls[0][0]) == _ptrs([ws[0], ws[1], ws[1]]) and calls[0][2] == [True, False, True]
    assert pks[0].get_wino(ws[0]) is served and len(calls) == 1
    images = [pks[0].get_wino(ws[0], True), pks[1].get_wino(ws[1]), pks[1].get_wino(ws[1], True)]
    assert all(t is o for t, o in zip(images, calls[0][3])) and len(calls) == 1
    with torch.no_grad():
        ws[1].add_(1.0)
    ops.prepack_wino([(pks[0], ws[0], True), (pks[1], ws[1], False), (pks[1], ws[1], True)])
    assert len(calls) == 2 and _ptrs(calls[1][0]) == _ptrs([ws[1], ws[1]]) and calls[1][2] == [False, True]
    assert all(o is t for o, t in zip(calls[1][3], images[1:]))        # re-packed into their own storage
    assert pks[1].get_wino(ws[1]) is images[1] and pks[1].get_wino(ws[1], True) is images[2] and len(calls) == 2
