"""What the catalogue entry points share (scarlet_amd/_catalog.py) and the one refusal of
measure_blends and render_blends with its three switches.  No GPU, and no library."""

import ctypes

import numpy as np
import pytest

import render_blends_cases as rc
from init_blends_cases import scene
from measure_sources_cases import component


def test_chunks():
    from scarlet_amd._catalog import chunks

    items = [(0, 5), (1, 5), (2, 20), (3, 1)]
    assert chunks([], 10) == []
    assert chunks(items, 1) == [[0], [1], [2], [3]]
    assert chunks(items, 1 << 62) == [[0, 1, 2, 3]]
    # an item beyond the budget is a chunk of its own, and what follows starts anew
    assert chunks(items, 10) == [[0, 1], [2], [3]]
    # the positions are whatever the caller pairs with the bytes
    a, b = object(), object()
    assert chunks([(a, 6), (b, 6)], 10) == [[a], [b]]


def test_offsets():
    from scarlet_amd._catalog import offsets

    off, total = offsets([6, 0, 10])
    assert off.dtype == np.int64 and list(off) == [0, 6, 6] and total == 16
    off, total = offsets([])
    assert off.dtype == np.int64 and off.shape == (0,) and total == 0 and type(total) is int
    off, total = offsets(np.array([3, 4], np.int32) * np.int64(1 << 31))
    assert list(off) == [0, 3 << 31] and total == 7 << 31


def test_cat():
    from scarlet_amd._catalog import cat

    for dtype in (np.float32, np.float64):
        none = cat([], dtype)
        assert none.dtype == dtype and none.shape == (0,)
    both = cat([np.arange(2, dtype=np.float32), np.arange(3, dtype=np.float32)], np.float64)
    assert both.dtype == np.float32 and list(both) == [0, 1, 0, 1, 2]  # (the parts' own type)


def test_defaults():
    from scarlet_amd import _catalog

    assert _catalog.WORKING_SET_BYTES == 1 << 30
    assert _catalog.defaults(None, None) == (1 << 30, 0)
    assert _catalog.defaults(1, "2") == (1, 2)


def test_call_args_against_a_hand_written_list():
    """One table, one input and an output that is not asked for (``flux`` of render_blends
    without REWEIGHT): a null pointer of size 0."""
    from scarlet_amd._catalog import call_args

    table = np.zeros(3, np.dtype([("a", "i4"), ("b", "i8")], align=True))
    seds = np.arange(5, dtype=np.float64)
    args = call_args([table], [(seds, ctypes.c_double)], [(None, ctypes.c_float)])
    assert len(args) == 6
    assert args[:2] == [3, table.ctypes.data]
    assert isinstance(args[2], ctypes.POINTER(ctypes.c_double))
    assert ctypes.cast(args[2], ctypes.c_void_p).value == seds.ctypes.data
    assert args[3:] == [5, None, 0]
    assert call_args([], [], []) == []


@pytest.fixture(scope="module")
def blends():
    return {name: blend for name, blend, _ in rc.catalogue()}


def _changed(change):
    """A one-source blend on a 2 x 25 x 31 frame with a 5 x 5 stamp, its observation changed."""
    import scarlet_amd as scarlet

    frame, obs = scene(1, (2, 25, 31), (5, 5), [])
    change(obs)
    return scarlet.Blend([component(frame, np.random.RandomState(5), (3, 4, 5, 5))], [obs])


def test_refusal_zero_weights(blends):
    from scarlet_amd.measure import _refusal

    blend = blends["zero weight"]
    assert _refusal(blend) == ("a weight that is zero, negative or not finite", None)
    assert _refusal(blend, zero_weights=True) == (None, (3, 5, 5))

    def negative(obs):
        obs.weights[1, 2, 3] = -1

    blend = _changed(negative)
    assert _refusal(blend) == ("a weight that is zero, negative or not finite", None)
    assert _refusal(blend, zero_weights=True) == ("a weight that is negative or not finite", None)


def test_refusal_null_subset(blends):
    from scarlet_amd.measure import _refusal

    blend = blends["subset null"]  # (it has a pixel without weight, too)
    reason = ("a NullRenderer of a subset of the frame's bands", None)
    assert _refusal(blend) == _refusal(blend, zero_weights=True) == reason
    assert _refusal(blend, zero_weights=True, null_subset=True) == (None, (3, 1, 1))
    assert _refusal(blend, null_subset=True) == (
        "a weight that is zero, negative or not finite", None)


def test_refusal_plain_data():
    import numpy.ma as ma

    from scarlet_amd.measure import _refusal

    def masked(obs):
        obs.data = ma.masked_invalid(obs.data)

    def wide(obs):
        obs.weights = obs.weights.astype(np.float64)

    blend = _changed(masked)
    assert _refusal(blend) == (None, (2, 5, 5))
    assert _refusal(blend, plain_data=True) == ("data that are not a plain float32 array", None)
    blend = _changed(wide)
    reason = ("weights that are not a plain float32 array", None)
    assert _refusal(blend) == _refusal(blend, plain_data=True) == reason


def test_the_two_plans_ask_with_their_switches(blends):
    """plan_measure_blends asks with every switch off, plan_render_blends with every switch on."""
    import scarlet_amd as scarlet
    from scarlet_amd.measure import _refusal

    names = list(blends)
    _, m_refused = scarlet.plan_measure_blends([blends[n] for n in names])
    _, r_refused = scarlet.plan_render_blends([blends[n] for n in names])
    for i, name in enumerate(names):
        assert m_refused.get(i) == _refusal(blends[name])[0]
        assert r_refused.get(i) == _refusal(blends[name], zero_weights=True, null_subset=True,
                                            plain_data=True)[0]
