"""lite.fit_spectra_blends on the device: the spectra against the float64 restatement of
``multifit_seds`` (tests/init_oracle.py::joint_fit) within the error bound of the normal
equations, everything else bit for bit what the loop of ``fit_spectra`` leaves; the same bits
in any chunking and order; malformed tables refused at the C entries.

Worst observed |batch - oracle| over the bound (MI355X): 0.0077 for float64 spectra
(one-component); float32 spectra equal the oracle's cast to float32 in every bit but in
7x5-5x9 (2.7e-9 of the bound).  The loop's float32 FFT convolution is up to 1.8 bounds away in
float32 and 1.8e3 to 2.5e6 in float64."""

import ctypes

import numpy as np
import pytest

import fit_spectra_cases as cases
from conftest import golden

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(name, dtype):
    """``cases.oracle`` of a case, computed once."""
    key = (name, np.dtype(dtype).name)
    if key not in _ORACLE:
        _ORACLE[key] = cases.oracle(cases.make_blend(name, dtype))
    return _ORACLE[key]


def _spectra(blend):
    return np.stack([c.sed for c in blend.components])


_ratio = cases.ratio_to_bound


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", cases.NAMES)
def test_spectra_against_the_float64_oracle(name, dtype):
    from scarlet_amd import lite

    seds64, cond, n_pix = _oracle(name, dtype)
    blend, copy = cases.make_blend(name, dtype), cases.make_blend(name, dtype)
    assert lite.plan_fit_spectra_blends([blend])[1] == []
    assert lite.fit_spectra_blends([blend])[0] is blend
    got = _spectra(blend)
    assert got.dtype == dtype and got.shape == seds64.shape
    ratio = _ratio(got, seds64, cond, n_pix, dtype)
    copy.fit_spectra()
    print("%s %s: cond %.3g, |batch - oracle| / bound %.3g, |loop - oracle| / bound %.3g"
          % (name, np.dtype(dtype).name, cond, ratio,
             _ratio(_spectra(copy), seds64, cond, n_pix, dtype)))
    assert ratio <= 1, (name, ratio)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_same_components_survive_as_in_the_loop(name, clip):
    """Per source and in the blend's own order.

    The eight blends of ``reweight_cases`` have a source whose box lies wholly outside the
    frame, grown box included, and shares no pixel with another column: its least-squares
    spectrum is an exact 0, and the loop's float32 FFT convolution leaves round-off of either
    sign there (measured on an MI355X: 5e-10 to 8e-8 in the largest band, next to 0.5 to 2 for
    the components on the frame), so the loop keeps the component in five of the eight and
    drops it in three.  With ``clip=True`` such a blend goes through the loop, and the plan
    says so; every other case, and all of them with ``clip=False``, take the device."""
    from scarlet_amd import lite

    blend, copy = cases.make_blend(name), cases.make_blend(name)
    index = {id(c): k for k, c in enumerate(blend.components)}
    copy_index = {id(c): k for k, c in enumerate(copy.components)}
    groups, fallback = lite.plan_fit_spectra_blends([blend], clip)
    if clip and name in cases.reweight_cases.CASES:
        assert not groups and "do not reach" in fallback[0][1]
    else:
        assert len(groups) == 1 and not fallback
    lite.fit_spectra_blends([blend], clip=clip)
    copy.fit_spectra(clip)
    assert ([[index[id(c)] for c in s.components] for s in blend.sources]
            == [[copy_index[id(c)] for c in s.components] for s in copy.sources])
    assert [index[id(c)] for c in blend.components] == [copy_index[id(c)] for c in copy.components]


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", cases.NAMES)
def test_arrays_are_written_in_place_and_nothing_else_changes(name, clip):
    from scarlet_amd import lite

    blend = cases.make_blend(name)
    arrays = [c.sed for c in blend.components]
    index = {id(c): k for k, c in enumerate(blend.components)}
    before = cases.state(blend)
    lite.fit_spectra_blends([blend], clip=clip)
    kept = [index[id(c)] for c in blend.components]
    assert kept == sorted(kept)
    assert kept == [index[id(c)] for s in blend.sources for c in s.components]
    if clip:
        assert all(np.any(c.sed) and np.all(c.sed >= 0) for c in blend.components)
    else:
        assert len(kept) == len(arrays)
        assert all(np.all(c.sed >= c.floor) for c in blend.components)
    for c in blend.components:
        assert c.sed is arrays[index[id(c)]]
    # morphologies, boxes and optimizer state: unchanged in every bit
    after = cases.state(blend)
    assert [before[1][k] for k in kept] == after[1]


def test_the_reference_fitted_scene(hsc):
    """hsc_cosmos_35 after the reference's FISTA fit, 43 x 43 stamp: within the bound of the
    oracle, and within the distance test_gpu_facade.py allows the loop from the reference's own
    multifit_seds."""
    from scarlet_amd import lite

    g = golden("lite_fista")
    blend = cases.hsc_blend(hsc, g)
    assert lite.plan_fit_spectra_blends([blend]) == ({(np.dtype(np.float32), 5, 43, 43): [0]}, [])
    seds64, cond, n_pix = cases.oracle(blend)
    lite.fit_spectra_blends([blend])
    got = _spectra(blend)
    ratio = _ratio(got, seds64, cond, n_pix, np.float32)
    far = np.abs(got - g["multifit_seds"]).max() / np.abs(g["multifit_seds"]).max()
    print("hsc: cond %.3g, |batch - oracle| / bound %.3g, |batch - reference| / max %.3g"
          % (cond, ratio, far))
    assert ratio <= 1
    assert far < 2e-3


GROUP = ["union-15", "disjoint", "union-17", "present-32", "components-64"]


def test_one_group_in_chunks_and_orders_gives_the_same_bits():
    from scarlet_amd import _catalog, lite
    from scarlet_amd.lite import spectra

    key = (np.dtype(np.float32), 2, 3, 3)

    def run(order, budget=None, twice=False):
        blends = [cases.make_blend(n) for n in GROUP]
        assert list(lite.plan_fit_spectra_blends(blends)[0]) == [key]
        lite.fit_spectra_blends([blends[i] for i in order], _working_set_bytes=budget)
        if twice:  # (the spectra are no input of the fit)
            lite.fit_spectra_blends([blends[i] for i in order], _working_set_bytes=budget)
        return [_spectra(b) for b in blends]

    plans = [spectra._plan_blend(cases.make_blend(n))[1] for n in GROUP]
    middle = sum(spectra._plan_bytes(p, key) for p in plans[:3])
    items = [(p, spectra._plan_bytes(p, key)) for p in plans]
    assert 1 < len(_catalog.chunks(items, middle)) < len(GROUP)
    forward = list(range(len(GROUP)))
    want = run(forward)
    for order, budget, twice in ((forward, middle, False), (forward, 1, False),
                                 ([3, 1, 4, 0, 2], None, False), ([4, 3, 2, 1, 0], middle, False),
                                 (forward, None, True)):
        for name, a, b in zip(GROUP, want, run(order, budget, twice)):
            assert np.array_equal(a, b), (name, order, budget, twice)
    # the sums themselves: the disjoint pair's entry is an exact 0 wherever the blend stands
    for order in (forward, [3, 1, 4, 0, 2]):
        packed = spectra._pack([plans[i] for i in order], key)
        out = spectra._run_chunk(packed, key, 0)
        gram, rhs = spectra._normal_equations(packed, out, 2)[order.index(1)]
        assert np.all(gram[:, 0, 1] == 0) and np.all(gram[:, 1, 0] == 0)
        assert np.all(gram[:, [0, 1], [0, 1]] > 0) and np.all(rhs != 0)
        if order is forward:
            first = gram.copy(), rhs.copy()
        else:
            assert np.array_equal(gram, first[0]) and np.array_equal(rhs, first[1])
    # without a cross term each spectrum is its own quotient
    alone = np.where(first[1] / first[0][:, [0, 1], [0, 1]] < 0, 0, first[1] / first[0][:, [0, 1], [0, 1]])
    assert np.allclose(want[1].T, np.maximum(alone, 1e-20), rtol=1e-6)


def _even():
    blend = cases.make_blend("7x5-3x3")
    blend.observation.diff_kernel.image = np.ones((3, 4, 3), np.float32) / 12
    blend.observation.mode = "real"  # (the loop then refuses the stamp before it convolves)
    return blend


def _catalogue():
    return [cases.make_blend("7x5-3x3"), cases.make_blend("union-16", np.float64),
            cases.reweight_cases.make_blend("7x5-3x3", mixed=True), cases.make_blend("union-17"),
            cases.make_blend("present-33"), cases.make_blend("7x5-3x3", np.float64),
            cases.make_blend("union-15"), cases.make_blend("three-tiles", np.float64), _even()]


def test_mixed_catalogue():
    """float32 and float64 groups, a mixed-dtype blend, one past a limit and, last, an even
    stamp: every blend of a device group equals its single-blend call, the others equal the
    loop, whose exception for the even stamp surfaces after everything else is done."""
    from scarlet_amd import lite

    groups, fallback = lite.plan_fit_spectra_blends(_catalogue())
    assert [i for i, _ in fallback] == [2, 4, 8]
    assert [len(v) for v in groups.values()] == [1, 1, 2, 1, 1]
    together, alone = _catalogue(), _catalogue()
    with pytest.raises(ValueError, match="odd height and width"):
        lite.fit_spectra_blends(together)
    with pytest.raises(ValueError, match="odd height and width"):
        alone[8].fit_spectra()
    for i, (a, b) in enumerate(zip(together[:8], alone[:8])):
        if i in (2, 4):
            b.fit_spectra()
        else:
            lite.fit_spectra_blends([b])
        assert np.array_equal(_spectra(a), _spectra(b)), i
        assert _spectra(a).dtype == a.observation.images.dtype
    assert np.array_equal(_spectra(together[8]), _spectra(_even()))  # untouched


def test_malformed_tables_are_refused_and_leave_the_output_alone():
    """smi_lite_spectra_* validates the plan on the host: nothing out of range is launched,
    nothing is written."""
    from scarlet_amd import _lib
    from scarlet_amd.lite import spectra

    lib = _lib.load()
    blend = cases.make_blend("union-17")
    key, _ = spectra._spectra_key(blend)

    def call(change=None, stamp=key[2:], null=None, counts=None):
        p = spectra._pack([spectra._plan_blend(blend)[1]], key)
        if change:
            table, field, value = change
            p[table][field][0] = value
        out = np.full(p["n_out"], 7.25)
        args = [0, key[1], stamp[0], stamp[1]]
        for name in ("blends", "comps"):
            n = len(p[name]) if counts is None else counts.get(name, len(p[name]))
            args += [n, None if null == name else p[name].ctypes.data]
        for arr, t in ((p["images"], ctypes.c_float), (p["stamps"], ctypes.c_double),
                       (p["morphs"], ctypes.c_float), (out, ctypes.c_double)):
            args += [_lib.ptr(arr, t), arr.size]
        status = lib.smi_lite_spectra_f32(*args)
        return status, out

    status, out = call()
    assert status == 0 and not np.any(out == 7.25)
    bad = [dict(counts={"blends": -1}), dict(counts={"comps": -1}),      # a negative count
           dict(change=("blends", "fh", spectra.MAX_EXTENT + 1)),          # beyond the extent limit
           dict(change=("comps", "h", spectra.MAX_EXTENT + 1)),
           dict(change=("comps", "h", 18)),                                # leaves the union box
           dict(change=("comps", "y0", 0)),
           dict(stamp=(4, 3)), dict(stamp=(3, 2)),                         # an even stamp
           dict(stamp=(spectra.MAX_STAMP + 2, 3)),
           dict(change=("comps", "morph_off", 10 ** 9)),                   # offsets past buffers
           dict(change=("comps", "morph_off", 82)),
           dict(change=("blends", "image_off", 1)),
           dict(change=("blends", "stamp_off", 1)),
           dict(change=("blends", "out_off", 1)),
           dict(change=("blends", "out_off", -1)),
           dict(change=("blends", "n_comp", spectra.MAX_COMPONENTS + 1)),
           dict(change=("blends", "n_comp", 0)),
           dict(change=("blends", "comp0", 1)),
           dict(null="blends"), dict(null="comps")]                        # a null table
    for kwargs in bad:
        status, out = call(**kwargs)
        assert status == -1, kwargs
        assert np.all(out == 7.25), kwargs
    # more than MAX_PRESENT components on one tile: refused by the entry as by the plan
    crowd = cases.make_blend("present-33")
    boxes, union = spectra._geometry(crowd)
    p = spectra._pack([dict(blend=crowd, boxes=boxes, union=union,
                            stamp=spectra._stamp_of(crowd))], key)
    with pytest.raises(_lib.ScarletAmdError, match="status -1"):
        spectra._run_chunk(p, key, 0)
