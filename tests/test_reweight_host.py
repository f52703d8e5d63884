"""lite.weight_blends without a GPU: the NumPy oracle against the reference's own fluxes, and
the host planning (rectangles, offsets, groups, fallbacks, chunks) of lite/measure.py."""

import numpy as np
import pytest

import reweight_cases as cases
import reweight_oracle
from conftest import golden

def golden_scene(hsc, g, dtype=np.float32):
    """Arguments of ``reweight_oracle.reweight`` for the fitted FISTA scene of the golden."""
    comps = [(g["b_sed_%d" % k].astype(dtype), g["b_morph_%d" % k].astype(dtype),
              tuple(int(v) for v in g["b_origin_%d" % k])) for k in range(int(g["n_comp"]))]
    py, px = hsc["psfs"].shape[-2] // 2, hsc["psfs"].shape[-1] // 2
    return (hsc["images"].astype(dtype), hsc["weights"].astype(dtype), (py, px),
            g["diff_kernel"].astype(dtype), comps, [[k] for k in range(len(comps))])


def test_oracle_reproduces_the_reference_fluxes(hsc):
    """The float32 oracle gives the ten ``flux_*`` arrays the reference wrote for its fitted
    FISTA scene (tests/golden/lite_fista.npz): shapes and ``flux_origin_*`` equal, values
    within 1e-5 of each array's largest absolute value.  Measured worst case: 2.6e-6 (four
    of the ten boxes leave the 58 x 48 frame; the stamp is 43 x 43)."""
    g = golden("lite_fista")
    assert any(int(v) < 0 for k in range(10) for v in g["b_origin_%d" % k])
    worst = cases.check_against_golden(reweight_oracle.reweight(*golden_scene(hsc, g)), g)
    print("worst relative deviation from the golden: %.3g" % worst)


def test_oracle_convolution_is_the_tap_loop():
    """The shifted block adds equal the per-pixel loop: accumulator from 0, taps row-major,
    one rounded multiply and one rounded add, taps outside the array skipped."""
    rng = np.random.RandomState(3)
    img = rng.normal(size=(1, 6, 5)).astype(np.float32)
    stamp = rng.normal(size=(1, 3, 5)).astype(np.float32)
    want = np.zeros_like(img)
    for y in range(6):
        for x in range(5):
            acc = np.float32(0)
            for ky in range(3):
                for kx in range(5):
                    r, c = y - (ky - 1), x - (kx - 2)
                    if 0 <= r < 6 and 0 <= c < 5:
                        acc = np.float32(acc + np.float32(stamp[0, ky, kx] * img[0, r, c]))
            want[0, y, x] = acc
    assert np.array_equal(reweight_oracle.convolve(img, stamp), want)
    with pytest.raises(ValueError):
        reweight_oracle.convolve(img, np.ones((1, 2, 3), np.float32))


def test_cases_exercise_the_clamps():
    """Over the synthetic cases the oracle clamps ratios to 1, zeroes ratios where the total
    is 0 and meets masked pixels -- and so does every frame size on its own."""
    for names in (["7x5-none", "7x5-3x3", "7x5-5x9", "7x5-15x15"], ["33x31-bcast", "33x31-C7"],
                  ["64x65-C1"], ["31x33-big-psf"]):
        stats = {}
        for name in names:
            cases.oracle(cases.make_blend(name), stats=stats)
        assert stats["clamped"] > 0 and stats["zeroed"] > 0 and stats["masked"] > 0, (names, stats)


# ------------------------------------------------------------------ planning
def test_rectangles_offsets_and_empty_boxes():
    from scarlet_amd.lite import measure

    blend = cases.make_blend("33x31-C7")  # frame corner (3, -2), psf half (4, 4)
    H, W, C = 33, 31, 7
    plan = measure._plan_blend(blend)
    assert plan["scene"] == len(blend.components) == 8
    # scene components: clipped to the frame, relative to its corner
    rects = [(c[1], c[2], c[3], c[4], c[5], c[6]) for c in plan["comps"][:8]]
    assert rects[0] == (2, 1, 5, 5, 0, 0)            # inside
    assert rects[2] == (0, W // 2 - 2, 3, 5, 2, 0)   # top edge: two rows cut, morph row 2 first
    assert rects[3] == (H // 2 - 2, 0, 5, 2, 0, 3)   # left edge
    assert rects[4] == (H - 3, 1, 3, 5, 0, 0)        # bottom edge
    assert rects[5] == (1, W - 2, 5, 2, 0, 0)        # right edge
    assert rects[6][2] == 0 or rects[6][3] == 0      # wholly outside: empty
    # source components: unclipped, may be negative
    src = {id(c[0]): (c[1], c[2], c[3], c[4], c[5], c[6]) for c in plan["comps"][8:]}
    assert src[id(blend.sources[1].components[0])] == (-2, W // 2 - 2, 5, 5, 0, 0)
    # output rectangles: the grown box inside the frame
    s = plan["sources"]
    assert s[0][1:] == (8, 2, 0, 0, (C, 7 + 4, 9 + 4))  # rows 2..7, columns 1..9, grown by 4, clipped
    assert s[1][3:] == (0, W // 2 - 6, (C, 7, 13))
    assert s[3][3:] == (H - 7, 0, (C, 7, 10))
    assert s[5][5] == (C, 0, 7) and s[5][1] is not None       # misses the frame: empty
    assert s[6][1] is None                                      # null source
    for (src_, comp0, n, y0, x0, shape), source in zip(s, blend.sources):
        if comp0 is not None:
            assert [c[0] for c in plan["comps"][comp0:comp0 + n]] == source.components
            if np.prod(shape):  # (an empty rectangle is never sent to the device)
                assert 0 <= y0 and 0 <= x0 and y0 + shape[1] <= H and x0 + shape[2] <= W

    key = measure._group_key(blend)
    assert key == (np.dtype(np.float32), C, 3, 5)
    packed = measure._pack([plan], key, True)
    # offsets: results back to back in source order, empty and null sources take no room
    sizes = [int(np.prod(x[5])) for x in s if x[1] is not None and np.prod(x[5]) > 0]
    assert list(packed["sources"]["out_off"]) == list(np.cumsum([0] + sizes[:-1]))
    assert packed["n_out"] == sum(sizes) and len(packed["results"]) == 6
    assert packed["blends"]["n_comp"][0] == 8 and packed["blends"]["image_off"][0] == 0
    # every descriptor stays inside its buffer
    comps = packed["comps"]
    live = (comps["h"] > 0) & (comps["w"] > 0)
    last = comps["morph_off"] + (comps["h"] - 1) * comps["stride"] + comps["w"]
    assert (comps["morph_off"][live] >= 0).all() and (last[live] <= packed["morphs"].size).all()
    assert (comps["sed_off"] + C <= packed["seds"].size).all()
    # a morphology shared by the scene and its source is packed once
    assert packed["morphs"].size == sum(c.morph.size for c in blend.components)
    # masked images: zero weights zero the pixel
    img = packed["images"].reshape(C, H, W)
    assert (img[:, 1:3, 0:2] == 0).all() and np.array_equal(img[1, 5:], blend.observation.images[1, 5:])
    # the records are the C structs of include/scarlet_amd.h
    assert (measure._BLEND_DESC.itemsize, measure._SOURCE_DESC.itemsize,
            measure._COMP_DESC.itemsize) == (32, 40, 40)

    # the flux boxes come out in the coordinates of the observation
    out = np.arange(packed["n_out"], dtype=np.float32)
    measure._assign([plan], packed, out)
    assert blend.sources[6].flux == 0 and blend.sources[6].flux_box.shape == (0, 0, 0)
    assert blend.sources[5].flux.shape == (C, 0, 7) == blend.sources[5].flux_box.shape
    assert blend.sources[0].flux_box.origin == (0, 3, -2) and blend.sources[0].flux[0, 0, 1] == 1
    assert blend.sources[1].flux.base is None  # an array of its own, not a view of the chunk
    for got, (_, origin) in zip(blend.sources, cases.oracle(blend)):
        if origin is not None:
            assert tuple(got.flux_box.origin) == origin


def test_groups_keep_input_order_and_mixed_dtypes_fall_back():
    from scarlet_amd.lite import measure

    names = ["7x5-3x3", "33x31-bcast", "64x65-C1", "31x33-big-psf", "7x5-none"]
    blends = [cases.make_blend(n) for n in names]
    blends.insert(2, cases.make_blend("7x5-3x3", mixed=True))
    blends.append(cases.make_blend("33x31-bcast", dtype=np.float64))
    blends.append(cases.make_blend("7x5-3x3", seed=1))
    groups, fallback = measure.plan_blends(blends)
    f4, f8 = np.dtype(np.float32), np.dtype(np.float64)
    assert fallback == [2]
    assert groups == {(f4, 3, 3, 3): [0, 7], (f4, 3, 5, 5): [1], (f4, 1, 7, 5): [3],
                      (f4, 2, 3, 3): [4], (f4, 3, 1, 1): [5], (f8, 3, 5, 5): [6]}
    assert list(groups)[0] == (f4, 3, 3, 3)  # order of first appearance
    # a source of another dtype, or a stamp beyond the LDS tile, falls back too
    odd = cases.make_blend("7x5-3x3")
    odd.sources[0].dtype = np.float64
    assert measure._group_key(odd) is None
    assert measure._stamp_fits(43, 43, 8) and not measure._stamp_fits(47, 47, 8)
    assert measure._stamp_fits(73, 73, 4) and not measure._stamp_fits(75, 75, 4)


def test_chunks_cover_every_source_once():
    from scarlet_amd import _catalog
    from scarlet_amd.lite import measure

    blends = [cases.make_blend("7x5-3x3", seed=s) for s in range(5)]
    key = measure._group_key(blends[0])
    plans = [measure._plan_blend(b) for b in blends]
    items = [(p, measure._plan_bytes(p, key)) for p in plans]
    assert len(_catalog.chunks(items, _catalog.WORKING_SET_BYTES)) == 1
    need = (measure._plan_elements(plans[0]) + 27) * 4
    for budget, n in ((1, 5), (need, 5), (2 * need, 3), (5 * need, 1)):
        chunks = _catalog.chunks(items, budget)
        assert len(chunks) == n
        assert [id(p) for c in chunks for p in c] == [id(p) for p in plans]
        seen = []
        for c in chunks:
            packed = measure._pack(c, key, True)
            seen += [id(r[0]) for r in packed["results"]]
            assert len(packed["blends"]) == len(c)
        want = [id(s[0]) for p in plans for s in p["sources"] if s[1] is not None and np.prod(s[5])]
        assert seen == want and len(set(seen)) == len(seen)


def test_even_stamp_is_refused_before_any_gpu_work():
    from types import SimpleNamespace

    from scarlet_amd import lite

    blend = cases.make_blend("7x5-3x3")
    blend.observation.diff_kernel = SimpleNamespace(image=np.ones((3, 4, 3), np.float32))
    with pytest.raises(ValueError, match="odd height and width"):
        lite.weight_blends([cases.make_blend("7x5-none"), blend])
